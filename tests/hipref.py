"""Test plumbing for the GPU parity tests: synthetic RVE inputs (numpy) and thin wrappers that move them through the
C ABI of libexaconstit_hip.so using torch tensors as device buffers.  The oracle (tests/orc.py) is the checker."""
import ctypes as C

import numpy as np


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    d = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (d if d > 0 else 1.0)


def random_quats(n, seed=20240928):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def make_rve(orc, N, p=1, distort=0.0, seed=1):
    """Cartesian N^3 mesh of the unit cube through the oracle's mesh builder (x fastest), optionally distorted."""
    n = (p + 1) ** 3
    E = N ** 3
    NN = (N * p + 1) ** 3
    conn = np.zeros(n * E, dtype=np.int32)
    X = np.zeros(NN * 3)
    orc.lib().orc_mesh(p, N, N, N, C.c_double(1.0), C.c_double(1.0), C.c_double(1.0), orc._ip(conn), orc._p(X))
    if distort > 0:
        rng = np.random.default_rng(seed)
        X = X + distort / (N * p) * rng.uniform(-1, 1, X.shape)
    G = np.zeros(n * 3 * n)
    W = np.zeros(n)
    orc.lib().orc_ref_elem(p, orc._p(G), orc._p(W))
    return dict(N=N, p=p, n=n, Q=n, E=E, NN=NN, conn=conn, X=X, G=G, W=W)


# ---- inputs of the high-order operator tests (tests/test_high_order_inputs_host.py asserts that they can tell index slips apart) -------
HO_SHEAR = np.array([[0.0, 0.15, -0.1], [0.05, 0.0, 0.12], [-0.08, 0.07, 0.0]])
HO_AMP = 0.06
HO_DT = 0.37


def warp_nodes(X, amp=HO_AMP):
    """smooth warp X' = X + S X + amp U(X) of byNODES coordinates: every Jacobian gets off-diagonal entries and a varying determinant, and
    no element inverts however the Gauss-Lobatto nodes cluster (a per-node jitter inverts elements at p >= 4)"""
    x, y, z = np.asarray(X).reshape(3, -1)
    U = np.stack([np.sin(2.1 * y + 0.3) * np.cos(1.7 * z), np.sin(1.9 * z + 0.5) * np.cos(2.3 * x), np.sin(2.2 * x + 0.7) * np.cos(1.3 * y)])
    P = np.stack([x, y, z])
    return (P + HO_SHEAR @ P + amp * U).ravel()


def nonsym_tangent(P, seed):
    """_spd_tangent of test_gpu_parity.py with the asymmetry raised to 30 % of scale: 50 (A A^T + 6 I) + 15 randn, (6,6,P) column-major per point"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((P, 6, 6))
    Cm = 50.0 * (A @ A.transpose(0, 2, 1) + 6 * np.eye(6)) + 15.0 * rng.standard_normal((P, 6, 6))
    return np.ascontiguousarray(Cm.transpose(0, 2, 1)).ravel()


def transpose_points(a, m):
    """per-point transpose of a field of column-major m x m matrices"""
    return np.ascontiguousarray(np.asarray(a).reshape(-1, m, m).transpose(0, 2, 1)).ravel()


_ho_cache = {}


def ho_inputs(orc, p, N):
    """warped N^3 mesh of order p with its oracle Jacobians and the seeded random fields of the high-order tests (cached, read-only)"""
    key = (p, N)
    if key not in _ho_cache:
        rve = make_rve(orc, N, p=p)
        rve["X"] = warp_nodes(rve["X"])
        E, Q, n, NN = rve["E"], rve["Q"], rve["n"], rve["NN"]
        P = E * Q
        rng = np.random.default_rng(1000 * p + N)
        xe = l_to_e(rve, rve["X"])
        J = np.zeros(9 * P); orc.lib().orc_jacobians(p, E, orc._p(xe), orc._p(J))
        eDS = np.zeros(3 * n * E)
        orc.lib().orc_element_eds(Q, E, n, orc._p(rve["W"]), orc._p(rve["G"]), orc._p(J), orc._p(eDS))
        inp = dict(rve=rve, p=p, N=N, E=E, Q=Q, n=n, NN=NN, P=P, xe=xe, J=J, eDS=eDS, dt=HO_DT, Cm=nonsym_tangent(P, seed=100 * p + N),
                   sig=rng.standard_normal(6 * P), x_e=rng.standard_normal(3 * n * E), y0=rng.standard_normal(3 * n * E),
                   xL=rng.standard_normal(3 * NN), yL0=rng.standard_normal(3 * NN), mask=(rng.uniform(size=3 * NN) < 0.1).astype(np.uint8),
                   field=rng.standard_normal(3 * n * E), qf=rng.standard_normal(6 * P))
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ho_cache[key] = inp
    return _ho_cache[key]


def _ro(orc, a):
    """pointer to an input array of the oracle: float64 and contiguous, or the oracle would read something else"""
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return orc._p(a)


class HighOrderOracle:
    """the oracle's side of the high-order tests on one ho_inputs() set; J, C, W and eDS can be replaced to mutate the reference's inputs"""

    def __init__(self, orc, inp):
        self.orc, self.inp, self.lib = orc, inp, orc.lib()
        r = inp["rve"]
        self.Q, self.E, self.n, self.G, self.W = inp["Q"], inp["E"], inp["n"], r["G"], r["W"]

    def _f(self, a):
        return _ro(self.orc, a)

    def residual(self, sig=None, J=None, y0=None):
        i = self.inp
        y = np.array(i["y0"] if y0 is None else y0)
        self.lib.orc_element_vector(self.Q, self.E, self.n, self._f(self.W), self._f(self.G), self._f(i["J"] if J is None else J),
                                    self._f(i["sig"] if sig is None else sig), self.orc._p(y))
        return y

    def eds(self, W=None, J=None):
        out = np.zeros(3 * self.n * self.E)
        self.lib.orc_element_eds(self.Q, self.E, self.n, self._f(self.W if W is None else W), self._f(self.G), self._f(self.inp["J"] if J is None else J), self.orc._p(out))
        return out

    def residual_bbar(self, dense=True, sig=None, eDS=None):
        i = self.inp
        y = np.array(i["y0"])
        f = self.lib.orc_element_vector_bbar if dense else self.lib.orc_add_mult_pa_bbar
        f(self.Q, self.E, self.n, self._f(self.W), self._f(self.G), self._f(i["J"]), self._f(i["eDS"] if eDS is None else eDS),
          self._f(i["sig"] if sig is None else sig), self.orc._p(y))
        return y

    def pa_action(self, Cm=None, J=None, x=None, y0=None):
        """TransformMatGradTo4D -> AssembleGradPA -> AddMultGradPA onto y0"""
        i = self.inp; P = i["P"]
        C4 = np.zeros(81 * P); D4 = np.zeros(81 * P)
        y = np.array(i["y0"] if y0 is None else y0)
        self.lib.orc_transform_4d(C.c_int64(P), self._f(i["Cm"] if Cm is None else Cm), self.orc._p(C4))
        self.lib.orc_assemble_grad_pa(self.Q, self.E, C.c_double(i["dt"]), self._f(self.W), self._f(i["J"] if J is None else J), self.orc._p(C4), self.orc._p(D4))
        self.lib.orc_add_mult_grad_pa(self.Q, self.E, self.n, self._f(self.G), self.orc._p(D4), self._f(i["x_e"] if x is None else x), self.orc._p(y))
        return y

    def pa_diag(self, Cm=None, J=None):
        i = self.inp
        d = np.zeros(3 * self.n * self.E)
        self.lib.orc_assemble_grad_diag_pa(self.Q, self.E, self.n, C.c_double(i["dt"]), self._f(self.W), self._f(self.G), self._f(i["J"] if J is None else J),
                                           self._f(i["Cm"] if Cm is None else Cm), self.orc._p(d))
        return d

    def ea(self, bbar=False, Cm=None):
        i = self.inp
        emat = np.zeros(9 * self.n * self.n * self.E)
        Cm = i["Cm"] if Cm is None else Cm
        if bbar:
            self.lib.orc_assemble_ea_bbar(self.Q, self.E, self.n, C.c_double(i["dt"]), self._f(self.W), self._f(self.G), self._f(i["J"]), self._f(i["eDS"]), self._f(Cm), self.orc._p(emat))
        else:
            self.lib.orc_assemble_ea(self.Q, self.E, self.n, C.c_double(i["dt"]), self._f(self.W), self._f(self.G), self._f(i["J"]), self._f(Cm), self.orc._p(emat))
        return emat

    def ea_mult(self, emat, x=None, y0=None):
        y = np.array(self.inp["y0"] if y0 is None else y0)
        self.lib.orc_ea_mult(self.E, self.n, self._f(emat), self._f(self.inp["x_e"] if x is None else x), self.orc._p(y))
        return y

    def ea_diag(self, emat):
        d = np.zeros(3 * self.n * self.E)
        self.lib.orc_ea_diag(self.E, self.n, self._f(emat), self.orc._p(d))
        return d


def l_to_e(rve, L):
    n, E, NN = rve["n"], rve["E"], rve["NN"]
    conn = rve["conn"].reshape(E, n)
    out = np.zeros((E, 3, n))
    for c in range(3):
        out[:, c, :] = L[conn + NN * c]
    return out.ravel()


def e_to_l(rve, Ev):
    """transpose of l_to_e: sums the element contributions (E, 3, n) into an L-vector (byNODES)"""
    n, E, NN = rve["n"], rve["E"], rve["NN"]
    conn = rve["conn"].reshape(E, n)
    out = np.zeros(3 * NN)
    for c in range(3):
        np.add.at(out, conn + NN * c, np.asarray(Ev).reshape(E, 3, n)[:, c, :])
    return out


def velocity_field(rve, scale=1.0, seed=7):
    """Nodal velocity of a perturbed uniaxial tension: v = L0 x + noise (SURVEY 8(d) kernel micro-benchmark shape)."""
    rng = np.random.default_rng(seed)
    NN = rve["NN"]
    X = rve["X"].reshape(3, NN)
    L0 = np.diag([-0.45e-3, -0.45e-3, 1.0e-3]) + 1e-4 * np.array([[0, 0.3, -0.2], [-0.3, 0, 0.1], [0.2, -0.1, 0]])
    v = (L0 @ X) * scale
    v += 1.0e-4 * scale / rve["N"] * rng.uniform(-1, 1, v.shape)
    return v.ravel()


class Dev:
    """torch-backed device buffers (allocator only)."""

    def __init__(self):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("GPU parity tests need a HIP device")
        self.dev = torch.device("cuda:0")

    def up(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.dev)

    def zeros(self, n, dtype=None):
        return self.torch.zeros(int(n), dtype=dtype or self.torch.float64, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize()


def ptr(t):
    return C.c_void_p(t.data_ptr())
