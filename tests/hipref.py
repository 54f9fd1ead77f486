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


# ---- load paths off the tension history of velocity_field (tests/offpath.py runs them; tests/test_offpath_inputs_host.py asserts on the oracle
# alone that each reaches the branch of the point update it was built for) ------------------------------------------------------------------
PATH_T = np.diag([-0.45e-3, -0.45e-3, 1.0e-3])                     # the tension rate every path starts with
PATH_START_DTS = (0.005, 0.195, 0.4, 0.4)                           # ... for these steps, so that a path branches off in plastic flow
PATH_SPIN_AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
PATH_NAMES = ("reversal", "shear", "volume", "rate", "hold", "rotation")
# The rate factors 10, 100, 1000, 100, 10, 1, 0.1, 0.1, 1 in an order in which every down-jump starts above the flow stress of the new rate.
# With one strain increment of 4e-4 per step the Kocks-Mecking stress is still climbing elastically at 100 x and 1000 x, so in the order
# 1000 -> 100 -> 10 it goes on rising through the two down-jumps (measured on the oracle: 3.25 -> 4.05 -> 4.73); the same steps reordered
# rise on every up-jump and fall on every down-jump, which is what tests/test_offpath_inputs_host.py asserts.
PATH_RATE_FACTORS = (10.0, 100.0, 1000.0, 1.0, 0.1, 0.1, 1.0, 10.0, 100.0)
# The pure spin that ends `rotation`: (angle, dt).  With D = 0 the solver scales its residual by 1 / max(|dev D|, 1 / (1e6 dt)), here 1e6 dt,
# and the rotation rows of the residual are a difference of two numbers of size |W|: their round-off, |W| 1e6 dt 1.1e-16 = angle x 1.1e-10, is
# at the Voce tolerance of 1e-10 when the angle is 0.3 rad (the oracle itself then fails at 37 of 1728 points, and at 2 at 0.1 rad).  0.02 rad
# is still the large-angle branch (th2 = 4e-4 >= 1e-4) and leaves a factor of 50.
PATH_PURE_SPIN = (0.02, 0.02)


def spin_matrix(angle_rate, axis=PATH_SPIN_AXIS):
    """skew W with axial vector angle_rate * axis: W x = w cross x"""
    a = angle_rate * np.asarray(axis, dtype=np.float64)
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def load_path(name):
    """the steps (D, W, dt) of a named load path: D symmetric, W skew, 3 x 3, rates per second"""
    Z = np.zeros((3, 3))
    T = PATH_T
    start = [(T, Z, dt) for dt in PATH_START_DTS]
    if name == "reversal":       # elastic unloading, the zero crossing of every resolved shear stress, reverse yield
        return start + [(-T, Z, dt) for dt in (0.05, 0.2, 0.25, 0.5, 0.5, 1.0)]
    if name == "shear":          # simple shear from the first step: D and W of equal size, other slip systems than tension's
        Ls = np.zeros((3, 3)); Ls[0, 1] = 1.0e-3
        return [(0.5 * (Ls + Ls.T), 0.5 * (Ls - Ls.T), dt) for dt in (0.005, 0.2, 0.5, 1.0, 2.0, 5.0)]
    if name == "volume":         # relative volume up to ~1.009, then down to 0.970 ... 0.978 (the last step at dt = 1.4, not 1.0: the jitter has a trace,
        # and at 1.0 a third of the points ended between 0.980 and 0.983, above the 0.98 tests/test_offpath_inputs_host.py asserts for every point)
        return start + [(T + k * np.eye(3), Z, dt) for k, dt in ((2.0e-3, 0.5), (2.0e-3, 1.0), (-5.0e-3, 1.0), (-5.0e-3, 1.4))]
    if name == "rate":           # jumps of the strain rate over four decades at a constant strain increment per step
        return start + [(f * T, Z, 0.4 / f) for f in PATH_RATE_FACTORS]
    if name == "hold":           # exactly zero velocity, then rates below and just above the solver's "no deformation" threshold.  The last step
        # (1e-3, not part of the first statement of this path) is the one whose |dev D| = 1.2e-6 lies between 1e-8 gam_w and 1e-6 / dt for
        # every model: at 1e-7 |dev D| = 1.2e-10 is still below 1e-8 gam_w (gam_w = 1 /s Voce, ~30 /s Kocks-Mecking)
        return start + [(f * T, Z, dt) for f, dt in ((0.0, 1.0), (1.0e-12, 1.0), (1.0e-7, 1.0), (1.0e-5, 0.5), (1.0e-3, 0.5))]
    if name == "rotation":       # lattice-rotation increments of 0.02 ... 0.5 rad in one step under tension, then a pure spin (D = 0)
        # (the 0.5 rad step at dt = 0.2, not 0.4: at 0.4 one point of the FCC Voce models needs 106 evaluations on the oracle, and the oracle itself
        #  runs into its limit of 200 there when its Jacobians are perturbed in the last bit - tests/test_offpath_inputs_host.py asserts the margin)
        steps = [(T, spin_matrix(ang / dt), dt) for ang, dt in ((0.02, 0.2), (0.05, 0.2), (0.2, 0.2), (0.5, 0.2))]
        return start + steps + [(Z, spin_matrix(PATH_PURE_SPIN[0] / PATH_PURE_SPIN[1]), PATH_PURE_SPIN[1])]
    raise KeyError(name)


def path_step(rve, x0, D, W, dt, rng):
    """One step of a load path on byNODES coordinates x0: end-of-step coordinates x1 = x0 + dt D x0 and nodal velocity v = (D + W) x1 + jitter.
    ModelSetup takes the Jacobians of x1 and the velocity independently, so the point update sees the velocity gradient D + W up to the
    jitter, tr L = tr D, and a spin of any size costs no spurious stretch.  The jitter is sized by |D| alone (a tenth of it across an element,
    the proportion of velocity_field; by 1e-6 /s where D = 0 and W != 0; none where both vanish: a hold at exactly zero velocity)."""
    NN = rve["NN"]
    X0 = np.asarray(x0).reshape(3, NN)
    X1 = X0 + dt * (D @ X0)
    v = (D + W) @ X1
    dn = np.linalg.norm(D)
    size = 0.1 * dn if dn > 0 else (1.0e-6 if np.any(W != 0) else 0.0)
    if size > 0:
        v = v + size / (rve["N"] * rve["p"]) * rng.uniform(-1, 1, v.shape)
    return X1.ravel(), v.ravel()


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
