"""Reference side of the element-field tests (tests/test_gpu_element_fields.py; tests/test_element_field_inputs_host.py asserts on it alone):
the column table of exa_element_fields in numpy, the order-p hexahedron shape values built from numpy's Legendre polynomials and the
undistorted oracle mesh (none of the library's tables), the tetrahedron inputs on tet_mesh_util's independent tables, and the seeded point
data.  Everything runs in float64 or, for the precision check of the host module, in np.longdouble."""
import ctypes as C
import os

import numpy as np

import hipref
import tet_mesh_util as T

NF = 37
AVERAGED = slice(4, NF)         # every column that is a det J-weighted average of point data, or a function of such averages
CENTROID = slice(1, 4)
TET_MESH = dict(N=3, perturb=0.3, shuffle=True, seed=5)      # E = 162: three blocks, the last with 34 elements


RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "element_field_checks.txt")


class Check:
    """the measured lines of one test: printed at once (a failing assertion must not swallow them) and, by record(), kept in
    profiles/element_field_checks.txt under profiles/high_order_checks.txt's convention: with EXA_WRITE_RECORDS=1 the lines replace the
    block '[key]' of the record file"""

    def __init__(self, key):
        self.key, self.lines = key, []

    def say(self, text):
        print(text)
        self.lines.append(text)

    def record(self):
        if os.environ.get("EXA_WRITE_RECORDS") != "1":
            return
        blocks, cur = {}, None
        if os.path.exists(RECORD):
            for ln in open(RECORD).read().splitlines():
                if ln.startswith("[") and ln.endswith("]"):
                    cur = ln[1:-1]; blocks[cur] = []
                elif cur is not None:
                    blocks[cur].append(ln)
        blocks[self.key] = list(self.lines)
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        with open(RECORD, "w") as f:
            for k in sorted(blocks):
                f.write("[%s]\n%s\n" % (k, "\n".join(blocks[k])))


def _det3(Jm):
    """det of (..., 3, 3): numpy's LU in float64 (what the reference has always used), the cofactor expansion in extended precision"""
    if Jm.dtype == np.float64:
        return np.linalg.det(Jm)
    return (Jm[..., 0, 0] * (Jm[..., 1, 1] * Jm[..., 2, 2] - Jm[..., 1, 2] * Jm[..., 2, 1])
            - Jm[..., 0, 1] * (Jm[..., 1, 0] * Jm[..., 2, 2] - Jm[..., 1, 2] * Jm[..., 2, 0])
            + Jm[..., 0, 2] * (Jm[..., 1, 0] * Jm[..., 2, 1] - Jm[..., 1, 1] * Jm[..., 2, 0]))


def point_weights(J, W):
    """W_q det J_q, (E, Q); J (E,Q,9) column-major dx_i/dxi_j"""
    Jm = J.reshape(J.shape[0], J.shape[1], 3, 3).transpose(0, 1, 3, 2)    # [.., i, j]
    return W[None, :] * _det3(Jm)


def element_fields_numpy(J, S, SV, W, xq, w=None):
    """J (E,Q,9) column-major dx_i/dxi_j, S (E,Q,6), SV (E,Q,28), W (Q), xq (E,Q,3) -> (E,37); w: the point weights, if not W det J"""
    if w is None:
        w = point_weights(J, W)
    vol = w.sum(1)
    avg = lambda f: np.einsum("eq,eqk->ek", w, f) / vol[:, None]      # noqa: E731
    s = avg(S)
    sv = avg(SV)
    out = np.zeros((J.shape[0], NF), dtype=w.dtype)
    out[:, 0] = vol
    out[:, 1:4] = avg(xq)
    out[:, 4:10] = s
    out[:, 10] = np.sqrt(0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2 + 6 * (s[:, 3:6] ** 2).sum(1)))
    out[:, 11] = s[:, :3].sum(1) / 3
    out[:, 12] = sv[:, 0]
    out[:, 13] = sv[:, 1]
    out[:, 14] = sv[:, 13]
    out[:, 15:27] = sv[:, 14:26]
    qt = sv[:, 9:13]
    out[:, 27:31] = qt / np.sqrt((qt * qt).sum(1))[:, None]
    e = sv[:, 4:9]
    r2, r6 = np.sqrt(w.dtype.type(2)), np.sqrt(w.dtype.type(6))
    t1, t2, v = e[:, 0] / r2, e[:, 1] / r6, np.log(sv[:, 26])
    out[:, 31:37] = np.stack([t1 - t2 + v, -t1 - t2 + v, np.sqrt(w.dtype.type(2) / 3) * e[:, 1] + v, e[:, 4] / r2, e[:, 3] / r2, e[:, 2] / r2], 1)
    return out


# the bound of tests/test_gpu_element_fields.py per column: 1e-13 of the column's scale, 1e-12 for the elastic-strain columns
BASE_BOUND = np.where(np.arange(NF) >= 31, 1e-12, 1e-13)


def gpu_bounds(ref, ref_extended):
    """The GPU bound of a case, per column: BASE_BOUND where the float64 reference is within a tenth of it of the same reference in extended
    precision, ten times that distance where it is not (the reference's own round-off must not decide the comparison)"""
    prec = column_errors(ref, ref_extended)
    return np.where(prec <= BASE_BOUND / 10, BASE_BOUND, 10 * prec), prec


def column_errors(got, ref):
    """largest |got - ref| of every column over the largest |ref| of the column"""
    ref = np.asarray(ref)
    scale = np.maximum(np.abs(ref).max(axis=0), 1e-300)
    return np.asarray(np.abs(np.asarray(got) - ref).max(axis=0) / scale, dtype=np.float64)


# ---- one-dimensional tables from the Legendre polynomials ---------------------------------------------------------------------------------
def _legendre(n, x):
    """P_n, P_n' and P_n'' at x (|x| < 1 for the derivatives) by the three-term recurrence, in the type of x"""
    p0, p1 = np.ones_like(x), x
    for k in range(1, n):
        p0, p1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
    if n == 0:
        p0, p1 = np.zeros_like(x), np.ones_like(x)
    d1 = n * (p0 - x * p1) / (1 - x * x)
    d2 = (2 * x * d1 - n * (n + 1) * p1) / (1 - x * x)
    return p1, d1, d2


def gauss_points(np1, dtype=np.float64):
    """the np1 Gauss-Legendre points and weights on [0, 1]: numpy's leggauss, polished by two Newton steps in `dtype`"""
    x, w = np.polynomial.legendre.leggauss(np1)
    x = x.astype(dtype)
    for _ in range(2):
        P, d1, _ = _legendre(np1, x)
        x = x - P / d1
    _, d1, _ = _legendre(np1, x)
    w = 2 / ((1 - x * x) * d1 * d1)
    return (x + 1) / 2, w / 2


def lobatto_nodes(p, dtype=np.float64):
    """the p + 1 Gauss-Lobatto nodes on [0, 1]: the roots of P_p' (numpy's, polished by two Newton steps in `dtype`) and the end points"""
    r = np.sort(np.real(np.polynomial.legendre.Legendre.basis(p).deriv().roots())).astype(dtype) if p > 1 else np.zeros(0, dtype)
    for _ in range(2 if p > 1 else 0):
        _, d1, d2 = _legendre(p, r)
        r = r - d1 / d2
    x = np.concatenate([np.array([-1], dtype), r, np.array([1], dtype)])
    return (x + 1) / 2


def equispaced_nodes(p, dtype=np.float64):
    return np.arange(p + 1, dtype=dtype) / p


def lagrange(nodes, x):
    """V[i, k] = l_i(x_k) and D[i, k] = l_i'(x_k) of the Lagrange basis on `nodes`"""
    m = len(nodes)
    V = np.ones((m, len(x)), dtype=x.dtype); D = np.zeros((m, len(x)), dtype=x.dtype)
    for i in range(m):
        for a in range(m):
            if a != i:
                V[i] *= (x - nodes[a]) / (nodes[i] - nodes[a])
        for a in range(m):
            if a == i:
                continue
            t = np.ones(len(x), dtype=x.dtype) / (nodes[i] - nodes[a])
            for b in range(m):
                if b != i and b != a:
                    t *= (x - nodes[b]) / (nodes[i] - nodes[b])
            D[i] += t
    return V, D


# ---- hexahedra ----------------------------------------------------------------------------------------------------------------------------
def node_lattice(orc, N, p):
    """(ijk (E, n, 3), dist): the index of the nearest Gauss-Lobatto node per axis of every node of every element of the undistorted
    oracle mesh, and the largest distance from it in reference units"""
    rve0 = hipref.make_rve(orc, N, p=p)
    E, n, NN = rve0["E"], rve0["n"], rve0["NN"]
    X = rve0["X"].reshape(3, NN)
    xe = X[:, rve0["conn"].reshape(E, n)]                           # (3, E, n)
    lo = xe.min(axis=2, keepdims=True)
    xi = (xe - lo) * N                                              # reference coordinates in [0, 1]
    d = np.abs(xi[..., None] - lobatto_nodes(p)[None, None, None, :])
    return d.argmin(-1).transpose(1, 2, 0), float(d.min(-1).max())


def hex_tables(orc, N, p, dtype=np.float64, nodes=None):
    """N[a, q], G[q, j, a] = dN_a/dxi_j and W[q] of the order-p hexahedron in the oracle's node numbering; point q = qx + np (qy + np qz)"""
    ijk, _ = node_lattice(orc, N, p)
    ijk = ijk[0]                                                    # the same in every element (asserted by the host module)
    np1 = p + 1
    xg, wg = gauss_points(np1, dtype)
    V, D = lagrange(lobatto_nodes(p, dtype) if nodes is None else nodes, xg)
    q = np.arange(np1 ** 3)
    qi, qj, qk = q % np1, (q // np1) % np1, q // (np1 * np1)
    i, j, k = ijk[:, 0, None], ijk[:, 1, None], ijk[:, 2, None]
    Nv = V[i, qi] * V[j, qj] * V[k, qk]                             # (n, Q)
    G = np.stack([D[i, qi] * V[j, qj] * V[k, qk], V[i, qi] * D[j, qj] * V[k, qk], V[i, qi] * V[j, qj] * D[k, qk]], 0).transpose(2, 0, 1)
    return Nv, G, wg[qi] * wg[qj] * wg[qk]


def transpose_points(np1):
    """the point with the x and z indices exchanged, for every point"""
    q = np.arange(np1 ** 3)
    return q // (np1 * np1) + np1 * ((q // np1) % np1) + np1 * np1 * (q % np1)


def point_data(E, Q, seed, dtype=np.float64):
    """S = 100 randn; state = randn, slot 26 in [0.95, 1.05], slots 9..12 a unit quaternion per element + 0.1 randn per point, renormalised
    (the norm of the averaged orientation stays well away from zero at Q = 343)"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((E, Q, 6)) * 100.0
    SV = rng.standard_normal((E, Q, 28))
    SV[:, :, 26] = rng.uniform(0.95, 1.05, (E, Q))
    qe = rng.standard_normal((E, 4))
    qe /= np.linalg.norm(qe, axis=1, keepdims=True)
    qp = qe[:, None, :] + 0.1 * rng.standard_normal((E, Q, 4))
    SV[:, :, 9:13] = qp / np.linalg.norm(qp, axis=2, keepdims=True)
    return S.astype(dtype), SV.astype(dtype)


_cache = {}


def hex_case(orc, p, N, dtype=np.float64):
    """inputs and reference rows of the warped N^3 mesh of order p (hipref.ho_inputs, the oracle's Jacobians): dict, cached, read-only"""
    key = ("hex", p, N, np.dtype(dtype).name)
    if key not in _cache:
        inp = hipref.ho_inputs(orc, p, N)
        E, Q, n = inp["E"], inp["Q"], inp["n"]
        Nv, _, W = hex_tables(orc, N, p, dtype)
        xe = inp["xe"].reshape(E, 3, n).astype(dtype)
        J = inp["J"].reshape(E, Q, 9).astype(dtype)
        S, SV = point_data(E, Q, 7000 + 10 * p + N, dtype)
        xq = np.einsum("ean,nq->eqa", xe, Nv)
        c = dict(p=p, N=N, E=E, Q=Q, n=n, NN=inp["NN"], conn=inp["rve"]["conn"], xe=xe, J=J, S=S, SV=SV, W=W, Nv=Nv, xq=xq,
                 ref=element_fields_numpy(J, S, SV, W, xq))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = c
    return _cache[key]


# ---- tetrahedra ---------------------------------------------------------------------------------------------------------------------------
def tet_mesh_arrays(L, path, order):
    """E, NN, n, conn (E, n) flat and X (3, NN) flat of a file mesh as the library's reader builds it (one rank; host code only)"""
    info = (C.c_int64 * 8)(); err = C.create_string_buffer(512)
    assert L.exa_mesh_partition_query_order(path.encode(), 0, 1, order, info, None, None, None, None, None, None, None, err, 512) == 0, err.value
    E, NN, n = info[0], info[1], info[7]
    conn = np.zeros(n * E, np.int32); X = np.zeros(3 * NN)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.exa_mesh_partition_query_order(path.encode(), 0, 1, order, info, vp(conn), vp(X), None, None, None, None, None, err, 512) == 0
    return E, NN, n, conn, X


def tet_case(L, tmp_dir, p, warped=False, dtype=np.float64):
    """inputs and reference rows of the perturbed, shuffled Kuhn mesh TET_MESH at order p, straight-sided or with every node moved by
    hipref.warp_nodes.  Tables: tet_mesh_util.ref_tables_numpy.  The centroid columns of `ref` are the volume-weighted centroid of the
    interpolated geometry; `vertex_mean` is what DESIGN 4.9 states the kernel writes.  dict, cached, read-only"""
    key = ("tet", p, warped, np.dtype(dtype).name)
    if key not in _cache:
        path = T.write_mfem(os.path.join(str(tmp_dir), "fieldref_k3.mesh"), T.kuhn_cube(**TET_MESH))
        E, NN, n, conn, X = tet_mesh_arrays(L, path, p)
        if warped:
            X = hipref.warp_nodes(X)
        Gt, Wt, Nt = T.ref_tables_numpy(p)
        Q = Wt.size
        xe = hipref.l_to_e({"E": E, "n": n, "NN": NN, "conn": conn}, X).reshape(E, 3, n).astype(dtype)
        J = np.ascontiguousarray(np.einsum("eia,qja->eqji", xe, Gt.reshape(Q, 3, n).astype(dtype))).reshape(E, Q, 9)
        S, SV = point_data(E, Q, 9000 + 10 * p + int(warped), dtype)
        W = Wt.astype(dtype)
        xq = np.einsum("ean,qn->eqa", xe, Nt.reshape(Q, n).astype(dtype))
        c = dict(p=p, E=E, Q=Q, n=n, NN=NN, conn=conn, X=X, xe=xe, J=J, S=S, SV=SV, W=W, xq=xq, ref=element_fields_numpy(J, S, SV, W, xq),
                 vertex_mean=xe[:, :, :4].mean(axis=2))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = c
    return _cache[key]
