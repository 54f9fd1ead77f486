"""Intragranular misorientation and lattice curvature on the GPU: the three launches of exa_curvature_* and
Driver.lattice_curvature() against a NumPy restatement of the definitions (float64, plain loops over elements and vertex nodes) on hand-built
rows and on stepped synthetic RVEs: a linear rotation field, a grain boundary, tetrahedra at p = 1 and 2, several loopback ranks, a periodic
cell, and the files of an options-file run.

Tolerance GPU vs NumPy: per column |d| <= 1e-10 x the largest magnitude of the column.  The two quadrature layouts share every code path of
these entry points (only the [E][EXA_NFIELDS] rows are read), so the ABI tests run on one."""
import ctypes as C
import os
import threading
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import hipref
import tet_mesh_util as T
from hipref import ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
DTS = np.array([0.005, 0.1, 0.2])
# the driver runs are pulled to about 1 % strain (6 steps at ten times the default rate), so that the misorientations reach the 1e-3 rad the
# tolerances are stated for: omega is formed from differences of unit-quaternion components, whose last bit (1.1e-16) puts an absolute floor of a
# few 1e-16 rad under every rotation vector - 1e-11 of a 4e-5 rad field (what 0.03 % strain gives) would be below one bit of the input
DTS_RUN = np.array([0.005, 0.05, 0.1, 0.2, 0.3, 0.4])
VZ_RUN = 1.0e-2
# The partitions add up the PCG dot products in different orders.  With the default tolerances (Newton 5e-5, Krylov 1e-7 relative) the last Newton
# correction carries a linear-solve error of about 5e-5 x 1e-7 = 5e-12 of the solution, which differs between rank counts: the converged STATES
# then agree to a few 1e-12 only, whatever the analysis does.  With Newton at 1e-12 and Krylov at 1e-8 the last correction is below 1e-8 of the
# solution and its error below 1e-16, so the states agree to round-off and the comparison tests the analysis.  (The Krylov tolerance is not
# tighter: the single-reduction PCG of several ranks stagnates before 1e-10 on 3^3-element partitions and runs to its iteration limit.)
TIGHT = dict(newton=(50, 1e-12, 1e-14), krylov=(500, 1e-8, 1e-30))
COLS = {"RotationVector": (0, 3), "GROD": (3, 1), "KAM": (4, 1), "LatticeCurvature": (5, 9), "NyeNorm": (14, 1), "GNDDensity": (15, 1)}
# corner signs of the hexahedron's vertices in connectivity order, on the reference cube [-1, 1]^3
HEX_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], float)
TET_DN = np.array([[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)


def _props():
    return np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _axis_quat(n, theta):
    theta = np.asarray(theta, float)
    return np.concatenate([np.cos(0.5 * theta)[..., None], np.sin(0.5 * theta)[..., None] * np.asarray(n, float)], -1)


def _qmul(a, b):
    """Hamilton product"""
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def grain_means_numpy(V, q, grain, qref):
    """unit grain means as DESIGN 4.7 forms them: normalised sum of V s q with s = sign(q . q_ref); {grain id: qbar}"""
    out = {}
    for g in np.unique(grain):
        acc = np.zeros(4)
        for e in np.flatnonzero(grain == g):
            acc += V[e] * (1.0 if q[e] @ qref[g] >= 0.0 else -1.0) * q[e]
        out[int(g)] = acc / np.linalg.norm(acc)
    return out


def curvature_numpy(V, q, grain, qbar, verts, xv, burgers):
    """The definitions of DESIGN 4.14 in plain loops.  V (E,), q (E, 4), grain (E,), qbar {grain id: unit mean}, verts (E, nv) a key per vertex
    node (equal keys = one node, all copies included), xv (E, nv, 3) the element's own vertex coordinates.  Returns rows (E, 16), summary (7,)."""
    E, nv = verts.shape
    om = np.zeros((E, 3))
    for e in range(E):
        qb = qbar[int(grain[e])]
        d = _qmul(q[e], np.array([qb[0], -qb[1], -qb[2], -qb[3]]))
        if d[0] < 0.0:
            d = -d
        nrm = np.linalg.norm(d[1:])
        if nrm > 0.0:
            om[e] = 2.0 * np.arctan2(nrm, d[0]) * d[1:] / nrm
    svw, sv, ids = {}, {}, {}
    for e in range(E):
        for a in range(nv):
            k = int(verts[e, a])
            svw[k] = svw.get(k, np.zeros(3)) + V[e] * om[e]
            sv[k] = sv.get(k, 0.0) + V[e]
            ids.setdefault(k, set()).add(int(grain[e]))
    rows = np.zeros((E, 16))
    for e in range(E):
        if nv == 8:
            dN = HEX_SIGNS / 8.0            # d N_a / d xi at the centre of [-1, 1]^3
        else:
            dN = TET_DN
        J = xv[e].T @ dN                    # dx_i / dxi_k
        dNdx = dN @ np.linalg.inv(J)
        kap = np.zeros((3, 3)); kam = []
        for a in range(nv):
            k = int(verts[e, a])
            if len(ids[k]) > 1:
                w = om[e]
            else:
                w = svw[k] / sv[k]
                kam.append(np.linalg.norm(w - om[e]))
            kap += np.outer(w, dNdx[a])
        alpha = kap.T - np.eye(3) * np.trace(kap)
        rows[e, 0:3] = om[e]
        rows[e, 3] = np.degrees(np.linalg.norm(om[e]))
        rows[e, 4] = np.degrees(np.mean(kam)) if kam else 0.0
        rows[e, 5:14] = kap.ravel()
        rows[e, 14] = np.linalg.norm(alpha)
        rows[e, 15] = rows[e, 14] / burgers
    summ = np.array([V.sum(), V @ rows[:, 3], V @ rows[:, 4], V @ rows[:, 15], rows[:, 3].max(), rows[:, 4].max(), rows[:, 15].max()])
    return rows, summ


def _close(got, ref, rel=1e-10, what=""):
    for c in range(ref.shape[1]):
        scale = np.abs(ref[:, c]).max()
        err = np.abs(got[:, c] - ref[:, c]).max()
        print(f"{what} column {c}: max |d| = {err:.3e}, scale {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
        assert err <= rel * scale, (what, c, err, scale)


def _close_summary(got, ref, rel=1e-10, what=""):
    err = np.abs(got - ref)
    print(f"{what} summary: {err / np.maximum(np.abs(ref), 1e-300)}")
    assert np.all(err <= rel * np.abs(ref)), (what, got, ref)


def hex_mesh(N):
    """N^3 unit-cube hexahedra, x fastest: conn (E, 8), X (NN, 3)"""
    n1 = N + 1
    k, j, i = np.meshgrid(np.arange(n1), np.arange(n1), np.arange(n1), indexing="ij")
    X = np.stack([i.ravel(), j.ravel(), k.ravel()], -1).astype(float) / N
    ez, ey, ex = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    off = ((HEX_SIGNS + 1) / 2).astype(int)
    conn = np.stack([(ex.ravel() + o[0]) + n1 * ((ey.ravel() + o[1]) + n1 * (ez.ravel() + o[2])) for o in off], -1)
    return conn.astype(np.int32), X


def _rows(V, cen, q):
    r = np.zeros((len(V), 37))
    r[:, 0] = V; r[:, 1:4] = cen; r[:, 27:31] = q
    return r


def run_abi(L, ctx, rows, grain, G, qbar_arr, conn, NN, X, burgers):
    """the three entry points on a context with this connectivity (conn (E, n), X (NN, 3)): rows (E, 16), summary (7,), nodal planes"""
    dev = hipref.Dev()
    E, n = conn.shape
    work, planes = L.curvature_sizes(E)
    assert planes % 3 == 0 and work > 0
    d_conn = dev.up(conn.ravel().astype(np.int32))
    ctx.check(L.exa_set_connectivity(ctx.h, ptr(d_conn), NN))
    xe = np.ascontiguousarray(X[conn].transpose(0, 2, 1)).ravel()          # (E, 3, n)
    d_rows, d_g, d_qb, d_xe = dev.up(rows.ravel()), dev.up(grain.astype(np.int32)), dev.up(qbar_arr.ravel()), dev.up(xe)
    d_work, d_nodal, d_out, d_sum = dev.zeros(work), dev.zeros(planes * NN), dev.zeros(16 * E), dev.zeros(7)
    ctx.check(L.exa_curvature_nodal(ctx.h, ptr(d_rows), ptr(d_g), G, ptr(d_qb), ptr(d_work), ptr(d_nodal), None))
    ctx.check(L.exa_curvature_elements(ctx.h, ptr(d_rows), ptr(d_g), G, ptr(d_qb), ptr(d_work), ptr(d_nodal), ptr(d_xe), burgers, ptr(d_out), None))
    ctx.check(L.exa_curvature_summary(ctx.h, ptr(d_rows), ptr(d_out), ptr(d_sum), None))
    dev.sync()
    return d_out.cpu().numpy().reshape(E, 16), d_sum.cpu().numpy(), d_nodal.cpu().numpy().reshape(planes, NN)


def _qbar_array(qbar, G):
    a = np.tile([1.0, 0.0, 0.0, 0.0], (G, 1))
    for g, v in qbar.items():
        a[g - 1] = v
    return a


AXIS = _unit(np.array([0.48, -0.6, 0.64]))
GRAD = np.array([0.06, 0.07, 0.045])          # rad per length: 0.8 x 0.175 rad = 8 degrees across the centroids of the unit cube


def linear_case(N):
    conn, X = hex_mesh(N)
    cen = X[conn].mean(1)
    V = np.full(len(conn), 1.0 / N ** 3)
    q = _axis_quat(AXIS, cen @ GRAD)
    return conn, X, cen, V, q


def test_linear_field_abi():
    """5^3 hexahedra (one full wave and a partial one), one grain, q_e = rotation by a . x_centroid about a fixed axis n: every column and the
    summary against NumPy, and kappa = n (x) a on the 27 elements without a surface node (exact in exact arithmetic: the rotations commute and
    the nodal mean of equal-volume centroids is the node)"""
    import exaconstit_amd.lib as L
    N = 5
    conn, X, cen, V, q = linear_case(N)
    E, NN = len(conn), len(X)
    grain = np.full(E, 3, np.int32); G = 4
    qbar = grain_means_numpy(V, q, grain, {3: _axis_quat(AXIS, 0.5 * GRAD.sum())})
    ref, rsum = curvature_numpy(V, q, grain, qbar, conn, X[conn], 2.5e-7)
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, 1, E)
    got, gsum, nodal = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 2.5e-7)
    again, asum, _ = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 2.5e-7)
    ctx.close()
    assert np.array_equal(got, again) and np.array_equal(gsum, asum)          # no atomics: the same bits on every call
    _close(got, ref, what="linear")
    _close_summary(gsum, rsum, what="linear")
    assert np.array_equal(nodal[4], np.bincount(conn.ravel(), minlength=NN))  # holder counts
    ijk = np.rint(cen * N - 0.5).astype(int)
    inner = np.all((ijk >= 1) & (ijk <= N - 2), axis=1)
    assert inner.sum() == 27
    exact = np.outer(AXIS, GRAD).ravel()
    for name, r in (("numpy", ref), ("gpu", got)):
        err = np.abs(r[inner, 5:14] - exact).max()
        print(f"{name}: max |kappa - n (x) a| = {err:.3e} of {np.abs(exact).max():.3e}")
        assert err <= 1e-9 * np.abs(exact).max(), name
    assert np.abs(got[:, 3].max() - np.degrees(0.4 * GRAD.sum())) < 1e-9       # GROD: half the spread, at the corner elements


def test_grain_boundary_abi():
    """4^3, two grains split at the plane x = 1/2: constant orientations 20 degrees apart give zero everywhere (the difference at the boundary is
    one-sided); a different linear field inside each grain is compared against NumPy (a missing mixed-node rule would show as degrees per element)"""
    import exaconstit_amd.lib as L
    N = 4
    conn, X = hex_mesh(N)
    cen = X[conn].mean(1)
    E, NN = len(conn), len(X)
    V = np.full(E, 1.0 / N ** 3)
    grain = np.where(cen[:, 0] < 0.5, 70000, 7).astype(np.int32); G = 70000      # the ids differ in both 16-bit halves' sums
    n2 = _unit(np.array([0.3, 0.9, -0.2]))
    q0 = {70000: _axis_quat(AXIS, 0.3), 7: _qmul(_axis_quat(n2, np.radians(20.0)), _axis_quat(AXIS, 0.3))}
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, 1, E)
    q = np.array([q0[int(g)] for g in grain])
    qbar = grain_means_numpy(V, q, grain, q0)
    got, gsum, nodal = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 1.0)
    for name in ("RotationVector", "KAM", "LatticeCurvature", "NyeNorm"):
        c0, n = COLS[name]
        print(name, np.abs(got[:, c0:c0 + n]).max())
        assert np.abs(got[:, c0:c0 + n]).max() <= 1e-13, name
    c, sl, sl2, sh, sh2 = nodal[4:9]
    mixed = (c * sl2 != sl * sl) | (c * sh2 != sh * sh)
    assert np.array_equal(mixed, np.abs(X[:, 0] - 0.5) < 1e-12)                  # exactly the nodes of the boundary plane
    # a different linear field inside each grain
    th = np.where(grain == 7, cen @ GRAD, cen @ np.array([-0.05, 0.02, 0.08]))
    q = np.array([_qmul(_axis_quat(AXIS if g == 7 else n2, t), q0[int(g)]) for g, t in zip(grain, th)])
    qbar = grain_means_numpy(V, q, grain, q0)
    ref, rsum = curvature_numpy(V, q, grain, qbar, conn, X[conn], 1.0)
    got, gsum, _ = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 1.0)
    ctx.close()
    _close(got, ref, what="boundary")
    _close_summary(gsum, rsum, what="boundary")
    assert ref[:, 3].max() < 5.0 and ref[:, 4].max() < 1.0                       # degrees: nothing of the 20 degree jump leaks in


def _hexahedra_abi(oracle, p):
    """2^3 hexahedra at order p: the recovery runs over the first 8 entries of the connectivity, the vertices in the order of HEX_SIGNS under
    the Gauss-Lobatto numbering too, and leaves the edge, face and interior nodes alone"""
    import exaconstit_amd.lib as L
    rve = hipref.make_rve(oracle, 2, p=p)
    E, n, NN = rve["E"], rve["n"], rve["NN"]
    assert (E, n, NN) == (8, (p + 1) ** 3, (2 * p + 1) ** 3)
    conn = rve["conn"].reshape(E, n); X = rve["X"].reshape(3, NN).T
    xv = X[conn[:, :8]]
    assert np.allclose(xv - xv[:, :1], (HEX_SIGNS + 1) / 4, rtol=0, atol=1e-14)          # corners of the element's cell, in vertex order
    cen = xv.mean(1)
    V = np.full(E, 1.0 / E)
    grain = np.where(cen[:, 0] < 0.5, 2, 5).astype(np.int32); G = 5
    n2 = _unit(np.array([0.3, 0.9, -0.2]))
    q0 = {2: _axis_quat(AXIS, 0.3), 5: _axis_quat(n2, 1.1)}
    th = np.where(grain == 2, cen @ GRAD, cen @ np.array([-0.05, 0.02, 0.08]))
    q = np.array([_qmul(_axis_quat(AXIS if g == 2 else n2, t), q0[int(g)]) for g, t in zip(grain, th)])
    qbar = grain_means_numpy(V, q, grain, q0)
    ref, rsum = curvature_numpy(V, q, grain, qbar, conn[:, :8], xv, 1.0)
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, p, E)
    got, gsum, nodal = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 1.0)
    ctx.close()
    _close(got, ref, what=f"hex p={p}")
    _close_summary(gsum, rsum, what=f"hex p={p}")
    vertex = np.zeros(NN, bool); vertex[conn[:, :8].ravel()] = True
    assert vertex.sum() == 27 and np.all(nodal[4][~vertex] == 0) and np.all(nodal[4][vertex] > 0)


def test_hexahedra_p2_abi(oracle):
    """27 nodes per element, 98 of the 125 nodes are no vertices"""
    _hexahedra_abi(oracle, 2)


def test_hexahedra_p3_abi(oracle):
    """64 nodes per element (k_curv_nodal with n = 64, nvert = 8), 316 of the 343 nodes are no vertices"""
    _hexahedra_abi(oracle, 3)


@pytest.mark.parametrize("p", [1, 2])
def test_tetrahedra_abi(tmp_path, p):
    """the 3 x 3 x 3-cell Kuhn mesh (162 tetrahedra, perturbed and shuffled) on a p = 1 and a p = 2 context: two grains, linear fields"""
    import exaconstit_amd.lib as L
    from test_gpu_tetrahedra import _mesh_arrays
    path = T.write_mfem(str(tmp_path / "k3.mesh"), T.kuhn_cube(3, perturb=0.3, shuffle=True, seed=5))
    E, NN, n, conn, Xl = _mesh_arrays(L, path, p)
    assert E == 162 and n == (4 if p == 1 else 10)
    conn = conn.reshape(E, n); X = Xl.reshape(3, NN).T
    xv = X[conn[:, :4]]
    cen = xv.mean(1)
    a, b, c = xv[:, 1] - xv[:, 0], xv[:, 2] - xv[:, 0], xv[:, 3] - xv[:, 0]
    V = np.abs(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0
    grain = np.where(cen[:, 0] + 0.3 * cen[:, 1] < 0.6, 1, 2).astype(np.int32); G = 2
    n2 = _unit(np.array([0.3, 0.9, -0.2]))
    q0 = {1: _axis_quat(AXIS, 0.3), 2: _axis_quat(n2, 1.1)}
    th = np.where(grain == 1, cen @ GRAD, cen @ np.array([-0.05, 0.02, 0.08]))
    q = np.array([_qmul(_axis_quat(AXIS if g == 1 else n2, t), q0[int(g)]) for g, t in zip(grain, th)])
    qbar = grain_means_numpy(V, q, grain, q0)
    ref, rsum = curvature_numpy(V, q, grain, qbar, conn[:, :4], xv, 1.0)
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, p, E, geometry=L.EXA_GEOM_TET)
    got, gsum, nodal = run_abi(L, ctx, _rows(V, cen, q), grain, G, _qbar_array(qbar, G), conn, NN, X, 1.0)
    ctx.close()
    _close(got, ref, what=f"tet p={p}")
    _close_summary(gsum, rsum, what=f"tet p={p}")
    vertex = np.zeros(NN, bool); vertex[conn[:, :4].ravel()] = True
    assert np.all(nodal[4][~vertex] == 0) and np.all(nodal[4][vertex] > 0)       # the recovery runs over the vertex nodes only


# ---- driver ---------------------------------------------------------------------------------------------------------------------------------

def four_grains(N):
    """four grains; the boundary between grains 1 | 2 and 3 | 4 is the plane z = 1/2, where a box of N^3 elements is cut between 2 (and 8) ranks"""
    i = np.arange(N ** 3)
    x, y, z = i % N, (i // N) % N, i // (N * N)
    return np.where(z < N // 2, np.where(x + y < N, 1, 2), np.where(x < N // 3 + 1, 3, 4)).astype(np.int32)


def _grain_quats(G, seed=11):
    return _unit(np.random.default_rng(seed).standard_normal((G, 4)))


def driver_numpy(d, N, burgers, periodic=False):
    """NumPy reference of a one-rank synthetic N^3 driver from element_fields(), the grain means of grain_averages() and nodal_field("coords");
    nodes are identified by their grid index (wrapped when periodic)"""
    f = d.element_fields()
    ga = d.grain_averages()
    qbar = {int(g): ga["LatticeOrientation"][k] for k, g in enumerate(ga["grain_id"])}
    xc, xr = d.nodal_field("coords"), d.nodal_field("coords_ref")
    n1 = N + 1
    ijk = np.rint(xr * N).astype(int)
    local = {int(i + n1 * (j + n1 * k)): m for m, (i, j, k) in enumerate(ijk)}
    gid = f["GlobalElementId"]
    ex, ey, ez = gid % N, (gid // N) % N, gid // (N * N)
    off = ((HEX_SIGNS + 1) / 2).astype(int)
    E = len(gid)
    verts = np.zeros((E, 8), np.int64); xv = np.zeros((E, 8, 3))
    for e in range(E):
        for a, o in enumerate(off):
            i, j, k = ex[e] + o[0], ey[e] + o[1], ez[e] + o[2]
            xv[e, a] = xc[local[int(i + n1 * (j + n1 * k))]]
            if periodic:
                i, j, k = i % N, j % N, k % N
            verts[e, a] = i + n1 * (j + n1 * k)
    rows, summ = curvature_numpy(f["ElementVolume"][:, 0], f["LatticeOrientation"], f["attribute"], qbar, verts, xv, burgers)
    return rows, summ, f, ga


def _got_rows(c):
    return np.concatenate([c[k].reshape(len(c["GROD"]), -1) for k in COLS], axis=1)


def _summary_of(summ):
    """the driver's summary values from the 7 sums / maxima of the reference"""
    return np.array([summ[1] / summ[0], summ[4], summ[2] / summ[0], summ[5], summ[3] / summ[0], summ[6]])


def _summary_arr(c):
    import exaconstit_amd.lib as L
    return np.array([c["summary"][k] for k in L.CURVATURE_SUMMARY])


def test_driver_against_numpy():
    import exaconstit_amd.lib as L
    N = 6
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS_RUN, vz=VZ_RUN)
    d.set_grains(four_grains(N), _grain_quats(4))
    for ti in range(1, len(DTS_RUN) + 1):
        assert d.step(ti)
    b = 2.5e-7
    got = d.lattice_curvature(burgers=b)
    again = d.lattice_curvature(burgers=b)
    for k in got:
        assert got[k] == again[k] if k == "summary" else np.array_equal(got[k], again[k]), k
    ref, rsum, f, ga = driver_numpy(d, N, b)
    assert np.array_equal(got["GlobalElementId"], f["GlobalElementId"]) and np.array_equal(got["attribute"], f["attribute"])
    assert got["RotationVector"].shape == (N ** 3, 3) and got["LatticeCurvature"].shape == (N ** 3, 9) and got["GROD"].shape == (N ** 3,)
    _close(_got_rows(got), ref, what="driver")
    _close_summary(_summary_arr(got), _summary_of(rsum), what="driver")
    assert abs(got["summary"]["volume"] - rsum[0]) <= 1e-12 * rsum[0]
    assert np.abs(got["RotationVector"]).max() > 5e-4 and got["KAM"].max() > 0.0 and got["NyeNorm"].max() > 0.0   # the state has moved
    assert np.array_equal(got["GNDDensity"], d.lattice_curvature(burgers=1.0)["NyeNorm"] * (1.0 / b))
    # against the per-grain misorientation that exists already
    mean = (ga["volume"] * ga["MisorientationMean"]).sum() / ga["volume"].sum()
    print("GROD mean", got["summary"]["GROD_mean"], mean, "max", got["summary"]["GROD_max"], ga["MisorientationMax"].max())
    assert abs(got["summary"]["GROD_mean"] - mean) <= 1e-10 * mean
    assert abs(got["summary"]["GROD_max"] - ga["MisorientationMax"].max()) <= 1e-10 * ga["MisorientationMax"].max()
    with pytest.raises(RuntimeError, match="Burgers"):
        d.lattice_curvature(burgers=0.0)
    d.close()


def test_driver_one_grain_per_element_is_zero():
    import exaconstit_amd.lib as L
    N = 4
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS)
    for ti in (1, 2):
        assert d.step(ti)
    got = d.lattice_curvature()
    for k in COLS:
        assert np.abs(got[k]).max() <= 1e-13, (k, np.abs(got[k]).max())
    d.close()


def _run_ranks(L, N, nranks, burgers):
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    res, errors = [None] * nranks, []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS_RUN, vz=VZ_RUN, rank=r, nranks=nranks, uid=gid, **TIGHT)
            d.set_grains(four_grains(N), _grain_quats(4))
            for ti in range(1, len(DTS_RUN) + 1):
                assert d.step(ti)
            res[r] = d.lattice_curvature(burgers=burgers)
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    L.exa_loopback_group_destroy(gid)
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    return res


@pytest.fixture(scope="module")
def one_rank_6():
    import exaconstit_amd.lib as L
    return _run_ranks(L, 6, 1, 2.5e-7)[0]


@pytest.mark.parametrize("nranks", [2, 8])
def test_loopback_ranks_match_one(one_rank_6, nranks):
    """the 6^3 run on 2 and 8 loopback ranks: the boundary of grains 1 | 2 and 3 | 4 lies on the rank cut z = 1/2, so a node there is unmixed on
    each rank and mixed globally.  Measured largest |d| / column scale: 1.8e-13 on 2 ranks and 5e-12 to 8.5e-12 on 8 ranks (three
    runs; the 3^3-element partitions of 8 ranks end their Newton solves closest to the bound)"""
    import exaconstit_amd.lib as L
    one = one_rank_6
    many = _run_ranks(L, 6, nranks, 2.5e-7)
    gids = np.concatenate([r["GlobalElementId"] for r in many])
    assert np.array_equal(np.sort(gids), np.arange(216))
    sides = [set(r["attribute"].tolist()) for r in many]
    assert any(s <= {1, 2} for s in sides) and any(s <= {3, 4} for s in sides)    # the cut separates the grains
    a = _got_rows(one)[np.argsort(one["GlobalElementId"])]
    b = np.concatenate([_got_rows(r) for r in many])[np.argsort(gids)]
    _close(b, a, rel=1e-11, what=f"{nranks} ranks")
    for r in many:
        assert r["summary"] == many[0]["summary"]                                 # every rank sees the all-reduced values
    _close_summary(_summary_arr(many[0]), _summary_arr(one), rel=1e-12, what=f"{nranks} ranks")


def test_periodic_cell():
    """4^3 periodic cell; grain 2 wraps around the x faces (columns x = 0 and x = N - 1): the elements on the two sides of the wrap see each other's
    values, which the reference reproduces by identifying nodes through their wrapped grid index"""
    import exaconstit_amd.lib as L
    N = 4
    i = np.arange(N ** 3)
    x, y = i % N, (i // N) % N
    grain = np.where((x == 0) | (x == N - 1), 2, np.where(y < 2, 1, 3)).astype(np.int32)
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    dts = DTS_RUN[:5]
    d = L.Driver.synthetic(N, _props(), quats.ravel(), dts)
    d.set_grains(grain, _grain_quats(3))
    d.set_periodic(10.0 * np.array([[1.0e-3, 2.0e-4, -1.0e-4], [-3.0e-4, -5.0e-4, 4.0e-4], [5.0e-4, -2.0e-4, -5.0e-4]]))
    for ti in range(1, len(dts) + 1):
        assert d.step(ti)
    got = d.lattice_curvature()
    ref, rsum, f, _ = driver_numpy(d, N, 1.0, periodic=True)
    _close(_got_rows(got), ref, what="periodic")
    _close_summary(_summary_arr(got), _summary_of(rsum), what="periodic")
    open_ref, _, _, _ = driver_numpy(d, N, 1.0, periodic=False)
    wrap = (f["GlobalElementId"] % N == 0) | (f["GlobalElementId"] % N == N - 1)
    assert np.abs(open_ref[wrap, 5:14] - ref[wrap, 5:14]).max() > 1e-6 * np.abs(ref[:, 5:14]).max()   # the wrap matters to the elements beside it
    d.close()


def _cell_array_names(floc, cycle):
    root = ET.parse(os.path.join(floc, "Cycle%06d" % cycle, "proc000000.vtu")).getroot()
    piece = root.find("UnstructuredGrid").find("Piece")
    names = {a.get("Name"): a.get("NumberOfComponents") for a in piece.find("CellData").findall("DataArray")}
    pv = ET.parse(os.path.join(floc, "Cycle%06d" % cycle, "data.pvtu")).getroot()
    pnames = [a.get("Name") for a in pv.find("PUnstructuredGrid").find("PCellData").findall("PDataArray")]
    assert sorted(pnames) == sorted(names)
    return names


def test_options_file_run_writes_files(tmp_path):
    import exaconstit_amd.lib as L
    from test_gpu_element_fields import _stage
    new = ("GROD", "KAM", "GNDDensity", "LatticeCurvature")
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir(); off.mkdir()
    toml = _stage(on, ["paraview = true", "steps = 1", "lattice_curvature = true", "lattice_curvature_burgers = 2.5e-7"], nsteps=3)
    d = L.Driver.from_toml(toml, out_dir=str(on), write_files=True)
    assert d.run() == 3
    last = d.lattice_curvature(burgers=2.5e-7)
    d.close()
    t = L.read_lattice_curvature(str(on / "lattice_curvature.txt"))
    assert np.array_equal(t["step"], [1, 2, 3]) and np.all(np.diff(t["time"]) > 0)
    assert len(open(str(on / "lattice_curvature.txt")).read().splitlines()) == 4                      # the header and one row per step
    for k in L.CURVATURE_SUMMARY:
        assert t[k][-1] == last["summary"][k], k                                                     # 17 significant digits: the same doubles
    names = _cell_array_names(str(on / "results" / "exaconstit"), 3)
    assert all(k in names for k in new) and names["LatticeCurvature"] == "9"
    assert all(k in _cell_array_names(str(on / "results" / "exaconstit"), 0) for k in new)
    toml = _stage(off, ["paraview = true", "steps = 1"], nsteps=3)
    d = L.Driver.from_toml(toml, out_dir=str(off), write_files=True)
    assert d.run() == 3
    d.close()
    assert not any(k in _cell_array_names(str(off / "results" / "exaconstit"), 3) for k in new)
    assert not os.path.exists(str(off / "lattice_curvature.txt"))
    # the text file does not need ParaView output
    txt = tmp_path / "txt"
    txt.mkdir()
    toml = _stage(txt, ["lattice_curvature = true", "lattice_curvature_burgers = 2.5e-7", 'lattice_curvature_fname = "lc.txt"'], nsteps=3)
    d = L.Driver.from_toml(toml, out_dir=str(txt), write_files=True)
    assert d.run() == 3
    d.close()
    t2 = L.read_lattice_curvature(str(txt / "lc.txt"))
    assert np.array_equal(t2["step"], [1, 2, 3])
    for k in L.CURVATURE_SUMMARY:                                                                     # (two runs: the atomic scatter of the PCG action orders its sums anew)
        assert np.allclose(t2[k], t[k], rtol=1e-8, atol=0), k
