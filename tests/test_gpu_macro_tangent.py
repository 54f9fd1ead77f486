"""Homogenised tangent of a periodic cell on the GPU: Driver.macro_tangent, the multi-column action behind its batched route
(Driver.grad_apply_columns) and the [Visualizations] macro_tangent output.

Voce FCC of tests/golden/refdata on generated N^3 cubes (Driver.synthetic + set_grains + set_periodic), five periodic Voronoi grains unless said
otherwise, the solver settings of tests/test_gpu_periodic.py (Newton rel 1e-10 / abs 1e-14, PCG rel 1e-12).  Correctness is pinned to a dense
reference assembled here: the raw operator K is probed column by column through the existing single-column action (which the existing suite pins
to the oracle), the periodic map P comes from the integer grid of the reference coordinates, and

    T_ref = A^T K A - A^T K P (P^T K P)^-1 P^T K A,       A = the nine affine fields, the corner group fixed.

Tolerance per entry (kl, m), from the dense matrices and the TRUE residuals the API reports (|b_m - K_uu w_m| recomputed by one more action):

    2 |(K^T A)_kl|_2 |K_uu^-1|_2 |r_m|_2 + 1e-12 max |T_ref|

- the first term is what an inexact solve can move the entry by (T - T_ref = a_kl^T K P K_uu^-1 r_m), the second the round-off of a sum of
O(100) products.  The measured figures are printed; EXA_WRITE_RECORDS=1 also writes them to profiles/macro_tangent_checks.txt."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hipref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
DTS = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()
LMAC = np.array([[1.0e-3, 2.0e-4, -1.0e-4], [-3.0e-4, -5.0e-4, 4.0e-4], [5.0e-4, -2.0e-4, -5.0e-4]])   # tests/test_gpu_periodic.py
LZ = np.diag([0.0, 0.0, 1.0e-3])                                                                          # tests/test_gpu_periodic_mixed.py
FREE_XY = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]])
TIGHT = dict(newton=(50, 1e-10, 1e-14), krylov=(20000, 1e-12, 1e-30))
RECORD = os.path.join(ROOT, "profiles", "macro_tangent_checks.txt")


def _record(key, lines):
    """the measured figures: printed and, when EXA_WRITE_RECORDS=1, kept in profiles/macro_tangent_checks.txt as the block '[key]'"""
    for ln in lines:
        print(ln)
    if os.environ.get("EXA_WRITE_RECORDS") != "1":
        return
    blocks, cur = {}, None
    if os.path.exists(RECORD):
        for ln in open(RECORD).read().splitlines():
            if ln.startswith("[") and ln.endswith("]"):
                cur = ln[1:-1]; blocks[cur] = []
            elif cur is not None:
                blocks[cur].append(ln)
    blocks[key] = list(lines)
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        for k in sorted(blocks):
            f.write("[%s]\n%s\n" % (k, "\n".join(blocks[k])))


def _voronoi(N, seeds=5, seed=7):
    """periodic Voronoi tessellation of the unit cube on the N^3 element centres (tests/test_gpu_periodic.py::_voronoi)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 1.0, (seeds, 3))
    c = (np.arange(N) + 0.5) / N
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    pts = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    d = pts[:, None, :] - s[None, :, :]
    d -= np.rint(d)
    return (np.argmin((d * d).sum(axis=2), axis=1) + 1).ravel()


def _props():
    return np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()


def _driver(L, N, nsteps, vgrad=LMAC, free=None, grains="voronoi", **kw):
    """a periodic synthetic driver, not stepped yet"""
    ori = np.loadtxt(os.path.join(REF, "voce_quats.ori")).reshape(-1, 4)
    args = dict(TIGHT); args.update(kw)
    d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:max(nsteps, 1)], **args)
    if grains == "voronoi":
        d.set_grains(_voronoi(N), ori[:5])
    elif grains == "single":
        d.set_grains(np.ones(N ** 3, dtype=np.int32), ori[3:4])
    d.set_periodic(vgrad, free)
    return d


def _stepped(L, N, nsteps, **kw):
    d = _driver(L, N, nsteps, **kw)
    for ti in range(1, nsteps + 1):
        assert d.step(ti), "Newton failed at step %d" % ti
    dg = d.diagnostics()
    assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0, dg
    return d


# ---------------------------------------------------------------------------------------------------------------- the dense reference
def _probe_K(d, nd):
    """the raw operator, column by column through the single-column action"""
    K = np.zeros((nd, nd))
    for j0 in range(0, nd, 16):
        nb = min(16, nd - j0)
        X = np.zeros((nb, nd)); X[np.arange(nb), j0 + np.arange(nb)] = 1.0
        K[:, j0:j0 + nb] = d.grad_apply_columns(X, batched=False).T
    return K


def _dense(d, N, p=1):
    """K (raw), A (nd, 9), P (nd, reduced dofs), T_ref (9, 9), |K_uu^-1|_2, row norms of A^T K and the box volume, for the state d stands at"""
    xr, xc = d.nodal_field("coords_ref"), d.nodal_field("coords")
    nn = xr.shape[0]; nd = 3 * nn
    grid = np.rint(xr * N * p).astype(int)
    assert np.abs(xr * N * p - grid).max() < 1e-9 and grid.min() == 0 and grid.max() == N * p
    K = _probe_K(d, nd)
    canon = grid % (N * p)
    key = canon[:, 0] + (N * p) * (canon[:, 1] + (N * p) * canon[:, 2])
    corner = np.all((grid == 0) | (grid == N * p), axis=1)
    assert corner.sum() == 8 and np.all(key[corner] == 0)
    groups = sorted(set(key[~corner].tolist()))
    col = {k: i for i, k in enumerate(groups)}
    P = np.zeros((nd, 3 * len(groups)))
    for g in range(nn):
        if not corner[g]:
            for c in range(3):
                P[g + nn * c, 3 * col[key[g]] + c] = 1.0
    org = xc.min(axis=0)
    A = np.zeros((nd, 9))
    for i in range(3):
        for j in range(3):
            A[np.arange(nn) + nn * i, 3 * i + j] = xc[:, j] - org[j]
    KA = K @ A
    Kuu = P.T @ K @ P
    T_ref = A.T @ KA - (A.T @ K @ P) @ np.linalg.solve(Kuu, P.T @ KA)
    inv_norm = 1.0 / np.linalg.svd(Kuu, compute_uv=False).min()
    rown = np.linalg.norm(K.T @ A, axis=0)                     # |(K^T A)_kl|_2
    # the cell's volume: the parallelepiped of the period vectors (corner differences of the current coordinates)
    c0 = np.where(np.all(grid == 0, axis=1))[0][0]
    per = np.stack([xc[np.where(np.all(grid == np.eye(3, dtype=int)[dd] * N * p, axis=1))[0][0]] - xc[c0] for dd in range(3)], axis=1)
    return dict(K=K, A=A, P=P, T_ref=T_ref, inv_norm=inv_norm, rown=rown, vol=abs(np.linalg.det(per)), nd=nd, nn=nn,
                asym=np.abs(K - K.T).max() / np.abs(K).max())


def _bound(ref, res):
    """tolerance per entry [(kl), m] for the true residuals res (9,)"""
    return 2.0 * np.outer(ref["rown"], res) * ref["inv_norm"] + 1e-12 * np.abs(ref["T_ref"]).max()


def _T(mt):
    return mt["dsig_dL"].reshape(9, 9) * mt["V"]


def _compare(mt, ref, what, factor=1.0, res=None):
    """T of a macro_tangent result against the dense reference; returns the record line"""
    b = factor * _bound(ref, mt["true_residual"] if res is None else res)
    err = np.abs(_T(mt) - ref["T_ref"])
    line = ("%s: route %s, iterations %s, true relative residuals %.1e .. %.1e (solver's own %.1e .. %.1e), worst |T - T_ref| / bound %.3e, worst |T - T_ref| %.3e of max |T_ref| %.3e; "
            "|K_uu^-1| %.3e, K asymmetry %.1e" % (what, "batched x%d" % mt["nch"] if mt["batched"] else "one by one", [int(i) for i in mt["iters"]], mt["true_rel"].min(), mt["true_rel"].max(),
                                                 mt["reduction"].min(), mt["reduction"].max(), (err / b).max(), err.max(), np.abs(ref["T_ref"]).max(), ref["inv_norm"], ref["asym"]))
    return err, b, line


_cache = {}


def _reference_p1(L):
    """the one-rank p = 1 reference of checks 5 and 6: N = 4, five grains, LMAC, after step 1; its dense matrices and its batched tangent"""
    if "p1" not in _cache:
        d = _stepped(L, 4, 1)
        ref = _dense(d, 4)
        mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000, batched=True)
        d.close()
        _cache["p1"] = (ref, mt)
    return _cache["p1"]


# ---------------------------------------------------------------------------------------------------------------- 1. batched action = single action
@pytest.mark.parametrize("N", [3, 5])
def test_batched_action_is_the_single_action(N):
    """N = 3: 27 elements, one partial wave; N = 5: 125 elements, two blocks, the second partial.  After a plastic step (step 8 of the schedule of
    check 3), random columns, NC = 1, 2, 3, 4, 9 (passes of 3, 2 and 1 columns and every remainder), raw and with the essential mask (assembled).
    Each column within 1e-12 max |column| of the single-column action: 5 x the 2e-13 the README records for route-to-route parity of K x - only
    the order of <= 8 atomic addends and FMA contraction may differ."""
    import exaconstit_amd.lib as L
    d = _stepped(L, N, 8, vgrad=LZ)                 # the 8 steps of tests/test_gpu_periodic_mixed.py: the last ones are plastic
    nd = 3 * d.nodal_field("coords").shape[0]
    rng = np.random.default_rng(3)
    lines, worst = [], 0.0
    for nch in (1, 2, 3):
        for nc in (1, 2, 3, 4, 9):
            X = rng.standard_normal((nc, nd))
            for assembled in (False, True):
                one = d.grad_apply_columns(X, assembled=assembled, batched=False)
                bat = d.grad_apply_columns(X, assembled=assembled, batched=True, nch=nch)
                for m in range(nc):
                    e = np.abs(bat[m] - one[m]).max() / np.abs(one[m]).max()
                    worst = max(worst, e)
                    assert e <= 1e-12, (nch, nc, assembled, m, e)
                if assembled:       # (the mask is in force: essential rows of the output are zero, and essential entries of the input do not matter)
                    X2 = X.copy(); X2[:, one[0] == 0.0] += 1.0
                    assert (one[0] == 0.0).sum() >= 24 and np.abs(d.grad_apply_columns(X2, assembled=True, batched=True, nch=nch) - one).max() <= 1e-12 * np.abs(one).max()
    lines.append("batched action, N = %d (%d elements): worst column deviation from the single-column action %.3e of max |column| (limit 1e-12), passes of 1, 2, 3 columns, NC = 1, 2, 3, 4, 9, raw and masked" % (N, N ** 3, worst))
    # a column's result does not depend on its neighbours in the pass: column 1 alone, and beside two others
    X = rng.standard_normal((3, nd))
    full = d.grad_apply_columns(X, batched=True, nch=3)
    alone = d.grad_apply_columns(X[1:2], batched=True, nch=3)
    lines.append("  column 1 of a pass of three against the same column alone: %.3e of max |column|" % (np.abs(full[1] - alone[0]).max() / np.abs(alone[0]).max()))
    assert np.abs(full[1] - alone[0]).max() <= 1e-12 * np.abs(alone[0]).max()
    # gated subset: columns 0 and 2 keep their sentinel bit for bit, column 1 is its ungated result
    sent = np.full((3, nd), -7.25e300); sent[1] = 0.0
    for nch in (1, 2, 3):
        got = d.grad_apply_columns(X, batched=True, nch=nch, gated=[1, 0, 1], y0=sent)
        assert np.array_equal(got[0].view(np.int64), sent[0].view(np.int64)) and np.array_equal(got[2].view(np.int64), sent[2].view(np.int64))
        assert np.abs(got[1] - full[1]).max() <= 1e-12 * np.abs(full[1]).max()
    got = d.grad_apply_columns(X, batched=True, gated=[1, 1, 1], y0=np.full((3, nd), 3.5))
    assert np.all(got == 3.5)
    _record("batched_action_N%d" % N, lines)
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 2. dense reference, elastic state
def test_dense_reference_elastic_state():
    """N = 3, p = 1, 64 nodes (192 x 192), five grains, after step 1 (elastic: K symmetric to round-off).  Both routes."""
    import exaconstit_amd.lib as L
    N = 3
    d = _stepped(L, N, 1)
    ref = _dense(d, N)
    assert ref["nd"] == 192
    lines = []
    for batched in (True, False):
        mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000, batched=batched)
        assert mt["batched"] == batched
        err, b, line = _compare(mt, ref, "dense reference, elastic, N = 3, batched = %s" % batched)
        lines.append(line)
        assert np.all(err <= b), (err / b).max()
        assert abs(mt["V"] - ref["vol"]) <= 1e-12 * ref["vol"], (mt["V"], ref["vol"])
        assert mt["dt"] == DTS[0]
        T = _T(mt)
        assert np.all(np.abs(T - T.T) <= b + b.T), (np.abs(T - T.T) / (b + b.T)).max()      # major symmetry
        lines.append("  V %.15e against the box %.15e; major symmetry |T - T^T| worst %.3e of its bound" % (mt["V"], ref["vol"], (np.abs(T - T.T) / (b + b.T)).max()))
        assert np.all(mt["flags"] == 1) and np.all(mt["true_rel"] <= 1e-10)
        # the Voigt stiffness is that of a stable elastic solid: symmetric to the same relative level, positive definite
        Cv = mt["C_voigt"]
        assert np.abs(Cv - Cv.T).max() <= 1e-9 * np.abs(Cv).max() and np.linalg.eigvalsh(0.5 * (Cv + Cv.T)).min() > 0
    # the automatic route and the Krylov options of the run (rel 1e-12, 20000 iterations)
    mt = d.macro_tangent()
    err, b, line = _compare(mt, ref, "  automatic route, Krylov options of the run")
    lines.append(line)
    assert np.all(err <= b)
    _record("dense_elastic", lines)
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 3. dense reference, plastic state
def test_dense_reference_plastic_state():
    """N = 4 after 8 steps of the schedule of tests/test_gpu_periodic_mixed.py (custom_dt.txt, L33 = 1e-3: past first yield).  K is not symmetric
    there; if CG stalls above rel_tol the true residual the API reports enters the bound - and must stay below 1e-6 for every column."""
    import exaconstit_amd.lib as L
    N = 4
    d = _stepped(L, N, 8, vgrad=LZ)
    ref = _dense(d, N)
    lines = []
    for batched in (True, False):
        mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000, batched=batched)
        err, b, line = _compare(mt, ref, "dense reference, plastic (8 steps), N = 4, batched = %s" % batched)
        lines.append(line)
        lines.append("  true relative residuals per column: %s" % " ".join("%.2e" % v for v in mt["true_rel"]))
        assert np.all(mt["true_rel"] <= 1e-6), mt["true_rel"]
        assert np.all(err <= b), (err / b).max()
        assert abs(mt["V"] - ref["vol"]) <= 1e-12 * ref["vol"]
    _record("dense_plastic", lines)
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 4. conventions against the oracle
@pytest.mark.parametrize("nsteps", [1, 8])
def test_conventions_against_the_oracle(nsteps):
    """One orientation in every element: the field is homogeneous, the fluctuation vanishes (|w| <= 1e-10 |a|), and T / V is the tangent of the
    point update contracted with the strain pattern of E_m, times the dt factor of fem::assemble_grad_pa.  The point update is the oracle's
    (orc_model_setup on one element driven by v = L x, step by step); tolerance: the 1e-7 (relative L2) tests/test_gpu_parity.py uses for the
    tangent against the oracle.  Step 1 is elastic, step 8 past yield."""
    import exaconstit_amd.lib as L
    import orc
    orc.build()
    N = 3
    d = _stepped(L, N, nsteps, vgrad=LZ, grains="single")
    mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000)
    assert np.all(mt["w_over_a"] <= 1e-10), mt["w_over_a"]
    # the oracle's chain of point updates on one element of the homogeneous field
    props = _props()
    q = np.loadtxt(os.path.join(REF, "voce_quats.ori")).reshape(-1, 4)[3]
    q = q / np.linalg.norm(q)
    rve = hipref.make_rve(orc, 1)
    P = rve["Q"]
    hist = np.zeros(26); orc.lib().orc_hist_init(0, 0, orc._p(props), len(props), orc._p(hist))
    sv0 = np.tile(np.concatenate([hist, [1.0, 0.0]]), P).reshape(P, 28); sv0[:, 9:13] = q
    sv0 = sv0.ravel(); s0 = np.zeros(6 * P)
    x = rve["X"].copy(); NN = rve["NN"]
    for k in range(nsteps):
        dt = DTS[k]
        X3 = x.reshape(3, NN)
        v = (LZ @ (X3 - X3.min(axis=1, keepdims=True))).ravel()
        x = x + v * dt
        xe = hipref.l_to_e(rve, x); ve = hipref.l_to_e(rve, v)
        J = np.zeros(9 * P); orc.lib().orc_jacobians(1, 1, orc._p(xe), orc._p(J))
        s1 = np.zeros(6 * P); sv1 = np.zeros(28 * P); cm = np.zeros(36 * P)
        nf = orc.lib().orc_model_setup(0, 0, orc._p(props), len(props), rve["Q"], 1, rve["n"], 28, C.c_double(dt), C.c_double(298.0), orc._p(J), orc._p(rve["G"]), orc._p(ve),
                                       orc._p(s0), orc._p(sv0), orc._p(s1), orc._p(sv1), orc._p(cm), None, 1, 0, 0)
        assert nf == 0
        s0, sv0 = s1, sv1
    c = cm[:36]                                  # sigma_i = sum_j c[i + 6 j] eps_j, Voigt 11 22 33 23 13 12 with engineering shears (pa_kernels.hip)
    vo = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (1, 2): 3, (2, 1): 3, (0, 2): 4, (2, 0): 4, (0, 1): 5, (1, 0): 5}
    want = np.zeros((3, 3, 3, 3))
    for k in range(3):
        for l in range(3):
            for m in range(3):
                for n in range(3):
                    want[k, l, m, n] = mt["dt"] * c[vo[(k, l)] + 6 * vo[(m, n)]]
    e = hipref.rel_l2(mt["dsig_dL"], want)
    # the average stress of the homogeneous cell is the oracle's point stress too (same tolerance as the stress of the parity test, 1e-9)
    es = hipref.rel_l2(d.avgs(0, 6)[-1], s1[:6])
    _record("oracle_conventions_%d" % nsteps, ["conventions, one orientation, N = 3, after step %d: |w| / |a| worst %.1e; T / V against dt x the oracle's point tangent: relative L2 %.3e (limit 1e-7); average stress against the point stress %.1e; tangent asymmetry of the point %.1e"
                                                % (nsteps, mt["w_over_a"].max(), e, es, np.abs(c.reshape(6, 6) - c.reshape(6, 6).T).max() / np.abs(c).max())])
    assert e < 1e-7, e
    # C_voigt: the point tangent itself, averaged over the two orders of a shear pair
    cv = c.reshape(6, 6).T                       # [i, j] = c[i + 6 j]
    assert hipref.rel_l2(mt["C_voigt"], cv) < 1e-7
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 5. routes and ranks
def _same_operator(L, what, mt, extra_lines=()):
    """a route that solves the SAME system as the one-rank batched p = 1 reference: twice the bound of check 2, with the larger of the two runs' residuals"""
    ref, mt0 = _reference_p1(L)
    res = np.maximum(mt["true_residual"], mt0["true_residual"])
    err, b, line = _compare(mt, ref, what, factor=2.0, res=res)
    _record("route_" + what.split(",")[0].replace(" ", "_"), [line] + list(extra_lines))
    assert np.all(err <= b), (what, (err / b).max())
    e2 = np.abs(_T(mt) - _T(mt0))
    assert np.all(e2 <= b), (what, (e2 / b).max())


def _own_operator(L, what, N, p=1, nsteps=1, can_batch=False, **kw):
    """a route whose operator differs from the p = 1 partial-assembly one: its own dense reference, twice the bound of check 2"""
    d = _stepped(L, N, nsteps, **kw)
    ref = _dense(d, N, p)
    lines = []
    for batched in ((True, False) if can_batch else (None,)):
        mt = d.macro_tangent(rel_tol=1e-12, max_iter=4000, batched=batched)
        assert mt["batched"] == bool(batched)
        err, b, line = _compare(mt, ref, what, factor=2.0)
        lines.append(line)
        assert np.all(err <= b), (what, (err / b).max())
        assert abs(mt["V"] - ref["vol"]) <= 1e-12 * ref["vol"]
    if not can_batch:
        with pytest.raises(RuntimeError, match="batched"):
            d.macro_tangent(batched=True)
    return d, ref, mt, lines


@pytest.mark.parametrize("route", ["p2", "ea", "p2_bbar_ea"])
def test_routes_with_their_own_operator(route):
    import exaconstit_amd.lib as L
    kw = {"p2": dict(order=2), "ea": dict(assembly=1), "p2_bbar_ea": dict(order=2, assembly=1, bbar=True)}[route]
    # (element assembly from the point records at p = 1 is a context the multi-column kernel serves - partial assembly on C^T: both routes there)
    d, ref, mt, lines = _own_operator(L, route + ", N = 4, after step 1", 4, p=kw.get("order", 1), can_batch=route == "ea", **kw)
    _record("route_" + route, lines)
    d.close()


def test_route_jacobi():
    import exaconstit_amd.lib as L
    d = _stepped(L, 4, 1, jacobi=True)
    for batched in (True, False):
        _same_operator(L, "jacobi %s, N = 4" % ("batched" if batched else "one by one"), d.macro_tangent(rel_tol=1e-12, max_iter=2000, batched=batched))
    d.close()


def test_route_deterministic(monkeypatch):
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    d = _stepped(L, 4, 1)
    mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000)
    assert not mt["batched"]
    with pytest.raises(RuntimeError, match="non-deterministic"):
        d.macro_tangent(batched=True)
    again = d.macro_tangent(rel_tol=1e-12, max_iter=2000)
    assert np.array_equal(mt["dsig_dL"].view(np.int64), again["dsig_dL"].view(np.int64))       # ordered sums everywhere: the same bits
    monkeypatch.delenv("EXA_DETERMINISTIC")
    _same_operator(L, "deterministic, N = 4", mt)
    d.close()


def test_route_mixed_and_its_condensed_tangent():
    """xx, yy free (uniaxial stress along z), 3 steps.  The tangent's solves fix all nine control slots, so T is that of the plain periodic space at
    the mixed run's state: its own dense reference; the condensed tangent against the condensation of that reference.  A first-order perturbation of
    S = C_pp - C_pf C_ff^-1 C_fp by entry errors <= eps gives |dS_ij| <= eps (1 + |X_.j|_1) (1 + |Y_i.|_1), X = C_ff^-1 C_fp, Y = C_pf C_ff^-1."""
    import exaconstit_amd.lib as L
    N = 4
    d = _stepped(L, N, 3, vgrad=LZ, free=FREE_XY)
    ref = _dense(d, N)
    lines = []
    for batched in (True, False):
        mt = d.macro_tangent(rel_tol=1e-12, max_iter=2000, batched=batched)
        assert mt["batched"] == batched
        err, b, line = _compare(mt, ref, "mixed (xx, yy free), N = 4, after step 3, batched = %s" % batched, factor=2.0)
        lines.append(line)
        assert np.all(err <= b), (err / b).max()
        assert np.array_equal(mt["free"], FREE_XY.astype(bool))
        f = FREE_XY.astype(bool).ravel(); pmask = ~f
        Cr = ref["T_ref"] / mt["V"]
        X = np.linalg.solve(Cr[np.ix_(f, f)], Cr[np.ix_(f, pmask)]); Y = Cr[np.ix_(pmask, f)] @ np.linalg.inv(Cr[np.ix_(f, f)])
        want = np.zeros((9, 9)); want[np.ix_(pmask, pmask)] = Cr[np.ix_(pmask, pmask)] - Cr[np.ix_(pmask, f)] @ X
        tol = np.zeros((9, 9)); tol[np.ix_(pmask, pmask)] = (b.max() / mt["V"]) * np.outer(1.0 + np.abs(Y).sum(axis=1), 1.0 + np.abs(X).sum(axis=0))
        got = mt["condensed"].reshape(9, 9)
        assert np.all(np.abs(got - want) <= tol), (np.abs(got - want)[np.ix_(pmask, pmask)] / tol[np.ix_(pmask, pmask)]).max()
        assert np.all(got[f] == 0.0) and np.all(got[:, f] == 0.0)
        lines.append("  condensed tangent: worst deviation %.3e of its bound; uniaxial modulus d sigma_33 / d L_33 / dt: condensed %.6e, unconstrained %.6e"
                     % ((np.abs(got - want)[np.ix_(pmask, pmask)] / tol[np.ix_(pmask, pmask)]).max(), got[8, 8] / mt["dt"], mt["dsig_dL"][2, 2, 2, 2] / mt["dt"]))
        assert got[8, 8] < mt["dsig_dL"][2, 2, 2, 2]       # letting the cell contract laterally softens it
    # the run goes on as if nothing had happened: mask, free bits and the realised gradient are the run's
    mi = d.macro_info()
    assert np.array_equal(mi["free"], FREE_XY.astype(bool))
    _record("route_mixed", lines)
    d.close()


def test_two_loopback_ranks():
    import exaconstit_amd.lib as L
    N, nranks = 4, 2
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    out, errors = [None] * nranks, []
    ori = np.loadtxt(os.path.join(REF, "voce_quats.ori")).reshape(-1, 4)

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:1], rank=r, nranks=nranks, uid=gid, **TIGHT)
            d.set_grains(_voronoi(N), ori[:5])
            d.set_periodic(LMAC)
            if not d.step(1):
                raise RuntimeError("rank %d: Newton failed" % r)
            out[r] = d.macro_tangent(rel_tol=1e-12, max_iter=2000)
            try:
                d.macro_tangent(batched=True)
                raise AssertionError("the batched route must be refused on several ranks")
            except RuntimeError as e:
                assert "one rank" in str(e)
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    L.exa_loopback_group_destroy(gid)
    assert np.array_equal(out[0]["dsig_dL"], out[1]["dsig_dL"]) and out[0]["V"] == out[1]["V"] and not out[0]["batched"]
    _same_operator(L, "two loopback ranks, N = 4", out[0])


# ---------------------------------------------------------------------------------------------------------------- 6. the run is undisturbed
def _state(d):
    st = d.stats()
    return dict(avgs=d.avgs(0, 6), v=d.nodal_field("velocity"), x=d.nodal_field("coords"), newton=list(st[0]), krylov=list(st[1]), calls=list(st[2]),
                stress=[d.qf_component(2, c) for c in range(6)], state=[d.qf_component(0, c) for c in (0, 2, 9, 13)], diag=d.diagnostics(), ninfo=d.newton_info(),
                timers_krylov=d.timers()["krylov_iters"])


@pytest.mark.parametrize("free", [None, FREE_XY], ids=["periodic", "mixed"])
def test_the_run_is_undisturbed(monkeypatch, free):
    """four steps at N = 4 with macro_tangent() after every step - before and after commit_step(), both routes in turn - against the same four steps
    without it: the same bits of state, stress, velocity, averages, Newton and Krylov counts.  Under EXA_DETERMINISTIC=1 a run reproduces its own
    bits; the batched route does not exist there, so the default mode runs as well: there the two runs agree as two plain runs do (the order of
    the atomic addends is free: averages to 1e-10, equal Newton counts)."""
    import exaconstit_amd.lib as L
    N, nsteps = 4, 4
    for det in (True, False):
        if det:
            monkeypatch.setenv("EXA_DETERMINISTIC", "1")
        else:
            monkeypatch.delenv("EXA_DETERMINISTIC", raising=False)
        runs = []
        for with_tangent in (False, True):
            d = _driver(L, N, nsteps, vgrad=LZ if free is not None else LMAC, free=free)
            for ti in range(1, nsteps + 1):
                assert d.step(ti, commit=False)
                if with_tangent:
                    a = d.macro_tangent(batched=None if det else (ti % 2 == 0))
                d.commit_step()
                if with_tangent:
                    b = d.macro_tangent(batched=None if det else (ti % 2 == 1))
                    # the same state on both sides of the commit: the same tangent (to the solves' tolerance)
                    assert np.abs(a["dsig_dL"] - b["dsig_dL"]).max() <= 1e-8 * np.abs(a["dsig_dL"]).max()
                    assert a["V"] == b["V"]
            runs.append(_state(d))
            d.close()
        r0, r1 = runs
        assert r0["newton"] == r1["newton"] and r0["calls"] == r1["calls"]
        if det:
            assert r0["krylov"] == r1["krylov"]
            for k in ("avgs", "v", "x"):
                assert np.array_equal(r0[k].view(np.int64), r1[k].view(np.int64)), k
            for k in ("stress", "state"):
                for a_, b_ in zip(r0[k], r1[k]):
                    assert np.array_equal(np.ascontiguousarray(a_).view(np.int64), np.ascontiguousarray(b_).view(np.int64)), k
            # Newton's last norm, the PCG diagnostics (last flag and reduction, counts) and the timers' iteration count are the run's own
            assert r0["ninfo"] == r1["ninfo"] and r0["diag"] == r1["diag"] and r0["timers_krylov"] == r1["timers_krylov"]
        else:
            assert np.abs(r0["avgs"] - r1["avgs"]).max() <= 1e-10 * np.abs(r0["avgs"]).max()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(tmp_path):
    import exaconstit_amd.lib as L
    N = 3
    d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:2], **TIGHT)
    assert d.step(1)
    with pytest.raises(RuntimeError, match="not periodic"):
        d.macro_tangent()
    d.close()
    d = _driver(L, N, 2)
    with pytest.raises(RuntimeError, match="no solved step"):
        d.macro_tangent()
    with pytest.raises(RuntimeError, match="no solved step"):
        d.grad_apply_columns(np.zeros((1, 3 * d.nodal_field("coords").shape[0])))
    assert d.step(1)
    good = d.macro_tangent()
    ck = str(tmp_path / "t.ckpt")
    d.save_checkpoint(ck)
    d.close()
    e = _driver(L, N, 2)
    e.load_checkpoint(ck)
    with pytest.raises(RuntimeError, match="since the restart"):
        e.macro_tangent()
    assert e.step(2)
    mt = e.macro_tangent()
    # steps 1 and 2 are both elastic: per strain increment (T / V carries the dt factor, 0.005 against 0.195) the two tangents are the same
    # stiffness up to the rate-dependent relaxation of the longer step (measured 3 %)
    a, b = mt["dsig_dL"] / mt["dt"], good["dsig_dL"] / good["dt"]
    assert np.all(np.isfinite(a)) and np.abs(a - b).max() < 0.1 * np.abs(b).max()
    with pytest.raises(RuntimeError, match="columns"):
        e.grad_apply_columns(np.zeros((17, 3 * e.nodal_field("coords").shape[0])))
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 8. resource report
def test_tangent_kernels_have_no_scratch():
    """no private segment in the loaded code object, for the column action at 1, 2 and 3 columns per pass (every record form), the affine columns and
    the contraction - read the way test_mixed_kernels_have_no_scratch reads it (hipFuncGetAttributes)"""
    import exaconstit_amd.lib as L
    hipref.Dev()
    sb = L.tangent_scratch_bytes()
    assert all(v == 0 for v in sb.values()), sb


# ---------------------------------------------------------------------------------------------------------------- the options route: file and checkpoint
def _toml(tmp_path, tag, N, macro, nsteps_total=40):
    os.makedirs(str(tmp_path), exist_ok=True)
    gfile = os.path.join(str(tmp_path), "grains_%s.txt" % tag)
    np.savetxt(gfile, _voronoi(N).reshape(-1, 1), fmt="%d")
    vis = "    steps = 2\n    avg_stress_fname = \"avg_stress.txt\"\n" + ("    macro_tangent = true\n    macro_tangent_rel_tol = 1e-11\n" if macro else "")
    L9 = "[" + ", ".join("[" + ", ".join(repr(float(x)) for x in row) + "]" for row in LMAC) + "]"
    txt = f'''Version = "0.6.0"
[Properties]
    temperature = 298
    [Properties.Matl_Props]
        floc = "{REF}/props_cp_voce.txt"
        num_props = 17
    [Properties.State_Vars]
        floc = "{REF}/state_cp_voce.txt"
        num_vars = 24
    [Properties.Grain]
        ori_state_var_loc = 9
        ori_stride = 4
        ori_type = "quat"
        num_grains = 500
        ori_floc = "{REF}/voce_quats.ori"
        grain_floc = "{gfile}"
[BCs]
    periodic = true
    essential_vel_grad = {L9}
[Model]
    mech_type = "exacmech"
    cp = true
    [Model.ExaCMech]
        xtal_type = "fcc"
        slip_type = "powervoce"
[Time]
    [Time.Custom]
        nsteps = {nsteps_total}
        floc = "{REF}/custom_dt.txt"
[Visualizations]
{vis}[Solvers]
    assembly = "PA"
    integ_model = "FULL"
    rtmodel = "GPU"
    [Solvers.NR]
        iter = 50
        rel_tol = 1e-10
        abs_tol = 1e-14
        nl_solver = "NR"
    [Solvers.Krylov]
        iter = 20000
        rel_tol = 1e-12
        abs_tol = 1e-30
        solver = "PCG"
[Mesh]
    type = "auto"
    ref_ser = 0
    p_refinement = 1
    [Mesh.Auto]
        length = [1.0, 1.0, 1.0]
        ncuts = [{N}, {N}, {N}]
'''
    path = os.path.join(str(tmp_path), tag + ".toml")
    open(path, "w").write(txt)
    return path


def test_file_output_and_checkpoint_section(tmp_path):
    """[Visualizations] macro_tangent = true with steps = 2: rows after steps 2 and 4, 17 digits, equal to what the interface returns at that state;
    the rows travel in a checkpoint section of their own, which exists only with the option on - a checkpoint of the same run without the option
    has the sections it always had."""
    import exaconstit_amd.lib as L
    N = 3
    out = tmp_path / "on"; os.makedirs(str(out))
    d = L.Driver.from_toml(_toml(tmp_path, "on", N, True), out_dir=str(out), write_files=True)
    for ti in range(1, 5):
        assert d.step(ti)
    rows = L.read_macro_tangent(str(out / "macro_tangent.txt"))
    assert [r["step"] for r in rows] == [2, 4]
    mt = d.macro_tangent(rel_tol=1e-11)
    assert rows[1]["dt"] == mt["dt"] == DTS[3] and rows[1]["V"] == mt["V"] and abs(rows[1]["time"] - DTS[:4].sum()) < 1e-12
    assert np.abs(rows[1]["dsig_dL"] - mt["dsig_dL"]).max() <= 1e-9 * np.abs(mt["dsig_dL"]).max()      # (two solves to 1e-11 of the same systems)
    ck_on = str(tmp_path / "on.ckpt"); d.save_checkpoint(ck_on)
    d.close()
    names_on = list(L.checkpoint_info(ck_on)["sections"])
    assert "macro_tangent" in names_on
    # a restart brings the rows back and rewrites the file from them
    out2 = tmp_path / "on2"; os.makedirs(str(out2))
    e = L.Driver.from_toml(_toml(tmp_path, "on", N, True), out_dir=str(out2), write_files=True, restart=ck_on)
    back = L.read_macro_tangent(str(out2 / "macro_tangent.txt"))
    assert len(back) == 2 and all(np.array_equal(a["dsig_dL"], b["dsig_dL"]) and a["V"] == b["V"] and a["time"] == b["time"] for a, b in zip(rows, back))
    assert e.step(5) and e.step(6)
    assert [r["step"] for r in L.read_macro_tangent(str(out2 / "macro_tangent.txt"))] == [2, 4, 6]
    e.close()
    # option off: no file, no section
    out3 = tmp_path / "off"; os.makedirs(str(out3))
    f = L.Driver.from_toml(_toml(tmp_path, "off", N, False), out_dir=str(out3), write_files=True)
    for ti in range(1, 5):
        assert f.step(ti)
    ck_off = str(tmp_path / "off.ckpt"); f.save_checkpoint(ck_off)
    f.close()
    assert not os.path.exists(str(out3 / "macro_tangent.txt"))
    names_off = list(L.checkpoint_info(ck_off)["sections"])
    assert "macro_tangent" not in names_off and [n for n in names_on if n != "macro_tangent"] == names_off
