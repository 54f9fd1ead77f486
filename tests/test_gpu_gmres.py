"""The restarted GMRES solver (host/krylov.hip, gmres_kernels.hip) on the GPU.

Kernels: gmres_ortho_probe runs the multi-dot and the multi-axpy on shapes a driver cannot produce, against long double and the summation bound
2 n eps sum |w_j a_j b_j|.  Solver: Driver.gmres_solve hands GMRES a right-hand side on the set-up of tests/test_gpu_pcg_reference.py (one solved step,
the dense K_uu probed through grad_apply_columns, check_every = 4); iterate, count, flag, reported reduction and restarts are compared with
tests/gmres_reference.py at the same iteration.  Every tolerance on x and on the reduction is 100 x the reference's own sensitivity (float64 reruns
with permuted dot products in both orthogonalisation orders), with the floor 1e-13 of max |x_k| on x; stopping iterations come from the chooser.
The run: the same steps under PCG and under GMRES.  Every test prints what it chose and measured; EXA_WRITE_RECORDS=1 keeps the lines in
profiles/gmres_checks.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import gmres_reference as G
import hipref
import test_gpu_pcg_reference as P
from test_gpu_pcg_reference import _Env, _dense_K, _on_ranks, _probed, _props, _say

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
RECORD = os.path.join(ROOT, "profiles", "gmres_checks.txt")
DTS, TIGHT, SEEDS, CE = P.DTS, P.TIGHT, P.SEEDS, P.CE
EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _record(key, lines):
    """the lines a test printed: with EXA_WRITE_RECORDS=1 kept in profiles/gmres_checks.txt as the block '[key]'"""
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
    import exaconstit_amd.lib as L
    with open(RECORD, "w") as f:
        f.write("# build %s, kernel build %s\n" % (L.exa_build_id().decode(), L.exa_kernel_build_id().decode()))
        for k in sorted(blocks):
            f.write("[%s]\n%s\n" % (k, "\n".join(blocks[k])))


def _chunk():
    """basis vectors per pass of the multi-dot kernel: the shapes below sit on either side of it"""
    import exaconstit_amd.lib as L
    assert 8 <= L.GMRES_MULTIDOT_CHUNK <= 16
    return L.GMRES_MULTIDOT_CHUNK


# ---------------------------------------------------------------------------------------------------------------- the two bandwidth kernels
def _basis(n, k, seed):
    """weights in (0, 1], k vectors orthonormal in the weighted product (n >= k; random unit vectors where n < k: no such basis exists) and w"""
    rng = np.random.default_rng(seed)
    wgt = 1.0 - rng.uniform(0.0, 1.0, n) * 0.999
    if n >= k:
        Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
        V = (Q / np.sqrt(wgt)[:, None]).T.astype(LD)
        for _ in range(2):                                   # orthonormal to long-double round-off, then rounded once
            for j in range(k):
                for l in range(j):
                    V[j] -= np.sum(wgt * V[l] * V[j], dtype=LD) * V[l]
                V[j] /= np.sqrt(np.sum(wgt * V[j] * V[j], dtype=LD))
        V = np.ascontiguousarray(V.astype(np.float64))
    else:
        V = rng.standard_normal((k, n))
        V /= np.sqrt((wgt * V * V).sum(axis=1))[:, None]
    return wgt, V, rng.standard_normal(n)


def _bound(n, wgt, V, w):
    """2 n eps sum_i |wgt_i v_ji w_i| per j"""
    return 2.0 * n * EPS * np.abs(wgt[None, :] * V * w[None, :]).sum(axis=1)


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4097])
@pytest.mark.parametrize("ki", [0, 1, 2, 3], ids=["k1", "kchunk", "kchunk+1", "k2chunk+3"])
def test_ortho_kernels(n, ki):
    """h = V^T W w against long double within the summation bound; w_out orthogonal to V within the same bound (where an orthonormal V exists); the gate
    closed: w_out = w bit for bit and no pass; two calls: the same bits"""
    import exaconstit_amd.lib as L
    ch = _chunk()
    k = (1, ch, ch + 1, 2 * ch + 3)[ki]
    wgt, V, w = _basis(n, k, 100 * n + k)
    bound = _bound(n, wgt, V, w)
    h_ref = np.array([np.sum(wgt.astype(LD) * V[j].astype(LD) * w.astype(LD), dtype=LD) for j in range(k)])
    lines = []
    for mode in ("never", "mgs") if n >= k else ("never",):
        out = L.gmres_ortho_probe(wgt, V, w, mode=mode)
        dev = np.abs(out["h"].astype(LD) - h_ref).astype(np.float64)
        if mode == "never":
            _say(lines, "n %d k %d (chunk %d) %s: max |h - h_ref| / bound %.3f, passes %d" % (n, k, ch, mode, float((dev / bound).max()), out["passes"]))
            assert np.all(dev <= bound), (dev / bound).max()
        assert out["passes"] == 1
        want = (w.astype(LD) - (out["h"].astype(LD)[:, None] * V.astype(LD)).sum(axis=0)).astype(np.float64)
        scale = np.abs(w) + (np.abs(out["h"])[:, None] * np.abs(V)).sum(axis=0)
        if mode == "never":
            assert np.all(np.abs(out["w_out"] - want) <= 2.0 * (k + 1) * EPS * scale)
        n2 = float(np.sum(wgt.astype(LD) * out["w_out"].astype(LD) ** 2, dtype=LD))
        assert abs(out["wnorm2"] - n2) <= 2.0 * n * EPS * n2 + 1e-300
        if n >= k:
            orth = np.abs(np.array([np.sum(wgt.astype(LD) * V[j].astype(LD) * out["w_out"].astype(LD), dtype=LD) for j in range(k)]).astype(np.float64))
            _say(lines, "   %s: max |V^T W w_out| / bound %.3f" % (mode, float((orth / bound).max())))
            assert np.all(orth <= bound), (mode, (orth / bound).max())
    a = L.gmres_ortho_probe(wgt, V, w)
    b = L.gmres_ortho_probe(wgt, V, w)
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["w_out"], b["w_out"]) and a["wnorm2"] == b["wnorm2"] and a["passes"] == b["passes"]
    z = L.gmres_ortho_probe(wgt, V, w, flag=1.0)
    assert z["passes"] == 0 and np.array_equal(z["w_out"], w)
    _record("kernels n%d k%d" % (n, k), lines)


@pytest.mark.parametrize("n", [257, 4097])
def test_second_pass_on_the_criterion(n):
    """w = V c + 1e-9 u: the first pass takes almost everything away, so the criterion asks for the second; afterwards w_out is orthogonal to V to
    the summation bound of its own size.  'never' stops after one pass."""
    import exaconstit_amd.lib as L
    k = _chunk() + 1
    wgt, V, u = _basis(n, k, 7 * n)
    rng = np.random.default_rng(n)
    c = rng.standard_normal(k); c /= np.linalg.norm(c)
    u /= np.sqrt((wgt * u * u).sum())
    w = c @ V + 1e-9 * u
    out = L.gmres_ortho_probe(wgt, V, w, mode="ifneeded")
    assert out["passes"] == 2
    nrm = np.sqrt(out["wnorm2"])
    orth = np.abs(np.array([np.sum(wgt.astype(LD) * V[j].astype(LD) * out["w_out"].astype(LD), dtype=LD) for j in range(k)]).astype(np.float64)) / nrm
    bound = _bound(n, wgt, V, out["w_out"]) / nrm
    lines = []
    _say(lines, "n %d k %d: |w_out| %.3e, max |V^T W w_out| / |w_out| %.3e, bound %.3e; h - c max %.2e" % (n, k, nrm, orth.max(), bound.max(), np.abs(out["h"] - c).max()))
    assert np.all(orth <= bound)
    assert np.abs(out["h"] - c).max() <= 1e-8
    assert L.gmres_ortho_probe(wgt, V, w, mode="never")["passes"] == 1
    assert L.gmres_ortho_probe(wgt, V, w, mode="always")["passes"] == 2
    r = np.random.default_rng(3).standard_normal(n)                       # a generic w keeps most of its norm: one pass
    assert L.gmres_ortho_probe(wgt, V, r, mode="ifneeded")["passes"] == 1
    _record("second_pass n%d" % n, lines)


# ---------------------------------------------------------------------------------------------------------------- drivers and their references
class _Ctx(P._Ctx):
    def history(self, key, kdim, b=None, kmax=G.K_MAX, **kw):
        """the GMRES(kdim) reference history of right-hand side b, computed once under (key, kdim) and never changed"""
        hk = (key, kdim, tuple(kw.get("orders", G.ORDERS)))
        if hk not in self.hist:
            self.hist[hk] = G.History(self.ld, self.b if b is None else b, kdim, kmax=kmax, seeds=SEEDS, apply64=self.f64, ess=self.ess, dinv=self.dinv, **kw)
        return self.hist[hk]


_ctxs = {}


def _ctx(*a, **kw):
    key = (a, tuple(sorted(kw.items())))
    if key not in _ctxs:
        _ctxs[key] = _Ctx(*a, **kw)
    return _ctxs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_drivers():
    yield
    for c in _ctxs.values():
        c.d.close()
    _ctxs.clear()


def _check(c, h, k, res, m, flag, what, lines, ess=None, red_hist=None):
    """column m of a gmres_solve result against iterate k of the reference history h: count, flag, restarts, x within tol_x(k), essential entries
    exactly 0, the reported reduction within 100 x its sensitivity (red_hist: the history whose sensitivity of the reduction applies, h itself
    unless given)"""
    tol_red = (h if red_hist is None else red_hist).tol_red(k)
    x = res["x"][m]
    want = np.asarray(h.x[k], np.float64)
    dev = float(np.abs(x - want).max() / h.xmax[k])
    red_ref = float(h.red[k])
    red_dev = abs(res["reduction"][m] - red_ref) / red_ref
    ref_line = "   reference " + h.describe(k)
    if ref_line not in lines:
        _say(lines, ref_line)
    _say(lines, "%s: count %d (reference %d), flag %d, restarts %d (reference %d), second passes %d, |x - x_k| %.2e of max |x_k| (tol_x %.2e), reduction %.6e off by %.2e (tolerance %.2e), beta0 off by %.1e"
         % (what, res["iters"][m], k, res["flags"][m], res["restarts"][m], h.restarts(k), res["reorth_passes"][m], dev, h.tol_x(k), res["reduction"][m], red_dev, tol_red,
            abs(res["beta0"][m] - float(h.res[0])) / float(h.res[0])))
    assert res["iters"][m] == k, (what, res["iters"][m], k)
    assert res["flags"][m] == flag, (what, res["flags"][m], flag)
    assert res["restarts"][m] == h.restarts(k), (what, res["restarts"][m], h.restarts(k))
    assert h.x_ok(k), (what, "an iterate off by one could pass at this k", h.describe(k))
    assert dev <= h.tol_x(k), (what, dev, h.tol_x(k))
    assert not x[c.ess if ess is None else ess].any(), (what, "essential entries of x moved")
    assert red_dev <= tol_red, (what, red_dev, tol_red)


def _centred(h, prefer=None):
    k, rel = h.choose(prefer)
    assert 1 <= k <= 25 and h.bn[k] <= G.GAP * h.bn[:k].min() and h.sens_bn[k] <= 1e-6
    assert h.tol_x(k) == max(G.X_FACTOR * h.sens_x[k], G.X_FLOOR) and h.tol_x(k) <= G.STEP_FRACTION * h.step[k] / h.xmax[k]
    return k, rel


PRECOND = pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])


@PRECOND
def test_unrestarted_caps_and_stop(jacobi):
    """N = 3, 192 unknowns, GMRES(30): caps 1, 3, 4, 5, 8 (either side of a poll) and chunk + 1, chunk + 2 (the multi-dot's second chunk begins),
    and one centred stop"""
    c = _ctx(3, jacobi=jacobi)
    ch = c.d.krylov_info()["multidot_chunk"]
    assert ch == _chunk()
    h = c.history("b", 30)
    lines = []
    _say(lines, "%s: %d dofs, %d essential, multi-dot chunk %d" % (c.name, c.nd, c.ess.sum(), ch))
    for m in (1, 3, 4, 5, 8, ch + 1, ch + 2):
        res = c.d.gmres_solve(c.b, 0.0, 0.0, m, 30, check_every=CE)
        _check(c, h, m, res, 0, G.MAX_ITER, "cap %d" % m, lines)
    k, rel = _centred(h)
    res = c.d.gmres_solve(c.b, rel, 0.0, 200, 30, check_every=CE)
    _check(c, h, k, res, 0, G.CONVERGED, "centred stop, rel_tol %.9e" % rel, lines)
    res = c.d.gmres_solve(c.b, 0.0, float(np.sqrt(h.threshold(k))), 200, 30, check_every=CE)
    _check(c, h, k, res, 0, G.CONVERGED, "abs_tol governs", lines)
    z = c.d.gmres_solve(np.zeros(c.nd), 1e-8, 0.0, 50, 30)
    assert z["iters"][0] == 0 and z["flags"][0] == G.CONVERGED and not z["x"].any() and z["reduction"][0] == 0.0
    z = c.d.gmres_solve(c.b, 0.0, 0.0, 0, 30)
    assert z["iters"][0] == 0 and z["flags"][0] == G.MAX_ITER and not z["x"].any()
    _record("unrestarted N3 %s" % ("jacobi" if jacobi else "identity"), lines)


@PRECOND
def test_restarted_caps_and_stop(jacobi):
    """N = 3, GMRES(5): caps 4, 5, 6 and 10, 11 (either side of the first and the second restart) and a centred stop after the second restart"""
    c = _ctx(3, jacobi=jacobi)
    h = c.history("b", 5)
    lines = []
    _say(lines, "%s, GMRES(5): admissible stops %s" % (c.name, h.admissible()))
    for m in (4, 5, 6, 10, 11):
        res = c.d.gmres_solve(c.b, 0.0, 0.0, m, 5, check_every=CE)
        _check(c, h, m, res, 0, G.MAX_ITER, "cap %d" % m, lines)
    k, rel = _centred(h, 13)
    assert 11 <= k <= 15, k
    res = c.d.gmres_solve(c.b, rel, 0.0, 200, 5, check_every=CE)
    _check(c, h, k, res, 0, G.CONVERGED, "centred stop after the second restart, rel_tol %.9e" % rel, lines)
    assert res["restarts"][0] == 2
    _record("restarted N3 %s" % ("jacobi" if jacobi else "identity"), lines)


def test_p2_element_assembly():
    """N = 2, p = 2, element assembly (375 unknowns): GMRES(30) and GMRES(5), a cap on each side of the first restart and a centred stop"""
    c = _ctx(2, p=2, assembly=1)
    lines = []
    _say(lines, "%s: %d dofs, %d essential" % (c.name, c.nd, c.ess.sum()))
    for kdim, caps, kmax in ((30, (30, 31), 31), (5, (5, 6), G.K_MAX)):
        h = c.history("b", kdim, kmax=kmax)
        for m in caps:
            res = c.d.gmres_solve(c.b, 0.0, 0.0, m, kdim, check_every=CE)
            _check(c, h, m, res, 0, G.MAX_ITER, "GMRES(%d) cap %d" % (kdim, m), lines)
        k, rel = _centred(h)
        res = c.d.gmres_solve(c.b, rel, 0.0, 200, kdim, check_every=CE)
        _check(c, h, k, res, 0, G.CONVERGED, "GMRES(%d) centred stop" % kdim, lines)
    _record("p2 EA N2", lines)


@pytest.mark.parametrize("mode", ["ifneeded", "always", "never", "mgs", None], ids=["ifneeded", "always", "never", "mgs", "unset"])
def test_every_orthogonalisation(mode):
    """N = 3, Jacobi: each value of EXA_GMRES_ORTHO (and the variable unset) against the reference's iterate at the centred stop of GMRES(30) and at a
    cap of 9 under GMRES(5); second passes: every step under 'always', none under 'never' and 'mgs'.

    One deviation from the common tolerances, for 'never' and for the reported reduction alone.  The common sensitivity comes from float64 reruns in
    the two stable orders, modified Gram-Schmidt and Gram-Schmidt with a second pass.  One pass of classical Gram-Schmidt loses orthogonality faster
    than either, and the residual norm the rotations carry is only as good as the basis is orthonormal: that is a property of the method the switch
    selects, not of its kernels.  So the reduction a 'never' solve reports is held to 100 x the sensitivity of float64 reruns in its own order
    (gmres_reference order "cgs1", the same permutations), which the test prints beside the common one.  x, count, flag and restarts of 'never'
    stay at the common tolerances, and the other four cases are untouched."""
    c = _ctx(3, jacobi=True)
    h = c.history("b", 30)
    k, rel = _centred(h)
    h5 = c.history("b", 5)
    lines = []
    own30 = own5 = None
    if mode == "never":
        own30, own5 = c.history("b", 30, orders=("cgs1",)), c.history("b", 5, orders=("cgs1",))
        _say(lines, "one pass: sensitivity of the reduction in its own order %.2e at k = %d (stable orders %.2e), GMRES(5) at k = 9 %.2e (%.2e)"
             % (own30.sens_red[k], k, h.sens_red[k], own5.sens_red[9], h5.sens_red[9]))
    with _Env(EXA_GMRES_ORTHO=mode):
        res = c.d.gmres_solve(c.b, rel, 0.0, 200, 30, check_every=CE)
        cap = c.d.gmres_solve(c.b, 0.0, 0.0, 9, 5, check_every=CE)
    if mode == "always":
        assert res["reorth_passes"][0] == res["iters"][0] and cap["reorth_passes"][0] == 9
    if mode in ("never", "mgs"):
        assert res["reorth_passes"][0] == 0 and cap["reorth_passes"][0] == 0
    _check(c, h5, 9, cap, 0, G.MAX_ITER, "EXA_GMRES_ORTHO=%s, GMRES(5) cap 9" % mode, lines, red_hist=own5)
    _check(c, h, k, res, 0, G.CONVERGED, "EXA_GMRES_ORTHO=%s" % mode, lines, red_hist=own30)
    _record("orthogonalisation %s N3 jacobi" % mode, lines)


def test_orthogonalisation_argument():
    """the probe's ortho argument wins over the environment; a value that is none of the four is refused"""
    c = _ctx(3, jacobi=True)
    h = c.history("b", 30)
    k, rel = _centred(h)
    lines = []
    with _Env(EXA_GMRES_ORTHO="never"):
        a = c.d.gmres_solve(c.b, rel, 0.0, 200, 30, ortho="always")
    _check(c, h, k, a, 0, G.CONVERGED, "ortho argument always under EXA_GMRES_ORTHO=never", lines)
    assert a["reorth_passes"][0] == k
    with _Env(EXA_GMRES_ORTHO="gram"):
        with pytest.raises(RuntimeError, match="EXA_GMRES_ORTHO"):
            c.d.gmres_solve(c.b, rel, 0.0, 200, 30)


def test_multigrid():
    """N = 4 under one V-cycle per application, against the reference with the dense M^-1 (precond_apply on unit vectors, as
    test_gpu_pcg_reference.test_multigrid_loop): one cap and one centred stop"""
    import exaconstit_amd.lib as L
    N = 4
    d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:1], **TIGHT)
    d.set_preconditioner("multigrid")
    assert d.step(1)
    before = _probed(d)
    d.mg_setup()
    c = _Ctx.__new__(_Ctx)
    c.d, c.N, c.jacobi, c.nd, c.hist, c.name = d, N, False, 3 * d.nodal_field("coords").shape[0], {}, "N = 4, p = 1, PA, multigrid"
    c.K = _dense_K(d, c.nd)
    c.ess = np.diag(c.K) == 0.0
    Minv = np.zeros((c.nd, c.nd))
    e = np.zeros(c.nd)
    for j in range(c.nd):
        e[:] = 0.0; e[j] = 1.0
        Minv[:, j] = d.precond_apply(e)
    c.dinv = None
    c.ld, c.f64 = P.R.dense_apply(c.K)
    c.b = c.rhs(1)
    h = c.history("b", 30, Minv=np.asarray(Minv, LD))
    lines = []
    _say(lines, c.name)
    res = d.gmres_solve(c.b, 0.0, 0.0, 5, 30, check_every=CE)
    _check(c, h, 5, res, 0, G.MAX_ITER, "cap 5", lines)
    k, rel = _centred(h)
    res = d.gmres_solve(c.b, rel, 0.0, 200, 30, check_every=CE)
    _check(c, h, k, res, 0, G.CONVERGED, "centred stop", lines)
    assert _probed(d) == before
    d.close()
    _record("multigrid N4", lines)


@PRECOND
def test_two_loopback_ranks(jacobi):
    """N = 3 on two loopback ranks (the set-up of test_gpu_pcg_reference.test_two_loopback_ranks): the all-reduce of a column sits between the sums of
    the table and the scalar stage.  A cap of 5 ends the solve one iteration into a chunk of 4; a centred stop.  Both ranks report the same count,
    flag and reduction; x against the one-system reference on the global dense operator."""
    import exaconstit_amd.lib as L
    N, nranks = 3, 2
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    part = [L.partition_nodes(N, r, nranks)[0] for r in range(nranks)]
    NN = L.partition_nodes(N, 0, nranks)[1]
    ND = 3 * NN
    gdof = [np.concatenate([p + NN * comp for comp in range(3)]) for p in part]
    drivers = [None] * nranks

    def create(r):
        d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:1], jacobi=jacobi, rank=r, nranks=nranks, uid=gid, **TIGHT)
        drivers[r] = d
        if not d.step(1):
            raise RuntimeError("rank %d: Newton failed" % r)
        rows = np.zeros((len(gdof[r]), ND))
        for j0 in range(0, ND, 16):
            nb = min(16, ND - j0)
            Xg = np.zeros((nb, ND)); Xg[np.arange(nb), j0 + np.arange(nb)] = 1.0
            rows[:, j0:j0 + nb] = d.grad_apply_columns(Xg[:, gdof[r]], assembled=True).T
        return rows, _probed(d)

    made = _on_ranks(nranks, create)
    K = np.full((ND, ND), np.nan)
    K[gdof[0], :] = made[0][0]
    K[gdof[1], :] = made[1][0]
    assert not np.isnan(K).any()
    inv = [np.full(ND, -1) for _ in range(nranks)]
    for r in range(nranks):
        inv[r][gdof[r]] = np.arange(len(gdof[r]))
    shared = np.where((inv[0] >= 0) & (inv[1] >= 0))[0]
    c = _Ctx.__new__(_Ctx)
    c.N, c.jacobi, c.nd, c.hist, c.K = N, jacobi, ND, {}, K
    c.name = "N = 3 on two loopback ranks, %s" % ("Jacobi" if jacobi else "identity")
    c.ess = np.diag(K) == 0.0
    c.dinv = P.R.jacobi_dinv(K, c.ess) if jacobi else None
    c.ld, c.f64 = P.R.dense_apply(K)
    c.b = c.rhs(1)
    h = c.history("b", 30)
    k, rel = _centred(h)
    lines = []
    _say(lines, "%s: %d global dofs, %d on shared nodes; rel_tol %.9e" % (c.name, ND, len(shared), rel))
    runs = [("stop", rel, 200), ("cap 5", 0.0, 5)]

    def solve(r):
        return [drivers[r].gmres_solve(c.b[gdof[r]], rl, 0.0, mi, 30, check_every=CE) for _, rl, mi in runs]

    got = _on_ranks(nranks, solve)
    for i, (name, rl, mi) in enumerate(runs):
        a, b2 = got[0][i], got[1][i]
        kk, flag = (k, G.CONVERGED) if name == "stop" else (mi, G.MAX_ITER)
        assert a["iters"][0] == b2["iters"][0] and a["flags"][0] == b2["flags"][0] and a["reduction"][0] == b2["reduction"][0]
        for r, got_r in ((0, a), (1, b2)):
            xg = np.asarray(h.x[kk], np.float64).copy()      # the other rank's part: the reference itself
            xg[gdof[r]] = got_r["x"][0]
            res = dict(got_r); res["x"] = xg[None, :]
            _check(c, h, kk, res, 0, flag, "rank %d, %s" % (r, name), lines)
    after = _on_ranks(nranks, lambda r: _probed(drivers[r]))
    assert [m[1] for m in made] == after
    _on_ranks(nranks, lambda r: drivers[r].close())
    L.exa_loopback_group_destroy(gid)
    _record("two_ranks N3 %s" % ("jacobi" if jacobi else "identity"), lines)


def test_same_bits_in_every_run():
    """EXA_DETERMINISTIC=1: two gmres_solve calls on one driver return identical bits, stop and cap"""
    c = _ctx(3, jacobi=True, det=True, dense=False)
    b = np.random.default_rng(11).standard_normal(c.nd)
    for args in ((1e-6, 0.0, 200, 30), (0.0, 0.0, 12, 5)):
        a1 = c.d.gmres_solve(b, *args, check_every=CE)
        a2 = c.d.gmres_solve(b, *args, check_every=CE)
        assert np.array_equal(a1["x"], a2["x"]) and a1["iters"][0] == a2["iters"][0] and a1["reduction"][0] == a2["reduction"][0] and a1["resid"][0] == a2["resid"][0]
        assert a1["iters"][0] > 0 and a1["x"].any()


def test_refusals():
    import exaconstit_amd.lib as L
    d = L.Driver.synthetic(3, _props(), hipref.random_quats(27).ravel(), DTS[:1], **TIGHT)
    nd = 3 * d.nodal_field("coords").shape[0]
    with pytest.raises(RuntimeError, match="no solved step"):
        d.gmres_solve(np.ones(nd), 1e-8, 0.0, 10, 30)
    assert d.step(1)
    for kdim in (0, 101):
        with pytest.raises(RuntimeError, match="gmres_kdim"):
            d.gmres_solve(np.ones(nd), 1e-8, 0.0, 10, kdim)
        with pytest.raises(RuntimeError, match="gmres_kdim"):
            d.set_krylov("gmres", kdim=kdim)
    with pytest.raises(RuntimeError, match="pcg"):
        d.set_krylov("minres")
    with pytest.raises(RuntimeError, match="1 to 16 columns"):
        d.gmres_solve(np.ones((17, nd)), 1e-8, 0.0, 10, 30)
    assert d.krylov_info()["solver"] == "pcg" and d.krylov_info()["kdim"] == 0
    d.close()


def test_switching_the_solver_keeps_the_runs_counters():
    """set_krylov between two steps: diagnostics() and timers() of the run go on counting across the switch, in both directions"""
    import exaconstit_amd.lib as L
    d = L.Driver.synthetic(3, _props(), hipref.random_quats(27).ravel(), DTS[:3], jacobi=True, newton=TIGHT["newton"], krylov=(20, 1e-12, 1e-30))
    assert d.step(1)                                     # a cap of 20: every solve stops at it and is counted
    t1, g1 = d.timers(), d.diagnostics()
    assert t1["krylov_iters"] > 0 and g1["pcg_not_converged"] > 0 and g1["pcg_worst_capped_reduction"] > 0.0
    d.set_krylov("gmres", kdim=30)
    assert d.timers()["krylov_iters"] == t1["krylov_iters"] and d.diagnostics() == g1 and d.krylov_info()["restarts"] == 0
    assert d.step(2)
    t2, g2 = d.timers(), d.diagnostics()
    assert t2["krylov_iters"] > t1["krylov_iters"] and g2["pcg_not_converged"] > g1["pcg_not_converged"]
    assert g2["pcg_worst_capped_reduction"] >= g1["pcg_worst_capped_reduction"]
    d.set_krylov("pcg")
    assert d.timers()["krylov_iters"] == t2["krylov_iters"] and d.diagnostics() == g2 and d.krylov_info()["solver"] == "pcg"
    d.close()


# ---------------------------------------------------------------------------------------------------------------- the run
def _rows_close(a, b, yard, what, lines):
    """stress rows a and b within 100 x the yardstick (the difference of two PCG runs at Krylov rel_tol 1e-12 and 1e-13), relative to the largest
    entry, with the floor 1e-12"""
    big = np.abs(a).max()
    dev = np.abs(a - b).max() / big
    tol = 100.0 * max(yard, 1e-12)
    _say(lines, "%s: GMRES against PCG %.2e of the largest entry; PCG at 1e-12 against PCG at 1e-13 %.2e; tolerance %.2e" % (what, dev, yard, tol))
    assert dev <= tol, (what, dev, tol)


def _run(make, nsteps, gmres_kdim=None):
    d = make()
    if gmres_kdim:
        d.set_krylov("gmres", kdim=gmres_kdim)
    for ti in range(1, nsteps + 1):
        assert d.step(ti), ti
    out = dict(avg=d.avgs(0, 6), newton=[int(v) for v in d.stats()[0]], krylov=[int(v) for v in d.stats()[1]], diag=d.diagnostics(), info=d.krylov_info(), timers=d.timers())
    d.close()
    return out


def _pair(make_at, nsteps, what, lines, kdim=30):
    """PCG at 1e-12, PCG at 1e-13 and GMRES at 1e-12 on the same steps"""
    p12, p13, g12 = _run(lambda: make_at(1e-12), nsteps), _run(lambda: make_at(1e-13), nsteps), _run(lambda: make_at(1e-12), nsteps, kdim)
    yard = np.abs(p12["avg"] - p13["avg"]).max() / np.abs(p12["avg"]).max()
    _say(lines, "%s: Newton %s, Krylov iterations PCG %s GMRES(%d) %s, restarts %d, second passes %d, basis %d bytes"
         % (what, g12["newton"], p12["krylov"], kdim, g12["krylov"], g12["info"]["restarts"], g12["info"]["reorth_passes"], g12["info"]["basis_bytes"]))
    assert g12["newton"] == p12["newton"]
    assert g12["diag"]["pcg_not_converged"] == 0 and p12["diag"]["pcg_not_converged"] == 0 and g12["diag"]["pcg_indefinite_iters"] == 0
    assert g12["info"]["solver"] == "gmres" and g12["info"]["kdim"] == kdim and p12["info"]["solver"] == "pcg"
    assert g12["timers"]["krylov_iters"] > 0 and g12["info"]["basis_bytes"] > 0
    _rows_close(g12["avg"], p12["avg"], yard, what, lines)


def test_run_under_gmres():
    """Driver.synthetic(4, ..., jacobi) over three steps as it is and after set_krylov("gmres", kdim=30): every step converges, the same Newton
    counts, the volume-average stress rows agree"""
    import exaconstit_amd.lib as L
    lines = []

    def make_at(rel):
        return L.Driver.synthetic(4, _props(), hipref.random_quats(64).ravel(), DTS[:3], jacobi=True, newton=TIGHT["newton"], krylov=(20000, rel, 1e-30))
    _pair(make_at, 3, "N = 4, Jacobi, three steps", lines)
    _record("run N4 jacobi", lines)


def test_run_under_gmres_periodic_mixed():
    """the same pair on a periodic cell with free xx and yy (mixed loading): the control entries are unknowns of the Krylov solver; the second step is
    plastic"""
    import exaconstit_amd.lib as L
    lines = []
    LZ, FREE_XY = np.diag([0.0, 0.0, 1.0e-3]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]])

    def make_at(rel):
        d = L.Driver.synthetic(4, _props(), hipref.random_quats(64, seed=16).ravel(), np.array([0.4, 0.4]), jacobi=True, newton=TIGHT["newton"], krylov=(20000, rel, 1e-30))
        d.set_periodic(LZ, FREE_XY)
        return d
    _pair(make_at, 2, "N = 4 periodic, free xx yy, two steps", lines)
    _record("run N4 periodic mixed", lines)


def test_options_file_with_gmres(tmp_path):
    """voce_pa.toml with solver = "GMRES" and gmres_kdim = 20, two steps, against the file as it is (both with the Krylov rel_tol at 1e-12)"""
    import exaconstit_amd.lib as L
    text = open(os.path.join(REF, "voce_pa.toml")).read()
    for fl in os.listdir(REF):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    assert 'solver = "PCG"' in text and "rel_tol = 1e-7" in text
    lines = []

    def variant(tag, rel, gm):
        t = text.replace("rel_tol = 1e-7", "rel_tol = %g" % rel)
        if gm:
            t = t.replace('solver = "PCG"', 'solver = "GMRES"\n        gmres_kdim = 20')
        p = tmp_path / (tag + ".toml")
        p.write_text(t)
        return lambda: L.Driver.from_toml(str(p), out_dir=str(tmp_path), write_files=False)

    p12, p13, g12 = _run(variant("p12", 1e-12, False), 2), _run(variant("p13", 1e-13, False), 2), _run(variant("g12", 1e-12, True), 2)
    yard = np.abs(p12["avg"] - p13["avg"]).max() / np.abs(p12["avg"]).max()
    _say(lines, "voce_pa.toml: Newton %s, Krylov iterations PCG %s GMRES(20) %s, restarts %d" % (g12["newton"], p12["krylov"], g12["krylov"], g12["info"]["restarts"]))
    assert g12["info"]["solver"] == "gmres" and g12["info"]["kdim"] == 20 and p12["info"]["solver"] == "pcg"
    assert g12["newton"] == p12["newton"] and g12["diag"]["pcg_not_converged"] == 0
    _rows_close(g12["avg"], p12["avg"], yard, "voce_pa.toml, two steps", lines)
    _record("options file voce_pa", lines)


def test_zz_every_probed_driver_is_as_it_was():
    """after all probe calls of this module, each of its drivers reports the stats(), diagnostics() and timers()["krylov_iters"] it had before them"""
    for c in _ctxs.values():
        assert _probed(c.d) == c.before, c.name
