"""Every PCG loop of host/krylov.hip against a reference conjugate-gradient solve computed elsewhere (tests/pcg_reference.py: a numpy transcription of
MFEM's CGSolver::Mult in long double).  Driver.pcg_solve hands a loop a right-hand side; what comes back - iterates, iteration count, flag, reported
reduction - is compared with the reference at the same iteration.

Set-up: Driver.synthetic with the tight Newton and Krylov options of tests/test_gpu_macro_tangent.py, one solved step; the dense K_uu probed through
grad_apply_columns(assembled=True, batched=False), 16 unit columns per call; b a seeded random vector with zero essential entries; Jacobi: 1 / diag(K_uu)
on the free rows, 1 on the essential ones; check_every = 4 throughout, so that 25 iterations span several chunks.

No tolerance is a fixed number.  The reference is run a second time in float64 with the addends of its dot products permuted (several permutations); how
far that moves (r_k, z_k), the reduction and x_k is the reference's own sensitivity at iteration k.  x must be within tol_x(k) = max(100 x sensitivity of
x_k, 1e-13) of max |x_k|, the reduction within 100 x its sensitivity (the 100 covers a summation order on the GPU that is neither of the CPU's, with
atomics in the action).  Stopping iterations come from the chooser: the threshold is the geometric mean of (r_k, z_k) and the smallest earlier value,
which must be at least 25 % larger, so a right solver stops exactly at k; and tol_x(k) is at most 1 % of the step x_k - x_(k-1), so an iterate off by
one can never pass.  Every test prints what it chose and measured; EXA_WRITE_RECORDS=1 keeps the lines in profiles/pcg_checks.txt."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hipref
import pcg_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
DTS = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()
TIGHT = dict(newton=(50, 1e-10, 1e-14), krylov=(20000, 1e-12, 1e-30))      # tests/test_gpu_macro_tangent.py
RECORD = os.path.join(ROOT, "profiles", "pcg_checks.txt")
CE = 4                                                                      # check_every of every probe call
CAPS = (1, 3, 4, 5, 8)
SEEDS = (1, 2, 3, 4, 5)                                                     # permutations behind a sensitivity


def _say(lines, text):
    """one measured line: printed at once (a failing assertion must not swallow it) and kept for _record"""
    print(text)
    lines.append(text)


def _record(key, lines):
    """the lines a test printed: with EXA_WRITE_RECORDS=1 kept in profiles/pcg_checks.txt as the block '[key]'"""
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


def _props():
    return np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()


# ---------------------------------------------------------------------------------------------------------------- drivers and their references
class _Env:
    """environment variables for the length of a with-block (the solver reads its switches per solve, the routes per driver)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _probed(d):
    return dict(stats=[list(x) for x in d.stats()], diag=d.diagnostics(), krylov_iters=d.timers()["krylov_iters"])


def _dense_K(d, nd):
    K = np.zeros((nd, nd))
    for j0 in range(0, nd, 16):
        nb = min(16, nd - j0)
        X = np.zeros((nb, nd)); X[np.arange(nb), j0 + np.arange(nb)] = 1.0
        K[:, j0:j0 + nb] = d.grad_apply_columns(X, assembled=True, batched=False).T
    return K


class _Ctx:
    """a synthetic driver after one solved step, the dense K_uu of that state, its essential set, the base right-hand side and the reference histories"""

    def __init__(self, N, p=1, assembly=0, jacobi=False, det=False, dense=True, nsteps=1):
        import exaconstit_amd.lib as L
        self.N, self.p, self.jacobi, self.det = N, p, jacobi, det
        self.name = "N = %d, p = %d, %s, %s%s" % (N, p, "EA" if assembly else "PA", "Jacobi" if jacobi else "identity", ", deterministic" if det else "")
        with _Env(EXA_DETERMINISTIC="1" if det else None):
            self.d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3).ravel(), DTS[:nsteps], assembly=assembly, jacobi=jacobi, order=p, **TIGHT)
        assert self.d.step(1), "Newton failed"
        dg = self.d.diagnostics()
        assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0, dg
        self.before = _probed(self.d)
        self.nd = 3 * self.d.nodal_field("coords").shape[0]
        self.hist = {}
        if not dense:
            return
        self.K = _dense_K(self.d, self.nd)
        self.ess = np.diag(self.K) == 0.0
        assert 0 < self.ess.sum() < self.nd // 2 and not self.K[self.ess, :].any() and not self.K[:, self.ess].any()
        assert np.all(np.diag(self.K)[~self.ess] > 0.0)
        self.dinv = R.jacobi_dinv(self.K, self.ess) if jacobi else None
        self.ld, self.f64 = R.dense_apply(self.K)
        self.b = self.rhs(1)

    def rhs(self, seed):
        b = np.random.default_rng(1000 * self.N + seed).standard_normal(self.nd)
        b[self.ess] = 0.0
        return b

    def history(self, key, b=None, kmax=R.K_MAX):
        """the reference history of right-hand side b, computed once under `key` and never changed"""
        if key not in self.hist:
            self.hist[key] = R.History(self.ld, self.b if b is None else b, kmax=kmax, seeds=SEEDS, apply64=self.f64, ess=self.ess, dinv=self.dinv)
        return self.hist[key]


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


def _check(c, h, k, res, m, flag, what, lines, scale=1.0):
    """column m of a probe result against iterate k of the reference history h (scaled by `scale` for a right-hand side scaled so): count, flag, x within tol_x(k),
    essential entries exactly 0, the reported reduction within 100 x its sensitivity.  Returns the deviation of x."""
    x = res["x"][m]
    want = np.asarray(h.x[k] * np.longdouble(scale), np.float64)
    xmax = h.xmax[k] * abs(scale)
    dev = float(np.abs(x - want).max() / xmax) if xmax > 0 else float(np.abs(x).max())
    red_ref = float(h.red[k])
    red_dev = abs(res["reduction"][m] - red_ref) / red_ref if red_ref > 0 else abs(res["reduction"][m])
    ref_line = "   reference " + h.describe(k)           # the reference's figures at this iterate: once per test
    if ref_line not in lines:
        _say(lines, ref_line)
    _say(lines, "%s: count %d (reference %d), flag %d, |x - x_k| %.2e of max |x_k| (tol_x %.2e), reduction %.6e off by %.2e (tolerance %.2e), (r0, z0) off by %.1e, last (r, z) off by %.1e"
         % (what, res["iters"][m], k, res["flags"][m], dev, h.tol_x(k), res["reduction"][m], red_dev, h.tol_red(k),
            abs(res["r0z0"][m] / (scale * scale) - float(h.bn[0])) / float(h.bn[0]), abs(res["rz"][m] / (scale * scale) - float(h.bn[k])) / float(h.bn[k])))
    assert res["iters"][m] == k, (what, res["iters"][m], k)
    assert res["flags"][m] == flag, (what, res["flags"][m], flag)
    assert res["indefinite"][m] == 0
    assert h.x_ok(k), (what, "an iterate off by one could pass at this k", h.describe(k))
    assert dev <= h.tol_x(k), (what, dev, h.tol_x(k))
    assert not x[c.ess].any(), (what, "essential entries of x moved")
    assert red_dev <= h.tol_red(k), (what, red_dev, h.tol_red(k))
    return dev


def _centred(h, prefer=None):
    """the chooser's pick with its conditions asserted"""
    k, rel = h.choose(prefer)
    assert 1 <= k <= 25 and h.bn[k] <= 0.8 * h.bn[:k].min() and h.sens_bn[k] <= 1e-6
    assert h.tol_x(k) == max(100.0 * h.sens_x[k], 1e-13) and h.tol_x(k) <= 0.01 * h.step[k] / h.xmax[k]
    return k, rel


SHAPES = [(3, 1, 0), (7, 1, 0), (2, 2, 0), (3, 1, 1)]
SHAPE_IDS = ["N3", "N7", "N2p2", "N3EA"]
PRECOND = pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])


# ---------------------------------------------------------------------------------------------------------------- a. threshold-centred stop
@PRECOND
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_threshold_centred_stop(shape, jacobi):
    """192 dofs (one partial block), 1536 dofs (six blocks of partial sums), 375 dofs at p = 2, and element assembly at N = 3: the solve stops at the
    chooser's k with CONVERGED, x_k, zero essential entries and the reference's reduction; e. the same count when abs_tol carries the threshold"""
    N, p, asm = shape
    c = _ctx(N, p=p, assembly=asm, jacobi=jacobi)
    h = c.history("b")
    k, rel = _centred(h)
    lines = []
    _say(lines, "%s: %d dofs, %d essential; rel_tol %.9e" % (c.name, c.nd, c.ess.sum(), rel))
    res = c.d.pcg_solve(c.b, rel, 0.0, 200, check_every=CE)
    _check(c, h, k, res, 0, R.CONVERGED, "a. centred stop", lines)
    res = c.d.pcg_solve(c.b, 0.0, np.sqrt(h.threshold(k)), 200, check_every=CE)
    _check(c, h, k, res, 0, R.CONVERGED, "e. abs_tol governs", lines)
    _record("a_e_centred_stop %s %s" % (SHAPE_IDS[SHAPES.index(shape)], "jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- b. route matrix
ROUTES = [(g, r) for g in (False, True) for r in (None, "1")]


def _route_name(g, r):
    return "graph %s, %s" % ("on" if g else "off", "reduction launches" if r else "consumer-side reductions")


@PRECOND
@pytest.mark.parametrize("N", [3, 7])
def test_route_matrix(N, jacobi):
    """graph replay on / off x EXA_PCG_REDUCE_LAUNCH unset / 1 (consumer-side reductions, whose count travels in ITERS_NEXT, or the one-block reduction
    launches): each against the reference; under EXA_DETERMINISTIC=1 the four give the same bits of x and the same count"""
    c = _ctx(N, jacobi=jacobi)
    h = c.history("b")
    k, rel = _centred(h)
    lines = []
    _say(lines, "%s: rel_tol %.9e" % (c.name, rel))
    for g, r in ROUTES:
        with _Env(EXA_PCG_REDUCE_LAUNCH=r):
            res = c.d.pcg_solve(c.b, rel, 0.0, 200, check_every=CE, graph=g)
        _check(c, h, k, res, 0, R.CONVERGED, "b. " + _route_name(g, r), lines)
    cd = _ctx(N, jacobi=jacobi, det=True, dense=False)
    got = []
    for g, r in ROUTES:
        with _Env(EXA_PCG_REDUCE_LAUNCH=r):
            got.append(cd.d.pcg_solve(c.b, rel, 0.0, 200, check_every=CE, graph=g))
            got.append(cd.d.pcg_solve(c.b, 0.0, 0.0, 5, check_every=CE, graph=g))      # (and the cap one iteration into the second chunk)
    for a in got[2::2]:
        assert np.array_equal(a["x"], got[0]["x"]) and a["iters"][0] == got[0]["iters"][0] == k and a["flags"][0] == got[0]["flags"][0] == R.CONVERGED
        assert a["reduction"][0] == got[0]["reduction"][0] and a["rz"][0] == got[0]["rz"][0]
    for a in got[3::2]:
        assert np.array_equal(a["x"], got[1]["x"]) and a["iters"][0] == got[1]["iters"][0] == 5 and a["flags"][0] == got[1]["flags"][0] == R.MAX_ITER
        assert a["reduction"][0] == got[1]["reduction"][0]
    dev = np.abs(got[0]["x"][0] - np.asarray(h.x[k], np.float64)).max() / h.xmax[k]
    assert dev <= h.tol_x(k)
    _say(lines, "deterministic mode: the four routes give the same bits of x, count %d and reduction; |x - x_k| %.2e of max |x_k|" % (k, dev))
    _record("b_route_matrix N%d %s" % (N, "jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- c. cap
@PRECOND
@pytest.mark.parametrize("N", [3, 7])
def test_cap(N, jacobi):
    """rel_tol = abs_tol = 0, max_iter = m: m iterations, MAX_ITER, x_m - the replayed chunk of 4 overshoots every cap but 4 and 8 and must do nothing once
    the cap is reached; graph on and off agree"""
    c = _ctx(N, jacobi=jacobi)
    h = c.history("b")
    lines = []
    _say(lines, c.name)
    for m in CAPS:
        xs = []
        for g, r in ROUTES:
            with _Env(EXA_PCG_REDUCE_LAUNCH=r):
                res = c.d.pcg_solve(c.b, 0.0, 0.0, m, check_every=CE, graph=g)
            _check(c, h, m, res, 0, R.MAX_ITER, "c. cap %d, %s" % (m, _route_name(g, r)), lines)
            xs.append(res["x"][0])
        for x in xs[1:]:
            assert np.abs(x - xs[0]).max() <= h.tol_x(m) * h.xmax[m]
    _record("c_cap N%d %s" % (N, "jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- d. stops at chunk edges
def _clustered_rhs(c, seed, width):
    """a combination of `width` neighbouring eigenvectors of the preconditioned operator plus a little of everything: the first step removes most of it"""
    f = ~c.ess
    s = np.sqrt(c.dinv[f]) if c.jacobi else np.ones(f.sum())
    Kff = c.K[np.ix_(f, f)]
    lam, U = np.linalg.eigh(0.5 * (Kff + Kff.T) * s[:, None] * s[None, :])
    rng = np.random.default_rng(seed)
    i0 = rng.integers(0, len(lam) - width)
    u = U[:, i0:i0 + width] @ rng.standard_normal(width) + 0.05 * rng.standard_normal(len(lam)) / np.sqrt(len(lam)) * np.sqrt(width)
    b = np.zeros(c.nd); b[f] = u / s
    return b


@PRECOND
def test_stops_at_chunk_edges(jacobi):
    """N = 3: stops at k = 1 (the first iteration of the first chunk), 4 (the last one) and 5 (the first of the second chunk), each with a right-hand side
    for which the chooser admits that k - random vectors first, then combinations of neighbouring eigenvectors of the dense K_uu"""
    c = _ctx(3, jacobi=jacobi)
    lines = []
    _say(lines, c.name)
    cands = [("random %d" % s, (lambda s=s: c.rhs(s))) for s in (1, 2, 3)] + [("eigenvector cluster %d x %d" % (s, w), (lambda s=s, w=w: _clustered_rhs(c, s, w))) for w in (3, 8, 20) for s in (1, 2)]
    for target in (1, 4, 5):
        for name, make in cands:
            key = "b" if name == "random 1" else "d " + name
            h = c.history(key, make())
            if target in h.admissible():
                break
        else:
            raise AssertionError("no right-hand side among the candidates admits a stop at k = %d" % target)
        k, rel = _centred(h, target)
        assert k == target
        b = c.b if key == "b" else make()
        for g in (False, True):
            res = c.d.pcg_solve(b, rel, 0.0, 200, check_every=CE, graph=g)
            _check(c, h, k, res, 0, R.CONVERGED, "d. stop at %d, %s, graph %s" % (k, name, "on" if g else "off"), lines)
    _record("d_chunk_edges N3 %s" % ("jacobi" if jacobi else "identity"), lines)


@PRECOND
def test_stops_either_side_of_a_chunk_edge_N7(jacobi):
    """N = 7, the base right-hand side: the admissible stops nearest to a chunk edge on either side (k = 4 j and 4 j + 1 where the chooser allows them)"""
    c = _ctx(7, jacobi=jacobi)
    h = c.history("b")
    adm = h.admissible()
    lo = [k for k in adm if k % 4 == 0] or [max(k for k in adm if k <= 4 * (adm[-1] // 4))]
    hi = [k for k in adm if k % 4 == 1 and k > 1] or [min(k for k in adm if k > lo[0])]
    lines = []
    _say(lines, "%s: admissible stops %s" % (c.name, adm))
    for k0 in (lo[0], hi[0]):
        k, rel = _centred(h, k0)
        assert k == k0
        for g in (False, True):
            res = c.d.pcg_solve(c.b, rel, 0.0, 200, check_every=CE, graph=g)
            _check(c, h, k, res, 0, R.CONVERGED, "d. stop at %d, graph %s" % (k, "on" if g else "off"), lines)
    _record("d_chunk_edges N7 %s" % ("jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- f, g. b = 0 and reuse
@PRECOND
@pytest.mark.parametrize("N", [3, 7])
def test_zero_rhs_and_reuse(N, jacobi):
    """one solver object, one solution buffer, columns b, 0, -2 b in turn (the second and third replay the chunk the first captured and start from the
    record it left): each column matches its own reference; the zero column takes no iteration and stays exactly 0 with reduction 0; the third has
    the first's count and -2 x its x"""
    c = _ctx(N, jacobi=jacobi)
    h = c.history("b")
    k, rel = _centred(h)
    lines = []
    _say(lines, "%s: rel_tol %.9e" % (c.name, rel))
    B = np.stack([c.b, np.zeros(c.nd), -2.0 * c.b])
    for g, r in ROUTES:
        with _Env(EXA_PCG_REDUCE_LAUNCH=r):
            res = c.d.pcg_solve(B, rel, 0.0, 200, check_every=CE, graph=g)
            cap = c.d.pcg_solve(B, 0.0, 0.0, 5, check_every=CE, graph=g)
        what = "g. reuse, " + _route_name(g, r)
        _check(c, h, k, res, 0, R.CONVERGED, what + ", b", lines)
        _check(c, h, k, res, 2, R.CONVERGED, what + ", -2 b", lines, scale=-2.0)
        assert res["iters"][2] == res["iters"][0] and np.abs(res["x"][2] + 2.0 * res["x"][0]).max() <= h.tol_x(k) * 2.0 * h.xmax[k]
        _check(c, h, 5, cap, 0, R.MAX_ITER, what + ", cap 5, b", lines)
        _check(c, h, 5, cap, 2, R.MAX_ITER, what + ", cap 5, -2 b", lines, scale=-2.0)
        for z in (res, cap):
            assert z["iters"][1] == 0 and z["flags"][1] == R.CONVERGED and not z["x"][1].any() and z["reduction"][1] == 0.0 and z["r0z0"][1] == 0.0
    _record("f_g_zero_and_reuse N%d %s" % (N, "jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- h. lockstep
def _common_rel(h1, h2):
    """(k1, k2, rel) with k1 != k2 and one rel_tol whose threshold clears both neighbours of both histories by the chooser's 11 %, or None"""
    for k1 in reversed(h1.admissible()):
        for k2 in reversed(h2.admissible()):
            if k1 == k2:
                continue
            lo = max(float(h1.bn[k1] / h1.bn[0]), float(h2.bn[k2] / h2.bn[0])) * 1.11
            hi = min(float(h1.bn[:k1].min() / h1.bn[0]), float(h2.bn[:k2].min() / h2.bn[0])) / 1.11
            if lo < hi:
                return k1, k2, float(np.sqrt(np.sqrt(lo * hi)))
    return None


@pytest.mark.parametrize("N,jacobi", [(3, False), (3, True), (7, False)], ids=["N3-identity", "N3-jacobi", "N7-identity"])
def test_lockstep_columns(N, jacobi):
    """SolveColumns on b, 0, 1e3 b and an unrelated b' that stops elsewhere, with 1, 2 and 3 columns per pass: each column has the count, flag and x of
    its own reference - a column that has stopped does not move while the others go on -, the zero column stays exactly 0"""
    c = _ctx(N, jacobi=jacobi)
    h, h3, h2 = c.history("b"), c.history("1e3 b", 1e3 * c.b), c.history("b'", c.rhs(2))
    lines = []
    _say(lines, c.name)
    common = _common_rel(h, h2)
    if common:
        k, k2, rel = common
        cap, flag2 = 200, R.CONVERGED
        _say(lines, "b' by one rel_tol %.9e admissible for both: b stops at %d, b' at %d" % (rel, k, k2))
        assert all(h2.conditions(k2))
    else:
        # b stops at its centred threshold, b' runs into the cap later: its (r, z) must stay clear of the threshold by the chooser's 11 % up to the cap
        k, rel = _centred(h, 6)
        k2 = next(m for m in range(k + 2, 26) if float(h2.bn[:m + 1].min() / h2.bn[0]) > 1.11 * rel * rel and h2.x_ok(m))
        cap, flag2 = k2, R.MAX_ITER
        _say(lines, "b' by the cap (no single rel_tol admissible for both): rel_tol %.9e stops b at %d, b' runs to the cap %d" % (rel, k, k2))
    assert all(h.conditions(k)) and all(h3.conditions(k))
    thr3 = rel * rel * float(h3.bn[0])
    assert float(h3.bn[k]) * 1.11 <= thr3 <= float(h3.bn[:k].min()) / 1.11
    B = np.stack([c.b, np.zeros(c.nd), 1e3 * c.b, c.rhs(2)])
    for nch in (1, 2, 3):
        c.d.set_tangent_route(nch=nch)
        res = c.d.pcg_solve(B, rel, 0.0, cap, check_every=CE, columns=True)
        what = "h. lockstep, %d per pass" % nch
        _check(c, h, k, res, 0, R.CONVERGED, what + ", b", lines)
        _check(c, h3, k, res, 2, R.CONVERGED, what + ", 1e3 b", lines)
        _check(c, h2, k2, res, 3, flag2, what + ", b'", lines)
        assert res["iters"][1] == 0 and res["flags"][1] == R.CONVERGED and not res["x"][1].any() and res["reduction"][1] == 0.0
    c.d.set_tangent_route(nch=0)
    _record("h_lockstep N%d %s" % (N, "jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- i. multigrid
def test_multigrid_loop():
    """SolveMultigrid at N = 4 against the reference with the dense M^-1 of one V-cycle (precond_apply on unit vectors; linear and symmetric to 1e-12 of
    its largest entry): the centred stop and the caps"""
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
    assert 0 < c.ess.sum() < c.nd // 2
    Minv = np.zeros((c.nd, c.nd))
    e = np.zeros(c.nd)
    for j in range(c.nd):
        e[:] = 0.0; e[j] = 1.0
        Minv[:, j] = d.precond_apply(e)
    big = np.abs(Minv).max()
    v = np.random.default_rng(5).standard_normal(c.nd)
    v /= np.abs(v).sum()                                # M^-1 v is then a combination of the columns with coefficients that sum to 1 in modulus
    lin = np.abs(d.precond_apply(v) - Minv @ v).max()
    sym = np.abs(Minv - Minv.T).max()
    lines = []
    _say(lines, "%s: M^-1 largest entry %.3e, asymmetry %.2e of it, M^-1 v against the dense product (|v|_1 = 1) off by %.2e of it" % (c.name, big, sym / big, lin / big))
    assert sym <= 1e-12 * big and lin <= 1e-12 * big
    c.dinv = None
    c.ld, c.f64 = R.dense_apply(c.K)
    c.b = c.rhs(1)
    Ml = np.asarray(Minv, np.longdouble)
    h = R.History(c.ld, c.b, seeds=SEEDS, apply64=c.f64, ess=c.ess, Minv=Ml)
    k, rel = _centred(h)
    res = d.pcg_solve(c.b, rel, 0.0, 200, check_every=CE)
    _check(c, h, k, res, 0, R.CONVERGED, "i. centred stop", lines)
    res = d.pcg_solve(c.b, 0.0, np.sqrt(h.threshold(k)), 200, check_every=CE)
    _check(c, h, k, res, 0, R.CONVERGED, "i. abs_tol governs", lines)
    for m in CAPS:
        res = d.pcg_solve(c.b, 0.0, 0.0, m, check_every=CE)
        _check(c, h, m, res, 0, R.MAX_ITER, "i. cap %d" % m, lines)
    z = d.pcg_solve(np.zeros(c.nd), 1e-8, 0.0, 50, check_every=CE)
    assert z["iters"][0] == 0 and z["flags"][0] == R.CONVERGED and not z["x"].any() and z["reduction"][0] == 0.0
    assert _probed(d) == before
    d.close()
    _record("i_multigrid N4", lines)


# ---------------------------------------------------------------------------------------------------------------- j. two loopback ranks
def _on_ranks(nranks, fn, timeout=120):
    """fn(r) on one thread per rank (tests/test_gpu_multirank.py); no retry"""
    out, errors = [None] * nranks, []

    def work(r):
        try:
            out[r] = fn(r)
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=timeout) for t in th]
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    return out


@PRECOND
def test_two_loopback_ranks(jacobi):
    """N = 3 on two loopback ranks: the single-reduction loop every multi-rank run uses and the two-reduction branch (EXA_PCG_TWO_REDUCTIONS=1: k_cg_beta /
    k_cg_den behind an all-reduce) against the reference on the global dense operator, which the two drivers build themselves, with unit weights.
    Centred stop and caps; the cap of 5 ends the solve one iteration into a chunk of 4, whose remaining all-reduces must change nothing.  Both ranks
    report the same count, flag and reduction, and the same bits of x on shared nodes."""
    import exaconstit_amd.lib as L
    N, nranks = 3, 2
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    part = [L.partition_nodes(N, r, nranks)[0] for r in range(nranks)]
    NN = L.partition_nodes(N, 0, nranks)[1]
    ND = 3 * NN
    gdof = [np.concatenate([p + NN * comp for comp in range(3)]) for p in part]      # global dof of every local dof (byNODES on both sides)
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
    inv = [np.full(ND, -1) for _ in range(nranks)]
    for r in range(nranks):
        inv[r][gdof[r]] = np.arange(len(gdof[r]))
    shared = np.where((inv[0] >= 0) & (inv[1] >= 0))[0]
    mism = np.abs(made[0][0][inv[0][shared]] - made[1][0][inv[1][shared]]).max() / np.abs(made[0][0]).max()
    assert len(shared) >= 3 * 16 and mism <= 1e-13, mism      # the copies of a shared row: the same halo sum in another order of <= 8 + 8 addends
    K[gdof[1], :] = made[1][0]
    assert not np.isnan(K).any()
    c = _Ctx.__new__(_Ctx)
    c.N, c.jacobi, c.nd, c.hist, c.K = N, jacobi, ND, {}, K
    c.name = "N = 3 on two loopback ranks, %s" % ("Jacobi" if jacobi else "identity")
    c.ess = np.diag(K) == 0.0
    assert 0 < c.ess.sum() < ND // 2 and not K[c.ess, :].any() and not K[:, c.ess].any()
    c.dinv = R.jacobi_dinv(K, c.ess) if jacobi else None
    c.ld, c.f64 = R.dense_apply(K)
    c.b = c.rhs(1)
    h = c.history("b")
    k, rel = _centred(h)
    lines = []
    _say(lines, "%s: %d global dofs, %d on shared nodes (rows agree to %.1e); rel_tol %.9e" % (c.name, ND, len(shared), mism, rel))
    runs = [("stop", rel, 200)] + [("cap %d" % m, 0.0, m) for m in CAPS]

    def solve(r):
        return [drivers[r].pcg_solve(c.b[gdof[r]], rl, 0.0, mi, check_every=CE) for _, rl, mi in runs]

    for two in (None, "1"):
        with _Env(EXA_PCG_TWO_REDUCTIONS=two):
            got = _on_ranks(nranks, solve)
        for i, (name, rl, mi) in enumerate(runs):
            a, b2 = got[0][i], got[1][i]
            kk, flag = (k, R.CONVERGED) if name == "stop" else (mi, R.MAX_ITER)
            assert a["iters"][0] == b2["iters"][0] and a["flags"][0] == b2["flags"][0] and a["reduction"][0] == b2["reduction"][0]
            xg = np.full(ND, np.nan)
            xg[gdof[0]] = a["x"][0]
            assert np.array_equal(xg[shared], b2["x"][0][inv[1][shared]]), "the ranks disagree on shared nodes"
            xg[gdof[1]] = b2["x"][0]
            res = dict(a); res["x"] = xg[None, :]
            _check(c, h, kk, res, 0, flag, "j. %s, %s" % ("two reductions" if two else "single reduction", name), lines)
    after = _on_ranks(nranks, lambda r: _probed(drivers[r]))
    assert [m[1] for m in made] == after

    def close(r):
        drivers[r].close()
    _on_ranks(nranks, close)
    L.exa_loopback_group_destroy(gid)
    _record("j_two_ranks N3 %s" % ("jacobi" if jacobi else "identity"), lines)


# ---------------------------------------------------------------------------------------------------------------- k. one strided size
def test_strided_size():
    """N = 45, p = 1: 292 008 dofs - more than the 1024 x 256 one pass of the reduction grids covers, more than the 512 x 256 of the single-reduction dots:
    every reduction kernel strides.  No dense matrix: the reference takes its action from grad_apply_columns(assembled=True), one column per iteration.
    Identity only: no probe exposes the operator's diagonal at this size.  Cap of 5 (one iteration into the second chunk): count, flag, x_5."""
    N = 45
    c = _ctx(N, dense=False)
    assert c.nd == 3 * 46 ** 3 and c.nd > 1024 * 256
    d = c.d
    rng = np.random.default_rng(45)
    y = d.grad_apply_columns(rng.standard_normal((1, c.nd)), assembled=True)[0]
    c.ess = y == 0.0                                   # the masked operator leaves exact zeros in the essential rows, and only there
    assert 46 * 46 <= c.ess.sum() < c.nd // 10
    c.dinv = None
    c.b = c.rhs(1)

    def act(v):
        return d.grad_apply_columns(np.asarray(v, np.float64)[None, :], assembled=True)[0]

    h = R.History(act, c.b, kmax=5, seeds=(1, 2), ess=c.ess)
    lines = []
    _say(lines, "%s: %d dofs, %d essential" % (c.name, c.nd, c.ess.sum()))
    for g, r in [(None, None), (True, None), (False, "1")]:
        with _Env(EXA_PCG_REDUCE_LAUNCH=r):
            res = d.pcg_solve(c.b, 0.0, 0.0, 5, check_every=CE, graph=g)
        _check(c, h, 5, res, 0, R.MAX_ITER, "k. cap 5, graph %s, %s" % ({None: "as the run", True: "on", False: "off"}[g], "reduction launches" if r else "consumer-side reductions"), lines)
    _record("k_strided N45 identity", lines)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import exaconstit_amd.lib as L
    d = L.Driver.synthetic(3, _props(), hipref.random_quats(27).ravel(), DTS[:1], **TIGHT)
    nd = 3 * d.nodal_field("coords").shape[0]
    with pytest.raises(RuntimeError, match="no solved step"):
        d.pcg_solve(np.ones(nd), 1e-8, 0.0, 10)
    assert d.step(1)
    with pytest.raises(RuntimeError, match="1 to 16 columns"):
        d.pcg_solve(np.ones((17, nd)), 1e-8, 0.0, 10)
    x = np.zeros(nd); i1 = (C.c_int * 1)(); d1 = (C.c_double * 2)()
    dp = C.POINTER(C.c_double)
    for nrhs, mode, graph, msg in ((0, 0, -1, b"between 1 and 16 columns"), (17, 0, -1, b"between 1 and 16 columns"), (1, 2, -1, b"mode 0"), (1, 0, 2, b"graph -1")):
        err = C.create_string_buffer(512)
        assert L.exa_driver_pcg_solve(d.h, nrhs, x.ctypes.data_as(dp), 1e-8, 0.0, 10, 0, graph, mode, x.ctypes.data_as(dp), i1, i1, d1, i1, d1, err, 512) == -1
        assert msg in err.value, err.value
    d.close()


# ---------------------------------------------------------------------------------------------------------------- l. the run is undisturbed
def test_the_run_is_undisturbed():
    """EXA_DETERMINISTIC=1, N = 3, two steps: a driver probed after step 1 - every route, the cap, b = 0, a refused lockstep call - reports the stats,
    diagnostics and Krylov total it had before, and its step 2 gives the bits of a driver that was never probed"""
    import exaconstit_amd.lib as L

    def make():
        with _Env(EXA_DETERMINISTIC="1"):
            d = L.Driver.synthetic(3, _props(), hipref.random_quats(27).ravel(), DTS[:2], **TIGHT)
        assert d.step(1)
        return d

    a, b = make(), make()
    nd = 3 * a.nodal_field("coords").shape[0]
    before = _probed(a)
    rhs = np.random.default_rng(9).standard_normal((3, nd))
    for g, r in ROUTES:
        with _Env(EXA_PCG_REDUCE_LAUNCH=r):
            a.pcg_solve(rhs, 1e-6, 0.0, 200, check_every=CE, graph=g)
            a.pcg_solve(rhs, 0.0, 0.0, 5, check_every=CE, graph=g)
    a.pcg_solve(np.zeros(nd), 1e-6, 0.0, 200)
    with pytest.raises(RuntimeError, match="non-deterministic"):
        a.pcg_solve(rhs, 1e-6, 0.0, 200, columns=True)
    assert _probed(a) == before
    assert a.step(2) and b.step(2)
    for f in ("velocity", "coords"):
        assert np.array_equal(a.nodal_field(f), b.nodal_field(f))
    assert np.array_equal(a.avgs(0, 6), b.avgs(0, 6)) and [list(x) for x in a.stats()] == [list(x) for x in b.stats()]
    da, db = a.diagnostics(), b.diagnostics()
    assert da == db and a.timers()["krylov_iters"] == b.timers()["krylov_iters"]
    a.close(); b.close()


def test_zz_every_probed_driver_is_as_it_was():
    """after all probe calls of this module, each of its drivers reports the stats(), diagnostics() and timers()["krylov_iters"] it had before them"""
    for c in _ctxs.values():
        assert _probed(c.d) == c.before, c.name
