"""The geometric multigrid preconditioner on periodic cells ("periodic cells"), mixed loading included, on the GPU.

Notation.  A level with n local dofs and m canonical unknowns: E is the n x m 0/1 expansion (one value on every image of a node), held here as the
index array red_of_dof (E u = u[red_of_dof]) with rep_dof picking one image per unknown.  The reduced operator of level l is A^_l, defined by
mg_apply(l, E u) = E A^_l u.  P^ is the periodic trilinear interpolation: the Kronecker product of 1-D circulant interpolations of shape 2 nc x nc
(a midpoint takes 1/2 + 1/2, the last midpoint wraps to node 0), built in numpy below from nothing the code under test owns.  The images come from
the partition probe's canonical ids (lib.partition_periodic)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hipref
import pcg_reference as R
import test_gpu_macro_tangent as MT
import test_gpu_pcg_reference as PR
import test_gpu_periodic as TP
import test_gpu_periodic_mixed as TM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
LMAC, LZ, FREE_XY, TIGHT = TP.LMAC, TM.LZ, TM.FREE_XY, MT.TIGHT
RECORD = os.path.join(ROOT, "profiles", "mg_periodic_checks.txt")


def _record(key, lines):
    """the measured figures: printed and, when EXA_WRITE_RECORDS=1, kept in profiles/mg_periodic_checks.txt as the block '[key]'"""
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


def _props():
    return np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()


def _opt_in(toml):
    """the options file with Solvers.Krylov.mg_periodic = true next to its preconditioner = "multigrid" (multigrid on a periodic cell is opt-in)"""
    txt = open(toml).read()
    key = 'preconditioner = "multigrid"\n'
    if key in txt:
        open(toml, "w").write(txt.replace(key, key + "        mg_periodic = true\n"))
    return toml


def _pdriver(N, dts, vgrad=LMAC, free=None, precond="multigrid", levels=0, seed=16, **kw):
    """a periodic synthetic N^3 driver (one grain per element, seeded orientations), not stepped yet"""
    import exaconstit_amd.lib as L
    d = L.Driver.synthetic(N, _props(), hipref.random_quats(N ** 3, seed=seed).ravel(), np.asarray(dts, dtype=np.float64), assembly=0, **kw)
    d.set_periodic(vgrad, free)
    if precond != "identity":
        d.set_preconditioner(precond, levels=levels, periodic=True) if precond == "multigrid" else d.set_preconditioner(precond)
    return d


# ---------------------------------------------------------------------------------------------------------------- the reduced space, in numpy
class _Level:
    """index maps of a level with M = (M0, M1, M2) elements: local node i + (M0 + 1) (j + (M1 + 1) k), canonical node (i mod M0) + M0 (...)"""

    def __init__(self, M):
        import exaconstit_amd.lib as L
        self.M = tuple(int(v) for v in M)
        canon = np.asarray(L.partition_periodic(self.M, 0, 1)["canon"], dtype=np.int64)
        M0, M1, M2 = self.M
        self.nn = canon.size
        assert self.nn == (M0 + 1) * (M1 + 1) * (M2 + 1)
        c0, c1, c2 = canon % (M0 + 1), (canon // (M0 + 1)) % (M1 + 1), canon // ((M0 + 1) * (M1 + 1))
        assert c0.max() == M0 - 1 and c1.max() == M1 - 1 and c2.max() == M2 - 1
        red = c0 + M0 * (c1 + M1 * c2)
        self.m = M0 * M1 * M2
        assert np.array_equal(np.unique(red), np.arange(self.m))
        self.red_of_dof = np.concatenate([red + self.m * c for c in range(3)])
        rep = np.full(self.m, -1, dtype=np.int64)
        rep[red[::-1]] = np.arange(self.nn)[::-1]                       # the image with the lowest local index
        self.rep_dof = np.concatenate([rep + self.nn * c for c in range(3)])
        self.images = np.bincount(red, minlength=self.m)
        assert sorted(np.unique(self.images).tolist()) == [1, 2, 4, 8] and (self.images == 8).sum() == 1
        self.corner = np.concatenate([(np.arange(self.m) == 0)] * 3)    # canonical node 0: the eight corners

    def expand(self, u):
        return np.ascontiguousarray(np.asarray(u)[self.red_of_dof])

    def reduce(self, y, what):
        """the reduced vector of a local one whose images must carry the same bits"""
        yr = y[self.rep_dof]
        assert np.array_equal(yr[self.red_of_dof].view(np.int64), np.asarray(y).view(np.int64)), "%s: the images of a node differ" % what
        return yr


def _p1d_periodic(nc):
    """1-D circulant interpolation 2 nc x nc: nested vertices, a midpoint takes 1/2 + 1/2, the last midpoint wraps to node 0"""
    P = np.zeros((2 * nc, nc))
    for f in range(2 * nc):
        if f % 2 == 0:
            P[f, f // 2] = 1.0
        else:
            P[f, f // 2] += 0.5
            P[f, (f // 2 + 1) % nc] += 0.5
    return P


def _P_periodic(Mc):
    """P^ from the level with Mc coarse elements per direction to the one with 2 Mc; reduced dof = canonical node + m * component"""
    P3 = np.kron(_p1d_periodic(Mc[2]), np.kron(_p1d_periodic(Mc[1]), _p1d_periodic(Mc[0])))
    return np.kron(np.eye(3), P3)


def _dense_reduced(d, level, lv):
    A = np.zeros((3 * lv.m, 3 * lv.m))
    e = np.zeros(3 * lv.m)
    for j in range(3 * lv.m):
        e[:] = 0.0; e[j] = 1.0
        A[:, j] = lv.reduce(d.mg_apply(level, lv.expand(e)), "mg_apply level %d" % level)
    return A


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _check_hierarchy(d, M, nlevels, what):
    """image equality (bitwise) of mg_apply, mg_transfer (both ways), mg_diag and precond_apply; the Galerkin product, the transfers and the
    diagonals against numpy; essential rows and columns (the corners) zero at every level.  The bounds are those of
    tests/test_gpu_multigrid.py::test_galerkin_hierarchy for the same products.  Returns A^_0."""
    info = d.mg_info()
    assert info["periodic"] and info["control_dofs"] == 0
    assert info["levels"] == nlevels and [list(b) for b in info["boxes"]] == [[m >> l for m in M] for l in range(nlevels + 1)]
    assert np.all(info["lmax"] > 0.0)
    lv = [_Level([m >> l for m in M]) for l in range(nlevels + 1)]
    A = [_dense_reduced(d, 0, lv[0])]
    free = [np.abs(np.diag(A[0])) > 0.0]
    assert np.array_equal(~free[0], lv[0].corner)
    lines = ["%s: reduced fine operator %d x %d, relative asymmetry %.3e" % (what, A[0].shape[0], A[0].shape[0], np.linalg.norm(A[0] - A[0].T) / np.linalg.norm(A[0]))]
    for level in range(1, nlevels + 1):
        c, f = lv[level], lv[level - 1]
        P = _P_periodic(c.M)
        assert P.shape == (3 * f.m, 3 * c.m)
        fc = free[-1][np.array([np.flatnonzero(P[:, j] == 1.0)[0] for j in range(P.shape[1])])]      # the finer mask at the surviving nodes
        assert np.array_equal(~fc, c.corner)
        Mh = np.diag(fc.astype(float))
        want = Mh @ P.T @ A[-1] @ P @ Mh
        got = _dense_reduced(d, level, c)
        e_gal = _rel(got, want)
        x = np.random.default_rng(level).standard_normal(3 * c.m)
        e_p = _rel(f.reduce(d.mg_transfer(level - 1, 0, c.expand(x)), "prolongation to level %d" % (level - 1)), P @ x)
        y = np.random.default_rng(level + 7).standard_normal(3 * f.m)
        e_r = _rel(c.reduce(d.mg_transfer(level - 1, 1, f.expand(y)), "restriction to level %d" % level), P.T @ y)
        lines.append("  level %d (%s elements): Galerkin product off by %.3e, prolongation %.3e, restriction %.3e" % (level, "x".join(str(v) for v in c.M), e_gal, e_p, e_r))
        assert e_gal < 1e-11, (level, e_gal)
        assert e_p < 1e-15 and e_r < 1e-14, (level, e_p, e_r)
        assert not got[c.corner, :].any() and not got[:, c.corner].any()
        A.append(want); free.append(fc)
    assert not A[0][lv[0].corner, :].any() and not A[0][:, lv[0].corner].any()
    for level in range(nlevels + 1):
        dg = lv[level].reduce(d.mg_diag(level), "mg_diag level %d" % level)
        e_d = _rel(dg, np.diag(A[level]))
        lines.append("  level %d: diagonal off by %.3e" % (level, e_d))
        assert e_d < 1e-11, (level, e_d)
    rng = np.random.default_rng(11)
    for k in range(3):
        u = rng.standard_normal(3 * lv[0].m) * free[0]
        z = lv[0].reduce(d.precond_apply(lv[0].expand(u)), "precond_apply")
        assert not z[lv[0].corner].any() and u @ z > 0.0
    _record(what.split(",")[0].replace(" ", "_"), lines)
    return A[0], lv


# ---------------------------------------------------------------------------------------------------------------- 2. the hierarchy on 8^3
@pytest.fixture(scope="module")
def plastic8_periodic():
    """tests/test_gpu_multigrid.py::plastic8 plus set_periodic: 8^3 after one plastic step, 2 coarse levels (4^3 and 2^3 elements)"""
    d = _pdriver(8, [0.5])
    assert d.step(1)
    d.mg_setup()
    yield d
    d.close()


def test_galerkin_hierarchy_on_a_periodic_cell(plastic8_periodic):
    _check_hierarchy(plastic8_periodic, (8, 8, 8), 2, "hierarchy 8^3, after one plastic step")


# ---------------------------------------------------------------------------------------------------------------- 3. a box that is not a cube
def test_galerkin_hierarchy_on_a_box(tmp_path):
    """8 x 12 x 4 elements from an options file: one coarse level, three different strides (transposed wrap indices would show)"""
    import exaconstit_amd.lib as L
    M = (8, 12, 4)
    g = (np.arange(M[0] * M[1] * M[2]) % 7) + 1
    toml = _opt_in(TP._toml(tmp_path, "box", g, N=8, precond="multigrid"))
    txt = open(toml).read()
    assert "ncuts = [8, 8, 8]" in txt
    open(toml, "w").write(txt.replace("ncuts = [8, 8, 8]", "ncuts = [%d, %d, %d]" % M))
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    assert d.step(1)
    d.mg_setup()
    _check_hierarchy(d, M, 1, "hierarchy 8x12x4, options file")
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the preconditioner as an operator
def _check_preconditioner_periodic(d, A0, lv, sym_tol):
    """tests/test_gpu_multigrid.py::_check_preconditioner in the reduced space: B^ u . u > 0, zero on the essential unknowns, u_i . B^ u_j symmetric"""
    free = np.abs(np.diag(A0)) > 0.0
    rng = np.random.default_rng(5)
    us = [rng.standard_normal(free.size) * free for _ in range(5)]
    Bs = [lv.reduce(d.precond_apply(lv.expand(u)), "precond_apply") for u in us]
    assert d.mg_info()["vcycle_ms"] > 0.0
    for u, Bu in zip(us, Bs):
        assert np.all(Bu[~free] == 0.0)
        assert u @ Bu > 0.0
    for i in range(5):
        for j in range(i + 1, 5):
            a, b = us[i] @ Bs[j], us[j] @ Bs[i]
            assert abs(a - b) <= sym_tol * np.linalg.norm(us[i]) * np.linalg.norm(Bs[j]), (i, j, a, b)


def test_preconditioner_is_symmetric_positive_and_masked_on_a_periodic_cell():
    """the bound of tests/test_gpu_multigrid.py: 1e-10 on the elastic state, ten times the measured operator asymmetry on the plastic one"""
    lv = _Level((8, 8, 8))
    for tag, dt in (("elastic", 0.05), ("plastic", 0.5)):
        d = _pdriver(8, [dt])
        assert d.step(1)
        d.mg_setup()
        A0 = _dense_reduced(d, 0, lv)
        asym = np.linalg.norm(A0 - A0.T) / np.linalg.norm(A0)
        print("%s periodic fine operator: relative asymmetry %.3e" % (tag, asym))
        if tag == "elastic":
            assert asym < 1e-13
        _check_preconditioner_periodic(d, A0, lv, 1e-10 if tag == "elastic" else max(1e-10, 10.0 * asym))
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the PCG loop
def test_multigrid_loop_on_a_periodic_cell():
    """tests/test_gpu_pcg_reference.py::test_multigrid_loop at N = 4, periodic: SolveMultigrid against the reference CG on the reduced system, with
    the dense reduced K^ = E^T W apply(E .) (every canonical unknown once) and the dense M^^-1 of one V-cycle from precond_apply on image-equal unit
    vectors.  The weighted dot product of two image-equal vectors is the plain one of their reduced vectors, which is what the reference sums."""
    N = 4
    d = _pdriver(N, PR.DTS[:1], seed=16, **TIGHT)
    assert d.step(1)
    before = PR._probed(d)
    d.mg_setup()
    lv = _Level((N, N, N))
    nr = 3 * lv.m
    c = PR._Ctx.__new__(PR._Ctx)
    c.d, c.N, c.jacobi, c.nd, c.hist, c.name = d, N, False, nr, {}, "N = 4, p = 1, PA, periodic, multigrid"
    K = np.zeros((nr, nr))
    for j0 in range(0, nr, 16):
        nb = min(16, nr - j0)
        X = np.zeros((nb, nr)); X[np.arange(nb), j0 + np.arange(nb)] = 1.0
        Y = d.grad_apply_columns(np.stack([lv.expand(x) for x in X]), assembled=True, batched=False)
        K[:, j0:j0 + nb] = np.stack([lv.reduce(y, "assembled action") for y in Y]).T
    c.K = K
    c.ess = np.diag(K) == 0.0
    assert np.array_equal(c.ess, lv.corner)
    Minv = np.zeros((nr, nr))
    e = np.zeros(nr)
    for j in range(nr):
        e[:] = 0.0; e[j] = 1.0
        Minv[:, j] = lv.reduce(d.precond_apply(lv.expand(e)), "precond_apply")
    big = np.abs(Minv).max()
    v = np.random.default_rng(5).standard_normal(nr)
    v /= np.abs(v).sum()
    lin = np.abs(lv.reduce(d.precond_apply(lv.expand(v)), "precond_apply") - Minv @ v).max()
    sym = np.abs(Minv - Minv.T).max()
    lines = []
    PR._say(lines, "%s: M^-1 largest entry %.3e, asymmetry %.2e of it, M^-1 v against the dense product (|v|_1 = 1) off by %.2e of it" % (c.name, big, sym / big, lin / big))
    assert sym <= 1e-12 * big and lin <= 1e-12 * big
    c.dinv = None
    c.ld, c.f64 = R.dense_apply(c.K)
    c.b = np.random.default_rng(1000 * N + 1).standard_normal(nr)
    c.b[c.ess] = 0.0
    h = R.History(c.ld, c.b, seeds=PR.SEEDS, apply64=c.f64, ess=c.ess, Minv=np.asarray(Minv, np.longdouble))

    def solve(b, *a):
        res = d.pcg_solve(lv.expand(b), *a, check_every=PR.CE)
        res["x"] = np.stack([lv.reduce(x, "the PCG iterate") for x in res["x"]])
        return res
    k, rel = PR._centred(h)
    PR._check(c, h, k, solve(c.b, rel, 0.0, 200), 0, R.CONVERGED, "i. centred stop", lines)
    PR._check(c, h, k, solve(c.b, 0.0, np.sqrt(h.threshold(k)), 200), 0, R.CONVERGED, "i. abs_tol governs", lines)
    for m in PR.CAPS:
        PR._check(c, h, m, solve(c.b, 0.0, 0.0, m), 0, R.MAX_ITER, "i. cap %d" % m, lines)
    z = solve(np.zeros(nr), 1e-8, 0.0, 50)
    assert z["iters"][0] == 0 and z["flags"][0] == R.CONVERGED and not z["x"].any() and z["reduction"][0] == 0.0
    assert PR._probed(d) == before
    d.close()
    _record("multigrid_loop_N4_periodic", lines)


# ---------------------------------------------------------------------------------------------------------------- 6. runs
def test_option_file_with_multigrid_matches_identity(tmp_path):
    """a periodic 10^3 options file, first 4 steps: the criterion of tests/test_gpu_multigrid.py::test_option_files_with_multigrid"""
    import exaconstit_amd.lib as L
    g = TP._voronoi(10).ravel()
    out = {}
    for tag, pc in (("identity", None), ("multigrid", "multigrid")):
        d = TP._run(L, _opt_in(TP._toml(tmp_path, tag, g, N=10, precond=pc)), 4, tmp_path / tag)      # (asserts pcg_not_converged == 0)
        out[tag] = (d.avgs(0, 6), d.stats(), d.mg_info() if pc else None)
        d.close()
    s_id, s_mg = out["identity"][0], out["multigrid"][0]
    info = out["multigrid"][2]
    assert info["levels"] == 1 and info["periodic"] and info["control_dofs"] == 0
    _record("option_file_10", ["periodic 10^3, 4 steps: Krylov identity %s, multigrid %s; average stress apart by %.3e of the largest"
                               % (TP._ints(out["identity"][1][1]), TP._ints(out["multigrid"][1][1]), np.max(np.abs(s_mg - s_id)) / np.abs(s_id).max())])
    assert np.max(np.abs(s_mg - s_id)) < 1e-6 * np.abs(s_id).max()


def test_translation_invariance_under_multigrid(tmp_path):
    """tests/test_gpu_periodic.py::test_translation_invariance with the periodic runs under multigrid, and that test's own bound: 1e-3 of what the
    same roll does under the face conditions"""
    import exaconstit_amd.lib as L
    N = 8
    g0 = TP._voronoi(N)
    g1 = np.roll(g0, shift=(2, 1, 3), axis=(0, 1, 2))
    res = {}
    for bc in ("per", "ess"):
        for tag, g in (("a", g0), ("b", g1)):
            d = TP._run(L, _opt_in(TP._toml(tmp_path, bc + tag, g.ravel(), N=N, periodic=(bc == "per"), precond="multigrid" if bc == "per" else None)), TP.NSTEPS, tmp_path / (bc + tag))
            f = d.element_fields()
            S = np.zeros((N, N, N, 6)); S.reshape(-1, 6)[f["GlobalElementId"]] = f["Stress"]
            res[bc + tag] = (d.avgs(0, 6), S, TP._ints(d.stats()[1]))
            d.close()
    scale = np.abs(res["pera"][0]).max()
    d_ess = np.abs(res["essa"][0] - res["essb"][0]).max()
    d_per = np.abs(res["pera"][0] - res["perb"][0]).max()
    d_elem = np.abs(np.roll(res["perb"][1], shift=(-2, -1, -3), axis=(0, 1, 2)) - res["pera"][1]).max()
    _record("translation_invariance", ["translation invariance under multigrid, 8^3, %d steps: d_ess %.3e, d_per %.3e (%.3e of |avg stress|), per-element stress %.3e, bound %.3e; Krylov %s / %s"
                                       % (TP.NSTEPS, d_ess, d_per, d_per / scale, d_elem, 1e-3 * d_ess, res["pera"][2], res["perb"][2])])
    assert d_ess > 1e-4 * scale
    assert d_per <= 1e-3 * d_ess
    assert d_elem <= 1e-3 * d_ess


def test_multigrid_cuts_krylov_iterations_on_a_periodic_cell():
    """The conditions of tests/test_gpu_multigrid.py::test_multigrid_cuts_krylov_iterations on a periodic cell under L = diag(0, 0, 1e-3): the factor
    3 and the slack 5 are the project's own for the prescribed-face case (nobody had measured them on a periodic cell before this test)."""
    dts = [0.1, 0.2, 0.3]
    runs = {}
    for tag, N in (("mg32", 32), ("id32", 32), ("mg16", 16)):
        d = _pdriver(N, dts, vgrad=LZ, precond="multigrid" if tag.startswith("mg") else "identity")
        for ti in (1, 2, 3):
            assert d.step(ti), (tag, ti)
        runs[tag] = (d.stats(), d.diagnostics())
        d.close()
    kmg, kid, k16 = runs["mg32"][0][1], runs["id32"][0][1], runs["mg16"][0][1]
    _record("iteration_cut", ["periodic cell, L = diag(0, 0, 1e-3), dts %s; Krylov per step: multigrid 32^3 %s, identity 32^3 %s, multigrid 16^3 %s; capped solves: multigrid %d, identity %d"
                              % (dts, TP._ints(kmg), TP._ints(kid), TP._ints(k16), runs["mg32"][1]["pcg_not_converged"], runs["id32"][1]["pcg_not_converged"])])
    assert runs["mg32"][1]["pcg_not_converged"] == 0
    assert kmg.sum() * 3 <= kid.sum()
    assert kmg[0] <= k16[0] + 5


# ---------------------------------------------------------------------------------------------------------------- 7. ranks
def _run_ranks(nranks, N, dts, levels, vgrad=LMAC, free=None, precond="multigrid", tangent=None, **kw):
    import exaconstit_amd.lib as L
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    res = [None] * nranks
    errors = []

    def work(r):
        try:
            d = _pdriver(N, dts, vgrad=vgrad, free=free, precond=precond, levels=levels, rank=r, nranks=nranks, uid=gid, **kw)
            for ti in range(1, len(dts) + 1):
                if not d.step(ti):
                    raise RuntimeError(f"rank {r}: Newton failed at step {ti}")
            res[r] = (d.avgs(0, 6), d.stats(), d.diagnostics(), d.mg_info() if precond == "multigrid" else None, d.macro_info())
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
def one_rank_16():
    return _run_ranks(1, 16, [0.25, 0.25], 2)[0]


@pytest.mark.parametrize("nranks", [2, 8])
def test_partitioned_periodic_multigrid_matches_single_rank(one_rank_16, nranks):
    """the criteria of tests/test_gpu_multigrid.py::test_partitioned_multigrid_matches_single_rank.  One rank runs the fused kernels, several ranks
    the unfused ones with the cell's sum: this pins the two to each other; lmax needs the canonical seed"""
    one = one_rank_16
    got = _run_ranks(nranks, 16, [0.25, 0.25], 2)
    assert one[3]["levels"] == 2 and one[3]["periodic"] and one[2]["pcg_not_converged"] == 0
    for s, st, diag, info, _ in got:
        assert info["levels"] == 2 and info["periodic"]
        assert np.max(np.abs(s - one[0])) < 1e-9 * np.abs(one[0]).max()
        assert list(st[0]) == list(one[1][0])
        assert np.all(np.abs(st[1] - one[1][1]) <= 1), (list(st[1]), list(one[1][1]))
        assert diag["pcg_not_converged"] == 0
        assert np.allclose(info["lmax"], one[3]["lmax"], rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- 8. mixed loading
@pytest.fixture(scope="module")
def mixed8(tmp_path_factory):
    """8^3, xx and yy free (uniaxial stress along z), 4 steps of the schedule of tests/test_gpu_periodic_mixed.py, under Jacobi and under multigrid;
    the multigrid driver stays open"""
    import exaconstit_amd.lib as L
    tmp = tmp_path_factory.mktemp("mg_mixed")
    g = TM._voronoi(8).ravel()
    out = {}
    for tag in ("jacobi", "multigrid"):
        d, hist = TM._run(L, _opt_in(TM._toml(tmp, tag, g, N=8, precond=tag)), 4, tmp / tag)      # (asserts pcg_not_converged == 0)
        out[tag] = dict(avgs=d.avgs(0, 6).copy(), hist=hist, stats=d.stats(), d=d)
    out["jacobi"]["d"].close()
    yield out
    out["multigrid"]["d"].close()


def test_mixed_loading_multigrid_against_jacobi(mixed8):
    jac, mg = mixed8["jacobi"], mixed8["multigrid"]
    d = mg["d"]
    Lj, Lm = jac["hist"][-1][1]["vel_grad"], mg["hist"][-1][1]["vel_grad"]
    e_L = np.abs(Lm - Lj).max() / np.abs(Lj).max()
    e_s = np.abs(mg["avgs"] - jac["avgs"]).max() / np.abs(jac["avgs"]).max()
    _record("mixed_8", ["mixed loading 8^3 (xx, yy free), 4 steps: realised gradient apart by %.3e, average stress by %.3e; Newton %s / %s, Krylov jacobi %s, multigrid %s"
                        % (e_L, e_s, TP._ints(jac["stats"][0]), TP._ints(mg["stats"][0]), TP._ints(jac["stats"][1]), TP._ints(mg["stats"][1]))])
    assert e_L < 1e-6 and e_s < 1e-6
    assert Lm[0, 0] < 0 and Lm[1, 1] < 0
    assert TM._lateral_check(mg["avgs"], mg["hist"], "mixed_8_lateral", "mixed loading under multigrid, lateral stress:")
    info = d.mg_info()
    assert info["periodic"] and info["control_dofs"] == 2 and info["levels"] == 2


def test_mixed_loading_control_block(mixed8):
    """precond_apply: zero on the essential slots, r / d on the two free control slots, d the diagonal entry of the reduced operator there - the
    face resultant of the raw action on the expansion of a unit H_id (1 on component i of every node of the top face of pair d), probed here
    through grad_apply_columns - and the V-cycle output elsewhere, untouched by the control entries of r"""
    import exaconstit_amd.lib as L
    d = mixed8["multigrid"]["d"]
    N = 8
    t = L.partition_periodic_mixed(N, 0, 1)
    nn = (N + 1) ** 3
    x0 = d.nodal_field("coords_ref")
    grid = np.rint(x0 * N).astype(int)
    corner = np.flatnonzero(np.all((grid == 0) | (grid == N), axis=1))
    assert corner.size == 8
    slots = {}
    for i in (0, 1):                                                    # H_00 on (c_1, x), H_11 on (c_2, y)
        cd = np.flatnonzero(np.all(grid == np.eye(3, dtype=int)[i] * N, axis=1))[0]
        slots[i] = cd + nn * i
    d.mg_setup()
    dg = d.mg_diag(0)
    ess = np.zeros(3 * nn, bool)
    for c in range(3):
        ess[corner + nn * c] = True
    for s in slots.values():
        ess[s] = False
    rng = np.random.default_rng(3)
    lv = _Level((N, N, N))
    u = rng.standard_normal(3 * lv.m)
    r = lv.expand(u)
    r[ess] = 0.0
    r[list(slots.values())] = [0.7, -1.3]
    z = d.precond_apply(r)
    assert not z[ess].any()
    for i, s in slots.items():
        top = np.flatnonzero(grid[:, i] == N)
        assert sorted(top.tolist()) == sorted(np.asarray(t["faces"][i]).tolist())
        pe = np.zeros(3 * nn); pe[top + nn * i] = 1.0
        d_ref = pe @ d.grad_apply_columns(pe[None, :], assembled=False, batched=False)[0]
        print("control slot %d: d %.9e, face resultant of the raw action on the unit expansion %.9e, z %.9e" % (s, dg[s], d_ref, z[s]))
        assert d_ref > 0.0 and abs(dg[s] - d_ref) <= 1e-12 * d_ref
        assert abs(z[s] - r[s] / dg[s]) <= 4e-16 * abs(r[s] / dg[s])
    # The fluctuation block does not see the control entries of r.  The fine action scatters with atomics (this driver is not in deterministic
    # mode), so two V-cycles on the same r differ in their last bits: that difference, measured here, is the yardstick - a leak of the control
    # entries (0.7 and -1.3 among entries of order 1) would be fifteen orders above it.
    keep = np.ones(3 * nn, bool); keep[list(slots.values())] = False
    noise = max(np.abs(d.precond_apply(r) - z).max(), 1e-16 * np.abs(z).max())
    r2 = r.copy(); r2[list(slots.values())] = 0.0
    z2 = d.precond_apply(r2)
    print("V-cycle repeated on the same r: %.3e; without the control entries of r: %.3e (max |z| %.3e)" % (noise, np.abs(z2[keep] - z[keep]).max(), np.abs(z).max()))
    assert np.abs(z2[keep] - z[keep]).max() <= 10.0 * noise and not z2[~keep].any()
    d.mg_setup()


def test_mixed_loading_on_two_ranks(mixed8):
    """the same mixed run (synthetic driver) on 2 loopback ranks against one rank: the criteria of tests/test_gpu_periodic_mixed.py::test_ranks_match_one_rank"""
    dts = TM.DTS[:4]
    kw = dict(vgrad=LZ, free=FREE_XY, newton=(50, 1e-10, 1e-14), krylov=(20000, 1e-12, 1e-30))
    one = _run_ranks(1, 8, dts, 0, **kw)[0]
    got = _run_ranks(2, 8, dts, 0, **kw)
    scale = np.abs(one[0]).max()
    assert one[3]["control_dofs"] == 2 and one[2]["pcg_not_converged"] == 0
    for s, st, dg, info, mi in got:
        assert np.abs(s - one[0]).max() < 1e-6 * scale
        assert list(st[0]) == list(one[1][0])
        assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0
        assert info["control_dofs"] == 2 and info["periodic"]
        assert np.abs(mi["vel_grad"] - one[4]["vel_grad"]).max() < 1e-6 * 1e-3
        assert np.array_equal(mi["vel_grad"], got[0][4]["vel_grad"])


# ---------------------------------------------------------------------------------------------------------------- 9. macro tangent
def _tangent_pair(free, vgrad, dts):
    """macro_tangent of one state under Jacobi and under multigrid at the TIGHT tolerances, and the dense reference of tests/test_gpu_macro_tangent.py
    taken on the Jacobi driver"""
    N = 8
    mts = {}
    ref = None
    for tag in ("jacobi", "multigrid"):
        d = _pdriver(N, dts, vgrad=vgrad, free=free, precond=tag, **TIGHT)
        for ti in range(1, len(dts) + 1):
            assert d.step(ti)
        dg = d.diagnostics()
        assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0, dg
        mts[tag] = d.macro_tangent(rel_tol=1e-12, max_iter=4000)
        if tag == "jacobi":
            ref = MT._dense(d, N)
        else:
            assert not mts[tag]["batched"]                             # the columns go one by one through the V-cycle
            info = d.mg_info()
            assert info["control_dofs"] == (0 if free is None else int(np.sum(free)))      # the run's hierarchy is back after the evaluation
        d.close()
    return mts, ref


def _check_tangent_pair(mts, ref, what):
    """the cross-route check of tests/test_gpu_macro_tangent.py::_same_operator: both against the dense reference and against each other within twice
    the bound of the larger true residual; every column's true residual below the bound that file sets at rel_tol 1e-12 on a plastic state (1e-6)"""
    res = np.maximum(mts["jacobi"]["true_residual"], mts["multigrid"]["true_residual"])
    lines = []
    for tag in ("jacobi", "multigrid"):
        err, b, line = MT._compare(mts[tag], ref, "%s, %s" % (what, tag), factor=2.0, res=res)
        lines.append(line)
        lines.append("  true relative residuals per column: %s" % " ".join("%.2e" % v for v in mts[tag]["true_rel"]))
        assert np.all(err <= b), (tag, (err / b).max())
        assert np.all(mts[tag]["true_rel"] <= 1e-6), (tag, mts[tag]["true_rel"])
    e2 = np.abs(MT._T(mts["multigrid"]) - MT._T(mts["jacobi"]))
    lines.append("  multigrid against jacobi: worst |T_mg - T_jac| / bound %.3e" % (e2 / b).max())
    _record(what.split(",")[0].replace(" ", "_"), lines)
    assert np.all(e2 <= b), (e2 / b).max()
    return b


def test_macro_tangent_under_multigrid():
    mts, ref = _tangent_pair(None, LMAC, [0.5])
    _check_tangent_pair(mts, ref, "macro tangent 8^3 periodic, after one plastic step")


def test_macro_tangent_under_multigrid_on_the_mixed_run():
    """the mixed run of check 8 (synthetic driver): T and the condensed tangent; the condensed one within the first-order bound of
    tests/test_gpu_macro_tangent.py::test_route_mixed_and_its_condensed_tangent against the condensation of the dense reference"""
    mts, ref = _tangent_pair(FREE_XY, LZ, TM.DTS[:4])
    b = _check_tangent_pair(mts, ref, "macro tangent 8^3 mixed (xx, yy free), after 4 steps")
    f = FREE_XY.astype(bool).ravel(); pmask = ~f
    for tag in ("jacobi", "multigrid"):
        mt = mts[tag]
        Cr = ref["T_ref"] / mt["V"]
        X = np.linalg.solve(Cr[np.ix_(f, f)], Cr[np.ix_(f, pmask)]); Y = Cr[np.ix_(pmask, f)] @ np.linalg.inv(Cr[np.ix_(f, f)])
        want = np.zeros((9, 9)); want[np.ix_(pmask, pmask)] = Cr[np.ix_(pmask, pmask)] - Cr[np.ix_(pmask, f)] @ X
        tol = np.zeros((9, 9)); tol[np.ix_(pmask, pmask)] = (b.max() / mt["V"]) * np.outer(1.0 + np.abs(Y).sum(axis=1), 1.0 + np.abs(X).sum(axis=0))
        got = mt["condensed"].reshape(9, 9)
        assert np.all(np.abs(got - want) <= tol), (tag, (np.abs(got - want)[np.ix_(pmask, pmask)] / tol[np.ix_(pmask, pmask)]).max())
        assert np.all(got[f] == 0.0) and np.all(got[:, f] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- 10. determinism
@pytest.mark.parametrize("free", [None, FREE_XY], ids=["periodic", "mixed"])
def test_deterministic_periodic_multigrid_run(monkeypatch, free):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    out = []
    for _ in range(2):
        d = _pdriver(16 if free is None else 8, [0.25, 0.25], vgrad=LMAC if free is None else LZ, free=free)
        assert d.step(1) and d.step(2)
        out.append((d.avgs(0, 6), d.stats(), d.mg_info()["lmax"]))
        d.close()
    assert np.array_equal(out[0][0].view(np.int64), out[1][0].view(np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    assert np.array_equal(out[0][2], out[1][2])


# ---------------------------------------------------------------------------------------------------------------- 11. resource report, interface
def test_periodic_multigrid_kernels_have_no_scratch():
    """k_mg_stencil_apply_periodic and k_mg_restrict_periodic in the loaded code object, as tests/test_gpu_periodic.py::test_periodic_sum_has_no_scratch reads it"""
    import exaconstit_amd.lib as L
    hipref.Dev()
    out = (C.c_int * 2)(-1, -1)
    assert L.exa_mg_periodic_scratch_bytes(out) == 0
    assert list(out) == [0, 0]


def test_either_order_and_the_refusals_that_stay():
    """set_periodic and set_preconditioner("multigrid", periodic=True) in either order give the same hierarchy and the same run; without
    periodic=True either call refuses the other as before; a box that cannot be halved is still refused"""
    res = []
    for order in (0, 1):
        import exaconstit_amd.lib as L
        d = L.Driver.synthetic(8, _props(), hipref.random_quats(512, seed=16).ravel(), np.array([0.5]), assembly=0)
        if order == 0:
            d.set_periodic(LMAC)
            with pytest.raises(RuntimeError, match="mg_periodic"):
                d.set_preconditioner("multigrid", levels=1)
            d.set_preconditioner("multigrid", levels=1, periodic=True)
        else:
            d.set_preconditioner("multigrid", levels=1)
            with pytest.raises(RuntimeError, match="mg_periodic"):
                d.set_periodic(LMAC)
            d.set_preconditioner("multigrid", levels=1, periodic=True); d.set_periodic(LMAC)
        info = d.mg_info()
        assert info["periodic"] and info["levels"] == 1
        assert d.step(1)
        res.append((d.avgs(0, 6), d.stats(), d.mg_info()["lmax"]))
        d.close()
    assert np.abs(res[0][0] - res[1][0]).max() <= 1e-9 * np.abs(res[0][0]).max()
    assert np.allclose(res[0][2], res[1][2], rtol=1e-9) and list(res[0][1][0]) == list(res[1][1][0])
    d = _pdriver(5, [0.5], precond="identity")
    with pytest.raises(RuntimeError, match="no coarse level"):
        d.set_preconditioner("multigrid", periodic=True)
    d.close()
