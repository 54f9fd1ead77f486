"""Geometric multigrid preconditioner of the PCG (Solvers.Krylov.preconditioner = "multigrid", host/multigrid.hpp) on the GPU: the Galerkin
hierarchy against dense numpy products, the properties of the V-cycle as an operator, the same physics as the identity preconditioner and
the CPU oracle, fewer Krylov iterations, several loopback ranks against one, and bit-reproducibility in the deterministic mode."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")


def _props():
    return np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()


def _quats(N, seed=16):
    import hipref
    return hipref.random_quats(N ** 3, seed=seed)


def _synth(N, dts, **kw):
    import exaconstit_amd.lib as L
    return L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=0, **kw)


def _p1d(nc):
    """1-D interpolation (2 nc - 1) x nc: nested vertices, midpoints get 1/2 + 1/2"""
    nf = 2 * nc - 1
    P = np.zeros((nf, nc))
    for i in range(nf):
        if i % 2 == 0:
            P[i, i // 2] = 1.0
        else:
            P[i, i // 2] = P[i, i // 2 + 1] = 0.5
    return P


def _P(nc):
    """P of level l + 1 -> l on a box of nc = (ncx, ncy, ncz) coarse nodes; node = i + nx (j + ny k), dof = node + NN * comp"""
    P3 = np.kron(_p1d(nc[2]), np.kron(_p1d(nc[1]), _p1d(nc[0])))
    return np.kron(np.eye(3), P3)


def _dense(d, level):
    n = d.mg_level_dofs(level)
    A = np.zeros((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[:] = 0.0
        e[j] = 1.0
        A[:, j] = d.mg_apply(level, e)
    return A


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def plastic8():
    """8^3 synthetic RVE after one plastic step with the multigrid preconditioner (2 coarse levels: 4^3 and 2^3 elements)"""
    d = _synth(8, [0.5])
    d.set_preconditioner("multigrid")
    assert d.step(1)
    d.mg_setup()                 # the residual evaluation that ended the solve renewed the fine operator: rebuild on it
    yield d
    d.close()


def _asym(d):
    A = _dense(d, 0)
    return np.linalg.norm(A - A.T) / np.linalg.norm(A)


def test_galerkin_hierarchy(plastic8):
    d = plastic8
    info = d.mg_info()
    assert info["levels"] == 2 and [list(b) for b in info["boxes"]] == [[8, 8, 8], [4, 4, 4], [2, 2, 2]]
    assert np.all(info["lmax"] > 0.0) and info["setup_ms"] > 0.0
    A = [_dense(d, 0)]
    free = [np.abs(np.diag(A[0])) > 0.0]
    asym = np.linalg.norm(A[0] - A[0].T) / np.linalg.norm(A[0])
    print(f"fine operator: relative asymmetry {asym:.3e}")
    assert np.all(A[0][~free[0], :] == 0.0) and np.all(A[0][:, ~free[0]] == 0.0)     # essential rows and columns are zero
    for level, nc in ((1, (5, 5, 5)), (2, (3, 3, 3))):
        P = _P(nc)
        # the level mask is the finer mask at the surviving nodes (every second node: rows of P with a single 1)
        surv = np.array([np.flatnonzero(P[:, j] == 1.0)[0] for j in range(P.shape[1])])
        fc = free[-1][surv]
        M = np.diag(fc.astype(float))
        want = M @ P.T @ A[-1] @ P @ M
        got = _dense(d, level)
        assert _rel(got, want) < 1e-11, (level, _rel(got, want))
        x = np.random.default_rng(level).standard_normal(P.shape[1])
        assert _rel(d.mg_transfer(level - 1, 0, x), P @ x) < 1e-15
        y = np.random.default_rng(level + 7).standard_normal(P.shape[0])
        assert _rel(d.mg_transfer(level - 1, 1, y), P.T @ y) < 1e-14
        A.append(want)
        free.append(fc)
    for level in range(3):
        dg = d.mg_diag(level)
        assert _rel(dg, np.diag(A[level])) < 1e-11, level


def _check_preconditioner(d, sym_tol):
    free = np.abs(d.mg_diag(0)) > 0.0
    rng = np.random.default_rng(5)
    us = [rng.standard_normal(free.size) * free for _ in range(5)]
    Bs = [d.precond_apply(u) for u in us]
    assert d.mg_info()["vcycle_ms"] > 0.0
    for u, Bu in zip(us, Bs):
        assert np.all(Bu[~free] == 0.0)
        assert u @ Bu > 0.0
    for i in range(5):
        for j in range(i + 1, 5):
            a, b = us[i] @ Bs[j], us[j] @ Bs[i]
            assert abs(a - b) <= sym_tol * np.linalg.norm(us[i]) * np.linalg.norm(Bs[j]), (i, j, a, b)


def test_preconditioner_is_symmetric_positive_and_masked():
    """Elastic state (symmetric tangent): B is symmetric to round-off.  Plastic state: the ExaCMech tangent is not exactly symmetric (its
    relative asymmetry is measured here), and B, a polynomial in D^-1 A, is symmetric up to that asymmetry."""
    d = _synth(8, [0.05])        # 0.005 % strain: elastic
    d.set_preconditioner("multigrid")
    assert d.step(1)
    d.mg_setup()
    a_el = _asym(d)
    print(f"elastic fine operator: relative asymmetry {a_el:.3e}")
    assert a_el < 1e-13
    _check_preconditioner(d, 1e-10)
    d.close()
    d = _synth(8, [0.5])
    d.set_preconditioner("multigrid")
    assert d.step(1)
    d.mg_setup()
    a_pl = _asym(d)
    print(f"plastic fine operator: relative asymmetry {a_pl:.3e}")
    _check_preconditioner(d, max(1e-10, 10.0 * a_pl))
    d.close()


def test_hierarchy_build_is_bit_reproducible(monkeypatch):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    st = []
    for _ in range(2):
        d = _synth(8, [0.5])
        d.set_preconditioner("multigrid")
        assert d.step(1)
        d.mg_setup()
        st.append([d.mg_stencil(1), d.mg_stencil(2), d.mg_diag(0), d.mg_info()["lmax"]])
        d.close()
    for a, b in zip(*st):
        assert np.array_equal(a, b)


def test_config1_with_multigrid_matches_oracle(oracle):
    """BASELINE config 1 (tests/test_gpu_driver.py::test_config1_16cubed_one_step) with the multigrid preconditioner"""
    orc = oracle
    N = 16
    props = _props()
    quats = _quats(N)
    dts = np.array([0.5])
    case = dict(nx=N, ny=N, nz=N, p=1, length=[1.0, 1.0, 1.0], xtal=0, kin=0, props=props, temp_k=298.0,
                elem_grain=np.arange(N ** 3, dtype=np.int32), quats=quats, dts=dts, auto=None,
                bc_steps=[1], bc_ids=[[1, 2, 3, 4]], bc_comps=[[3, 1, 2, 3]], bc_vals=[[0.0] * 11 + [1.0e-3]], bc_vgrad=[[0.0] * 9],
                assembly=0, nl_solver=0, newton_rel=5e-5, newton_abs=5e-10, newton_iter=25, krylov_rel=1e-7, krylov_abs=1e-27, krylov_iter=1000,
                additional_avgs=False, integ=0)
    ref = orc.run_case(case)
    assert ref["failed"] == 0
    d = _synth(N, dts)
    d.set_preconditioner("multigrid")
    assert d.step(1)
    s = d.avgs(0, 6)
    assert np.max(np.abs(s[0] - ref["avg_stress"][0])) < 1e-6 * abs(ref["avg_stress"][0, 2])
    newton, krylov, _ = d.stats()
    assert list(newton) == list(ref["newton_iters"])
    assert d.diagnostics()["pcg_not_converged"] == 0
    print(f"config 1 with multigrid: Newton {list(newton)}, Krylov {list(krylov)}")
    d.close()


def _with_multigrid(tmp_path, case):
    text = open(os.path.join(REF, case + ".toml")).read()
    for fl in os.listdir(REF):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    text = text.replace("[Solvers.Krylov]", '[Solvers.Krylov]\n    preconditioner = "multigrid"')
    p = tmp_path / (case + "_mg.toml")
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("case", ["voce_pa", "mtsdd_bcc", "voce_ea_cs"])
def test_option_files_with_multigrid(tmp_path, case):
    import exaconstit_amd.lib as L
    nsteps = 4
    out = {}
    for tag, path in (("identity", os.path.join(REF, case + ".toml")), ("multigrid", _with_multigrid(tmp_path, case))):
        d = L.Driver.from_toml(path, out_dir=str(tmp_path), write_files=False)
        for ti in range(1, nsteps + 1):
            assert d.step(ti), (tag, ti)
        out[tag] = (d.avgs(0, 6), d.stats(), d.diagnostics(), d.mg_info() if tag == "multigrid" else None)
        d.close()
    s_id, s_mg = out["identity"][0], out["multigrid"][0]
    assert out["multigrid"][3]["levels"] == 1                          # 10^3 elements: one coarse level of 5^3
    assert np.max(np.abs(s_mg - s_id)) < 1e-6 * np.abs(s_id).max()
    assert out["multigrid"][2]["pcg_not_converged"] == 0
    print(f"{case}: Krylov identity {list(out['identity'][1][1])}, multigrid {list(out['multigrid'][1][1])}")


def test_multigrid_cuts_krylov_iterations():
    dts = [0.1, 0.2, 0.3]        # 0.01 %, 0.03 %, 0.06 % strain: elastic, first yield, plastic
    runs = {}
    for tag, N in (("mg32", 32), ("id32", 32), ("mg16", 16)):
        d = _synth(N, dts)
        if tag.startswith("mg"):
            d.set_preconditioner("multigrid")
        for ti in (1, 2, 3):
            assert d.step(ti), (tag, ti)
        runs[tag] = (d.stats(), d.diagnostics())
        d.close()
    kmg, kid, k16 = runs["mg32"][0][1], runs["id32"][0][1], runs["mg16"][0][1]
    print(f"Krylov per step: multigrid 32^3 {list(kmg)}, identity 32^3 {list(kid)}, multigrid 16^3 {list(k16)}")
    assert runs["mg32"][1]["pcg_not_converged"] == 0
    assert kmg.sum() * 3 <= kid.sum()
    assert kmg[0] <= k16[0] + 5


def _run_ranks(nranks, N, dts, levels):
    import exaconstit_amd.lib as L
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    res = [None] * nranks
    errors = []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=0, rank=r, nranks=nranks, uid=gid)
            d.set_preconditioner("multigrid", levels=levels)
            for ti in range(1, len(dts) + 1):
                if not d.step(ti):
                    raise RuntimeError(f"rank {r}: Newton failed at step {ti}")
            res[r] = (d.avgs(0, 6), d.stats(), d.diagnostics(), d.mg_info())
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


@pytest.mark.parametrize("nranks", [2, 8])
def test_partitioned_multigrid_matches_single_rank(nranks):
    dts = [0.25, 0.25]
    one = _run_ranks(1, 16, dts, 2)[0]
    got = _run_ranks(nranks, 16, dts, 2)
    for s, st, diag, info in got:
        assert info["levels"] == 2
        assert np.max(np.abs(s - one[0])) < 1e-9 * np.abs(one[0]).max()
        assert list(st[0]) == list(one[1][0])
        assert np.all(np.abs(st[1] - one[1][1]) <= 1), (list(st[1]), list(one[1][1]))
        assert diag["pcg_not_converged"] == 0
        assert np.allclose(info["lmax"], one[3]["lmax"], rtol=1e-9)


def test_deterministic_multigrid_run(monkeypatch):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    out = []
    for _ in range(2):
        d = _synth(16, [0.25, 0.25])
        d.set_preconditioner("multigrid")
        assert d.step(1) and d.step(2)
        out.append((d.avgs(0, 6), d.stats()))
        d.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def test_refused_decomposition():
    import exaconstit_amd.lib as L
    d = _synth(6, [0.5])                 # 6^3 on one rank: one level (3^3)
    d.set_preconditioner("multigrid")
    assert d.mg_info()["levels"] == 1
    d.close()
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(2, gid) == 0
    msgs = [None, None]

    def work(r):
        dd = L.Driver.synthetic(10, _props(), _quats(10), np.array([0.5]), assembly=0, rank=r, nranks=2, uid=gid)
        try:
            dd.set_preconditioner("multigrid")
        except RuntimeError as e:
            msgs[r] = str(e)
        dd.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    L.exa_loopback_group_destroy(gid)
    assert all(m is not None and "no coarse level" in m for m in msgs), msgs
