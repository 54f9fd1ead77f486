"""Multigrid preconditioner under the B-bar integrator (Solvers.Krylov.mg_bbar, DESIGN 4.6 "B-bar") on the GPU: at p = 2, level 1 and the fine
diagonal read off the point records and the element-average gradients against the probed ones (both record forms, one wave of elements, several
waves, a partial wave on a box of unequal sides); the hierarchy at p = 2 and p = 1 against dense numpy products of the B-bar action; the V-cycle as
an operator at p = 1; the fall-backs to probing; the same physics as the identity preconditioner with fewer Krylov iterations; two loopback ranks
against one; and the refusals that stay.

Measured on one MI355X (one session): records against probe build at p = 2 B-bar, max |difference| / max |entry| 6.5e-16 ... 1.9e-15 for the stencil
and both diagonals on all six cases; hierarchy against the dense products 1.9e-16 ... 5.3e-16 (plastic fine operator: relative asymmetry 6.0e-4 at
p = 2, 2.6e-4 at p = 1); 8^3, three steps, Krylov iterations per step identity against multigrid at smoother degree 2: p = 2 B-bar 459 / 1082 / 2704
against 26 / 74 / 188, p = 1 B-bar 203 / 390 / 792 against 20 / 39 / 90, every solve converged (degree 3: 22 / 61 / 155 and 16 / 33 / 77)."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_multigrid import _P, _check_preconditioner, _dense, _props, _quats, _rel
from test_gpu_multigrid_p2 import _box_toml

pytestmark = pytest.mark.gpu


def _synth(N, dts, order=2, **kw):
    import exaconstit_amd.lib as L
    return L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=1, bbar=True, order=order, **kw)


def _mg(d, order=2, **kw):
    d.set_preconditioner("multigrid", p2=order == 2, bbar=True, **kw)
    return d


def _bbar_box_toml(tmp_path, ncuts):
    """the p = 2 multigrid box of the p = 2 tests under element assembly and B-bar, with the key"""
    text = open(_box_toml(tmp_path, ncuts)).read()
    for old, new in (('assembly = "PA"', 'assembly = "EA"\n    integ_model = "BBAR"'), ("mg_p2 = true", "mg_p2 = true\n    mg_bbar = true")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    p = tmp_path / "box_p2_bbar.toml"
    p.write_text(text)
    return str(p)


def _state(case, tmp_path):
    import exaconstit_amd.lib as L
    if case == "n4":          # 64 elements: exactly one wave of the element-blocked layout
        return _mg(_synth(4, [0.5]))
    if case == "n6":          # 216 elements: three waves and a partial one
        return _mg(_synth(6, [0.5]))
    assert case == "box462"   # 48 elements: a partial wave, unequal sides
    return L.Driver.from_toml(_bbar_box_toml(tmp_path, (4, 6, 2)), out_dir=str(tmp_path), write_files=False)


@pytest.mark.parametrize("form", ["compact", "full"])
@pytest.mark.parametrize("case", ["n4", "n6", "box462"])
def test_records_build_equals_probe_build_bbar(case, form, tmp_path, monkeypatch):
    """The pin on the B-bar forms of the record kernels: the probes go through the B-bar action of the driver, which the driver tests tie to the oracle."""
    if form == "full":
        monkeypatch.setenv("EXA_TANGENT_FORM", "full")      # the 46-double records of the set-up pass instead of the compact ones
    d = _state(case, tmp_path)
    assert d.step(1)
    got = {}
    for tag, from_records in (("records", True), ("probe", False)):
        d.set_mg_p2_build(from_records)
        d.mg_setup()
        info = d.mg_info()
        assert info["level1_build"] == tag and info["order"][:2] == [2, 1] and info["bbar"] is True
        got[tag] = (d.mg_stencil(1), d.mg_diag(0), d.mg_diag(1))
    d.close()
    for name, a, b in zip(("stencil(1)", "diag(0)", "diag(1)"), got["records"], got["probe"]):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f"B-bar {case} {form}: {name} max |records - probe| / max |probe| = {err:.3e}")
        assert np.max(np.abs(b)) > 0.0 and err < 1e-11, (name, err)


def _check_hierarchy(d, boxes):
    """level l = M P^T A P M from the densified level-0 action, and the diagonals, to 1e-11 (test_galerkin_hierarchy_p2)"""
    A = [_dense(d, 0)]
    free = [np.abs(np.diag(A[0])) > 0.0]
    assert 0 < np.count_nonzero(~free[0]) < free[0].size
    print(f"fine B-bar operator: relative asymmetry {np.linalg.norm(A[0] - A[0].T) / np.linalg.norm(A[0]):.3e}")
    assert np.all(A[0][~free[0], :] == 0.0) and np.all(A[0][:, ~free[0]] == 0.0)     # essential rows and columns are zero
    for level, nc in enumerate(boxes, start=1):
        P = _P(nc)
        surv = np.array([np.flatnonzero(P[:, j] == 1.0)[0] for j in range(P.shape[1])])
        fc = free[-1][surv]
        M = np.diag(fc.astype(float))
        want = M @ P.T @ A[-1] @ P @ M
        got = _dense(d, level)
        print(f"level {level}: |A - M P^T A P M| / |.| = {_rel(got, want):.3e}")
        assert _rel(got, want) < 1e-11, (level, _rel(got, want))
        A.append(want)
        free.append(fc)
    for level in range(len(boxes) + 1):
        dg = d.mg_diag(level)
        print(f"level {level}: |diag - diag(A)| / |.| = {_rel(dg, np.diag(A[level])):.3e}")
        assert _rel(dg, np.diag(A[level])) < 1e-11, level
    assert np.all(d.mg_diag(0)[~free[0]] == 0.0)
    return A[0]


@pytest.fixture(scope="module")
def plastic4_p2():
    """4^3 p = 2 B-bar RVE (9^3 nodes) after one plastic step, 2 coarse levels: 5^3 vertices and 3^3"""
    d = _mg(_synth(4, [0.5]))
    assert d.step(1)
    d.mg_setup()
    yield d
    d.close()


@pytest.fixture(scope="module")
def plastic4_p1():
    """4^3 p = 1 B-bar RVE (5^3 nodes) after one plastic step, 1 coarse level: 3^3"""
    d = _mg(_synth(4, [0.5], order=1), order=1)
    assert d.step(1)
    d.mg_setup()
    yield d
    d.close()


def test_galerkin_hierarchy_p2_bbar(plastic4_p2):
    info = plastic4_p2.mg_info()
    assert info["levels"] == 2 and info["order"] == [2, 1, 1] and info["level1_build"] == "records" and info["bbar"] is True
    assert [plastic4_p2.mg_level_dofs(l) for l in range(3)] == [3 * 9 ** 3, 3 * 5 ** 3, 3 * 3 ** 3]
    _check_hierarchy(plastic4_p2, ((5, 5, 5), (3, 3, 3)))


def test_galerkin_hierarchy_p1_bbar(plastic4_p1):
    info = plastic4_p1.mg_info()
    assert info["levels"] == 1 and info["order"] == [1, 1] and info["level1_build"] is None and info["bbar"] is True
    assert [plastic4_p1.mg_level_dofs(l) for l in range(2)] == [3 * 5 ** 3, 3 * 3 ** 3]
    _check_hierarchy(plastic4_p1, ((3, 3, 3),))


def test_preconditioner_is_symmetric_positive_and_masked_p1_bbar(plastic4_p1):
    d = _mg(_synth(4, [0.05], order=1), order=1)       # 0.005 % strain: elastic
    assert d.step(1)
    d.mg_setup()
    _check_preconditioner(d, 1e-10)
    d.close()
    A = _dense(plastic4_p1, 0)
    a_pl = np.linalg.norm(A - A.T) / np.linalg.norm(A)
    print(f"plastic fine p = 1 B-bar operator: relative asymmetry {a_pl:.3e}")
    _check_preconditioner(plastic4_p1, max(1e-10, 10.0 * a_pl))


def _steps(order=2, N=4, mg=True, dts=(0.1, 0.2, 0.3)):
    d = _synth(N, list(dts), order=order)
    if mg:
        _mg(d, order)
    for ti in range(1, len(dts) + 1):
        assert d.step(ti), ti
    out = (d.avgs(0, 6), d.stats(), d.diagnostics(), d.mg_info() if mg else None)
    d.close()
    return out


def test_deterministic_mode_probes_and_reproduces_bbar(monkeypatch):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    # (two steps, elastic and first yield: at 4^3 p = 2 B-bar the Newton iteration of a third step of 0.03 % strain does not converge, whatever the
    #  preconditioner - the identity run stops at the same iteration)
    a, b = _steps(dts=(0.1, 0.2)), _steps(dts=(0.1, 0.2))
    assert a[3]["level1_build"] == "probe" and a[3]["order"] == [2, 1, 1] and a[3]["bbar"] is True
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))          # Newton, Krylov and model-call counts


def test_assembled_matrices_probe_bbar(monkeypatch):
    monkeypatch.setenv("EXA_EA_ASSEMBLED", "1")
    d = _mg(_synth(4, [0.5]))
    assert d.step(1)
    assert d.mg_info()["level1_build"] == "probe"
    d.close()


@pytest.mark.parametrize("order", [2, 1])
def test_multigrid_bbar_solves_and_cuts_krylov_iterations(order):
    ident = _steps(order, N=8, mg=False)
    mg = _steps(order, N=8)
    print(f"8^3 p = {order} B-bar EA: Newton {list(mg[1][0])}, Krylov identity {list(ident[1][1])}, multigrid {list(mg[1][1])}, "
          f"not converged identity {ident[2]['pcg_not_converged']} multigrid {mg[2]['pcg_not_converged']}, build {mg[3]['level1_build']}, degree {mg[3]['degree']}")
    assert mg[3]["bbar"] is True and mg[3]["order"] == ([2, 1, 1, 1] if order == 2 else [1, 1, 1])
    assert np.max(np.abs(mg[0] - ident[0])) < 1e-6 * np.abs(ident[0]).max()
    assert list(mg[1][0]) == list(ident[1][0])
    assert mg[2]["pcg_not_converged"] == 0
    assert mg[1][1].sum() < ident[1][1].sum()


def _run_ranks(nranks, N, dts, levels):
    import exaconstit_amd.lib as L
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    res = [None] * nranks
    errors = []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=1, bbar=True, rank=r, nranks=nranks, uid=gid, order=2)
            d.set_preconditioner("multigrid", levels=levels, p2=True, bbar=True)
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


def test_partitioned_multigrid_bbar_matches_single_rank():
    one = _run_ranks(1, 8, [0.5], 2)[0]               # one plastic step
    got = _run_ranks(2, 8, [0.5], 2)
    for s, st, diag, info in got:
        assert info["levels"] == 2 and info["order"] == [2, 1, 1] and info["level1_build"] == "records" and info["bbar"] is True
        assert np.max(np.abs(s - one[0])) < 1e-9 * np.abs(one[0]).max()
        assert list(st[0]) == list(one[1][0])
        assert np.all(np.abs(st[1] - one[1][1]) <= 1), (list(st[1]), list(one[1][1]))
        assert np.allclose(info["lmax"], one[3]["lmax"], rtol=1e-9)


def test_scratch_and_refusals_bbar():
    import exaconstit_amd.lib as L
    sb = L.mg_p2_bbar_scratch_bytes()
    assert len(sb) == 9 and all(v == 0 for v in sb.values()), sb
    old = 'is not built for integ_model = "BBAR"'
    for order, kw in ((1, {}), (2, dict(p2=True))):          # without bbar=True: the refusal B-bar always had
        d = _synth(4, [0.5], order=order)
        with pytest.raises(RuntimeError, match=old):
            d.set_preconditioner("multigrid", **kw)
        d.close()
    d = _synth(4, [0.5])                                      # bbar=True does not stand in for p2=True
    with pytest.raises(RuntimeError, match="p_refinement = 1"):
        d.set_preconditioner("multigrid", bbar=True)
    d.close()
    new = "mg_bbar = true is not built for BCs.periodic = true"
    L1 = np.diag([1e-3, 0.0, 0.0])
    for periodic_key in (False, True):
        d = _mg(_synth(4, [0.5], order=1), order=1, periodic=periodic_key)
        with pytest.raises(RuntimeError, match=new):
            d.set_periodic(L1)
        d.close()
        d = _synth(4, [0.5], order=1)
        d.set_periodic(L1)
        with pytest.raises(RuntimeError, match=new):
            d.set_preconditioner("multigrid", bbar=True, periodic=periodic_key)
        d.close()
