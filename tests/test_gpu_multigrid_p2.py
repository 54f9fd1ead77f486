"""Multigrid preconditioner at p = 2 (Solvers.Krylov.mg_p2, DESIGN 4.6 "p = 2") on the GPU: the hierarchy with the vertex level against dense numpy
products, level 1 and the fine diagonal read off the point records against the probed ones (both record forms, PA and the transposed EA route,
a partial wave of elements, several waves), the fall-backs to probing, the V-cycle as an operator, the same physics as the identity
preconditioner with fewer Krylov iterations, several loopback ranks against one, and the refusals that stay."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from test_gpu_multigrid import REF, _P, _check_preconditioner, _dense, _props, _quats, _rel

pytestmark = pytest.mark.gpu


def _synth(N, dts, assembly=0, **kw):
    import exaconstit_amd.lib as L
    return L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=assembly, order=2, **kw)


def _mg(d, **kw):
    d.set_preconditioner("multigrid", p2=True, **kw)
    return d


@pytest.fixture(scope="module")
def plastic4():
    """4^3 synthetic p = 2 RVE (64 elements: one wave; 9^3 nodes, 2187 dofs) after one plastic step, 2 coarse levels: 5^3 vertices and 3^3"""
    d = _mg(_synth(4, [0.5]))
    assert d.step(1)
    d.mg_setup()
    yield d
    d.close()


def test_galerkin_hierarchy_p2(plastic4):
    d = plastic4
    info = d.mg_info()
    assert info["levels"] == 2 and info["order"] == [2, 1, 1] and info["level1_build"] == "records"
    assert [list(b) for b in info["boxes"]] == [[4, 4, 4], [4, 4, 4], [2, 2, 2]]
    assert [d.mg_level_dofs(l) for l in range(3)] == [3 * 9 ** 3, 3 * 5 ** 3, 3 * 3 ** 3]
    assert np.all(info["lmax"] > 0.0) and info["setup_ms"] > 0.0
    A = [_dense(d, 0)]
    free = [np.abs(np.diag(A[0])) > 0.0]
    assert 0 < np.count_nonzero(~free[0]) < free[0].size
    print(f"fine p = 2 operator: relative asymmetry {np.linalg.norm(A[0] - A[0].T) / np.linalg.norm(A[0]):.3e}")
    assert np.all(A[0][~free[0], :] == 0.0) and np.all(A[0][:, ~free[0]] == 0.0)     # essential rows and columns are zero
    for level, nc in ((1, (5, 5, 5)), (2, (3, 3, 3))):
        P = _P(nc)
        surv = np.array([np.flatnonzero(P[:, j] == 1.0)[0] for j in range(P.shape[1])])
        fc = free[-1][surv]
        M = np.diag(fc.astype(float))
        want = M @ P.T @ A[-1] @ P @ M
        got = _dense(d, level)
        print(f"level {level}: |A - M P^T A P M| / |.| = {_rel(got, want):.3e}")
        assert _rel(got, want) < 1e-11, (level, _rel(got, want))
        x = np.random.default_rng(level).standard_normal(P.shape[1])
        assert _rel(d.mg_transfer(level - 1, 0, x), P @ x) < 1e-15
        y = np.random.default_rng(level + 7).standard_normal(P.shape[0])
        assert _rel(d.mg_transfer(level - 1, 1, y), P.T @ y) < 1e-14
        A.append(want)
        free.append(fc)
    for level in range(3):
        dg = d.mg_diag(level)
        print(f"level {level}: |diag - diag(A)| / |.| = {_rel(dg, np.diag(A[level])):.3e}")
        assert _rel(dg, np.diag(A[level])) < 1e-11, level
    assert np.all(d.mg_diag(0)[~free[0]] == 0.0)


def _box_toml(tmp_path, ncuts):
    """voce_pa.toml on a generated ncuts box at p = 2 with the multigrid keys"""
    text = open(os.path.join(REF, "voce_pa.toml")).read()
    for fl in os.listdir(REF):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    for old, new in (("[Solvers.Krylov]", '[Solvers.Krylov]\n    preconditioner = "multigrid"\n    mg_p2 = true'), ("prefinement = 1", "p_refinement = 2"),
                     ("ref_ser = 1", "ref_ser = 0"), ("ncuts = [5, 5, 5]", "ncuts = [%d, %d, %d]" % tuple(ncuts))):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    p = tmp_path / "box_p2.toml"
    p.write_text(text)
    return str(p)


def _state(case, tmp_path):
    import exaconstit_amd.lib as L
    if case == "pa4":
        return _mg(_synth(4, [0.5], assembly=0))
    if case == "ea4":        # the transposed route: on a plastic state the tangent's asymmetry (~1e-4) makes a missing transpose visible
        return _mg(_synth(4, [0.5], assembly=1))
    if case == "pa6":        # 216 elements: three waves and a tail
        return _mg(_synth(6, [0.5], assembly=0))
    assert case == "box462"  # 48 elements: a partial wave, unequal sides
    return L.Driver.from_toml(_box_toml(tmp_path, (4, 6, 2)), out_dir=str(tmp_path), write_files=False)


@pytest.mark.parametrize("form", ["compact", "full"])
@pytest.mark.parametrize("case", ["pa4", "ea4", "box462", "pa6"])
def test_records_build_equals_probe_build(case, form, tmp_path, monkeypatch):
    if form == "full":
        monkeypatch.setenv("EXA_TANGENT_FORM", "full")      # the 46-double records of the set-up pass instead of the compact ones
    d = _state(case, tmp_path)
    assert d.step(1)
    got = {}
    for tag, from_records in (("records", True), ("probe", False)):
        d.set_mg_p2_build(from_records)
        d.mg_setup()
        info = d.mg_info()
        assert info["level1_build"] == tag and info["order"][:2] == [2, 1]
        got[tag] = (d.mg_stencil(1), d.mg_diag(0), d.mg_diag(1))
    d.close()
    for name, a, b in zip(("stencil(1)", "diag(0)", "diag(1)"), got["records"], got["probe"]):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f"{case} {form}: {name} max |records - probe| / max |probe| = {err:.3e}")
        assert np.max(np.abs(b)) > 0.0 and err < 1e-11, (name, err)


def _three_steps(assembly=0, N=4, mg=True):
    d = _synth(N, [0.1, 0.2, 0.3], assembly=assembly)
    if mg:
        _mg(d)
    for ti in (1, 2, 3):
        assert d.step(ti), ti
    out = (d.avgs(0, 6), d.stats(), d.diagnostics(), d.mg_info() if mg else None)
    d.close()
    return out


def test_deterministic_mode_probes_and_reproduces(monkeypatch):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    a, b = _three_steps(), _three_steps()
    assert a[3]["level1_build"] == "probe" and a[3]["order"] == [2, 1, 1]
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))          # Newton, Krylov and model-call counts


def test_without_model_records_probes(monkeypatch):
    rec = _three_steps()
    assert rec[3]["level1_build"] == "records"
    monkeypatch.setenv("EXA_TANGENT_RECORDS", "off")
    prb = _three_steps()
    assert prb[3]["level1_build"] == "probe"
    assert np.max(np.abs(prb[0] - rec[0])) < 1e-9 * np.abs(rec[0]).max()
    monkeypatch.delenv("EXA_TANGENT_RECORDS")
    monkeypatch.setenv("EXA_EA_ASSEMBLED", "1")
    d = _mg(_synth(4, [0.5], assembly=1))
    assert d.step(1)
    assert d.mg_info()["level1_build"] == "probe"
    d.close()


def test_preconditioner_is_symmetric_positive_and_masked_p2(plastic4):
    d = _mg(_synth(4, [0.05]))       # 0.005 % strain: elastic
    assert d.step(1)
    d.mg_setup()
    _check_preconditioner(d, 1e-10)
    d.close()
    A = _dense(plastic4, 0)
    a_pl = np.linalg.norm(A - A.T) / np.linalg.norm(A)
    print(f"plastic fine p = 2 operator: relative asymmetry {a_pl:.3e}")
    _check_preconditioner(plastic4, max(1e-10, 10.0 * a_pl))


@pytest.mark.parametrize("assembly", [0, 1])
def test_multigrid_p2_solves_and_cuts_krylov_iterations(assembly):
    ident = _three_steps(assembly, N=8, mg=False)
    mg = _three_steps(assembly, N=8)
    print(f"8^3 p = 2 {'EA' if assembly else 'PA'}: Newton {list(mg[1][0])}, Krylov identity {list(ident[1][1])}, multigrid {list(mg[1][1])}, "
          f"not converged identity {ident[2]['pcg_not_converged']} multigrid {mg[2]['pcg_not_converged']}, build {mg[3]['level1_build']}")
    assert mg[3]["levels"] == 3 and mg[3]["order"] == [2, 1, 1, 1]
    assert np.max(np.abs(mg[0] - ident[0])) < 1e-6 * np.abs(ident[0]).max()
    assert list(mg[1][0]) == list(ident[1][0])
    assert mg[2]["pcg_not_converged"] == 0
    assert mg[1][1].sum() < ident[1][1].sum()
    if assembly == 0:        # mesh independence on the elastic step
        d = _mg(_synth(16, [0.1]))
        assert d.step(1)
        k16 = d.stats()[1]
        assert d.diagnostics()["pcg_not_converged"] == 0
        d.close()
        print(f"elastic step: multigrid 16^3 p = 2 Krylov {list(k16)}, 8^3 {mg[1][1][0]}")
        assert k16[0] <= mg[1][1][0] + 5


def _run_ranks(nranks, N, dts, levels):
    import exaconstit_amd.lib as L
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    res = [None] * nranks
    errors = []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), _quats(N), np.asarray(dts, dtype=np.float64), assembly=0, rank=r, nranks=nranks, uid=gid, order=2)
            d.set_preconditioner("multigrid", levels=levels, p2=True)
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


@pytest.fixture(scope="module")
def one_rank():
    return _run_ranks(1, 8, [0.5], 2)[0]               # one plastic step


@pytest.mark.parametrize("nranks", [2, 8])
def test_partitioned_multigrid_p2_matches_single_rank(nranks, one_rank):
    one = one_rank
    got = _run_ranks(nranks, 8, [0.5], 2)             # 8 ranks: 4^3 elements each, the vertex level and one more
    for s, st, diag, info in got:
        assert info["levels"] == 2 and info["order"] == [2, 1, 1] and info["level1_build"] == "records"
        assert np.max(np.abs(s - one[0])) < 1e-9 * np.abs(one[0]).max()
        assert list(st[0]) == list(one[1][0])
        assert np.all(np.abs(st[1] - one[1][1]) <= 1), (list(st[1]), list(one[1][1]))
        assert diag["pcg_not_converged"] == 0
        assert np.allclose(info["lmax"], one[3]["lmax"], rtol=1e-9)


def test_scratch_and_refusals():
    import exaconstit_amd.lib as L
    sb = L.mg_p2_scratch_bytes()
    assert len(sb) == 8 and all(v == 0 for v in sb.values()), sb
    d = _synth(4, [0.5])
    with pytest.raises(RuntimeError, match="p_refinement = 1"):
        d.set_preconditioner("multigrid")
    d.close()
    d = _synth(4, [0.5], assembly=1, bbar=True)
    with pytest.raises(RuntimeError, match="BBAR"):
        d.set_preconditioner("multigrid", p2=True)
    d.close()
    d = _mg(_synth(4, [0.5]))
    with pytest.raises(RuntimeError, match="p_refinement = 2"):
        d.set_periodic(np.diag([1e-3, 0.0, 0.0]))
    with pytest.raises(RuntimeError, match="p_refinement = 2"):
        d.set_periodic(np.diag([1e-3, 0.0, 0.0]), free=[[1, 0, 0], [0, 0, 0], [0, 0, 0]])
    d.close()
    d = L.Driver.synthetic(2, _props(), _quats(2), np.array([0.5]), assembly=0, order=3)
    with pytest.raises(RuntimeError, match="p_refinement >= 3"):
        d.set_preconditioner("multigrid", p2=True)
    d.close()
