"""Lean end-of-step state of the driver's record launches: the element-blocked record launches leave the inputs of the 12 slip rates
in state slots 14..19 and exa_slip_rates_from_state writes the rates when a reader asks.  A driver created with EXA_LEAN_STATE=off keeps the
launch that writes all 28 slots; every comparison here is bit for bit against such a driver.

Two runs are compared bit for bit, so both must see the same inputs.  The default (atomic) mode - the only one in which the record launches run:
EXA_DETERMINISTIC=1 takes the tangent-field route - adds the element contributions of a node in the order the waves reach it.  The integrator
kernels give one wave to each block of 64 elements, so a rank with a single block (N = 4, N = 4 on two ranks, p = 2 at N = 2) has no second wave
to race with and the real Newton / PCG solve repeats its bits; these shapes run the time steps of custom_dt.txt through step().  N = 5 has two
blocks whose waves share a layer of nodes: two solves of it differ at round-off whatever the state holds (tests/test_gpu_checkpoint.py says
the same of every multi-block run).  Its lean and full launches are therefore fed the same trajectory by construction: the kinematic drive of the
benchmark (bench_prepare: prescribed nodal velocities, constitutive launch and commit per step, no equilibrium solve) with the same 12 time steps,
which takes the points through the elastic-plastic transition as well."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
MODELS = {"fcc_voce": (False, 0, "props_cp_voce.txt"), "fcc_voce_nl": (False, 1, "props_cp_vocenl.txt"),
          "bcc_kmdd": (True, 2, "props_cp_mts.txt"), "fcc_kmdd": (False, 2, "props_cp_mts.txt")}
DTS = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()[:12]
# (N, order, ranks): one whole 64-element block | p = 2 | a block per rank, with a halo
SOLVED = {"N4": (4, 1, 1), "p2_N2": (2, 2, 1), "N4_2ranks": (4, 1, 2)}


@pytest.fixture(autouse=True)
def _atomic_mode(monkeypatch):
    for k in ("EXA_DETERMINISTIC", "EXA_QLAYOUT", "EXA_LEAN_STATE", "EXA_NEWTON_CAP", "EXA_TANGENT_RECORDS"):
        monkeypatch.delenv(k, raising=False)


def _driver(L, model, N, order=1, rank=0, nranks=1, uid=None):
    bcc, slip, pfile = MODELS[model]
    props = np.loadtxt(os.path.join(REF, pfile)).ravel()
    q = np.random.default_rng(1234 + N).standard_normal((N ** 3, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return L.Driver.synthetic(N, props, q.ravel(), DTS, bcc=bcc, slip=slip, order=order, rank=rank, nranks=nranks, uid=uid)


def _snap(d, which):
    """all 28 state and 6 stress components of the begin-of-step (0) or end-of-step (1) fields, as bit patterns"""
    return np.stack([d.qf_component(which, c) for c in range(28)] + [d.qf_component(2 + which, c) for c in range(6)]).view(np.int64)


def _solve(L, model, N, order, nranks, monkeypatch, lean):
    """the 12 steps through step(): per rank and step the fields after the uncommitted solve (which = 1) and after its commit (which = 0)"""
    monkeypatch.setenv("EXA_LEAN_STATE", "on" if lean else "off")
    gid = None
    if nranks > 1:
        gid = (C.c_ubyte * 128)()
        assert L.exa_loopback_group_create(nranks, gid) == 0
    out = [None] * nranks; errors = []

    def work(r):
        try:
            d = _driver(L, model, N, order, r, nranks, gid)
            snaps = []; tail = 0
            for ti in range(1, len(DTS) + 1):
                if not d.step(ti, commit=False):
                    raise RuntimeError("rank %d: Newton failed at step %d" % (r, ti))
                tail += int(d.nfev_hist(1)[5:].sum())
                end = _snap(d, 1)
                d.commit_step()
                snaps.append((end, _snap(d, 0)))
            dg = d.diagnostics()
            out[r] = dict(snaps=snaps, launches=dg["slip_rate_launches"], failed=dg["model_failed_points"], over4=tail)
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    if nranks == 1:
        work(0)
    else:
        th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        [t.start() for t in th]
        [t.join(timeout=300) for t in th]
        assert all(not t.is_alive() for t in th), "a rank hung"
        L.exa_loopback_group_destroy(gid)
    assert not errors, errors
    return out


def _compare(lean, full, what):
    for r, (a, b) in enumerate(zip(lean, full)):
        assert a["failed"] == 0 and b["failed"] == 0
        assert b["launches"] == 0, "EXA_LEAN_STATE=off must never materialise"
        assert a["launches"] >= len(DTS), "the lean driver materialised %d times: its launches were not lean" % a["launches"]
        for ti, ((a1, a0), (b1, b0)) in enumerate(zip(a["snaps"], b["snaps"]), 1):
            for which, x, y in ((1, a1, b1), (0, a0, b0)):
                bad = np.nonzero((x != y).any(axis=1))[0]
                assert bad.size == 0, "%s rank %d step %d which %d: rows (0..27 state, 28..33 stress) %s differ" % (what, r, ti, which, bad.tolist())
        rates = a["snaps"][-1][1][14:26].view(np.float64)
        assert np.abs(rates).max() > 0.0, "%s: no plastic point by step 12" % what


@pytest.mark.parametrize("case", sorted(SOLVED))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_solve_matches_full_state(monkeypatch, model, case):
    import exaconstit_amd.lib as L
    N, order, nranks = SOLVED[case]
    lean = _solve(L, model, N, order, nranks, monkeypatch, True)
    full = _solve(L, model, N, order, nranks, monkeypatch, False)
    _compare(lean, full, "%s %s" % (model, case))


def _kinematic(L, model, N, monkeypatch, lean):
    """the same 12 time steps under the benchmark's prescribed velocities: launch + commit per step, then one uncommitted launch from the new state"""
    monkeypatch.setenv("EXA_LEAN_STATE", "on" if lean else "off")
    d = _driver(L, model, N)
    snaps = []; tail = 0
    for k in range(len(DTS)):
        d.bench_prepare(DTS[k:k + 1])
        beg = _snap(d, 0)
        d.bench_model(1)
        tail += int(d.nfev_hist(1)[5:].sum())
        snaps.append((_snap(d, 1), beg))
    dg = d.diagnostics()
    d.close()
    return [dict(snaps=snaps, launches=dg["slip_rate_launches"], failed=dg["model_failed_points"], over4=tail)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_partial_block_matches_full_state(monkeypatch, model):
    """N = 5: 125 elements, a whole block and a partial one (see the module docstring for the trajectory)"""
    import exaconstit_amd.lib as L
    _compare(_kinematic(L, model, 5, monkeypatch, True), _kinematic(L, model, 5, monkeypatch, False), "%s N5" % model)


@pytest.mark.parametrize("case", ["N4", "N5"])
def test_tail_split_parks_the_strain(monkeypatch, case):
    """EXA_NEWTON_CAP=4: the points that need more than four evaluations are finished by the dense launches, which must leave the lean slots too"""
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_NEWTON_CAP", "4")
    if case == "N4":
        lean, full = (_solve(L, "bcc_kmdd", 4, 1, 1, monkeypatch, f) for f in (True, False))
    else:
        lean, full = (_kinematic(L, "bcc_kmdd", 5, monkeypatch, f) for f in (True, False))
    assert lean[0]["over4"] > 0, "no point went through the dense launch: the case does not test it"
    _compare(lean, full, "bcc_kmdd cap 4 %s" % case)


def test_rates_are_written_on_demand():
    import exaconstit_amd.lib as L
    d = _driver(L, "fcc_voce", 4)
    n = lambda: d.diagnostics()["slip_rate_launches"]   # noqa: E731
    for ti in (1, 2, 3):
        assert d.step(ti)
    for which in (0, 1):
        for c in list(range(14)) + [26, 27]:
            d.qf_component(which, c)
        for c in range(6):
            d.qf_component(2 + which, c)
    d.nfev_hist(0); d.avgs(0, 6)
    assert n() == 0, "a solve that reads no slip rate must not launch the materialisation"
    assert d.step(4, commit=False)
    assert n() == 0
    a = d.qf_component(1, 14)
    assert n() == 1
    assert np.array_equal(d.qf_component(1, 14), a) and n() == 1
    d.qf_component(1, 25)
    assert n() == 1, "one launch writes all 12 rates of a buffer"
    d.qf_component(0, 20)
    assert n() == 2, "the committed state of step 3 was still pending"
    d.commit_step()                                       # the buffers swap and keep their marks: nothing is pending now
    d.qf_component(0, 14); d.qf_component(1, 14)
    assert n() == 2
    assert d.step(5, commit=False)                        # new residual evaluations: the end-of-step buffer is lean again
    d.qf_component(0, 14)
    assert n() == 2
    d.qf_component(1, 14)
    assert n() == 3
    d.close()


def test_checkpoint_of_a_lean_driver(monkeypatch, tmp_path):
    """save at step 6 from a lean driver, restart, run on: the uninterrupted run's state; the file: the bytes an EXA_LEAN_STATE=off run writes"""
    import exaconstit_amd.lib as L

    def run(lean, first, last, load=None, save=None):
        monkeypatch.setenv("EXA_LEAN_STATE", "on" if lean else "off")
        d = _driver(L, "fcc_voce", 4)
        if load:
            d.load_checkpoint(load)
        for ti in range(first, last + 1):
            assert d.step(ti)
            if save and ti == save[0]:
                d.save_checkpoint(save[1])
        end = _snap(d, 0)
        vel = np.ascontiguousarray(d.nodal_field("velocity")).view(np.int64)
        n = d.diagnostics()["slip_rate_launches"]
        d.close()
        return end, vel, n
    ck_lean, ck_full = str(tmp_path / "lean.ckpt"), str(tmp_path / "full.ckpt")
    whole, v_whole, n_whole = run(True, 1, 12, save=(6, ck_lean))
    assert n_whole >= 1, "the checkpoint writer must have materialised the rates"
    run(False, 1, 6, save=(6, ck_full))
    assert open(ck_lean, "rb").read() == open(ck_full, "rb").read(), "a lean driver's checkpoint differs from the full-state one"
    rest, v_rest, _ = run(True, 7, 12, load=ck_lean)
    assert np.array_equal(whole, rest) and np.array_equal(v_whole, v_rest), "restart from a lean driver's checkpoint"
