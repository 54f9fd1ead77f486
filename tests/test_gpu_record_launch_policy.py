"""Launch policy of the element-blocked p = 1 record launch: a Voce launch that is not split and writes no Jacobian field runs the kernel
entry that has the tail-split plumbing compiled out (k_model_setup_rec_nt); EXA_MODEL_POLICY=off (read per launch) keeps the generic kernel.  Both
must leave the same bits, and a launch with a cap in force must stay on the generic kernel for its main and its dense launches.

Two runs are compared bit for bit, so both must see the same inputs (tests/test_gpu_lean_state.py has the long form of this): a mesh of one
64-element block has no second wave to race with in the atomic E->L sums, so its real Newton / PCG solve repeats its bits - N = 4 runs step() and
also compares a gradient action K x, which reads every number of the 26-number records the launch wrote.  N = 5 (a whole block and a partial one)
and N = 1 (8 points: every wave partial) are driven kinematically - prescribed nodal velocities, launch and commit per step, no equilibrium solve -
which feeds both runs the same trajectory by construction; the action needs a solved step and is compared at N = 4 only.
Every comparison is equality of int64 bit patterns; nothing here has a tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
# (bcc, slip, property file, Voce rate sensitivity m or None for the file's): m = 0.02 (exponent 1/m - 1 = 49) runs the KIN_XN49 instantiations;
# no committed Voce set has another one, so the last entry perturbs m: exponent 39, the instantiations without the compiled-in exponent
MODELS = {"fcc_voce": (False, 0, "props_cp_voce.txt", None), "bcc_voce": (True, 0, "props_cp_voce.txt", None),
          "fcc_voce_nl": (False, 1, "props_cp_vocenl.txt", None), "fcc_voce_m025": (False, 0, "props_cp_voce.txt", 0.025)}
M_INDEX = 7   # position of m in props_cp_voce.txt
DTS = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()[:12]   # through the elastic-plastic transition (tests/test_gpu_lean_state.py)


@pytest.fixture(autouse=True)
def _record_route(monkeypatch):
    for k in ("EXA_DETERMINISTIC", "EXA_QLAYOUT", "EXA_LEAN_STATE", "EXA_NEWTON_CAP", "EXA_TANGENT_RECORDS", "EXA_MODEL_POLICY", "EXA_VOCE_XN_CT", "EXA_JAC_FIELD"):
        monkeypatch.delenv(k, raising=False)


def _driver(L, model, N, assembly=0):
    bcc, slip, pfile, m = MODELS[model]
    props = np.loadtxt(os.path.join(REF, pfile)).ravel()
    if m is not None:
        assert props[M_INDEX] == 0.02, "props_cp_voce.txt: m is expected at index %d" % M_INDEX
        props[M_INDEX] = m
    q = np.random.default_rng(1234 + N).standard_normal((N ** 3, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return L.Driver.synthetic(N, props, q.ravel(), DTS, bcc=bcc, slip=slip, assembly=assembly)


def _snap(d, which):
    """all 28 state and 6 stress components of the begin-of-step (0) or end-of-step (1) fields, as bit patterns"""
    return np.stack([d.qf_component(which, c) for c in range(28)] + [d.qf_component(2 + which, c) for c in range(6)]).view(np.int64)


def _finish(d, snaps, over4, extra=None):
    dg = d.diagnostics()
    d.close()
    return dict(snaps=snaps, over4=over4, failed=dg["model_failed_points"], policy=dg["record_policy_launches"], generic=dg["record_generic_launches"], extra=extra)


def _kinematic(L, model, N, monkeypatch, policy, lean=True, cap=None):
    monkeypatch.setenv("EXA_MODEL_POLICY", "on" if policy else "off")
    monkeypatch.setenv("EXA_LEAN_STATE", "on" if lean else "off")
    if cap: monkeypatch.setenv("EXA_NEWTON_CAP", str(cap))
    else: monkeypatch.delenv("EXA_NEWTON_CAP", raising=False)
    d = _driver(L, model, N)
    snaps = []; over4 = 0
    for k in range(len(DTS)):
        d.bench_prepare(DTS[k:k + 1])
        d.bench_model(1)
        over4 += int(d.nfev_hist(1)[5:].sum())
        snaps.append(_snap(d, 1))
    return _finish(d, snaps, over4)


def _solved(L, model, monkeypatch, policy, lean, assembly):
    """N = 4 through step(); after the last step one gradient action on a seeded vector"""
    monkeypatch.setenv("EXA_MODEL_POLICY", "on" if policy else "off")
    monkeypatch.setenv("EXA_LEAN_STATE", "on" if lean else "off")
    d = _driver(L, model, 4, assembly)
    snaps = []; over4 = 0
    for ti in range(1, len(DTS) + 1):
        assert d.step(ti, commit=False), "Newton failed at step %d" % ti
        over4 += int(d.nfev_hist(1)[5:].sum())
        snaps.append(_snap(d, 1))
        d.commit_step()
    x = np.random.default_rng(99).standard_normal(3 * 5 ** 3)
    kx = d.grad_apply_columns(x)
    return _finish(d, snaps, over4, np.ascontiguousarray(kx).view(np.int64))


def _same_bits(a, b, what):
    assert a["failed"] == 0 and b["failed"] == 0
    for k, (x, y) in enumerate(zip(a["snaps"], b["snaps"]), 1):
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert bad.size == 0, "%s step %d: rows (0..27 state, 28..33 stress) %s differ" % (what, k, bad.tolist())
    assert a["over4"] > 0, "%s: no point with more than four evaluations - the Newton loop never ran" % what
    rates = a["snaps"][-1][[0]].view(np.float64)   # slot 0: effective shear rate
    assert np.abs(rates).max() > 0.0, "%s: no plastic point by step %d" % (what, len(DTS))


def _routes(on, off, what):
    assert on["policy"] > 0 and on["generic"] == 0, "%s: policy on, launches (policy, generic) = (%d, %d)" % (what, on["policy"], on["generic"])
    assert off["policy"] == 0 and off["generic"] > 0, "%s: EXA_MODEL_POLICY=off, launches (policy, generic) = (%d, %d)" % (what, off["policy"], off["generic"])


@pytest.mark.parametrize("N", [5, 4, 1])
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "full"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_policy_leaves_the_generic_bits(monkeypatch, model, lean, N):
    """N = 5: a whole and a partial 64-element block; N = 4: exactly one block; N = 1: 8 points, every wave partial"""
    import exaconstit_amd.lib as L
    on = _kinematic(L, model, N, monkeypatch, True, lean)
    off = _kinematic(L, model, N, monkeypatch, False, lean)
    what = "%s %s N%d" % (model, "lean" if lean else "full", N)
    _routes(on, off, what)
    _same_bits(on, off, what)


@pytest.mark.parametrize("assembly", [0, 1], ids=["PA", "EA"])
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "full"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_policy_leaves_the_generic_records(monkeypatch, model, lean, assembly):
    """the solved N = 4 run: state, stress and K x (EA: the launch stores the transposed block, trd)"""
    import exaconstit_amd.lib as L
    on = _solved(L, model, monkeypatch, True, lean, assembly)
    off = _solved(L, model, monkeypatch, False, lean, assembly)
    what = "%s %s %s N4 solved" % (model, "lean" if lean else "full", "EA" if assembly else "PA")
    _routes(on, off, what)
    _same_bits(on, off, what)
    assert np.abs(on["extra"].view(np.float64)).max() > 0.0
    assert np.array_equal(on["extra"], off["extra"]), "%s: K x differs in %d of %d entries" % (what, int((on["extra"] != off["extra"]).sum()), on["extra"].size)


@pytest.mark.parametrize("model", ["fcc_voce", "fcc_voce_m025"])
def test_capped_launch_stays_generic(monkeypatch, model):
    """EXA_NEWTON_CAP=4 on the N = 5 case: the sequence of capped and dense launches runs the generic kernel - the entry without tail-split
    arguments has no list to append to and must never be launched then - and finishes with the bits of the uncapped (policy) run, the comparison
    tests/test_gpu_lean_state.py::test_tail_split_parks_the_strain makes on this route"""
    import exaconstit_amd.lib as L
    capped = _kinematic(L, model, 5, monkeypatch, True, cap=4)
    plain = _kinematic(L, model, 5, monkeypatch, True)
    assert capped["over4"] > 0, "no point went through the dense launch: the case does not test it"   # (a count above the cap: finished by a dense launch)
    assert capped["policy"] == 0 and capped["generic"] > 0, "a capped launch ran the entry without tail-split arguments"
    assert plain["policy"] > 0 and plain["generic"] == 0
    assert capped["failed"] == 0
    _same_bits(plain, capped, "%s cap 4 N5" % model)
