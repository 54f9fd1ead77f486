"""The in-situ analyses as one object (host/analyses.hpp): what the output schedule and the one accessor of the element rows must keep.
  1. an options-file run with every analysis on writes, file by file, what the runs with one analysis on write;
  2. the launches of exa_element_fields (Driver.diagnostics()["element_field_launches"]) are those the schedule needs and no more;
  3. the stamp that decides whether the rows are those of the state at hand is invalidated by everything that changes the state;
  4. two loopback ranks stepped from Python see the same global values and count the same launches.
Options-file runs: the generated 4^3 cube of tests/test_gpu_periodic.py (_toml with the face conditions), 8 grains, 6 steps, EXA_DETERMINISTIC=1 (the
atomic record action differs in the last bits from run to run, and the files are compared byte by byte)."""
import contextlib
import ctypes as C
import glob
import os
import threading

import numpy as np
import pytest

from test_gpu_fatigue import DTS16, TIGHT, VZ, _props, _unit, eight_grains

pytestmark = pytest.mark.gpu

N = 4
HKL = [[1, 1, 1], [2, 0, 0], [2, 2, 0]]
SIGMA_Y = 0.2
BURGERS = 2.5e-7
KEYS = {"paraview": ["paraview = true"],
        "light_up": ["light_up = true", "light_up_hkl = [[1,1,1],[2,0,0],[2,2,0]]", "light_up_dist_tol_deg = 15.0"],
        "grain_avgs": ["grain_avgs = true"],
        "texture": ["texture = true"],
        "lattice_curvature": ["lattice_curvature = true", "lattice_curvature_burgers = %r" % BURGERS],
        "fatigue": ["fatigue = true", "fatigue_sigma_y = %r" % SIGMA_Y, "fatigue_cycle_steps = 3"]}


def _launches(d):
    return d.diagnostics()["element_field_launches"]


@contextlib.contextmanager
def _deterministic():
    old = os.environ.get("EXA_DETERMINISTIC")
    os.environ["EXA_DETERMINISTIC"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["EXA_DETERMINISTIC"]
        else:
            os.environ["EXA_DETERMINISTIC"] = old


def _run_keys(base, tag, keys):
    """6 steps with the analyses `keys` on and Visualizations.steps = 3 into base/tag; the options file lies beside it"""
    import exaconstit_amd.lib as L
    from test_gpu_periodic import _toml
    out = base / tag
    out.mkdir()
    toml = _toml(base / "cases", tag, eight_grains(N), N=N, periodic=False)
    t = open(toml).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    vis = ["steps = 3", 'avg_stress_fname = "avg_stress.txt"'] + [x for k in keys for x in KEYS[k]]
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis) + t[b:]
    assert "nsteps = 40" in t
    open(toml, "w").write(t.replace("nsteps = 40", "nsteps = 6", 1))
    d = L.Driver.from_toml(toml, out_dir=str(out))
    assert d.run() == 6
    launches = _launches(d)
    d.close()
    return dict(dir=str(out), launches=launches)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("schedule")
    with _deterministic():
        r = {"all": _run_keys(base, "all", list(KEYS))}
        for k in KEYS:
            r[k] = _run_keys(base, k, [k])
        r["no_fatigue"] = _run_keys(base, "no_fatigue", [k for k in KEYS if k != "fatigue"])
        r["no_fatigue_no_light_up"] = _run_keys(base, "no_fatigue_no_light_up", [k for k in KEYS if k not in ("fatigue", "light_up")])
    return r


def _text_files(d):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.txt")))


def test_all_on_against_one_on(runs):
    from test_gpu_element_fields import _read_cycle
    everything = _text_files(runs["all"]["dir"])
    seen = set()
    for k in KEYS:
        names = _text_files(runs[k]["dir"])
        assert "avg_stress.txt" in names and set(names) <= set(everything), (k, names)
        for f in names:
            a, b = open(os.path.join(runs[k]["dir"], f), "rb").read(), open(os.path.join(runs["all"]["dir"], f), "rb").read()
            assert a == b and len(a) > 0, (k, f)
        seen |= set(names)
    assert seen == set(everything)                                       # every file of the all-on run belongs to one of the keys
    assert {"lattice_strains.txt", "lattice_volumes.txt", "grain_avgs_000003.txt", "grain_avgs_000006.txt", "texture_000000.txt", "texture_000006.txt",
            "lattice_curvature.txt", "fatigue.txt", "fatigue_grains_000003.txt", "fatigue_grains_000006.txt"} <= seen, seen
    for cycle in (0, 3, 6):
        one = _read_cycle(os.path.join(runs["paraview"]["dir"], "results", "exaconstit"), cycle)
        full = _read_cycle(os.path.join(runs["all"]["dir"], "results", "exaconstit"), cycle)
        common = sorted(set(one) & set(full))
        assert "Stress" in common and "GROD" in full and "FIP" in full and "GROD" not in one
        for name in common:
            assert np.array_equal(np.asarray(one[name]), np.asarray(full[name])), (cycle, name)


def test_launch_counts(runs):
    import exaconstit_amd.lib as L
    got = {k: runs[k]["launches"] for k in ("all", "no_fatigue", "no_fatigue_no_light_up")}
    print("element-field launches:", {k: runs[k]["launches"] for k in runs})
    assert got["all"] == 7                          # the start of the accumulators, then one per committed step
    assert got["no_fatigue"] == 7                   # cycle 0 / texture 0, then one light-up row per step
    assert got["no_fatigue_no_light_up"] == 3       # cycle 0 / texture 0, steps 3 and 6
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:2], vz=VZ)
    assert d.step(1)
    n0 = _launches(d)
    d.element_fields(); d.grain_averages(); d.lattice_strains(HKL, tol_deg=15.0)
    assert _launches(d) - n0 == 1
    d.close()


def _same(a, b):
    """the same values in every entry (NaN, the lattice strain of an empty fibre, equal to NaN)"""
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_the_stamp_is_sound(tmp_path, monkeypatch):
    """Driver A asks for element_fields() - which always launches - before each probe; its twin B probes straight away and so depends on the stamp.
    Both hold the rows of the previous state when the state changes.

    After set_grains the grain means are the set orientations up to the rounding of the volume-weighted sum of the 8 equal quaternions of a grain and
    of its normalisation: each component within 8 eps, and GrainRotation = 2 atan2(|d_vec|, |d_0|) of the product with the reference orientation, whose
    vector part is three sums of four products that cancel in pairs, within 2 sqrt 3 (4 x 8 + 4) eps rad = 1.6e-12 degrees.  Exact equality and
    GrainRotation == 0 do not hold: 2.2e-16 and 1.6e-14 degrees were measured, the same figures before and after the analyses moved into one object.
    Rows held from the state before set_grains (one random orientation per element) put the means tens of degrees away."""
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    gq = _unit(np.random.default_rng(11).standard_normal((8, 4)))
    ck = str(tmp_path / "two.ckpt")

    def make():
        return L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:4], vz=VZ)

    def probe(d, explicit, what):
        """returns the two analyses; the counter rises by exactly one: A's explicit launch, or B's first probe after the state change"""
        n0 = _launches(d)
        if explicit:
            d.element_fields()
        g = d.grain_averages()
        n1 = _launches(d)
        s = d.lattice_strains(HKL, tol_deg=15.0)
        assert (n1 - n0, _launches(d) - n1) == (1, 0), (what, explicit, n0, n1, _launches(d))
        return g, s

    a, b = make(), make()
    res = {}
    for d, explicit in ((a, True), (b, False)):
        probe(d, explicit, "initial state")                              # rows of the one-grain-per-element state are held from here on
        d.set_grains(eight_grains(N), gq)
        res[explicit] = [probe(d, explicit, "after set_grains")]
        assert d.step(1, commit=False)
        res[explicit].append(probe(d, explicit, "after step(1, commit=False)"))
        d.commit_step()
        res[explicit].append(probe(d, explicit, "after commit_step"))
    assert a.step(2)
    a.save_checkpoint(ck)
    a.close(); b.close()
    for explicit in (True, False):
        d = make()
        d.set_grains(eight_grains(N), gq)
        d.element_fields()                                               # rows of the initial state, which the checkpoint replaces
        d.load_checkpoint(ck)
        res[explicit].append(probe(d, explicit, "after load_checkpoint"))
        d.close()
    for (ga, sa), (gb, sb) in zip(res[True], res[False]):
        _same(ga, gb); _same(sa, sb)
    g0 = res[False][0][0]
    dq = np.abs(g0["LatticeOrientation"] - gq).max()
    print("after set_grains: max |mean quaternion - set orientation| =", dq, " max rotation_deg =", g0["GrainRotation"].max())
    assert np.array_equal(g0["grain_id"], np.arange(1, 9))
    eps = np.finfo(float).eps
    assert dq <= 8 * eps and np.all(g0["GrainRotation"] <= np.degrees(2 * np.sqrt(3.0) * 36 * eps))
    # the four states differ: a probe that answered from the rows of an earlier state would have shown above
    s = [r[0]["Stress"] for r in res[False]]
    assert np.all(s[0] == 0.0) and np.all(s[1] == 0.0)                   # (commit = False leaves the begin-of-step state)
    assert np.abs(s[2]).max() > 0.0 and not np.array_equal(s[2], s[3])


def test_two_loopback_ranks():
    """the sequence of analyses after every step on two ranks of one device: the values over all ranks are the same on both, as are the launch counts"""
    import exaconstit_amd.lib as L
    nranks = 2
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    res, errors = [None] * nranks, []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:3], vz=VZ, rank=r, nranks=nranks, uid=gid, **TIGHT)
            d.set_grains(eight_grains(N), _unit(np.random.default_rng(11).standard_normal((8, 4))))
            d.enable_slip_activity()
            out = []
            for ti in range(1, 4):
                assert d.step(ti)
                f = d.element_fields()
                sa = d.slip_activity(k=0.5, sigma_y=SIGMA_Y)
                out.append(dict(lattice=d.lattice_strains(HKL, tol_deg=15.0), grains=d.grain_averages(), texture=d.pole_figures(),
                                curvature=d.lattice_curvature(BURGERS)["summary"], fatigue=sa["summary"], fatigue_grains=sa["grains"],
                                elements=len(f["GlobalElementId"]), launches=_launches(d)))
            res[r] = out
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    L.exa_loopback_group_destroy(gid)
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    assert sum(res[r][0]["elements"] for r in range(nranks)) == N ** 3
    for s0, s1 in zip(res[0], res[1]):
        for k in ("lattice", "grains", "texture", "fatigue_grains"):
            _same(s0[k], s1[k])
        assert s0["curvature"] == s1["curvature"] and s0["fatigue"] == s1["fatigue"]
        assert s0["launches"] == s1["launches"]
    # the start of the accumulators, then per step the commit's launch and the explicit one; the five analyses that follow share the latter
    assert [s["launches"] for s in res[0]] == [3, 5, 7]
