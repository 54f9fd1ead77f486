"""Host side of the slip-activity / fatigue analysis: the Visualizations.fatigue* options, the slip-plane normal tables against the
Schmid tensors the constitutive kernels use, the size query and the readers of the driver's two text files.  No GPU."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
# {111}<110> in the order of the slip rates (state slots 14 .. 25); the BCC {110}<111> table is this one with planes and directions exchanged
PLANES_111 = np.array([[1, 1, 1]] * 3 + [[-1, 1, 1]] * 3 + [[-1, -1, 1]] * 3 + [[1, -1, 1]] * 3, float)
DIRS_110 = np.array([[0, 1, -1], [-1, 0, 1], [1, -1, 0], [-1, 0, -1], [0, -1, 1], [1, 1, 0], [0, -1, -1], [1, 0, 1], [-1, 1, 0], [1, 0, -1], [0, 1, 1],
                     [-1, -1, 0]], float)


def _stage(tmp_path, vis_lines, name="voce_pa.toml"):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines) + t[b:]
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write(t)
    return path


def test_option_defaults_and_values(tmp_path):
    import exaconstit_amd.lib as L
    assert L.options_fatigue(_stage(tmp_path, [])) == dict(enabled=False, k=0.5, sigma_y=0.0, cycle_steps=0, fname="fatigue.txt")
    o = L.options_fatigue(_stage(tmp_path, ["fatigue = true", "fatigue_k = 0.25", "fatigue_sigma_y = 0.12", "fatigue_cycle_steps = 8", 'fatigue_fname = "f.txt"']))
    assert o == dict(enabled=True, k=0.25, sigma_y=0.12, cycle_steps=8, fname="f.txt")
    assert L.options_fatigue(_stage(tmp_path, ["fatigue_k = 0", "fatigue_sigma_y = 3"])) == dict(enabled=False, k=0.0, sigma_y=3.0, cycle_steps=0, fname="fatigue.txt")
    # the keys leave the other queries alone, the 20 slots of exa_options_query among them
    base = ["paraview = true", "steps = 3", "grain_avgs = true"]
    a = _stage(tmp_path, base, "a.toml")
    b = _stage(tmp_path, base + ["fatigue = true", "fatigue_sigma_y = 0.1", "fatigue_cycle_steps = 4"], "b.toml")
    assert L.options_grains(a) == L.options_grains(b) and L.options_texture(a) == L.options_texture(b)
    assert L.options_lattice_curvature(a) == L.options_lattice_curvature(b)
    out = []
    for p in (a, b):
        o20, err = np.full(20, -7.0), C.create_string_buffer(512)
        assert L.exa_options_query(p.encode(), o20.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0, err.value
        out.append(o20)
    assert np.array_equal(out[0], out[1]) and not np.any(out[0] == -7.0)


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(REFDATA) if f.endswith(".toml")))
def test_golden_option_files_leave_it_off(name):
    import exaconstit_amd.lib as L
    assert L.options_fatigue(os.path.join(REFDATA, name))["enabled"] is False


@pytest.mark.parametrize("lines,msg", [
    (["fatigue = 1"], "Visualizations.fatigue must be"),
    (['fatigue = "yes"'], "Visualizations.fatigue must be"),
    (["fatigue = true"], "fatigue_sigma_y"),                               # no default yield stress
    (["fatigue_k = -0.1", "fatigue_sigma_y = 1"], "fatigue_k"),
    (['fatigue_k = "k"'], "fatigue_k"),
    (["fatigue_sigma_y = 0"], "fatigue_sigma_y"),
    (["fatigue_sigma_y = -2"], "fatigue_sigma_y"),
    (['fatigue_sigma_y = "s"'], "fatigue_sigma_y"),
    (["fatigue_cycle_steps = -1"], "fatigue_cycle_steps"),
    (["fatigue_cycle_steps = 2.5"], "fatigue_cycle_steps"),
    (['fatigue_cycle_steps = "8"'], "fatigue_cycle_steps"),
    (['fatigue_fname = "out/f.txt"'], "fatigue_fname"),
    (['fatigue_fname = ""'], "fatigue_fname"),
    (["fatigue_fname = 3"], "fatigue_fname"),
])
def test_option_refusals(tmp_path, lines, msg):
    import exaconstit_amd.lib as L
    with pytest.raises(RuntimeError, match=msg):
        L.options_fatigue(_stage(tmp_path, lines))


def _vecd(T):
    """ExaCMech's deviatoric vector of sym(T) (oracle/ecmech_port.hpp, tensor_to_vecd)"""
    a, b = 1.0 / np.sqrt(2.0), 1.0 / np.sqrt(6.0)
    return np.array([a * (T[0, 0] - T[1, 1]), b * (2.0 * T[2, 2] - T[0, 0] - T[1, 1]), a * (T[0, 1] + T[1, 0]), a * (T[0, 2] + T[2, 0]), a * (T[1, 2] + T[2, 1])])


@pytest.mark.parametrize("xtal", ["fcc", "bcc"])
def test_slip_plane_normals(oracle, xtal):
    """unit length, orthogonal to the slip direction of the same system, and vecd(sym(s (x) m)) is the Schmid table of the oracle (slip_geom_fill),
    which the kernels' P_TAB restates: a wrong order or a wrong family of planes fails here"""
    import exaconstit_amd.lib as L
    models = (L.EXA_FCC_VOCE, L.EXA_FCC_VOCE_NL, L.EXA_FCC_KMDD) if xtal == "fcc" else (L.EXA_BCC_VOCE, L.EXA_BCC_VOCE_NL, L.EXA_BCC_KMDD)
    planes, dirs = (PLANES_111, DIRS_110) if xtal == "fcc" else (DIRS_110, PLANES_111)
    P, Q = np.zeros((5, 12)), np.zeros((3, 12))
    dp = C.POINTER(C.c_double)
    oracle.lib().orc_slip_geom(0 if xtal == "fcc" else 1, P.ctypes.data_as(dp), Q.ctypes.data_as(dp))
    for m in models:
        n = L.slip_plane_normals(m)
        assert n.shape == (12, 3)
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 2e-16
        assert np.abs(np.cross(n, planes)).max() <= 2e-16                       # parallel to the listed plane, same sense
        assert np.all(np.einsum("ij,ij->i", n, planes) > 0)
        s = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        assert np.abs(np.einsum("ij,ij->i", n, s)).max() <= 2e-16
        for a in range(12):
            assert np.abs(_vecd(np.outer(s[a], n[a])) - P[:, a]).max() <= 4e-16, (xtal, a)
    with pytest.raises(ValueError):
        L.slip_plane_normals(17)


def test_size_query():
    import exaconstit_amd.lib as L
    assert [L.slip_activity_sizes(E) for E in (0, 1, 64, 65, 125, 2 ** 21)] == [0, 60 * 64, 60 * 64, 60 * 128, 60 * 128, 60 * 2 ** 21]
    with pytest.raises(ValueError):
        L.slip_activity_sizes(-1)
    assert L.EXA_NSLIPACC == 12 * len(L.SLIP_ACC_PLANES) and L.EXA_NFIP == len(L.FIP_COLUMNS)


def test_fatigue_files_round_trip(tmp_path):
    import exaconstit_amd.lib as L
    dp = C.POINTER(C.c_double)
    err = C.create_string_buffer(512)
    rows = np.array([[8, 0.8, 0, 0.1, 1.0 / 3.0, 124, 2.0e-3, np.pi * 1e-2, 1.2345678901234567e-4],
                     [16, 1.6000000000000001, 9, -1.5e-7, 2.5e-3, 2 ** 40 + 3, 4.0e-3, 6.0e-2, 0.0]])
    p = str(tmp_path / "fatigue.txt")
    assert L.exa_fatigue_write(p.encode(), 1, rows[:1].ctypes.data_as(dp), 0, err, 512) == 0, err.value
    assert L.exa_fatigue_write(p.encode(), 1, rows[1:].copy().ctypes.data_as(dp), 1, err, 512) == 0, err.value
    assert len(open(p).read().splitlines()) == 3 and open(p).readline().startswith("# step time window_start_step")
    t = L.read_fatigue(p)
    assert t["step"].dtype == np.int64 and np.array_equal(t["step"], [8, 16]) and np.array_equal(t["window_start_step"], [0, 9])
    assert np.array_equal(t["FIP_max_element"], [124, 2 ** 40 + 3])
    for k, c in (("time", 1), ("FIP_mean", 3), ("FIP_max", 4), ("AccumulatedSlip_mean", 6), ("AccumulatedSlip_max", 7), ("ShearRange_max", 8)):
        assert np.array_equal(t[k], rows[:, c]), k                             # 17 significant digits: the same doubles
    ids = np.array([1, 3, 500], np.int32)
    vals = np.array([[0.25, 1.0 / 7.0, 0.2], [0.5, -1e-9, 3e-3], [0.25, 0.0, 0.0]])
    g = str(tmp_path / "fatigue_grains_000008.txt")
    assert L.exa_fatigue_grains_write(g.encode(), 3, ids.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(dp), err, 512) == 0, err.value
    r = L.read_fatigue_grains(g)
    assert np.array_equal(r["grain_id"], [1, 3, 500]) and np.array_equal(r["volume"], vals[:, 0])
    assert np.array_equal(r["FIP_mean"], vals[:, 1]) and np.array_equal(r["FIP_max"], vals[:, 2])
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("# step time\n1 0.1\n")
    with pytest.raises(ValueError, match="not a fatigue file"):
        L.read_fatigue(bad)
    with pytest.raises(ValueError, match="not a fatigue_grains file"):
        L.read_fatigue_grains(bad)
