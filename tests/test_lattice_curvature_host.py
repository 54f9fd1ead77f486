"""Host side of the lattice-curvature analysis: the Visualizations.lattice_curvature* options, the size query of the C ABI and the
reader of the driver's text file.  No GPU."""
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")


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
    assert L.options_lattice_curvature(_stage(tmp_path, [])) == dict(enabled=False, burgers=1.0, fname="lattice_curvature.txt")
    o = L.options_lattice_curvature(_stage(tmp_path, ["lattice_curvature = true", "lattice_curvature_burgers = 2.5e-7", 'lattice_curvature_fname = "lc.txt"']))
    assert o == dict(enabled=True, burgers=2.5e-7, fname="lc.txt")
    # the keys leave the other queries of the table alone
    base = ["paraview = true", "steps = 3", "grain_avgs = true"]
    a = _stage(tmp_path, base, "a.toml")
    b = _stage(tmp_path, base + ["lattice_curvature = true"], "b.toml")
    assert L.options_grains(a) == L.options_grains(b) and L.options_texture(a) == L.options_texture(b)


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(REFDATA) if f.endswith(".toml")))
def test_golden_option_files_leave_it_off(name):
    import exaconstit_amd.lib as L
    assert L.options_lattice_curvature(os.path.join(REFDATA, name))["enabled"] is False


@pytest.mark.parametrize("line,msg", [
    ("lattice_curvature = 1", "Visualizations.lattice_curvature must be"),
    ('lattice_curvature = "yes"', "Visualizations.lattice_curvature must be"),
    ("lattice_curvature_burgers = 0", "lattice_curvature_burgers"),
    ("lattice_curvature_burgers = -2.5e-7", "lattice_curvature_burgers"),
    ('lattice_curvature_burgers = "b"', "lattice_curvature_burgers"),
    ('lattice_curvature_fname = "out/lc.txt"', "lattice_curvature_fname"),
    ('lattice_curvature_fname = ""', "lattice_curvature_fname"),
    ("lattice_curvature_fname = 3", "lattice_curvature_fname"),
])
def test_option_refusals(tmp_path, line, msg):
    import exaconstit_amd.lib as L
    with pytest.raises(RuntimeError, match=msg):
        L.options_lattice_curvature(_stage(tmp_path, [line]))


def test_size_query():
    import ctypes as C
    import exaconstit_amd.lib as L
    for E in (0, 1, 125, 2 ** 21):
        work, planes = L.curvature_sizes(E)
        assert work >= 5 * E and planes >= 9 and planes % 3 == 0       # the record (omega, V, g); 9 nodal sums, in nodal 3-vectors
    assert L.curvature_sizes(64)[1] == L.curvature_sizes(2 ** 21)[1]
    with pytest.raises(ValueError):
        L.curvature_sizes(-1)
    pl = C.c_int()
    assert L.exa_curvature_sizes(10, None, C.byref(pl)) == 0 and pl.value == L.curvature_sizes(10)[1]
    assert L.EXA_NCURV == 16 and sorted(c0 for c0, _ in L.CURVATURE_COLUMNS.values()) == [0, 3, 4, 5, 14, 15]
    assert sum(n for _, n in L.CURVATURE_COLUMNS.values()) == L.EXA_NCURV


def test_read_lattice_curvature(tmp_path):
    import exaconstit_amd.lib as L
    p = str(tmp_path / "lc.txt")
    open(p, "w").write("# step time grod_mean_deg grod_max_deg kam_mean_deg kam_max_deg gnd_density_mean gnd_density_max\n"
                       "1 0.005 0.10000000000000001 0.5 0.01 0.02 1000.5 20000\n"
                       "3 0.30499999999999999 0.25 1.5 0.03 0.040000000000000001 3000 4.5e4\n")
    t = L.read_lattice_curvature(p)
    assert t["step"].dtype == np.int64 and np.array_equal(t["step"], [1, 3])
    assert np.array_equal(t["time"], [0.005, 0.305])
    assert np.array_equal(t["GROD_mean"], [0.1, 0.25]) and np.array_equal(t["GROD_max"], [0.5, 1.5])
    assert np.array_equal(t["KAM_mean"], [0.01, 0.03]) and np.array_equal(t["KAM_max"], [0.02, 0.04])
    assert np.array_equal(t["GNDDensity_mean"], [1000.5, 3000.0]) and np.array_equal(t["GNDDensity_max"], [20000.0, 45000.0])
    one = str(tmp_path / "one.txt")
    open(one, "w").write(open(p).read().splitlines()[0] + "\n2 0.1 1 2 3 4 5 6\n")
    assert np.array_equal(L.read_lattice_curvature(one)["KAM_max"], [4.0])
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("# step time\n1 0.1\n")
    with pytest.raises(ValueError, match="not a lattice_curvature file"):
        L.read_lattice_curvature(bad)
