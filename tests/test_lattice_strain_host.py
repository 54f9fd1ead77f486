"""Light-up analysis, host side: the cubic fibre axes of a plane family (exa_cubic_fiber_axes) against a numpy orbit of the 24 proper cubic
rotations, and the Visualizations.light_up_* options (exa_options_query_lightup): defaults, a full table, every refused value, the golden files.
No GPU."""
import itertools
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")


def cubic_rotations():
    """the 24 proper rotations of the cubic group: signed permutation matrices of determinant +1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for i in range(3):
                M[i, perm[i]] = signs[i]
            if np.linalg.det(M) > 0:
                out.append(M)
    assert len(out) == 24
    return out


def fiber_axes_numpy(hkl):
    """distinct unit axes of the orbit of hkl / |hkl|, c and -c folded (first non-zero component positive)"""
    c = np.asarray(hkl, float)
    c = c / np.linalg.norm(c)
    axes = []
    for S in cubic_rotations():
        a = S @ c
        nz = a[np.abs(a) > 0]
        if nz[0] < 0:
            a = -a
        if not any(np.allclose(a, b, atol=1e-14) for b in axes):
            axes.append(a)
    return np.array(axes)


@pytest.mark.parametrize("hkl,count", [((1, 1, 1), 4), ((2, 0, 0), 3), ((2, 2, 0), 6), ((3, 1, 1), 12), ((1, 2, 3), 24), ((0, 0, 5), 3), ((-1, 1, 1), 4)])
def test_cubic_fiber_axes(hkl, count):
    import exaconstit_amd.lib as L
    got = L.cubic_fiber_axes(*hkl)
    assert got.shape == (count, 3)
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-15)
    ref = fiber_axes_numpy(hkl)
    assert len(ref) == count
    # the same set of axes (folded by sign), each exactly once
    for a in ref:
        m = [i for i, b in enumerate(got) if np.allclose(a, b, atol=1e-15) or np.allclose(a, -b, atol=1e-15)]
        assert len(m) == 1, (a, got)
    # every axis is a signed permutation of hkl / |hkl|, bit for bit
    c = np.asarray(hkl, float) / np.sqrt(float(np.dot(hkl, hkl)))
    assert all(sorted(np.abs(a)) == sorted(np.abs(c)) for a in got)


def test_cubic_fiber_axes_refuses_000():
    import exaconstit_amd.lib as L
    with pytest.raises(ValueError):
        L.cubic_fiber_axes(0, 0, 0)
    assert L.exa_cubic_fiber_axes(1, 2, 3, None, 0) == 24          # count without output


def _stage(tmp_path, vis_lines):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines) + t[b:]
    path = os.path.join(str(tmp_path), "voce_pa.toml")
    open(path, "w").write(t)
    return path


def test_lightup_options_defaults(tmp_path):
    import exaconstit_amd.lib as L
    o = L.options_lightup(_stage(tmp_path, ["light_up = true"]))
    assert o == dict(enabled=False, hkl=[], s_dir=(0.0, 0.0, 1.0), tol_deg=5.0, strain_fname="lattice_strains.txt", volume_fname="lattice_volumes.txt")
    # the families alone do not switch the analysis on
    o = L.options_lightup(_stage(tmp_path, ["light_up = false", "light_up_hkl = [[1, 1, 1]]"]))
    assert not o["enabled"] and o["hkl"] == [(1, 1, 1)]
    o = L.options_lightup(_stage(tmp_path, ["light_up_hkl = [[1, 1, 1]]"]))
    assert not o["enabled"]


def test_lightup_options_full_table(tmp_path):
    import exaconstit_amd.lib as L
    o = L.options_lightup(_stage(tmp_path, ["light_up = true", "light_up_hkl = [[1,1,1],[2,0,0],[2,2,0],[3,1,1]]", "light_up_s_dir = [1.0, 0.0, 1.0]",
                                            "light_up_dist_tol_deg = 7.5", 'light_up_strain_fname = "ls.txt"', 'light_up_volume_fname = "lv.txt"']))
    assert o["enabled"]
    assert o["hkl"] == [(1, 1, 1), (2, 0, 0), (2, 2, 0), (3, 1, 1)]
    assert np.allclose(o["s_dir"], [np.sqrt(0.5), 0.0, np.sqrt(0.5)], rtol=0, atol=1e-15)
    assert o["tol_deg"] == 7.5 and o["strain_fname"] == "ls.txt" and o["volume_fname"] == "lv.txt"
    o = L.options_lightup(_stage(tmp_path, ["light_up = true", "light_up_hkl = [[-1, 2, 3]]", "light_up_dist_tol_deg = 90"]))
    assert o["enabled"] and o["hkl"] == [(-1, 2, 3)] and o["tol_deg"] == 90.0
    o = L.options_lightup(_stage(tmp_path, ["light_up = true", "light_up_hkl = [%s]" % ", ".join(["[1, 1, 1]"] * 16)]))
    assert len(o["hkl"]) == 16


@pytest.mark.parametrize("line,msg", [
    ("light_up_hkl = [[1, 1]]", "triple"),
    ("light_up_hkl = [[1, 1, 1, 1]]", "triple"),
    ("light_up_hkl = [[1, 1, 1], [2, 0]]", "triple"),
    ("light_up_hkl = [[0, 0, 0]]", "[0, 0, 0]"),
    ("light_up_hkl = [%s]" % ", ".join(["[1, 1, 1]"] * 17), "16"),
    ("light_up_hkl = [[1.5, 0, 0]]", "integers"),
    ("light_up_s_dir = [0, 0, 0]", "s_dir"),
    ("light_up_dist_tol_deg = 0", "(0, 90]"),
    ("light_up_dist_tol_deg = -5", "(0, 90]"),
    ("light_up_dist_tol_deg = 90.5", "(0, 90]"),
])
def test_lightup_options_refused(tmp_path, line, msg):
    import exaconstit_amd.lib as L
    lines = ["light_up = true", line]
    if not line.startswith("light_up_hkl"):
        lines.append("light_up_hkl = [[1, 1, 1]]")
    with pytest.raises(RuntimeError, match=msg.replace("[", r"\[").replace("]", r"\]").replace("(", r"\(").replace(")", r"\)")):
        L.options_lightup(_stage(tmp_path, lines))


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(REFDATA) if f.endswith(".toml")))
def test_golden_option_files_leave_lightup_off(name):
    import exaconstit_amd.lib as L
    o = L.options_lightup(os.path.join(REFDATA, name))
    assert not o["enabled"] and o["hkl"] == []
    assert o["s_dir"] == (0.0, 0.0, 1.0) and o["tol_deg"] == 5.0
