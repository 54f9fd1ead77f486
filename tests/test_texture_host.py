"""Texture, host side: the grid and its solid angles, the binning rules through exa_texture_bin (the code the kernel runs), the
quantum exponent, the Visualizations.texture* options (exa_options_query_texture) and that the existing queries ignore them.  No GPU."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
RESOLUTIONS = [2.0, 2.5, 3.0, 5.0, 6.0, 7.5, 9.0, 10.0, 15.0, 18.0, 30.0]


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


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_grid_solid_angles(res):
    import exaconstit_amd.lib as L
    na, nb = L.texture_grid(res)
    assert na == round(90 / res) and nb == round(360 / res)
    ae, be, sa = L.texture_cells(res)
    assert ae.shape == (na + 1,) and be.shape == (nb + 1,) and sa.shape == (na,)
    assert ae[-1] == 90.0 and be[-1] == 360.0
    assert abs(sa.sum() * nb - 2 * np.pi) < 1e-14
    assert np.all(sa > 0)


@pytest.mark.parametrize("res", [1.0, 1.5, 7.0, 31.0, 45.0, 0.0, -5.0, float("nan")])
def test_grid_refused(res):
    import exaconstit_amd.lib as L
    with pytest.raises(ValueError):
        L.texture_grid(res)
    with pytest.raises(ValueError):
        L.texture_bin([0, 0, 1], res)


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_bin_rules(res):
    import exaconstit_amd.lib as L
    na, nb = L.texture_grid(res)
    assert L.texture_bin([0, 0, 1], res) == (0, 0)
    assert L.texture_bin([0, 0, -1], res) == (0, 0)
    assert L.texture_bin([1, 0, 0], res) == (na - 1, 0)
    assert L.texture_bin([-1, 0, 0], res) == (na - 1, 0)
    assert L.texture_bin([0, -1, 0], res) == L.texture_bin([0, 1, 0], res) == (na - 1, nb // 4)
    assert L.texture_bin([0, 0, 5.0], res) == (0, 0)                               # not normalised: the same direction
    # just below alpha = res: ring 0; just above: ring 1 (beta in the middle of sector 0)
    for frac, ring in ((1 - 1e-9, 0), (1 + 1e-9, 1)):
        a = np.radians(res * frac)
        b = np.radians(0.5 * res)
        assert L.texture_bin([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)], res) == (ring, 0)
    # the lower hemisphere folds through the origin: p and -p share a bin
    rng = np.random.default_rng(int(res * 10))
    for p in rng.standard_normal((200, 3)):
        assert L.texture_bin(p, res) == L.texture_bin(-p, res)
    # the equator: p_z = 0 folds on the sign of p_y, then p_x
    assert L.texture_bin([0.3, -0.7, 0.0], res) == L.texture_bin([-0.3, 0.7, 0.0], res)


def _bin_numpy(p, res):
    """the binning rules restated in numpy"""
    p = np.array(p, float)
    x, y, z = p
    if z < 0 or (z == 0 and (y < 0 or (y == 0 and x < 0))):
        x, y, z = -x, -y, -z
    na, nb = round(90 / res), round(360 / res)
    a = np.degrees(np.arctan2(np.hypot(x, y), z))
    b = np.degrees(np.arctan2(y, x)) if (x != 0 or y != 0) else 0.0
    b = b + 360.0 if b < 0 else b
    return min(int(np.floor(a / res)), na - 1), int(np.floor(b / res)) % nb


def test_bins_match_numpy_off_edges():
    import exaconstit_amd.lib as L
    rng = np.random.default_rng(7)
    for res in (2.0, 5.0, 15.0):
        for p in rng.standard_normal((2000, 3)):
            assert L.texture_bin(p, res) == _bin_numpy(p, res)


def test_quantum_log2():
    import exaconstit_amd.lib as L
    for vmax, n in ((1.0, 1), (1e-3, 2097152), (0.37, 1000), (2.0 ** -40, 6221)):
        q = L.exa_texture_quantum_log2(vmax, n)
        assert 2.0 ** (q + 60) <= vmax * n < 2.0 ** (q + 61)
    assert L.exa_texture_quantum_log2(0.0, 10) == 0


def test_texture_options_defaults(tmp_path):
    import exaconstit_amd.lib as L
    d = L.options_texture(_stage(tmp_path, ["paraview = false"]))
    assert d == dict(enabled=False, hkl=[(1, 1, 1), (2, 0, 0), (2, 2, 0)], ipf_dirs=[(0.0, 0.0, 1.0)], res_deg=5.0, fname="texture")
    d = L.options_texture(_stage(tmp_path, ["texture = true", "texture_hkl = [[3, 1, 1]]", "texture_ipf_dirs = [[0, 0, 2], [1, 1, 0]]",
                                            "texture_res_deg = 10", 'texture_fname = "tex"']))
    assert d["enabled"] and d["hkl"] == [(3, 1, 1)] and d["res_deg"] == 10.0 and d["fname"] == "tex"
    assert np.allclose(d["ipf_dirs"], [(0, 0, 1), (np.sqrt(0.5), np.sqrt(0.5), 0)], rtol=0, atol=1e-15)
    d = L.options_texture(_stage(tmp_path, ["texture = true", "texture_ipf_dirs = []"]))
    assert d["ipf_dirs"] == [] and len(d["hkl"]) == 3


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(REFDATA) if f.endswith(".toml")))
def test_golden_option_files_leave_texture_off(name):
    import exaconstit_amd.lib as L
    assert L.options_texture(os.path.join(REFDATA, name))["enabled"] is False


@pytest.mark.parametrize("line,msg", [
    ("texture = 1", "Visualizations.texture must be"),
    ("texture_res_deg = 7", "texture_res_deg"),
    ("texture_res_deg = 1", "texture_res_deg"),
    ("texture_res_deg = 45", "texture_res_deg"),
    ('texture_res_deg = "5"', "texture_res_deg"),
    ("texture_hkl = [" + ", ".join(["[1, 1, 1]"] * 17) + "]", "texture_hkl"),
    ("texture_hkl = []", "texture_hkl"),
    ("texture_hkl = [[0, 0, 0]]", "texture_hkl"),
    ("texture_hkl = [[1, 1]]", "texture_hkl"),
    ("texture_hkl = [[1.5, 1, 0]]", "texture_hkl"),
    ("texture_ipf_dirs = [[0, 0, 0]]", "texture_ipf_dirs"),
    ("texture_ipf_dirs = [[0, 0, 1], [0, 0, 0]]", "texture_ipf_dirs"),
    ("texture_ipf_dirs = [[0, 0, 1], [0, 1, 0], [1, 0, 0], [1, 1, 1]]", "texture_ipf_dirs"),
    ("texture_ipf_dirs = [[0, 1]]", "texture_ipf_dirs"),
    ('texture_fname = "out/tex"', "texture_fname"),
    ('texture_fname = ""', "texture_fname"),
])
def test_texture_options_refused(tmp_path, line, msg):
    import exaconstit_amd.lib as L
    with pytest.raises(RuntimeError, match=msg):
        L.options_texture(_stage(tmp_path, ["texture = true", line] if not line.startswith("texture =") else [line]))


def test_existing_queries_unchanged_by_texture_keys(tmp_path):
    import exaconstit_amd.lib as L
    base = ["paraview = true", "steps = 3", "light_up = true", "light_up_hkl = [[1, 1, 1]]", 'floc = "vis/out"', "grain_avgs = true"]
    d0, d1 = tmp_path / "a", tmp_path / "b"
    d0.mkdir()
    d1.mkdir()
    p0 = _stage(d0, base)
    p1 = _stage(d1, base + ["texture = true", "texture_hkl = [[1, 1, 1], [3, 1, 1]]", "texture_ipf_dirs = [[1, 0, 0], [0, 1, 0]]",
                            "texture_res_deg = 10", 'texture_fname = "tex"'])

    def q20(p):
        out = np.zeros(20)
        err = C.create_string_buffer(512)
        assert L.exa_options_query(p.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0, err.value
        return out
    assert np.array_equal(q20(p0), q20(p1))
    assert L.options_vis(p0) == L.options_vis(p1)
    assert L.options_lightup(p0) == L.options_lightup(p1)
    assert L.options_grains(p0) == L.options_grains(p1)
    assert L.options_solver(p0) == L.options_solver(p1)
    assert L.options_texture(p0)["enabled"] is False and L.options_texture(p1)["enabled"] is True
