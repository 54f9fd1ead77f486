"""Host logic of the multigrid preconditioner (no GPU): the Solvers.Krylov.preconditioner keys and the level-count rule."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")


def _variant(tmp_path, base, krylov_lines="", edit=None):
    """base options file of tests/golden/refdata with its data files made absolute and extra [Solvers.Krylov] lines"""
    text = open(os.path.join(REF, base)).read()
    for fl in os.listdir(REF):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    if krylov_lines:
        assert text.count("[Solvers.Krylov]") == 1
        text = text.replace("[Solvers.Krylov]", "[Solvers.Krylov]\n" + krylov_lines)
    if edit:
        text = edit(text)
    p = tmp_path / ("v%d.toml" % len(os.listdir(str(tmp_path))))
    p.write_text(text)
    return str(p)


def _q(path):
    import exaconstit_amd.lib as L
    return L.options_solver(path)


def test_defaults_without_the_key():
    for base in ("voce_pa.toml", "voce_ea_cs.toml", "mtsdd_bcc.toml"):
        assert _q(os.path.join(REF, base)) == dict(preconditioner=None, mg_levels=0, mg_smoother_degree=2)


def test_all_values(tmp_path):
    assert _q(_variant(tmp_path, "voce_pa.toml", '    preconditioner = "jacobi"'))["preconditioner"] == "jacobi"
    assert _q(_variant(tmp_path, "voce_pa.toml", '    preconditioner = "Multigrid"')) == dict(preconditioner="multigrid", mg_levels=0, mg_smoother_degree=2)
    got = _q(_variant(tmp_path, "voce_ea_cs.toml", '    preconditioner = "multigrid"\n    mg_levels = 3\n    mg_smoother_degree = 5'))
    assert got == dict(preconditioner="multigrid", mg_levels=3, mg_smoother_degree=5)
    # the two multigrid keys are read only with "multigrid"
    got = _q(_variant(tmp_path, "voce_pa.toml", '    preconditioner = "jacobi"\n    mg_smoother_degree = 99'))
    assert got == dict(preconditioner="jacobi", mg_levels=0, mg_smoother_degree=2)
    # the existing 20-slot query is unchanged by the keys
    import ctypes as C
    import numpy as np
    import exaconstit_amd.lib as L
    a, b = np.zeros(20), np.zeros(20)
    err = C.create_string_buffer(512)
    assert L.exa_options_query(os.path.join(REF, "voce_pa.toml").encode(), a.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0
    assert L.exa_options_query(_variant(tmp_path, "voce_pa.toml", '    preconditioner = "multigrid"').encode(), b.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("lines,edit,msg", [
    ('    preconditioner = "amg"', None, 'must be "jacobi" or "multigrid"'),
    ('    preconditioner = "identity"', None, 'must be "jacobi" or "multigrid"'),
    ('    preconditioner = "multigrid"\n    mg_smoother_degree = 9', None, "mg_smoother_degree"),
    ('    preconditioner = "multigrid"\n    mg_smoother_degree = 0', None, "mg_smoother_degree"),
    ('    preconditioner = "multigrid"\n    mg_levels = -1', None, "mg_levels"),
    ('    preconditioner = "multigrid"', lambda t: t.replace("p_refinement = 1", "p_refinement = 2"), "p_refinement = 1"),
    ('    preconditioner = "multigrid"', lambda t: t.replace('assembly = "EA"', 'assembly = "EA"\n    integ_model = "BBAR"'), "BBAR"),
    ('    preconditioner = "multigrid"',
     lambda t: t.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh")).replace("ref_ser = 1", "ref_ser = 0"),
     "generated mesh"),
])
def test_refusals(tmp_path, lines, edit, msg):
    path = _variant(tmp_path, "voce_ea_cs.toml", lines, edit)
    with pytest.raises(RuntimeError) as e:
        _q(path)
    assert msg in str(e.value)


def test_file_mesh_without_multigrid_still_parses(tmp_path):
    edit = lambda t: t.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh")).replace("ref_ser = 1", "ref_ser = 0")  # noqa: E731
    assert _q(_variant(tmp_path, "voce_ea_cs.toml", '    preconditioner = "jacobi"', edit))["preconditioner"] == "jacobi"


@pytest.mark.parametrize("N,nranks,cap,levels", [
    (128, 1, 0, 6), (128, 2, 0, 5), (128, 8, 0, 5), (128, 1, 2, 2),
    (10, 1, 0, 1),                       # 5^3 coarse elements
    (10, 2, 0, 0),                       # a 10 x 10 x 5 box: refused
    ((12, 8, 6), 1, 0, 1),               # 6 x 4 x 3 after one level
    (16, 1, 0, 3), (16, 8, 0, 2), (16, 2, 0, 2), (32, 1, 0, 4), (8, 1, 0, 2),
    (12, 3, 0, 1),                       # a 12 x 12 x 4 box
    (7, 1, 0, 0),
])
def test_level_count_rule(N, nranks, cap, levels):
    import exaconstit_amd.lib as L
    assert L.mg_level_count(N, nranks, cap) == levels
