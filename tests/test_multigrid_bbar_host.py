"""Multigrid under the B-bar integrator, host side (no GPU; DESIGN 4.6, "B-bar"): [Solvers.Krylov] mg_bbar = true next to preconditioner = "multigrid"
makes integ_model = "BBAR" legal on a generated mesh, at p_refinement = 1 and - with mg_p2 = true - at 2; without the key the refusal it always had
comes back; what stays refused with the key says why; on a FULL file the key changes nothing."""
import os

import pytest

from test_mg_host import REF, _q, _variant
from test_periodic_host import _periodic_text

MG = '    preconditioner = "multigrid"\n'
BBAR = lambda t: t.replace('assembly = "EA"', 'assembly = "EA"\n    integ_model = "BBAR"')  # noqa: E731
P = lambda p: (lambda t: t.replace("p_refinement = 1", "p_refinement = %d" % p))  # noqa: E731
FILE_MESH = lambda t: t.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh")).replace("ref_ser = 1", "ref_ser = 0")  # noqa: E731
BASE = "voce_ea_cs.toml"


def _key(path):
    import exaconstit_amd.lib as L
    return L.options_mg_bbar(path)


def _base_text():
    text = open(os.path.join(REF, BASE)).read()
    assert 'type = "auto"' in text and BBAR(text) != text and P(2)(text) != text and FILE_MESH(text) != text
    return text


def test_key_makes_bbar_legal_at_p1(tmp_path):
    _base_text()
    path = _variant(tmp_path, BASE, MG + "    mg_bbar = true", BBAR)
    assert _q(path) == dict(preconditioner="multigrid", mg_levels=0, mg_smoother_degree=2)
    assert _key(path) is True


def test_key_makes_bbar_legal_at_p2_with_mg_p2(tmp_path):
    import exaconstit_amd.lib as L
    path = _variant(tmp_path, BASE, MG + "    mg_bbar = true\n    mg_p2 = true", lambda t: P(2)(BBAR(t)))
    assert _q(path) == dict(preconditioner="multigrid", mg_levels=0, mg_smoother_degree=2)
    assert _key(path) is True and L.options_mg_p2(path) is True
    # mg_bbar does not stand in for mg_p2: the order is refused as it always was
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, BASE, MG + "    mg_bbar = true", lambda t: P(2)(BBAR(t))))
    assert "p_refinement = 1 only" in str(e.value)


def test_key_is_reported_as_written_and_defaults_to_false(tmp_path):
    assert _key(_variant(tmp_path, BASE, MG + "    mg_bbar = true", BBAR)) is True
    assert _key(_variant(tmp_path, BASE, MG + "    mg_bbar = false")) is False
    assert _key(_variant(tmp_path, BASE, MG)) is False
    assert _key(os.path.join(REF, BASE)) is False


@pytest.mark.parametrize("lines", [MG, MG + "    mg_bbar = false"])
@pytest.mark.parametrize("order", [1, 2])
def test_without_the_key_the_old_refusal_comes_back(tmp_path, lines, order):
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, BASE, lines + ("    mg_p2 = true" if order == 2 else ""), lambda t: P(order)(BBAR(t))))
    assert 'preconditioner = "multigrid" is not built for integ_model = "BBAR"' in str(e.value)


@pytest.mark.parametrize("value", ["1", '"yes"', "0"])
def test_key_must_be_boolean(tmp_path, value):
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, BASE, MG + "    mg_bbar = " + value, BBAR))
    assert "mg_bbar must be true or false" in str(e.value)


@pytest.mark.parametrize("edit,msg", [
    (lambda t: FILE_MESH(BBAR(t)), "generated mesh"),
    (lambda t: P(3)(BBAR(t)), "p_refinement >= 3"),
])
def test_refusals_with_the_key(tmp_path, edit, msg):
    _base_text()
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, BASE, MG + "    mg_bbar = true\n    mg_p2 = true", edit))
    assert "multigrid" in str(e.value) and msg in str(e.value)


@pytest.mark.parametrize("mg_periodic", [True, False])
def test_periodic_bbar_is_refused(tmp_path, mg_periodic):
    import exaconstit_amd.lib as L
    text = _periodic_text()
    assert "[Solvers.Krylov]" in text and "ref_ser = 1" in text and "p_refinement = 1" in text and BBAR(text) != text
    keys = MG + "        mg_bbar = true\n" + ("        mg_periodic = true\n" if mg_periodic else "")
    text = text.replace("[Solvers.Krylov]", "[Solvers.Krylov]\n" + keys).replace("ref_ser = 1", "ref_ser = 0")
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    f = tmp_path / "case.toml"
    f.write_text(BBAR(text))
    with pytest.raises(RuntimeError) as e:
        L.options_solver(str(f))
    assert "mg_bbar" in str(e.value) and "periodic" in str(e.value) and "is not built for BCs.periodic = true" in str(e.value)
    # the same file without B-bar is read (with mg_periodic), and the key changes nothing in it
    if mg_periodic:
        f.write_text(text)
        assert L.options_solver(str(f))["preconditioner"] == "multigrid" and L.options_mg_bbar(str(f)) is True


def test_key_on_a_full_file_changes_nothing(tmp_path):
    import ctypes as C
    import numpy as np
    import exaconstit_amd.lib as L
    with_key, without = _variant(tmp_path, BASE, MG + "    mg_bbar = true"), _variant(tmp_path, BASE, MG)
    assert _q(with_key) == _q(without) == dict(preconditioner="multigrid", mg_levels=0, mg_smoother_degree=2)
    a, b = np.zeros(20), np.zeros(20)
    err = C.create_string_buffer(512)
    assert L.exa_options_query(with_key.encode(), a.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0
    assert L.exa_options_query(without.encode(), b.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0
    assert np.array_equal(a, b)
    assert L.options_mg_p2(with_key) is False
    # next to another preconditioner the key is not read at all, like the other multigrid keys
    assert _q(_variant(tmp_path, BASE, '    preconditioner = "jacobi"\n    mg_bbar = 7'))["preconditioner"] == "jacobi"
