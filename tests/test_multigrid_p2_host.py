"""Multigrid at p_refinement = 2, host side (no GPU; DESIGN 4.6, "p = 2"): [Solvers.Krylov] mg_p2 = true next to preconditioner = "multigrid" makes
p_refinement = 2 on a generated mesh legal; what stays refused with the key says why; the level-count rule with the vertex level."""
import os

import pytest

from test_mg_host import REF, _q, _variant
from test_periodic_host import _periodic_text

MG = '    preconditioner = "multigrid"\n'
# (voce_pa.toml spells the key "prefinement", which the reader ignores like the reference does: order 1)
P2 = lambda t: t.replace("p_refinement = 1", "p_refinement = 2").replace("prefinement = 1", "p_refinement = 2")  # noqa: E731
FILE_MESH = lambda t: t.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh")).replace("ref_ser = 1", "ref_ser = 0")  # noqa: E731


def _p2_key(path):
    import exaconstit_amd.lib as L
    return L.options_mg_p2(path)


@pytest.mark.parametrize("base", ["voce_pa.toml", "voce_ea_cs.toml"])      # partial assembly, element assembly; both Mesh.type = "auto"
def test_key_makes_p2_legal(tmp_path, base):
    text = open(os.path.join(REF, base)).read()
    assert 'type = "auto"' in text and P2(text) != text
    path = _variant(tmp_path, base, MG + "    mg_p2 = true", P2)
    assert _q(path) == dict(preconditioner="multigrid", mg_levels=0, mg_smoother_degree=2)
    assert _p2_key(path) is True
    # the key changes nothing at p = 1, and its default is off
    path = _variant(tmp_path, base, MG + "    mg_p2 = true")
    assert _q(path)["preconditioner"] == "multigrid" and _p2_key(path) is True
    assert _p2_key(_variant(tmp_path, base, MG)) is False
    assert _p2_key(os.path.join(REF, base)) is False
    # without the key, or with it off, p = 2 is refused with the message it always had
    for lines in (MG, MG + "    mg_p2 = false"):
        with pytest.raises(RuntimeError) as e:
            _q(_variant(tmp_path, base, lines, P2))
        assert "p_refinement = 1 only" in str(e.value)


@pytest.mark.parametrize("edit,msg", [
    (lambda t: P2(t).replace('assembly = "EA"', 'assembly = "EA"\n    integ_model = "BBAR"'), "BBAR"),
    (lambda t: FILE_MESH(P2(t)), "generated mesh"),
    (lambda t: t.replace("p_refinement = 1", "p_refinement = 3"), "p_refinement >= 3"),
])
def test_refusals_with_the_key(tmp_path, edit, msg):
    base = open(os.path.join(REF, "voce_ea_cs.toml")).read()
    assert edit(base) != P2(base) and edit(base) != base
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, "voce_ea_cs.toml", MG + "    mg_p2 = true", edit))
    assert "multigrid" in str(e.value) and msg in str(e.value)


@pytest.mark.parametrize("mg_periodic,free", [(False, False), (True, False), (True, True)])     # free: mixed loading, xx an unknown
def test_periodic_p2_is_refused(tmp_path, mg_periodic, free):
    import exaconstit_amd.lib as L
    text = _periodic_text(extra="    periodic_free = [[1, 0, 0], [0, 0, 0], [0, 0, 0]]\n" if free else "")
    extra = "        mg_periodic = true\n" if mg_periodic else ""
    assert "[Solvers.Krylov]" in text and "ref_ser = 1" in text and "p_refinement = 1" in text
    text = P2(text.replace("[Solvers.Krylov]", "[Solvers.Krylov]\n" + MG + "        mg_p2 = true\n" + extra).replace("ref_ser = 1", "ref_ser = 0"))
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    f = tmp_path / "case.toml"
    f.write_text(text)
    with pytest.raises(RuntimeError) as e:
        L.options_solver(str(f))
    assert "p_refinement = 2" in str(e.value) and "periodic" in str(e.value)
    # the same file at p = 1 (with mg_periodic) is read
    if mg_periodic:
        f.write_text(text.replace("p_refinement = 2", "p_refinement = 1"))
        assert L.options_solver(str(f))["preconditioner"] == "multigrid"


@pytest.mark.parametrize("value", ["1", '"yes"', "0"])
def test_key_must_be_boolean(tmp_path, value):
    with pytest.raises(RuntimeError) as e:
        _q(_variant(tmp_path, "voce_pa.toml", MG + "    mg_p2 = " + value, P2))
    assert "mg_p2 must be true or false" in str(e.value)


@pytest.mark.parametrize("N,nranks,cap,levels", [
    ((5, 5, 5), 1, 0, 1),
    ((10, 10, 10), 1, 0, 2),             # 10^3 vertices' box -> 5^3
    ((8, 8, 8), 1, 0, 3),
    ((10, 10, 10), 2, 0, 1),             # refused at p = 1 (a 10 x 10 x 5 box), the vertex level alone at p = 2
    ((8, 8, 8), 1, 1, 1),                # the cap counts coarse levels
    ((8, 8, 8), 1, 2, 2),
    ((7, 7, 7), 1, 0, 1),
    ((1, 1, 1), 1, 0, 1),
])
def test_level_count_rule_order2(N, nranks, cap, levels):
    import exaconstit_amd.lib as L
    assert L.mg_level_count_order(N, nranks, cap, 2) == levels


@pytest.mark.parametrize("N,nranks,cap", [
    (128, 1, 0), (128, 2, 0), (128, 8, 0), (128, 1, 2), (10, 1, 0), (10, 2, 0), ((12, 8, 6), 1, 0), (16, 1, 0), (16, 8, 0), (16, 2, 0), (32, 1, 0),
    (8, 1, 0), (12, 3, 0), (7, 1, 0),
])
def test_level_count_order1_is_the_p1_rule(N, nranks, cap):
    import exaconstit_amd.lib as L
    assert L.mg_level_count_order(N, nranks, cap, 1) == L.mg_level_count(N, nranks, cap)
    with pytest.raises(ValueError):
        L.mg_level_count_order(N, nranks, cap, 3)
