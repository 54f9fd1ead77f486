"""The multigrid preconditioner on a periodic cell, host side (no GPU; DESIGN 4.6, "periodic cells"): [BCs] periodic = true together with
[Solvers.Krylov] preconditioner = "multigrid" and mg_periodic = true is read, with and without periodic_free; without mg_periodic the combination
is refused as it always was, and the refusals that stay still carry their messages."""
import ctypes as C
import os

from test_periodic_host import REF, VGRAD, _periodic_text


def _precond(tmp_path, text):
    import exaconstit_amd.lib as L
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    f = tmp_path / "case.toml"
    f.write_text(text)
    out = (C.c_int * 3)(-1, -1, -1); err = C.create_string_buffer(512)
    rc = L.exa_options_query_solver(str(f).encode(), out, err, 512)
    return rc, err.value.decode(), list(out)


def _mg(text, extra="", opt_in=True):
    assert "[Solvers.Krylov]" in text and "ref_ser = 1" in text
    keys = '[Solvers.Krylov]\n        preconditioner = "multigrid"\n' + ("        mg_periodic = true\n" if opt_in else "") + extra
    return text.replace("[Solvers.Krylov]", keys).replace("ref_ser = 1", "ref_ser = 0")


def test_periodic_multigrid_is_read(tmp_path):
    rc, msg, out = _precond(tmp_path, _mg(_periodic_text()))
    assert rc == 0, msg
    assert out == [2, 0, 2]
    rc, msg, out = _precond(tmp_path, _mg(_periodic_text(), "        mg_levels = 1\n        mg_smoother_degree = 3\n"))
    assert rc == 0, msg
    assert out == [2, 1, 3]
    # uniaxial stress: xx and yy free
    rc, msg, out = _precond(tmp_path, _mg(_periodic_text(extra="    periodic_free = [[1, 0, 0], [0, 1, 0], [0, 0, 0]]\n")))
    assert rc == 0, msg
    assert out[0] == 2
    # the other preconditioners of a periodic file
    rc, msg, out = _precond(tmp_path, _periodic_text())
    assert rc == 0 and out[0] == 0, msg
    rc, msg, out = _precond(tmp_path, _periodic_text().replace("[Solvers.Krylov]", '[Solvers.Krylov]\n        preconditioner = "jacobi"'))
    assert rc == 0 and out[0] == 1, msg


def test_refusals_that_stay(tmp_path):
    # without the opt-in key the combination is refused, with a message that names the key
    for extra in ("", "        mg_periodic = false\n"):
        rc, msg, _ = _precond(tmp_path, _mg(_periodic_text(), extra, opt_in=False))
        assert rc == -1 and "periodic" in msg and "multigrid" in msg and "mg_periodic = true" in msg
    rc, msg, _ = _precond(tmp_path, _mg(_periodic_text(), "        mg_periodic = 1\n", opt_in=False))
    assert rc == -1 and "mg_periodic must be true or false" in msg
    # a file that is not periodic may carry the key
    rc, msg, out = _precond(tmp_path, _mg(open(os.path.join(REF, "voce_ea_cs.toml")).read()))
    assert rc == 0 and out[0] == 2, msg
    txt = _mg(_periodic_text())
    # file mesh: refused as a periodic file mesh or as a multigrid file mesh, whichever the reader meets first - both name the generated mesh
    other = txt.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh"))
    assert other != txt
    rc, msg, _ = _precond(tmp_path, other)
    assert rc == -1 and 'Mesh.type = "auto"' in msg
    nonper = _mg(open(os.path.join(REF, "voce_ea_cs.toml")).read())
    other = nonper.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh"))
    rc, msg, _ = _precond(tmp_path, other)
    assert rc == -1 and "multigrid" in msg and "needs a generated mesh" in msg
    # p = 2
    assert "p_refinement = 1" in txt
    rc, msg, _ = _precond(tmp_path, txt.replace("p_refinement = 1", "p_refinement = 2"))
    assert rc == -1 and "multigrid" in msg and "p_refinement = 1 only" in msg
    # B-bar
    assert '    assembly = "EA"' in txt and "integ_model" not in txt
    rc, msg, _ = _precond(tmp_path, txt.replace('    assembly = "EA"', '    assembly = "EA"\n    integ_model = "BBAR"'))
    assert rc == -1 and "multigrid" in msg and "BBAR" in msg
    # the smoother degree and the level count keep their ranges
    rc, msg, _ = _precond(tmp_path, _mg(_periodic_text(), "        mg_smoother_degree = 9\n"))
    assert rc == -1 and "mg_smoother_degree" in msg
    assert VGRAD in txt
