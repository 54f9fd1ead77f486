"""ParaView output of the per-element fields, host side: the VTU / PVTU / PVD writer (host/vtu.hpp) on a fixed two-hexahedron piece and the
Visualizations options (reference src/option_parser.cpp:540-570).  No GPU."""
import base64
import os
import shutil
import xml.etree.ElementTree as ET

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
DT = {"Float64": np.float64, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8}


def decode(da):
    """inline binary DataArray: base64(UInt32 byte count) followed by base64(data), two separately padded blocks"""
    txt = "".join(da.text.split())
    n = np.frombuffer(base64.b64decode(txt[:8]), np.uint32)[0]
    raw = base64.b64decode(txt[8:])
    assert len(raw) == n
    a = np.frombuffer(raw, DT[da.get("type")])
    nc = int(da.get("NumberOfComponents", "1"))
    return a.reshape(-1, nc) if nc > 1 else a


def arrays(section):
    return {da.get("Name"): da for da in section.findall("DataArray")}


def _selftest_mesh():
    NN = 12
    xr = np.zeros(3 * NN)
    xc = np.zeros(3 * NN)
    v = np.zeros(3 * NN)
    for g in range(NN):
        ijk = (float(g % 3), float((g // 3) % 2), float(g // 6))
        for c in range(3):
            m = g + NN * c
            xr[m] = ijk[c]
            xc[m] = ijk[c] + 0.01 * m
            v[m] = 0.5 * m
    return xr.reshape(3, NN).T, xc.reshape(3, NN).T, v.reshape(3, NN).T


@pytest.mark.parametrize("light_up", [0, 1])
def test_vtu_selftest_round_trip(tmp_path, light_up):
    import ctypes as C

    import exaconstit_amd.lib as L
    rng = np.random.default_rng(7 + light_up)
    fields = rng.standard_normal((2, L.EXA_NFIELDS))
    fields[:, 0] = [1.0, 1.25]
    d = str(tmp_path / "results" / "exaconstit")
    err = C.create_string_buffer(512)
    assert L.exa_vtu_selftest(d.encode(), fields.ctypes.data_as(C.POINTER(C.c_double)), light_up, err, 512) == 0, err.value

    # collection: both cycles with their times, each pointing at its parallel file
    pvd = ET.parse(os.path.join(d, "exaconstit.pvd")).getroot()
    assert pvd.get("type") == "Collection"
    ds = pvd.find("Collection").findall("DataSet")
    assert [(x.get("file"), float(x.get("timestep"))) for x in ds] == [("Cycle000000/data.pvtu", 0.0), ("Cycle000001/data.pvtu", 0.5)]

    xr, xc, v = _selftest_mesh()
    names_expected = {"ElementVolume", "LatticeOrientation", "Stress", "VonMisesStress", "HydrostaticStress", "DpEff", "EffPlasticStrain",
                      "ShearRate", "Hardness", "attribute", "GlobalElementId"} | ({"ElemCentroid", "XtalElasticStrain"} if light_up else set())
    for cyc in (0, 1):
        cdir = os.path.join(d, "Cycle%06d" % cyc)
        pv = ET.parse(os.path.join(cdir, "data.pvtu")).getroot()
        assert pv.get("type") == "PUnstructuredGrid"
        g = pv.find("PUnstructuredGrid")
        assert [p.get("Source") for p in g.findall("Piece")] == ["proc000000.vtu"]
        assert {a.get("Name") for a in g.find("PCellData").findall("PDataArray")} == names_expected
        assert {a.get("Name") for a in g.find("PPointData").findall("PDataArray")} == {"Displacement", "Velocity"}

        root = ET.parse(os.path.join(cdir, "proc000000.vtu")).getroot()
        assert root.get("type") == "UnstructuredGrid" and root.get("header_type") == "UInt32"
        piece = root.find("UnstructuredGrid").find("Piece")
        assert piece.get("NumberOfPoints") == "12" and piece.get("NumberOfCells") == "2"
        pts = decode(piece.find("Points").find("DataArray"))
        assert pts.shape == (12, 3) and np.array_equal(pts, xc)
        cells = arrays(piece.find("Cells"))
        conn = decode(cells["connectivity"])
        assert cells["connectivity"].get("type") == "Int32"
        assert np.array_equal(np.ravel(conn), [0, 1, 4, 3, 6, 7, 10, 9, 1, 2, 5, 4, 7, 8, 11, 10])
        assert np.array_equal(decode(cells["offsets"]), [8, 16])
        assert np.array_equal(decode(cells["types"]), [12, 12])                  # VTK_HEXAHEDRON
        pd = arrays(piece.find("PointData"))
        assert np.array_equal(decode(pd["Displacement"]), xc - xr)
        assert np.array_equal(decode(pd["Velocity"]), v)
        cd = arrays(piece.find("CellData"))
        assert set(cd) == names_expected
        for name, (c0, n) in L.ELEMENT_FIELDS.items():
            if name not in names_expected:
                continue
            assert cd[name].get("type") == "Float64"
            got = decode(cd[name])
            assert got.shape == ((2, n) if n > 1 else (2,)), name
            assert np.array_equal(got.reshape(2, n), fields[:, c0:c0 + n]), name          # bit for bit
        assert cd["attribute"].get("type") == "Int32" and np.array_equal(decode(cd["attribute"]), [1, 2])
        assert cd["GlobalElementId"].get("type") == "Int64" and np.array_equal(decode(cd["GlobalElementId"]), [10, 11])


def _vis_toml(tmp_path, lines):
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a = t.index("[Visualizations]")
    b = t.index("[Solvers]")
    path = os.path.join(str(tmp_path), "voce_pa.toml")
    open(path, "w").write(t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in lines) + t[b:])
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori")) and not os.path.exists(os.path.join(str(tmp_path), f)):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    return path


def test_options_query_vis(tmp_path):
    import exaconstit_amd.lib as L
    # the golden file as it stands: paraview off, steps 1, its own floc
    assert L.options_vis(os.path.join(REFDATA, "voce_pa.toml")) == dict(paraview=False, steps=1, light_up=False, floc="./exaconstit_p1")
    # edited
    p = _vis_toml(tmp_path, ['paraview = true', 'steps = 3', 'light_up = true', 'floc = "out/fields"', 'avg_stress_fname = "s.txt"'])
    assert L.options_vis(p) == dict(paraview=True, steps=3, light_up=True, floc="out/fields")
    # the reference's defaults (src/option_parser.cpp:540-570): steps 1, paraview / light_up off, floc "results/exaconstit"
    p = _vis_toml(tmp_path, ['avg_stress_fname = "s.txt"'])
    assert L.options_vis(p) == dict(paraview=False, steps=1, light_up=False, floc="results/exaconstit")
    # the other writers are read like the reference's file and leave the solve unchanged
    p = _vis_toml(tmp_path, ['visit = true', 'conduit = true', 'adios2 = true'])
    assert L.options_vis(p)["paraview"] is False
    p = _vis_toml(tmp_path, ['paraview = true', 'steps = 0'])
    with pytest.raises(RuntimeError, match="steps"):
        L.options_vis(p)
