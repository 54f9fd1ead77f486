"""Per-element output fields on the GPU: exa_element_fields against a numpy restatement of its column table (include/exaconstit_hip.h), in both
quadrature layouts, and the driver's ParaView output (Visualizations.paraview) built on it - cadence, bits of the files, agreement with the
volume averages, several ranks, the executable.

Every launch form of the kernel is compared with the reference of tests/fieldref.py on data that can fail: the four p = 1 and the p = 2
hexahedron forms in test_kernel_against_numpy, the run-time-order branch at p = 3 ... 6 (Gauss-Lobatto nodes differ from equispaced ones
there) and the tetrahedron form at p = 1 and 2, straight-sided and curved, in the cases below it; the driver-level cases tie the fields
of tetrahedral and p = 3 runs to the volume averages.  Bound: 1e-13 of a column's scale, 1e-12 for the elastic-strain columns
(fieldref.gpu_bounds).  The new cases print what they measured; EXA_WRITE_RECORDS=1 keeps the lines in profiles/element_field_checks.txt."""
import ctypes as C
import os
import shutil
import subprocess
import threading
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import fieldref as F
import hipref
from fieldref import element_fields_numpy
from test_field_output_host import arrays, decode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
EXE = os.path.join(ROOT, "exaconstit_amd", "mechanics")


def _shape_values(rve0, p):
    """N[e, a, q] of the order-p element from the lattice position of every node of the undistorted mesh (p <= 2: GLL nodes equispaced)"""
    np1 = p + 1
    xg, _ = np.polynomial.legendre.leggauss(np1)
    xg = 0.5 * (xg + 1.0)
    nodes = np.linspace(0.0, 1.0, np1)

    def lag(i, x):
        return np.prod([(x - nodes[m]) / (nodes[i] - nodes[m]) for m in range(np1) if m != i], axis=0)

    V = np.array([[lag(i, x) for x in xg] for i in range(np1)])     # V[i, qi]
    E, n, NN = rve0["E"], rve0["n"], rve0["NN"]
    X = rve0["X"].reshape(3, NN)
    conn = rve0["conn"].reshape(E, n)
    h = 1.0 / (rve0["N"] * p)
    lo = X[:, conn].min(axis=2)                                      # (3, E)
    ijk = np.rint((X[:, conn] - lo[:, :, None]) / h).astype(int)    # (3, E, n)
    q = np.arange(np1 ** 3)
    qi, qj, qk = q % np1, (q // np1) % np1, q // (np1 * np1)
    return V[ijk[0][:, :, None], qi] * V[ijk[1][:, :, None], qj] * V[ijk[2][:, :, None], qk]   # (E, n, Q)


def _to_layout(a, layout, qf_size):
    """(E, Q, W) -> the context's quadrature layout"""
    E, Q, W = a.shape
    if layout == 0:
        return a.ravel().copy()
    nb = (E + 63) // 64
    b = np.zeros((nb * 64, Q, W))
    b[:E] = a
    out = b.reshape(nb, 64, Q, W).transpose(0, 2, 3, 1).ravel()
    assert out.size == qf_size
    return out


def _from_layout(v, layout, E, Q, W):
    if layout == 0:
        return v.reshape(E, Q, W)
    nb = (E + 63) // 64
    return v.reshape(nb, Q, W, 64).transpose(0, 3, 1, 2).reshape(nb * 64, Q, W)[:E]


def _close(got, ref):
    for c in range(37):
        tol = 1e-12 if c >= 31 else 1e-13
        scale = max(np.abs(ref[:, c]).max(), 1e-300)
        assert np.max(np.abs(got[:, c] - ref[:, c])) <= tol * scale, (c, np.max(np.abs(got[:, c] - ref[:, c])) / scale)


@pytest.mark.parametrize("p,N", [(1, 5), (2, 3)])
@pytest.mark.parametrize("layout", [0, 1])
def test_kernel_against_numpy(oracle, p, N, layout):
    import exaconstit_amd.lib as L
    import hipref
    orc = oracle
    dev = hipref.Dev()
    rve = hipref.make_rve(orc, N, p=p, distort=0.15, seed=3)
    rve0 = hipref.make_rve(orc, N, p=p)
    E, Q, n, NN = rve["E"], rve["Q"], rve["n"], rve["NN"]
    props = np.loadtxt(os.path.join(orc.REFDATA, "props_cp_voce.txt")).ravel()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, p, E)
    ctx.check(L.exa_set_quadrature_layout(ctx.h, layout))
    qs = {w: L.exa_qf_size(ctx.h, w) for w in (6, 9, 28)}
    d_conn = dev.up(rve["conn"])
    ctx.check(L.exa_set_connectivity(ctx.h, hipref.ptr(d_conn), NN))
    d_X = dev.up(rve["X"])
    d_xe = dev.zeros(3 * n * E)
    d_J = dev.zeros(qs[9])
    ctx.check(L.exa_restrict(ctx.h, hipref.ptr(d_X), hipref.ptr(d_xe), None))
    ctx.check(L.exa_jacobians(ctx.h, hipref.ptr(d_xe), hipref.ptr(d_J), None))
    dev.sync()
    J = _from_layout(d_J.cpu().numpy(), layout, E, Q, 9)
    rng = np.random.default_rng(11 * p + layout)
    S = rng.standard_normal((E, Q, 6)) * 100.0
    SV = rng.standard_normal((E, Q, 28))
    SV[:, :, 26] = rng.uniform(0.95, 1.05, (E, Q))
    d_S = dev.up(_to_layout(S, layout, qs[6]))
    d_SV = dev.up(_to_layout(SV, layout, qs[28]))
    W = np.zeros(Q)
    G = np.zeros(n * 3 * Q)
    ctx.check(L.exa_shape_table(ctx.h, G.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))))
    Nv = _shape_values(rve0, p)                                       # (E, n, Q)
    xe = hipref.l_to_e(rve, rve["X"]).reshape(E, 3, n)
    xq = np.einsum("ean,enq->eqa", xe, Nv)
    ref = element_fields_numpy(J, S, SV, W, xq)

    outs = []
    for Jp in ([d_J, d_J] + ([None] if p == 1 else [])):
        d_out = dev.zeros(37 * E)
        ctx.check(L.exa_element_fields(ctx.h, hipref.ptr(Jp) if Jp is not None else None, hipref.ptr(d_S), hipref.ptr(d_SV), hipref.ptr(d_xe),
                                       hipref.ptr(d_out), None), "exa_element_fields")
        dev.sync()
        outs.append(d_out.cpu().numpy().reshape(E, 37))
    _close(outs[0], ref)
    assert np.array_equal(outs[0], outs[1])                            # same bits on every launch
    if p == 1:                                                         # det J from the node coordinates
        _close(outs[2], outs[0])
    if p > 1:                                                          # a Jacobian field is required there
        with pytest.raises(RuntimeError):
            ctx.check(L.exa_element_fields(ctx.h, None, hipref.ptr(d_S), hipref.ptr(d_SV), hipref.ptr(d_xe), hipref.ptr(d_out), None))
    ctx.close()


# ---- the other instantiations: hexahedra at p = 3 ... 6 and tetrahedra (reference: tests/fieldref.py, none of the library's tables;
# tests/test_element_field_inputs_host.py asserts that these inputs tell a wrong node table, point decode, weight table or staged row apart)
def _props():
    return np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()


def _close_to(ck, what, got, ref, tol):
    """_close with a bound per column (fieldref.gpu_bounds: the bounds of _close unless the reference itself is less precise); prints first"""
    err = F.column_errors(got, ref)
    worst = int(np.argmax(err / tol))
    ck.say(f"{what}: worst column {worst}: {err[worst]:.2e} of scale (<= {tol[worst]:.0e}); volume {err[0]:.2e}, centroid {err[1:4].max():.2e}, "
           f"averages {err[4:31].max():.2e}, elastic strain {err[31:].max():.2e}")
    assert np.all(err <= tol), (what, worst, err[worst])


def _launch(L, dev, c, E, geometry, with_J=True):
    """exa_element_fields on the first E elements of a case (AOS, a context of its own): rows (E, 37), or the return code and message when it refuses"""
    Q, n = c["Q"], c["n"]
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, c["p"], E, geometry=geometry)
    assert (ctx.n, ctx.Q) == (n, Q) and L.exa_qf_size(ctx.h, 9) == 9 * Q * E
    d = {k: dev.up(np.array(c[k][:E], dtype=np.float64).ravel()) for k in ("J", "S", "SV", "xe")}
    d_out = dev.zeros(F.NF * E)
    rc = L.exa_element_fields(ctx.h, hipref.ptr(d["J"]) if with_J else None, hipref.ptr(d["S"]), hipref.ptr(d["SV"]), hipref.ptr(d["xe"]), hipref.ptr(d_out), None)
    msg = (L.exa_last_error(ctx.h) or b"").decode()
    dev.sync()
    out = d_out.cpu().numpy().reshape(E, F.NF)
    ctx.close()
    return (rc, msg) if rc != 0 else out


NEEDS_J = ("exa_element_fields: a Jacobian field is required at p > 1 and for tetrahedra (only the p = 1 hexahedron recomputes det J from the "
           "coordinates)")


def _kernel_case(L, ck, what, c, tol, ref, geometry, edges):
    """the checks every new instantiation gets: the reference, the same bits from two launches, the refusal without a Jacobian field, and - at
    `edges` - contexts over the first E' elements, whose rows are the first rows of the full run bit for bit (each lane sums its own element
    in a fixed order, so nothing but the block arithmetic differs)"""
    dev = hipref.Dev()
    E = c["E"]
    got = _launch(L, dev, c, E, geometry)
    _close_to(ck, what, got, ref, tol)
    assert np.array_equal(_launch(L, dev, c, E, geometry), got)
    rc, msg = _launch(L, dev, c, E, geometry, with_J=False)
    ck.say(f"{what}: without a Jacobian field: {rc}, '{msg[:60]}...'")
    assert rc == L.EXA_ERR_ARG and msg == NEEDS_J
    for E1 in edges:
        part = _launch(L, dev, c, E1, geometry)
        ck.say(f"{what}: the first {E1} element(s) alone: {'the same bits' if np.array_equal(part, got[:E1]) else 'DIFFERENT'}")
        assert np.array_equal(part, got[:E1]), E1
    return got


@pytest.mark.parametrize("p,N", [(3, 5), (4, 2), (5, 2), (6, 2)])
def test_high_order_hexahedra_against_numpy(oracle, p, N):
    """the run-time-order branch (Basis1D by value, nat[], np = p + 1 up to 7) on the warped meshes of hipref.ho_inputs with the oracle's
    Jacobians: E = 125 at p = 3 (a full and a partial block), E = 8 above (343 points and nodes per element at p = 6)"""
    import exaconstit_amd.lib as L
    ck = F.Check(f"gpu hexahedra p={p} N={N}")
    c = F.hex_case(oracle, p, N)
    tol, prec = F.gpu_bounds(c["ref"], F.hex_case(oracle, p, N, np.longdouble)["ref"])
    ck.say(f"hex p={p} N={N}: E = {c['E']}, Q = {c['Q']}; float64 reference vs longdouble {prec.max():.2e}; bounds {tol[0]:.0e} / {tol[36]:.0e}")
    _kernel_case(L, ck, f"hex p={p} N={N}", c, tol, c["ref"], L.EXA_GEOM_HEX, (1, 64, 65) if p == 3 else ())
    ck.record()


@pytest.fixture(scope="module")
def tet_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fieldref")


@pytest.mark.parametrize("p,warped", [(1, False), (2, False), (2, True)])
def test_tetrahedra_against_numpy(tet_dir, p, warped):
    """TET = true on the perturbed, shuffled Kuhn mesh with E = 162 (three blocks, the last with 34 elements); at p = 2 also with every node
    moved by hipref.warp_nodes, so that det J varies inside an element.  Volume against sum_q W_q det J_q, the centroid against the mean of the
    four vertices, everything else against the det J-weighted averages"""
    import exaconstit_amd.lib as L
    what = f"tet p={p}{' warped' if warped else ''}"
    ck = F.Check("gpu " + what)
    c = F.tet_case(L, tet_dir, p, warped)
    tol, prec = F.gpu_bounds(c["ref"], F.tet_case(L, tet_dir, p, warped, np.longdouble)["ref"])
    ck.say(f"{what}: E = {c['E']}, Q = {c['Q']}; float64 reference vs longdouble {prec.max():.2e}; bounds {tol[0]:.0e} / {tol[36]:.0e}")
    ref = np.array(c["ref"])
    ref[:, 1:4] = c["vertex_mean"]
    got = _kernel_case(L, ck, what, c, tol, ref, L.EXA_GEOM_TET, (1, 64, 65) if p == 1 else ())
    if not warped:                                                   # straight-sided: the volume is that of the four vertices
        import tet_mesh_util as T
        vol = T.tet_volumes(c["X"].reshape(3, c["NN"]).T, c["conn"].reshape(c["E"], c["n"])[:, :4].astype(np.int64))
        dv = np.abs(got[:, 0] - vol).max() / vol.max()
        ck.say(f"{what}: volume vs tet_volumes {dv:.2e} (<= 1e-13)")
        assert dv <= 1e-13
    # the element-blocked layout stays refused on tetrahedra
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, p, c["E"], geometry=L.EXA_GEOM_TET)
    assert L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64) == L.EXA_ERR_UNSUPPORTED
    ctx.close()
    ck.record()


def _stage(tmp_path, vis_lines, nsteps=5):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")) and not f.endswith("_stress.txt"):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines + ['avg_stress_fname = "test_voce_pa_stress.txt"']) + t[b:]
    assert "nsteps = 40" in t
    t = t.replace("nsteps = 40", "nsteps = %d" % nsteps, 1)
    path = os.path.join(str(tmp_path), "voce_pa.toml")
    open(path, "w").write(t)
    return path


def _read_cycle(floc, cycle, rank=0):
    root = ET.parse(os.path.join(floc, "Cycle%06d" % cycle, "proc%06d.vtu" % rank)).getroot()
    piece = root.find("UnstructuredGrid").find("Piece")
    out = {k: decode(v) for k, v in arrays(piece.find("CellData")).items()}
    out.update({k: decode(v) for k, v in arrays(piece.find("PointData")).items()})
    out["Points"] = decode(piece.find("Points").find("DataArray"))
    out["connectivity"] = decode(arrays(piece.find("Cells"))["connectivity"])
    return out


def _pvd_cycles(floc):
    pvd = ET.parse(os.path.join(floc, os.path.basename(floc) + ".pvd")).getroot()
    return [(x.get("file"), float(x.get("timestep"))) for x in pvd.find("Collection").findall("DataSet")]


def test_driver_paraview_output(oracle, tmp_path):
    import exaconstit_amd.lib as L
    toml = _stage(tmp_path, ["paraview = true", "steps = 2", "light_up = true"])
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=True)
    assert d.run() == 5
    floc = os.path.join(str(tmp_path), "results", "exaconstit")
    cyc = _pvd_cycles(floc)
    assert [c[0] for c in cyc] == ["Cycle%06d/data.pvtu" % i for i in (0, 2, 4, 5)]
    assert sorted(x for x in os.listdir(floc) if x.startswith("Cycle")) == ["Cycle%06d" % i for i in (0, 2, 4, 5)]
    assert cyc[0][1] == 0.0 and all(cyc[i][1] < cyc[i + 1][1] for i in range(3))

    f = d.element_fields()
    vt = _read_cycle(floc, 5)
    for name in L.ELEMENT_FIELDS:
        assert np.array_equal(vt[name].reshape(f[name].shape), f[name]), name        # the file holds the driver's fields bit for bit
    assert np.array_equal(vt["GlobalElementId"], f["GlobalElementId"]) and np.array_equal(vt["attribute"], f["attribute"])
    grains = np.loadtxt(os.path.join(REFDATA, "grains.txt")).astype(int)
    g_ = f["GlobalElementId"]                                                        # ref_ser = 1: the 10^3 children of the 5^3 grain map
    parent = (g_ % 10) // 2 + 5 * (((g_ // 10) % 10) // 2) + 25 * ((g_ // 100) // 2)
    assert np.array_equal(f["attribute"], grains[parent])

    # tied to the volume averages, which are pinned to the reference's golden file
    vol = f["ElementVolume"][:, 0]
    avg = d.avgs(0, 6)[-1]
    assert np.max(np.abs((vol[:, None] * f["Stress"]).sum(0) / vol.sum() - avg)) <= 1e-12 * np.abs(avg).max()

    # Stress = det J-weighted element average of the converged stress (begin-of-step after the swap), det J from the written coordinates
    E = 1000
    conn = vt["connectivity"].reshape(E, 8)
    x_ref = vt["Points"] - vt["Displacement"]
    assert np.all(np.abs(x_ref * 10 - np.rint(x_ref * 10)) < 1e-12)                 # the undeformed 10^3 grid of the unit cube
    xe = (x_ref + vt["Displacement"])[conn]                                          # (E, 8, 3) converged coordinates
    g = np.array([0.21132486540518713, 0.78867513459481287])
    VX, VY, VZ = [0, 1, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1]
    n1 = lambda v, t: t if v else 1.0 - t                                           # noqa: E731
    d1 = lambda v: 1.0 if v else -1.0                                               # noqa: E731
    det = np.zeros((E, 8))
    for q in range(8):
        X_, Y_, Z_ = g[q & 1], g[(q >> 1) & 1], g[(q >> 2) & 1]
        Gq = np.array([[d1(VX[a]) * n1(VY[a], Y_) * n1(VZ[a], Z_), n1(VX[a], X_) * d1(VY[a]) * n1(VZ[a], Z_), n1(VX[a], X_) * n1(VY[a], Y_) * d1(VZ[a])]
                       for a in range(8)])
        det[:, q] = np.linalg.det(np.einsum("eai,aj->eij", xe, Gq))
    S = np.stack([d.qf_component(2, k).reshape(E, 8) for k in range(6)], 2)
    w = det / 8.0
    ref = np.einsum("eq,eqk->ek", w, S) / w.sum(1)[:, None]
    assert np.max(np.abs(ref - f["Stress"])) <= 1e-12 * np.abs(ref).max()
    d.close()

    # the same run with paraview off writes no results directory
    t2 = tmp_path / "off"
    t2.mkdir()
    toml = _stage(t2, ["paraview = false", "steps = 2", "light_up = true"], nsteps=2)
    d = L.Driver.from_toml(toml, out_dir=str(t2), write_files=True)
    assert d.run() == 2
    assert not os.path.exists(str(t2 / "results"))
    d.close()


def _volume_average_identity(ck, what, d, f):
    """sum_e V_e Stress_e / sum_e V_e is the last row of the volume averages, as test_driver_paraview_output holds for p = 1 hexahedra"""
    vol = f["ElementVolume"][:, 0]
    avg = d.avgs(0, 6)[-1]
    err = np.max(np.abs((vol[:, None] * f["Stress"]).sum(0) / vol.sum() - avg)) / np.abs(avg).max()
    spread = np.abs(f["Stress"] - avg).max() / np.abs(avg).max()
    ck.say(f"{what}: volume-weighted mean of the element stresses vs the volume average {err:.2e} (<= 1e-12); element stresses differ from it by up to {spread:.2f} of it")
    assert spread > 0.05                                                             # several grains: the state is not uniform
    assert err <= 1e-12


@pytest.mark.parametrize("p", [1, 2])
def test_driver_fields_on_a_tetrahedral_polycrystal(tmp_path, p):
    """two steps on the 384-tetrahedron file mesh of test_gpu_tetrahedra._poly (several grains): the fields against the volume averages; at
    p = 1, where the elements stay straight-sided, also Stress against the W_q-weighted mean of the point stresses (det J is one number per
    element) and ElementVolume against the tetrahedra of the coordinates the fields were taken in"""
    import exaconstit_amd.lib as L
    import tet_mesh_util as T
    from test_gpu_tetrahedra import _poly, _steps, _toml
    ck = F.Check(f"gpu driver tet p={p}")
    mesh = _poly(tmp_path)
    d = _steps(L, _toml(tmp_path, "fields%d" % p, mesh=mesh, p=p), 2, tmp_path)
    f = d.element_fields()
    E = len(f["GlobalElementId"])
    assert E == 384 and len(set(f["attribute"].tolist())) > 10
    _volume_average_identity(ck, f"tet p={p}", d, f)
    if p == 1:
        _, W, _ = T.ref_tables_numpy(1)
        S = np.stack([d.qf_component(2, k).reshape(E, W.size) for k in range(6)], 2)
        ref = np.einsum("q,eqk->ek", W, S) / W.sum()
        err = np.max(np.abs(ref - f["Stress"])) / np.abs(ref).max()
        inside = np.abs(S - S[:, :1]).max() / np.abs(ref).max()
        ck.say(f"tet p=1: Stress vs sum_q W_q S_q / sum_q W_q of the point stresses {err:.2e} (<= 1e-12); the point stresses of an element differ by {inside:.1e} "
               f"(a linear tetrahedron has one velocity gradient: this pins which rows are read, not the weights - test_tetrahedra_against_numpy does that)")
        assert err <= 1e-12
        # one rank: the driver keeps the reader's element and node order
        _, NN, n, conn, X0 = F.tet_mesh_arrays(L, mesh, 1)
        assert np.array_equal(f["GlobalElementId"], np.arange(E)) and np.array_equal(d.nodal_field("coords_ref"), X0.reshape(3, NN).T)
        vol = T.tet_volumes(d.nodal_field("coords"), conn.reshape(E, n).astype(np.int64))
        dv = np.abs(f["ElementVolume"][:, 0] - vol).max() / vol.max()
        moved = np.abs(vol - T.tet_volumes(X0.reshape(3, NN).T, conn.reshape(E, n).astype(np.int64))).max() / vol.max()
        ck.say(f"tet p=1: ElementVolume vs the tetrahedra of the end-of-step coordinates {dv:.2e} (<= 1e-13); the step moved the volumes by {moved:.2e}")
        assert dv <= 1e-13 and moved > 1e-9
    d.close()
    ck.record()


def test_driver_fields_on_order3_hexahedra(oracle, tmp_path):
    """two steps of the generated 5^3 mesh at p_refinement = 3 (125 grains): the run-time-order branch under the driver"""
    import exaconstit_amd.lib as L
    from test_gpu_driver import _variant_toml
    ck = F.Check("gpu driver hex p=3")
    toml = _variant_toml(tmp_path, "voce_pa.toml", [("prefinement = 1", "p_refinement = 3"), ("ref_ser = 1", "ref_ser = 0")], "p3fields")
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    for ti in (1, 2):
        assert d.step(ti)
    assert d.mesh_info()["order"] == 3 and d.mesh_info()["elements"] == 125
    _volume_average_identity(ck, "hex p=3", d, d.element_fields())
    d.close()
    ck.record()


def test_two_loopback_ranks_match_one(oracle, tmp_path):
    import exaconstit_amd.lib as L
    toml = _stage(tmp_path, ["paraview = true", "steps = 3"], nsteps=3)

    def run(nranks, out):
        os.makedirs(out, exist_ok=True)
        gid = (C.c_ubyte * 128)()
        assert L.exa_loopback_group_create(nranks, gid) == 0
        res, errors = [None] * nranks, []

        def work(r):
            try:
                d = L.Driver.from_toml(toml, out_dir=out, rank=r, nranks=nranks, uid=gid, write_files=True)
                assert d.run() == 3
                res[r] = d.element_fields()
                d.close()
            except Exception as e:   # noqa: BLE001
                errors.append((r, repr(e)))
        th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        [t.start() for t in th]
        [t.join(timeout=600) for t in th]
        L.exa_loopback_group_destroy(gid)
        assert not errors, errors
        assert all(not t.is_alive() for t in th), "a rank hung"
        return res

    one = run(1, str(tmp_path / "r1"))[0]
    two = run(2, str(tmp_path / "r2"))
    gids = np.concatenate([r["GlobalElementId"] for r in two])
    assert np.array_equal(np.sort(gids), np.arange(1000))
    order = np.argsort(one["GlobalElementId"])
    for name in L.ELEMENT_FIELDS:
        a = one[name][order]
        b = np.concatenate([r[name] for r in two])[np.argsort(gids)]
        assert np.max(np.abs(a - b)) <= 1e-9 * max(np.abs(a).max(), 1e-300), name
    floc = str(tmp_path / "r2" / "results" / "exaconstit")
    pv = ET.parse(os.path.join(floc, "Cycle000003", "data.pvtu")).getroot()
    assert [p.get("Source") for p in pv.find("PUnstructuredGrid").findall("Piece")] == ["proc000000.vtu", "proc000001.vtu"]
    for r in (0, 1):
        vt = _read_cycle(floc, 3, r)
        assert np.array_equal(vt["GlobalElementId"], two[r]["GlobalElementId"])


def test_executable_writes_pvd(tmp_path):
    assert os.path.exists(EXE)
    _stage(tmp_path, ["paraview = true", "steps = 2", 'floc = "vis/run"'], nsteps=5)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}
    r = subprocess.run([EXE, "-opt", "voce_pa.toml"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    cyc = _pvd_cycles(os.path.join(str(tmp_path), "vis", "run"))
    assert [c[0] for c in cyc] == ["Cycle%06d/data.pvtu" % i for i in (0, 2, 4, 5)]
