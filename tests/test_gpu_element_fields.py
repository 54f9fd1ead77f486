"""Per-element output fields on the GPU: exa_element_fields against a numpy restatement of its column table (include/exaconstit_hip.h), in both
quadrature layouts, and the driver's ParaView output (Visualizations.paraview) built on it - cadence, bits of the files, agreement with the
volume averages, several ranks, the executable."""
import ctypes as C
import os
import shutil
import subprocess
import threading
import xml.etree.ElementTree as ET

import numpy as np
import pytest

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


def element_fields_numpy(J, S, SV, W, xq):
    """J (E,Q,9) column-major dx_i/dxi_j, S (E,Q,6), SV (E,Q,28), W (Q), xq (E,Q,3) -> (E,37)"""
    Jm = J.reshape(J.shape[0], J.shape[1], 3, 3).transpose(0, 1, 3, 2)    # [.., i, j]
    w = W[None, :] * np.linalg.det(Jm)
    vol = w.sum(1)
    avg = lambda f: np.einsum("eq,eqk->ek", w, f) / vol[:, None]      # noqa: E731
    s = avg(S)
    sv = avg(SV)
    out = np.zeros((J.shape[0], 37))
    out[:, 0] = vol
    out[:, 1:4] = avg(xq)
    out[:, 4:10] = s
    out[:, 10] = np.sqrt(0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2 + 6 * (s[:, 3:6] ** 2).sum(1)))
    out[:, 11] = s[:, :3].sum(1) / 3
    out[:, 12] = sv[:, 0]
    out[:, 13] = sv[:, 1]
    out[:, 14] = sv[:, 13]
    out[:, 15:27] = sv[:, 14:26]
    qt = sv[:, 9:13]
    out[:, 27:31] = qt / np.linalg.norm(qt, axis=1)[:, None]
    e = sv[:, 4:9]
    t1, t2, v = e[:, 0] / np.sqrt(2), e[:, 1] / np.sqrt(6), np.log(sv[:, 26])
    out[:, 31:37] = np.stack([t1 - t2 + v, -t1 - t2 + v, np.sqrt(2.0 / 3.0) * e[:, 1] + v, e[:, 4] / np.sqrt(2), e[:, 3] / np.sqrt(2), e[:, 2] / np.sqrt(2)], 1)
    return out


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
