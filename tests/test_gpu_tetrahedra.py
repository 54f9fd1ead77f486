"""Tetrahedral meshes on the MI355X: C-ABI parity of a tetrahedron context against the oracle's table-driven functions (fed
the tables of this test), and end-to-end driver runs on Kuhn-split cubes read from MFEM v1.0 and Gmsh 2.2 files."""
import ctypes as C
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import hipref
import tet_mesh_util as T
from hipref import ptr, rel_l2

pytestmark = pytest.mark.gpu

REF = T.REFDATA


def _mesh_arrays(L, path, order):
    """conn (n, E) flat and X (NN, 3 byNODES) flat of a file mesh as the driver's reader builds it (one rank)."""
    info = (C.c_int64 * 8)(); err = C.create_string_buffer(512)
    assert L.exa_mesh_partition_query_order(path.encode(), 0, 1, order, info, None, None, None, None, None, None, None, err, 512) == 0, err.value
    E, NN, n = info[0], info[1], info[7]
    conn = np.zeros(n * E, np.int32); X = np.zeros(3 * NN)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.exa_mesh_partition_query_order(path.encode(), 0, 1, order, info, vp(conn), vp(X), None, None, None, None, None, err, 512) == 0
    return E, NN, n, conn, X


def _spd_tangent(P, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((P, 6, 6))
    Cm = A @ A.transpose(0, 2, 1) + 6 * np.eye(6)
    Cm *= 50.0
    Cm += 0.05 * rng.standard_normal((P, 6, 6))      # slightly non-symmetric, like a plasticity tangent
    return np.ascontiguousarray(Cm.transpose(0, 2, 1)).ravel()


@pytest.mark.parametrize("p,assembly", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_tet_abi_matches_oracle(oracle, tmp_path, p, assembly):
    """exa_jacobians, exa_model_setup, the residual, the fused exa_grad_apply_lvec, exa_grad_diagonal and exa_grad_get_ea of a tetrahedron context
    against the oracle's table-driven element functions on a distorted, shuffled Kuhn mesh with E = 162 (not a multiple of 64)."""
    import exaconstit_amd.lib as L
    orc = oracle
    dev = hipref.Dev()
    path = T.write_mfem(str(tmp_path / "k3.mesh"), T.kuhn_cube(3, perturb=0.3, shuffle=True, seed=5))
    E, NN, n, conn, X = _mesh_arrays(L, path, p)
    Gt, Wt, _ = T.ref_tables_numpy(p)
    Q = Wt.size; P = E * Q
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, p, E, assembly=assembly, geometry=L.EXA_GEOM_TET)
    assert L.exa_element_geometry(ctx.h) == L.EXA_GEOM_TET and (ctx.n, ctx.Q) == (n, Q)
    G, W = ctx.shape_table()
    assert np.abs(G - Gt).max() < 1e-14 and np.abs(W - Wt).max() < 1e-15
    rve = {"E": E, "n": n, "NN": NN, "conn": conn}
    xe = hipref.l_to_e(rve, X)
    Gq = Gt.reshape(Q, 3, n); xr = xe.reshape(E, 3, n)
    J = np.ascontiguousarray(np.einsum("eia,qja->eqji", xr, Gq)).ravel()      # J[i + 3 j + 9 (q + Q e)] = dx_i / dxi_j
    d_xe = dev.up(xe); d_J = dev.zeros(9 * P)
    ctx.check(L.exa_jacobians(ctx.h, ptr(d_xe), ptr(d_J), None))
    assert rel_l2(d_J.cpu().numpy(), J) < 1e-13
    # constitutive launch (reference layout)
    dt = 0.5
    rng = np.random.default_rng(2)
    d_q = dev.up(hipref.random_quats(E).ravel()); d_sv0 = dev.zeros(28 * P)
    ctx.check(L.exa_init_state(ctx.h, ptr(d_sv0), ptr(d_q), None))
    sv0 = d_sv0.cpu().numpy()
    v = 2e-3 * rng.standard_normal(3 * NN)
    ve = hipref.l_to_e(rve, v)
    s0 = np.zeros(6 * P); s1 = np.zeros(6 * P); sv1 = np.zeros(28 * P); cm = np.zeros(36 * P)
    assert orc.lib().orc_model_setup(0, 0, orc._p(props), len(props), Q, E, n, 28, C.c_double(dt), C.c_double(298.0), orc._p(J), orc._p(Gt), orc._p(ve),
                                     orc._p(s0), orc._p(sv0), orc._p(s1), orc._p(sv1), orc._p(cm), None, 1, 0, 0) == 0
    d_in = [dev.up(a) for a in (ve, s0)]
    d_out = [dev.zeros(6 * P), dev.zeros(28 * P), dev.zeros(36 * P)]
    ctx.check(L.exa_model_setup(ctx.h, dt, ptr(d_J), ptr(d_in[0]), ptr(d_in[1]), ptr(d_sv0), *[ptr(t) for t in d_out], None))
    assert ctx.check(L.exa_model_status(ctx.h, None)) == 0
    assert rel_l2(d_out[0].cpu().numpy(), s1) < 1e-9
    assert rel_l2(d_out[1].cpu().numpy().reshape(P, 28)[:, 13], sv1.reshape(P, 28)[:, 13]) < 1e-10
    assert rel_l2(d_out[2].cpu().numpy(), cm) < 1e-7
    # residual (E-vector route; the fused L-vector residual is a hexahedron kernel and refuses)
    sig = rng.standard_normal(6 * P)
    y_ref = np.zeros(3 * n * E)
    orc.lib().orc_element_vector(Q, E, n, orc._p(Wt), orc._p(Gt), orc._p(J), orc._p(sig), orc._p(y_ref))
    d_sig = dev.up(sig); d_y = dev.zeros(3 * n * E)
    ctx.check(L.exa_residual_setup(ctx.h, ptr(d_J), ptr(d_sig), None))
    ctx.check(L.exa_residual_apply(ctx.h, ptr(d_y), None))
    assert rel_l2(d_y.cpu().numpy(), y_ref) < 1e-12
    d_conn = dev.up(conn); ctx.check(L.exa_set_connectivity(ctx.h, ptr(d_conn), NN))
    assert L.exa_residual_lvec(ctx.h, ptr(d_J), ptr(d_sig), ptr(dev.zeros(3 * NN)), None) == L.EXA_ERR_UNSUPPORTED
    # gradient
    Cm = _spd_tangent(P, seed=8)
    x_e = rng.standard_normal(3 * n * E)
    emat = np.zeros(9 * n * n * E); diag_ref = np.zeros(3 * n * E); yg_ref = np.zeros(3 * n * E)
    orc.lib().orc_assemble_ea(Q, E, n, C.c_double(dt), orc._p(Wt), orc._p(Gt), orc._p(J), orc._p(Cm), orc._p(emat))
    if assembly == 0:
        C4 = np.zeros(81 * P); D4 = np.zeros(81 * P)
        orc.lib().orc_transform_4d(C.c_int64(P), orc._p(Cm), orc._p(C4))
        orc.lib().orc_assemble_grad_pa(Q, E, C.c_double(dt), orc._p(Wt), orc._p(J), orc._p(C4), orc._p(D4))
        orc.lib().orc_add_mult_grad_pa(Q, E, n, orc._p(Gt), orc._p(D4), orc._p(x_e), orc._p(yg_ref))
        orc.lib().orc_assemble_grad_diag_pa(Q, E, n, C.c_double(dt), orc._p(Wt), orc._p(Gt), orc._p(J), orc._p(Cm), orc._p(diag_ref))
    else:
        orc.lib().orc_ea_mult(E, n, orc._p(emat), orc._p(x_e), orc._p(yg_ref))
        orc.lib().orc_ea_diag(E, n, orc._p(emat), orc._p(diag_ref))
        ctx.check(L.exa_set_ea_matrix_free(ctx.h, 1))
    d_C = dev.up(Cm); d_x = dev.up(x_e); d_yg = dev.zeros(3 * n * E); d_diag = dev.zeros(3 * n * E)
    ctx.check(L.exa_grad_setup(ctx.h, dt, ptr(d_J), ptr(d_C), None))
    ctx.check(L.exa_grad_apply(ctx.h, ptr(d_x), ptr(d_yg), None))
    ctx.check(L.exa_grad_diagonal(ctx.h, ptr(d_diag), None))
    assert rel_l2(d_yg.cpu().numpy(), yg_ref) < 1e-12
    assert rel_l2(d_diag.cpu().numpy(), diag_ref) < 1e-12
    # the fused L-vector action (tet_kernels.hip), with and without a mask
    xL = rng.standard_normal(3 * NN); connr = conn.reshape(E, n)
    for mask in ((rng.uniform(size=3 * NN) < 0.1).astype(np.uint8), None):
        xin = xL if mask is None else np.where(mask, 0.0, xL)
        ye = np.zeros(3 * n * E)
        if assembly == 0:
            orc.lib().orc_add_mult_grad_pa(Q, E, n, orc._p(Gt), orc._p(D4), orc._p(hipref.l_to_e(rve, xin)), orc._p(ye))
        else:
            orc.lib().orc_ea_mult(E, n, orc._p(emat), orc._p(hipref.l_to_e(rve, xin)), orc._p(ye))
        yL_ref = np.zeros(3 * NN)
        for c in range(3):
            np.add.at(yL_ref, connr + NN * c, ye.reshape(E, 3, n)[:, c, :])
        d_xL = dev.up(xL); d_mask = dev.up(mask) if mask is not None else None; d_yL = dev.zeros(3 * NN)
        ctx.check(L.exa_grad_apply_lvec(ctx.h, ptr(d_xL), ptr(d_yL), ptr(d_mask) if d_mask is not None else None, None))
        assert rel_l2(d_yL.cpu().numpy(), yL_ref) < 1e-12
    if p == 1:   # J^-1 recomputed from registered nodal coordinates instead of read from the element record
        d_X = dev.up(X); ctx.check(L.exa_grad_set_coords(ctx.h, ptr(d_X)))
        d_yL2 = dev.zeros(3 * NN)
        ctx.check(L.exa_grad_apply_lvec(ctx.h, ptr(d_xL), ptr(d_yL2), None, None))
        assert rel_l2(d_yL2.cpu().numpy(), d_yL.cpu().numpy()) < 1e-13
        ctx.check(L.exa_grad_set_coords(ctx.h, None))
    if assembly == 1:
        d_em = dev.zeros(9 * n * n * E)
        ctx.check(L.exa_grad_get_ea(ctx.h, ptr(d_em), None))
        assert rel_l2(d_em.cpu().numpy(), emat) < 1e-12
    # hexahedron-only routes refuse
    assert L.exa_set_tangent_form(ctx.h, L.EXA_TANGENT_DEV5_BULK) == L.EXA_ERR_UNSUPPORTED
    assert L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64) == L.EXA_ERR_UNSUPPORTED
    assert L.exa_model_setup_lvec_records(ctx.h, dt, ptr(d_xL), ptr(d_xL), ptr(d_in[1]), ptr(d_sv0), ptr(d_out[0]), ptr(d_out[1]), ptr(d_J), None) == L.EXA_ERR_UNSUPPORTED
    # volume average: sum_q W_q detJ = mesh volume
    out = (C.c_double * 2)()
    ctx.check(L.exa_vol_avg(ctx.h, ptr(d_J), ptr(d_out[0]), 1, 0, out, None))
    assert abs(out[1] - 1.0) < 1e-13
    ctx.close()


# ---- driver runs ----------------------------------------------------------------------------------------------------------------
def _toml(tmp_path, tag, mesh=None, N=4, p=1, assembly="PA", bcs=None, precond=None, grains_file=None, newton=(5e-5, 5e-10), krylov=(1e-7, 1e-27),
          vis=""):
    """Options file: a file mesh (Mesh.type = "other") or the generated N^3 cube, Voce FCC, the reference's grains / orientations."""
    bcs = bcs or ('    essential_ids = [1, 2, 3, 4]\n    essential_comps = [3, 1, 2, 3]\n'
                  '    essential_vals = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.000, 0.001]\n')
    if mesh:
        meshs = '    type = "other"\n    floc = "%s"\n    ref_ser = 0\n    p_refinement = %d\n' % (mesh, p)
    else:
        meshs = '    type = "auto"\n    ref_ser = 0\n    p_refinement = %d\n    [Mesh.Auto]\n        length = [1.0, 1.0, 1.0]\n        ncuts = [%d, %d, %d]\n' % (p, N, N, N)
    txt = f'''Version = "0.6.0"
[Properties]
    temperature = 298
    [Properties.Matl_Props]
        floc = "{REF}/props_cp_voce.txt"
        num_props = 17
    [Properties.State_Vars]
        floc = "{REF}/state_cp_voce.txt"
        num_vars = 24
    [Properties.Grain]
        ori_state_var_loc = 9
        ori_stride = 4
        ori_type = "quat"
        num_grains = 500
        ori_floc = "{REF}/voce_quats.ori"
        grain_floc = "{grains_file or (REF + '/grains.txt')}"
[BCs]
{bcs}[Model]
    mech_type = "exacmech"
    cp = true
    [Model.ExaCMech]
        xtal_type = "fcc"
        slip_type = "powervoce"
[Time]
    [Time.Custom]
        nsteps = 40
        floc = "{REF}/custom_dt.txt"
[Visualizations]
    steps = 1
    avg_stress_fname = "avg_stress.txt"
{vis}[Solvers]
    assembly = "{assembly}"
    rtmodel = "GPU"
    [Solvers.NR]
        iter = 25
        rel_tol = {newton[0]}
        abs_tol = {newton[1]}
    [Solvers.Krylov]
        iter = 2000
        rel_tol = {krylov[0]}
        abs_tol = {krylov[1]}
        solver = "PCG"
{('        preconditioner = "%s"' % precond + chr(10)) if precond else ''}[Mesh]
{meshs}'''
    path = os.path.join(str(tmp_path), tag + ".toml")
    with open(path, "w") as f:
        f.write(txt)
    return path


def _steps(L, path, n, tmp_path, **kw):
    d = L.Driver.from_toml(path, out_dir=str(tmp_path), **kw)
    for ti in range(1, n + 1):
        assert d.step(ti), (path, ti)
    return d


HOMOG_BCS = ('    changing_ess_bcs = false\n    constant_strain_rate = true\n    essential_ids = [1, 2, 3, 4, 5, 6]\n'
             '    essential_comps = [-7, -7, -7, -7, -7, -7]\n    essential_vel_grad = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.001]]\n')


@pytest.mark.parametrize("p", [1, 2])
def test_homogeneous_deformation_is_exact_on_tets(tmp_path, p):
    """One grain, every face under the same velocity gradient: the exact solution is linear, so the perturbed tetrahedral mesh and the generated
    hexahedral one give the same averages, every element carries the average stress, and the grain / light-up outputs agree."""
    import exaconstit_amd.lib as L
    N, n = 3, 8
    g1 = str(tmp_path / "grains1.txt"); np.savetxt(g1, np.ones(N ** 3, int), fmt="%d")
    mesh = T.write_mfem(str(tmp_path / "k.mesh"), T.kuhn_cube(N, perturb=0.3, shuffle=True, seed=11, grains="one"))
    # (an absolute Newton floor is needed: the first step starts converged, its residual is round-off)
    tight = dict(newton=(1e-9, 1e-14), krylov=(1e-12, 1e-30), bcs=HOMOG_BCS, grains_file=g1, p=p)
    res = {}
    for tag, m in (("hex", None), ("tet", mesh)):
        d = _steps(L, _toml(tmp_path, "%s%d" % (tag, p), mesh=m, N=N, **tight), n, tmp_path)
        res[tag] = {"avg": d.avgs(0, 6), "fields": d.element_fields(), "grains": d.grain_averages(),
                    "lattice": d.lattice_strains([[1, 1, 1], [2, 0, 0], [2, 2, 0]], (0, 0, 1), 15.0), "info": d.mesh_info()}
        d.close()
    assert res["tet"]["info"]["geometry"] == "tet" and res["tet"]["info"]["nodes_per_elem"] == (4 if p == 1 else 10)
    a, b = res["hex"]["avg"], res["tet"]["avg"]
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), np.abs(a - b).max() / np.abs(a).max()
    s = res["tet"]["fields"]["Stress"]
    assert np.abs(s - b[-1]).max() <= 1e-9 * np.abs(b[-1]).max()
    # volumes of the deformed cube (trace L = 0.001 per unit time): the same on both meshes
    assert abs(res["tet"]["fields"]["ElementVolume"].sum() - res["hex"]["fields"]["ElementVolume"].sum()) < 1e-12
    ga, gb = res["hex"]["grains"], res["tet"]["grains"]
    assert list(ga["grain_id"]) == list(gb["grain_id"]) == [1]
    assert np.asarray(gb["EffPlasticStrain"]).max() > 0   # past yield
    for k in ("Stress", "XtalElasticStrain", "EffPlasticStrain", "LatticeOrientation", "volume"):
        assert np.abs(np.asarray(ga[k]) - np.asarray(gb[k])).max() <= 1e-9 * max(1e-300, np.abs(np.asarray(ga[k])).max()), k
    la, lb = res["hex"]["lattice"], res["tet"]["lattice"]
    assert np.array_equal(la["volume_fraction"], lb["volume_fraction"])
    assert np.allclose(la["strain"], lb["strain"], rtol=1e-9, atol=0, equal_nan=True)


def _poly(tmp_path, **kw):
    return T.write_mfem(str(tmp_path / "poly.mesh"), T.kuhn_cube(4, perturb=0.25, shuffle=True, seed=7, **kw))


@pytest.mark.parametrize("p", [1, 2])
def test_fused_action_equals_generic(tmp_path, monkeypatch, p):
    import exaconstit_amd.lib as L
    mesh = _poly(tmp_path)
    path = _toml(tmp_path, "poly%d" % p, mesh=mesh, p=p)
    n = 5 if p == 1 else 3
    d = _steps(L, path, n, tmp_path)
    fused = (d.avgs(0, 6), d.stats(), d.mesh_info()); d.close()
    monkeypatch.setenv("EXA_TET_ACTION", "generic")
    d = _steps(L, path, n, tmp_path)
    gen = (d.avgs(0, 6), d.stats(), d.mesh_info()); d.close()
    assert fused[2]["action_route"] == "tet_fused" and gen[2]["action_route"] == "generic_evector"
    assert fused[2]["qpts_per_elem"] == (5 if p == 1 else 14)
    assert np.abs(fused[0] - gen[0]).max() <= 1e-12 * np.abs(gen[0]).max()
    # Newton counts identical; a Krylov count of a 400-iteration solve may move by a few where the two summation orders round differently
    assert list(fused[1][0]) == list(gen[1][0])
    kf, kg = np.asarray(fused[1][1]), np.asarray(gen[1][1])
    assert np.all(np.abs(kf - kg) <= np.maximum(2, 0.01 * kg))


def test_pa_equals_ea_and_jacobi_runs(tmp_path):
    import exaconstit_amd.lib as L
    mesh = _poly(tmp_path)
    out = {}
    for asm in ("PA", "EA"):
        d = _steps(L, _toml(tmp_path, "a" + asm, mesh=mesh, assembly=asm), 4, tmp_path)
        out[asm] = (d.avgs(0, 6), d.stats()); d.close()
    # (element assembly applies C^T, partial assembly C, as in the reference: the same solution to the Krylov tolerance)
    assert np.abs(out["PA"][0] - out["EA"][0]).max() <= 1e-8 * np.abs(out["PA"][0]).max()
    assert list(out["PA"][1][0]) == list(out["EA"][1][0])
    d = _steps(L, _toml(tmp_path, "jac", mesh=mesh, precond="jacobi"), 4, tmp_path)
    s = d.avgs(0, 6); d.close()
    assert np.abs(s - out["PA"][0]).max() <= 1e-6 * np.abs(s).max()


def test_action_routes_reported(tmp_path, monkeypatch):
    """mesh_info()["action_route"] names the action that runs: the fused kernel for PA and matrix-free EA, the table-driven L-vector kernel on
    assembled element matrices (EXA_EA_ASSEMBLED=1), the E-vector route with EXA_TET_ACTION=generic; p = 1 with J^-1 read from the record
    (EXA_TET_APPLY_GEO=off) gives the averages of the default form."""
    import exaconstit_amd.lib as L
    mesh = _poly(tmp_path)
    res = {}
    for tag, env, asm in (("pa", {}, "PA"), ("ea", {}, "EA"), ("ea_asm", {"EXA_EA_ASSEMBLED": "1"}, "EA"), ("gen", {"EXA_TET_ACTION": "generic"}, "PA"),
                          ("stored", {"EXA_TET_APPLY_GEO": "off"}, "PA")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            d = _steps(L, _toml(tmp_path, "r" + tag, mesh=mesh, assembly=asm), 3, tmp_path)
            res[tag] = (d.mesh_info()["action_route"], d.avgs(0, 6)); d.close()
    assert [res[k][0] for k in ("pa", "ea", "ea_asm", "gen", "stored")] == ["tet_fused", "tet_fused", "generic_ea_lvec", "generic_evector", "tet_fused"]
    assert np.abs(res["ea"][1] - res["ea_asm"][1]).max() <= 1e-12 * np.abs(res["ea"][1]).max()
    assert np.abs(res["pa"][1] - res["stored"][1]).max() <= 1e-12 * np.abs(res["pa"][1]).max()


def test_two_loopback_ranks_equal_one(tmp_path):
    import threading
    import exaconstit_amd.lib as L
    mesh = _poly(tmp_path)
    path = _toml(tmp_path, "mr", mesh=mesh)
    n = 4
    d = _steps(L, path, n, tmp_path)
    one = (d.avgs(0, 6), d.stats()); d.close()
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(2, gid) == 0
    drivers, errors = [None, None], []

    def work(r):
        try:
            drivers[r] = _steps(L, path, n, tmp_path / ("r%d" % r), rank=r, nranks=2, uid=gid, write_files=(r == 0))
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
    os.makedirs(str(tmp_path / "r0"), exist_ok=True); os.makedirs(str(tmp_path / "r1"), exist_ok=True)
    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    assert not errors, errors
    assert all(not t.is_alive() for t in th)
    two = (drivers[0].avgs(0, 6), drivers[0].stats())
    assert 0 < drivers[0].mesh_info()["elements"] < 384
    for dd in drivers:
        dd.close()
    L.exa_loopback_group_destroy(gid)
    assert np.linalg.norm(one[0] - two[0]) <= 1e-11 * np.linalg.norm(one[0])
    assert list(one[1][0]) == list(two[1][0])
    assert np.max(np.abs(np.asarray(one[1][1]) - np.asarray(two[1][1]))) <= 1


def test_gmsh_equals_mfem(tmp_path, monkeypatch):
    """The same mesh from the two formats: identical partitions at p = 1 and 2, and - in the ordered mode, where nothing else can differ between
    two runs - bit-identical averages, Newton and Krylov counts (grain attributes and boundary masks enter both)."""
    import exaconstit_amd.lib as L
    m = T.kuhn_cube(4, perturb=0.25, shuffle=True, seed=7)
    paths = (T.write_mfem(str(tmp_path / "a.mesh"), m), T.write_gmsh(str(tmp_path / "a.msh"), m))
    for p in (1, 2):
        a, b = _mesh_arrays(L, paths[0], p), _mesh_arrays(L, paths[1], p)
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    out = []
    for path in paths:
        d = _steps(L, _toml(tmp_path, os.path.basename(path).replace(".", "_"), mesh=path), 4, tmp_path)
        out.append((d.avgs(0, 6), d.stats())); d.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert list(out[0][1][0]) == list(out[1][1][0]) and list(out[0][1][1]) == list(out[1][1][1])


def _arr(piece, name):
    import base64
    import struct
    for da in piece.iter("DataArray"):
        if da.get("Name") == name:
            raw = base64.b64decode(da.text.strip())
            # two blocks: UInt32 byte count (base64 of 4 bytes = 8 chars), then the data
            nb = struct.unpack("<I", base64.b64decode(da.text.strip()[:8]))[0]
            data = base64.b64decode(da.text.strip()[8:])[:nb]
            del raw
            dt = {"Int32": np.int32, "UInt8": np.uint8, "Float64": np.float64, "Int64": np.int64}[da.get("type")]
            return np.frombuffer(data, dtype=dt)
    raise KeyError(name)


def test_paraview_output_of_tets(tmp_path):
    import exaconstit_amd.lib as L
    mesh = _poly(tmp_path)
    path = _toml(tmp_path, "pv", mesh=mesh, p=2, vis='    paraview = true\n    floc = "vis/tets"\n')
    d = _steps(L, path, 2, tmp_path)
    d.close()
    root = ET.parse(os.path.join(str(tmp_path), "vis", "tets", "Cycle000002", "proc000000.vtu")).getroot()
    piece = root.find(".//Piece")
    E = int(piece.get("NumberOfCells"))
    assert E == 384
    types = _arr(piece, "types"); conn = _arr(piece, "connectivity"); offs = _arr(piece, "offsets")
    assert np.all(types == 10) and conn.size == 4 * E and offs[-1] == 4 * E
    vol = _arr(piece, "ElementVolume")
    X = _arr(piece.find("Points"), "Points").reshape(-1, 3)      # current configuration
    # the fields' volumes are those of the configuration the fields were taken in, the points are the written end-of-step coordinates
    assert abs(vol.sum() - T.tet_volumes(X, conn.reshape(E, 4).astype(np.int64)).sum()) < 1e-5
    assert abs(vol.sum() - 1.0) < 1e-3


def test_deterministic_tets_are_bitwise_reproducible(tmp_path, monkeypatch):
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    mesh = _poly(tmp_path)
    path = _toml(tmp_path, "det", mesh=mesh)
    runs = []
    for _ in range(2):
        d = _steps(L, path, 3, tmp_path)
        runs.append((d.avgs(0, 6), d.stats(), d.qf_component(3, 2), d.mesh_info())); d.close()
    assert runs[0][3]["action_route"] == "generic_evector"
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    assert list(runs[0][1][1]) == list(runs[1][1][1])


def test_neper_style_msh_through_the_executable(tmp_path):
    """`mechanics -opt x.toml` on a Gmsh 2.2 tetrahedral polycrystal at p_refinement = 2 with ParaView output: avg_stress.txt has one row per
    step and the cells are VTK_TETRA."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "exaconstit_amd", "mechanics")
    msh = T.write_gmsh(str(tmp_path / "grains.msh"), T.kuhn_cube(3, perturb=0.2, seed=9))
    toml = _toml(tmp_path, "neper", mesh=msh, p=2, vis='    paraview = true\n    floc = "vis/neper"\n')
    txt = open(toml).read().replace("nsteps = 40", "nsteps = 3")
    open(toml, "w").write(txt)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}
    r = subprocess.run([exe, "-opt", toml], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    s = np.loadtxt(str(tmp_path / "avg_stress.txt"))
    assert s.shape == (3, 6) and np.all(np.isfinite(s)) and s[-1, 2] > s[0, 2] > 0
    piece = ET.parse(str(tmp_path / "vis" / "neper" / "Cycle000003" / "proc000000.vtu")).getroot().find(".//Piece")
    assert int(piece.get("NumberOfCells")) == 162 and np.all(_arr(piece, "types") == 10)


def test_bbar_on_tets_is_refused_with_a_message(tmp_path):
    import exaconstit_amd.lib as L
    path = _toml(tmp_path, "bbar", mesh=_poly(tmp_path), assembly="EA")
    txt = open(path).read().replace('assembly = "EA"', 'assembly = "EA"\n    integ_model = "BBAR"')
    open(path, "w").write(txt)
    with pytest.raises(Exception, match="BBAR"):
        L.Driver.from_toml(path, out_dir=str(tmp_path))
