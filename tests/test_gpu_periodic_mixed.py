"""Mixed stress / velocity-gradient loading of a periodic cell on the GPU: [BCs] periodic_free / Driver.set_periodic(L, free).

Voce FCC of tests/golden/refdata, the generated 4^3 cube at p = 1 unless said otherwise, L33 = 1e-3 prescribed, all off-diagonals prescribed
zero, xx and yy free (uniaxial stress along z).  Solver settings are those of tests/test_gpu_periodic.py (Newton rel 1e-10 / abs 1e-14, PCG rel
1e-12, every solve converges - asserted).  NSTEPS = 8 steps of custom_dt.txt, the count of tests/test_gpu_periodic.py, reach a strain of 8e-4:
past first yield - the realised L11 + L22 goes from -0.65 L33 in steps 1 - 2 (elastic) to -0.99 L33 at step 8 (plastic flow keeps the volume)
and the axial stress flattens (2.9e-2 after step 2, 4.3e-2 after step 7, 4.4e-2 after step 8).  The step count is not checked on the CPU oracle:
its driver port has no periodic conditions.  The measured figures are printed; EXA_WRITE_RECORDS=1 also writes them to
profiles/periodic_mixed_checks.txt."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hipref
import partition_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
NSTEPS = 8
N0 = 4
DTS = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()
LZ = np.diag([0.0, 0.0, 1.0e-3])
FREE_XY = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]])


def _mat(L, fmt=repr):
    return "[" + ", ".join("[" + ", ".join(fmt(x) for x in row) + "]" for row in L) + "]"


def _toml(tmp_path, tag, grains, N=N0, p=1, assembly="PA", integ="FULL", nl="NR", precond=None, vgrad=(LZ,), update_steps=(1,), free=FREE_XY, ori=None):
    """the generated N^3 cube of tests/test_gpu_periodic.py::_toml, periodic under vgrad with the mask `free` (None: every entry prescribed)"""
    os.makedirs(str(tmp_path), exist_ok=True)
    gfile = os.path.join(str(tmp_path), "grains_%s.txt" % tag)
    np.savetxt(gfile, np.asarray(grains).reshape(-1, 1), fmt="%d")
    ori = ori or os.path.join(REF, "voce_quats.ori")
    if len(vgrad) > 1:
        bcs = "    periodic = true\n    changing_ess_bcs = true\n    update_steps = [%s]\n    essential_vel_grad = [%s]\n" % (
            ", ".join(str(s) for s in update_steps), ", ".join(_mat(v, lambda x: repr(float(x))) for v in vgrad))
    else:
        bcs = "    periodic = true\n    essential_vel_grad = %s\n" % _mat(vgrad[0], lambda x: repr(float(x)))
    if free is not None:
        bcs += "    periodic_free = %s\n" % _mat(np.asarray(free), lambda x: str(int(x)))
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
        ori_floc = "{ori}"
        grain_floc = "{gfile}"
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
[Solvers]
    assembly = "{assembly}"
    integ_model = "{integ}"
    rtmodel = "GPU"
    [Solvers.NR]
        iter = 50
        rel_tol = 1e-10
        abs_tol = 1e-14
        nl_solver = "{nl}"
    [Solvers.Krylov]
        iter = 20000
        rel_tol = 1e-12
        abs_tol = 1e-30
        solver = "PCG"
{('        preconditioner = "%s"' % precond + chr(10)) if precond else ''}[Mesh]
    type = "auto"
    ref_ser = 0
    p_refinement = {p}
    [Mesh.Auto]
        length = [1.0, 1.0, 1.0]
        ncuts = [{N}, {N}, {N}]
'''
    path = os.path.join(str(tmp_path), tag + ".toml")
    open(path, "w").write(txt)
    return path


def _voronoi(N=N0, seeds=5, seed=7):
    """periodic Voronoi tessellation of the unit cube on the N^3 element centres (tests/test_gpu_periodic.py::_voronoi)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 1.0, (seeds, 3))
    c = (np.arange(N) + 0.5) / N
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    pts = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    d = pts[:, None, :] - s[None, :, :]
    d -= np.rint(d)
    return (np.argmin((d * d).sum(axis=2), axis=1) + 1).reshape(N, N, N)


def _face_areas(A):
    """areas of the faces of pair d = 0, 1, 2 of the cell with the period vectors A[:, d]"""
    return np.array([np.linalg.norm(np.cross(A[:, (d + 1) % 3], A[:, (d + 2) % 3])) for d in range(3)])


def _run(L, toml, nsteps, out_dir, jacobi=False):
    """steps 1 .. nsteps; per step: Newton's bound and the macro info (all zero without mixed loading)"""
    os.makedirs(str(out_dir), exist_ok=True)
    d = L.Driver.from_toml(toml, out_dir=str(out_dir), jacobi=jacobi, write_files=False)
    hist = []
    for ti in range(1, nsteps + 1):
        assert d.step(ti), "Newton failed at step %d" % ti
        ni = d.newton_info()
        assert ni["norm"] <= ni["bound"] and ni["bound"] > 0
        hist.append((ni["bound"], d.macro_info()))
    dg = d.diagnostics()
    assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0, dg
    return d, hist


RECORD = os.path.join(ROOT, "profiles", "periodic_mixed_checks.txt")


def _record(key, lines):
    """the measured figures: printed and, when EXA_WRITE_RECORDS=1, kept in profiles/periodic_mixed_checks.txt as the block '[key]'"""
    for ln in lines:
        print(ln)
    if os.environ.get("EXA_WRITE_RECORDS") != "1":
        return
    blocks, cur = {}, None
    if os.path.exists(RECORD):
        for ln in open(RECORD).read().splitlines():
            if ln.startswith("[") and ln.endswith("]"):
                cur = ln[1:-1]; blocks[cur] = []
            elif cur is not None:
                blocks[cur].append(ln)
    blocks[key] = list(lines)
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        for k in sorted(blocks):
            f.write("[%s]\n%s\n" % (k, "\n".join(blocks[k])))


def _ints(a):
    return [int(x) for x in a]


def _lateral_check(avgs, hist, key, what):
    """|S_xx|, |S_yy| of the average stress within 2 x Newton's bound / face area and below 1e-6 |S_zz|, at every step.  The conjugate force of a
    free H_id is the resultant of face pair d, a row of the residual Newton bounds; the factor 2 is the one of
    tests/test_gpu_periodic.py::test_equilibrium_through_the_oracle; mean traction = resultant / area of the face."""
    lines, ok = [], True
    for k, (bound, mi) in enumerate(hist):
        area = _face_areas(mi["period"])
        sxx, syy, szz = abs(avgs[k, 0]), abs(avgs[k, 1]), abs(avgs[k, 2])
        lim = (2.0 * bound / area[0], 2.0 * bound / area[1])
        lines.append("  step %d: |S_xx| %.3e (limit %.3e) |S_yy| %.3e (limit %.3e) |S_zz| %.3e; resultants F_11 %.3e F_22 %.3e F_33 %.3e; realised L_11 %.6e L_22 %.6e L_33 %.6e"
                     % (k + 1, sxx, lim[0], syy, lim[1], szz, mi["resultants"][0, 0], mi["resultants"][1, 1], mi["resultants"][2, 2], mi["vel_grad"][0, 0], mi["vel_grad"][1, 1], mi["vel_grad"][2, 2]))
        ok = ok and sxx <= lim[0] and syy <= lim[1] and max(sxx, syy) < 1e-6 * szz
    _record(key, [what] + lines)
    return ok


# ---------------------------------------------------------------------------------------------------------------- 3. uniaxial stress
def test_uniaxial_stress_run(tmp_path):
    """The run completes with the lateral mean stress at Newton's tolerance and a lateral contraction; with every entry prescribed (the same file
    without periodic_free: uniaxial strain) the lateral stress is of the order of the axial one."""
    import exaconstit_amd.lib as L
    g = _voronoi().ravel()
    d, hist = _run(L, _toml(tmp_path, "uni", g), NSTEPS, tmp_path / "uni")
    avgs = d.avgs(0, 6)
    mi = d.macro_info()
    assert np.array_equal(mi["free"], FREE_XY.astype(bool))
    assert np.array_equal(d.periodic_info()["vel_grad"], mi["vel_grad"])
    for bound, m in hist:
        Lr = m["vel_grad"]
        assert Lr[0, 0] < 0 and Lr[1, 1] < 0
        assert abs(Lr[2, 2] - 1e-3) < 1e-15 and np.abs(Lr - np.diag(np.diag(Lr))).max() < 1e-15      # the prescribed entries
        assert abs(Lr[0, 0] + Lr[1, 1] + Lr[2, 2]) < abs(Lr[2, 2]) / 2
    ok = _lateral_check(avgs, hist, "uniaxial_stress", "uniaxial stress, %d^3, %d steps, Newton %s:" % (N0, NSTEPS, _ints(d.stats()[0])))
    d.close()
    e, _ = _run(L, _toml(tmp_path, "strain", g, free=None), NSTEPS, tmp_path / "strain")
    a2 = e.avgs(0, 6)
    assert not e.macro_info()["free"].any()
    e.close()
    _record("uniaxial_strain", ["the same file without periodic_free (uniaxial strain), step %d: S_xx / S_zz %.4f, S_yy / S_zz %.4f" % (NSTEPS, a2[-1, 0] / a2[-1, 2], a2[-1, 1] / a2[-1, 2])])
    assert abs(a2[-1, 0]) > 0.1 * abs(a2[-1, 2])
    assert ok


# ---------------------------------------------------------------------------------------------------------------- 4. homogeneous patch
def test_homogeneous_patch(tmp_path):
    """one orientation on the cube axes (the identity quaternion: no shear arises): the affine field with the realised gradient is the solution"""
    import exaconstit_amd.lib as L
    ori = os.path.join(str(tmp_path), "cube.ori")
    os.makedirs(str(tmp_path), exist_ok=True)
    np.savetxt(ori, np.tile([1.0, 0.0, 0.0, 0.0], (500, 1)))
    d, hist = _run(L, _toml(tmp_path, "homog", np.full(N0 ** 3, 3), ori=ori), NSTEPS, tmp_path / "homog")
    S = d.element_fields()["Stress"]
    spread = np.abs(S - S[0]).max() / np.abs(S[0]).max()
    x, v = d.nodal_field("coords"), d.nodal_field("velocity")
    xp = x - DTS[NSTEPS - 1] * v      # the velocity of the last step was imposed on the coordinates that step started from
    Lr = d.macro_info()["vel_grad"]
    fl = np.abs(v - (xp - xp.min(axis=0)) @ Lr.T).max() / np.abs(v).max()
    _record("homogeneous_patch", ["homogeneous patch, %d^3, %d steps: element stress spread %.3e, fluctuation / |v| %.3e, realised L_11 / L_33 %.6f" % (N0, NSTEPS, spread, fl, Lr[0, 0] / Lr[2, 2])])
    ok = _lateral_check(d.avgs(0, 6), hist, "homogeneous_patch_lateral", "homogeneous patch, lateral stress:")
    d.close()
    assert spread < 1e-11 and fl < 1e-11      # the bounds of tests/test_gpu_periodic.py::test_homogeneous_patch
    assert ok


# ---------------------------------------------------------------------------------------------------------------- 5. replay
def test_replay_through_the_prescribed_route(tmp_path):
    """the realised gradients of the mixed run, prescribed step by step through the fully prescribed periodic route, give the same run"""
    import exaconstit_amd.lib as L
    g = _voronoi().ravel()
    d, hist = _run(L, _toml(tmp_path, "mix", g), NSTEPS, tmp_path / "mix")
    a1, v1 = d.avgs(0, 6), d.nodal_field("velocity")
    d.close()
    Ls = [m["vel_grad"] for _, m in hist]
    e, _ = _run(L, _toml(tmp_path, "replay", g, vgrad=Ls, update_steps=range(1, NSTEPS + 1), free=None), NSTEPS, tmp_path / "replay")
    a2, v2 = e.avgs(0, 6), e.nodal_field("velocity")
    e.close()
    ds, dv = np.abs(a1 - a2).max() / np.abs(a1).max(), np.abs(v1 - v2).max() / np.abs(v1).max()
    _record("replay", ["replay, %d^3, %d steps: average stress %.3e of the largest, nodal velocity %.3e of the largest" % (N0, NSTEPS, ds, dv)])
    assert ds < 1e-6 and dv < 1e-6      # two converged runs of one problem (tests/test_gpu_periodic.py::test_ranks_match_one_rank)


# ---------------------------------------------------------------------------------------------------------------- 6. equilibrium
def test_equilibrium_through_the_oracle(oracle, tmp_path):
    """B^T sigma of the converged state assembled by the oracle's integrator, summed over each top face in numpy: the conjugate forces of the free
    entries vanish within Newton's bound, the one of L33 does not, and macro_info reports these sums"""
    import exaconstit_amd.lib as L
    orc = oracle
    N = N0
    d, hist = _run(L, _toml(tmp_path, "equi", _voronoi().ravel()), NSTEPS, tmp_path / "equi")
    part = pu.query((N, N, N), 0, 1)
    E, n, NN = part["E"], 8, part["NN"]
    assert list(d.element_fields()["GlobalElementId"]) == list(part["gid"])
    rve = hipref.make_rve(orc, N)
    rve["conn"] = part["conn"].astype(np.int32).ravel()
    Q, P = rve["Q"], E * rve["Q"]
    x = d.nodal_field("coords")
    xe = hipref.l_to_e(rve, np.ascontiguousarray(x.T).ravel())
    J = np.zeros(9 * P); orc.lib().orc_jacobians(1, E, orc._p(xe), orc._p(J))
    sig = np.ascontiguousarray(np.stack([d.qf_component(2, c).reshape(E, Q) for c in range(6)], axis=-1)).ravel()
    dmat = np.zeros(9 * P); orc.lib().orc_assemble_pa(Q, E, orc._p(rve["W"]), orc._p(J), orc._p(sig), orc._p(dmat))
    ye = np.zeros(3 * n * E); orc.lib().orc_add_mult_pa(Q, E, n, orc._p(rve["G"]), orc._p(dmat), orc._p(ye))
    r = hipref.e_to_l(rve, ye).reshape(3, NN).T.copy()
    t = L.partition_periodic_mixed(N, 0, 1)
    F = np.array([[r[t["faces"][dd], i].sum() for dd in range(3)] for i in range(3)])
    bound, mi = hist[-1]
    rel = np.abs(mi["resultants"] - F).max() / np.abs(F).max()
    _record("equilibrium", ["equilibrium, %d^3 after %d steps: oracle-assembled face resultants F_11 %.3e F_22 %.3e F_33 %.3e, Newton's bound %.3e; macro_info against them %.3e of the largest"
                            % (N, NSTEPS, F[0, 0], F[1, 1], F[2, 2], bound, rel)])
    d.close()
    assert abs(F[0, 0]) <= 2.0 * bound and abs(F[1, 1]) <= 2.0 * bound
    assert abs(F[2, 2]) > 1e6 * bound
    assert rel < 1e-9


# ---------------------------------------------------------------------------------------------------------------- 7. ranks
def _run_ranks(L, toml, nranks, nsteps, out_dir):
    os.makedirs(str(out_dir), exist_ok=True)
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    drivers, errors = [None] * nranks, []

    def work(r):
        try:
            drivers[r] = L.Driver.from_toml(toml, out_dir=str(out_dir), rank=r, nranks=nranks, uid=gid, write_files=False)
            for ti in range(1, nsteps + 1):
                if not drivers[r].step(ti):
                    raise RuntimeError(f"rank {r}: Newton failed at step {ti}")
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    out = [(d.avgs(0, 6), d.stats(), d.diagnostics(), d.macro_info()) for d in drivers]
    for d in drivers:
        d.close()
    L.exa_loopback_group_destroy(gid)
    return out


@pytest.fixture(scope="module")
def one_rank_reference(tmp_path_factory):
    import exaconstit_amd.lib as L
    tmp = tmp_path_factory.mktemp("mixed_ranks")
    toml = _toml(tmp, "ranks", _voronoi().ravel())
    d, hist = _run(L, toml, NSTEPS, tmp / "r1")
    ref = (toml, d.avgs(0, 6).copy(), list(d.stats()[0]), hist[-1][1])
    d.close()
    return ref


@pytest.mark.parametrize("nranks", [2, 8])
def test_ranks_match_one_rank(tmp_path, one_rank_reference, nranks):
    """process grids 1 x 1 x 2 and 2 x 2 x 2 (2^3 elements per rank) against one rank"""
    import exaconstit_amd.lib as L
    toml, ref, newton, mi1 = one_rank_reference
    got = _run_ranks(L, toml, nranks, NSTEPS, tmp_path / ("r%d" % nranks))
    scale = np.abs(ref).max()
    worst = max(np.abs(s - ref).max() for s, _, _, _ in got) / scale
    wl = max(np.abs(mi["vel_grad"] - mi1["vel_grad"]).max() for _, _, _, mi in got) / 1e-3
    _record("ranks_%d" % nranks, ["ranks, %d^3, %d steps: %d loopback ranks against one, largest average-stress difference %.3e of |avg stress|, realised gradient %.3e of L_33"
                                  % (N0, NSTEPS, nranks, worst, wl)])
    for s, st, dg, mi in got:
        assert np.abs(s - ref).max() < 1e-6 * scale
        assert list(st[0]) == newton
        assert dg["pcg_not_converged"] == 0 and dg["model_failed_points"] == 0
        assert np.array_equal(mi["vel_grad"], got[0][3]["vel_grad"]) and np.array_equal(mi["resultants"], got[0][3]["resultants"])      # every rank reports the same


# ---------------------------------------------------------------------------------------------------------------- 8. routes
LSHEAR = np.array([[0.0, 1.0e-3, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
FREE_YY = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]])
ROUTES = {"p2": dict(p=2, N=2), "ea": dict(assembly="EA"), "p2_bbar_ea": dict(p=2, N=2, assembly="EA", integ="BBAR"), "nrls": dict(nl="NRLS"),
          "jacobi": dict(precond="jacobi"), "reversal": dict(vgrad=(LZ, -LZ), update_steps=(1, 4)), "shear": dict(vgrad=(LSHEAR,), free=FREE_YY)}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes(tmp_path, route):
    import exaconstit_amd.lib as L
    kw = dict(ROUTES[route])
    N, nsteps = kw.pop("N", N0), 6
    d, hist = _run(L, _toml(tmp_path, route, _voronoi(N, seeds=5 if N > 2 else 3).ravel(), N=N, **kw), nsteps, tmp_path / route)
    a = d.avgs(0, 6)
    assert np.all(np.isfinite(a)) and a.shape == (nsteps, 6)
    lead = np.abs(a[:, 5] if route == "shear" else a[:, 2])      # S_xy under shear, S_zz under tension
    freed = np.abs(a[:, 1:2]) if route == "shear" else np.abs(a[:, 0:2])
    worst = (freed.max(axis=1) / lead).max()
    Lr = hist[-1][1]["vel_grad"]
    _record("route_" + route, ["route %s, %d^3, %d steps: Newton %s, largest freed stress / leading stress %.3e, realised diagonal %.4e %.4e %.4e"
                               % (route, N, nsteps, _ints(d.stats()[0]), worst, Lr[0, 0], Lr[1, 1], Lr[2, 2])])
    d.close()
    assert worst < 1e-6
    if route == "reversal":
        assert abs(Lr[2, 2] + 1.0e-3) < 1e-15 and Lr[0, 0] > 0 and Lr[1, 1] > 0      # (H A^-1: the prescribed entry to round-off)
    if route == "shear":
        assert abs(Lr[0, 1] - 1.0e-3) < 1e-15


def test_ill_posed_mask_is_refused_at_run_time(tmp_path):
    """prescribed L12 != 0 with xx free: after one step the period vector a_2 leans along x, so the prescribed L12 involves the unknown L11"""
    import exaconstit_amd.lib as L
    toml = _toml(tmp_path, "ill", _voronoi().ravel(), vgrad=(LSHEAR + LZ,), free=np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0]]))
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path / "ill"), write_files=False)
    assert d.step(1)
    with pytest.raises(RuntimeError, match=r"periodic_free: entry \(1,1\) of the velocity gradient is free and entry \(1,2\) is prescribed"):
        d.step(2)
    d.close()


# ---------------------------------------------------------------------------------------------------------------- 9. determinism, checkpoint
def _state(d):
    mi = d.macro_info()
    return [d.avgs(0, 6), d.nodal_field("velocity"), d.nodal_field("coords"), mi["vel_grad"], mi["period"], mi["resultants"]]


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)) for x, y in zip(a, b))


def test_deterministic_mode_gives_identical_bits(tmp_path, monkeypatch):
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    toml = _toml(tmp_path, "det", _voronoi().ravel())
    runs = []
    for k in range(2):
        d, _ = _run(L, toml, 5, tmp_path / ("det%d" % k))
        runs.append((_state(d), list(d.stats()[0]), list(d.stats()[1])))
        d.close()
    assert _same_bits(runs[0][0], runs[1][0])
    assert runs[0][1:] == runs[1][1:]


def test_checkpoint_resume_is_exact(tmp_path, monkeypatch):
    """stop after step 3, fresh driver, load, finish: bit for bit the uninterrupted run (EXA_DETERMINISTIC=1, the mode in which a run reproduces
    its own bits), the macro info included - the control values live in the velocity field"""
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    toml = _toml(tmp_path, "ckpt", _voronoi().ravel())
    k, n = 3, 6
    d, _ = _run(L, toml, n, tmp_path / "full")
    full = (_state(d), list(d.stats()[0]))
    d.close()
    os.makedirs(str(tmp_path / "cut"), exist_ok=True)
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path / "cut"))
    for ti in range(1, k + 1):
        assert d.step(ti)
    ck = str(tmp_path / "cut" / "cut.ckpt")
    d.save_checkpoint(ck)
    d.close()
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path / "cut"))
    d.load_checkpoint(ck)
    for ti in range(k + 1, n + 1):
        assert d.step(ti)
    cut = (_state(d), list(d.stats()[0]))
    d.close()
    assert full[1][k:] == cut[1][-(n - k):]
    assert _same_bits([full[0][0][k:]] + full[0][1:], [cut[0][0][-(n - k):]] + cut[0][1:])


# ---------------------------------------------------------------------------------------------------------------- launch budget, interface
def test_mixed_kernels_have_no_scratch():
    import exaconstit_amd.lib as L
    hipref.Dev()
    out = (C.c_int * 2)(-1, -1)
    assert L.exa_periodic_mixed_scratch_bytes(out) == 0
    assert list(out) == [0, 0]
    assert L.exa_periodic_sum_scratch_bytes() == 0


def test_set_periodic_with_a_mask_on_a_synthetic_driver(tmp_path):
    """Driver.synthetic + set_periodic(L, free) is the problem of the options file; the refusals of the interface"""
    import exaconstit_amd.lib as L
    N = N0
    g = _voronoi().ravel()
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    ori = np.loadtxt(os.path.join(REF, "voce_quats.ori")).reshape(-1, 4)
    d = L.Driver.synthetic(N, props, hipref.random_quats(N ** 3).ravel(), DTS[:4], newton=(50, 1e-10, 1e-14), krylov=(20000, 1e-12, 1e-30))
    assert not d.macro_info()["free"].any()
    d.set_grains(g, ori[:5])
    with pytest.raises(RuntimeError, match="off-diagonal pair"):
        d.set_periodic(LZ, free=[[0, 1, 0], [1, 0, 0], [0, 0, 0]])
    with pytest.raises(RuntimeError, match="all nine entries are free"):
        d.set_periodic(LZ, free=np.ones((3, 3)))
    d.set_periodic(LZ, free=FREE_XY)
    assert np.array_equal(d.macro_info()["free"], FREE_XY.astype(bool)) and np.array_equal(d.periodic_info()["vel_grad"], LZ)
    with pytest.raises(RuntimeError, match="multigrid"):
        d.set_preconditioner("multigrid")
    for ti in range(1, 5):
        assert d.step(ti)
    e, _ = _run(L, _toml(tmp_path, "syn", g), 4, tmp_path / "syn")
    assert np.abs(d.avgs(0, 6) - e.avgs(0, 6)).max() < 1e-9 * np.abs(e.avgs(0, 6)).max()
    assert np.abs(d.macro_info()["vel_grad"] - e.macro_info()["vel_grad"]).max() < 1e-9 * 1e-3
    d.close(); e.close()
