"""Checkpoint and restart on the GPU: the pack / unpack / checksum kernels against numpy, the file against the driver's state,
bit-exact resume of interrupted runs (one rank, rank threads on the loopback group, the `mechanics` executable), resume across rank counts,
output continuity and the refusals that need a driver.  Deterministic mode (EXA_DETERMINISTIC=1) unless a test says otherwise: with the
default FP64 atomics two uninterrupted runs already differ at round-off."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

import hipref
import tet_mesh_util as T
from hipref import ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
EXE = os.path.join(ROOT, "exaconstit_amd", "mechanics")
FIELD_SECTIONS = ("x_beg", "v_sol", "stress0", "matVars0")


@pytest.fixture(autouse=True)
def _deterministic(monkeypatch):
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    monkeypatch.delenv("EXA_QLAYOUT", raising=False)


# ---------------------------------------------------------------------------------------------------------------- kernels
def _canonical(x, layout, W, Q, E):
    """numpy re-indexing of a quadrature function in `layout` to (E, Q, W)"""
    if layout == 0:
        return x[:W * Q * E].reshape(E, Q, W)
    nb = (E + 63) // 64
    return np.ascontiguousarray(x.reshape(nb, Q, W, 64).transpose(0, 3, 1, 2)).reshape(nb * 64, Q, W)[:E]


def _roundtrip(L, dev, ctx, layout, W, Q, E, seed):
    import torch
    rng = np.random.default_rng(seed)
    n = int(L.exa_qf_size(ctx.h, W))
    assert n == (W * Q * E if layout == 0 else W * 64 * Q * ((E + 63) // 64))
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    x[::97] = -0.0
    x[5::101] = np.inf
    d_x = dev.up(x)
    d_can = dev.zeros(W * Q * E)
    d_ck = torch.zeros(2, dtype=torch.int64, device=dev.dev)
    d_ck[0] = 12345                                                        # the launch clears it
    ctx.check(L.exa_qf_pack(ctx.h, W, ptr(d_x), ptr(d_can), ptr(d_ck), None))
    can = d_can.cpu().numpy()
    want = _canonical(x, layout, W, Q, E)
    assert np.array_equal(can.view(np.int64), np.ascontiguousarray(want).ravel().view(np.int64)), "pack != numpy re-indexing"
    cks = int(np.ascontiguousarray(want).ravel().view(np.uint64).sum(dtype=np.uint64))
    assert int(d_ck.cpu().numpy().view(np.uint64)[0]) == cks, "device checksum (pack)"
    sentinel = -7.25
    d_y = torch.full((n,), sentinel, dtype=torch.float64, device=dev.dev)
    ctx.check(L.exa_qf_unpack(ctx.h, W, ptr(d_can), ptr(d_y), ptr(d_ck[1:]), None))
    y = d_y.cpu().numpy()
    assert int(d_ck.cpu().numpy().view(np.uint64)[1]) == cks, "device checksum (unpack)"
    assert np.array_equal(_canonical(y, layout, W, Q, E).view(np.int64), want.view(np.int64)), "unpack(pack(x)) != x"
    if layout == 1:                                                        # padding lanes of the last block keep what they held
        pad = np.ones(((E + 63) // 64) * 64, bool); pad[:E] = False
        yb = y.reshape(-1, Q, W, 64).transpose(0, 3, 1, 2).reshape(-1, Q, W)
        assert np.all(yb[pad] == sentinel)
    else:
        assert np.array_equal(y.view(np.int64), x.view(np.int64))
    ctx.check(L.exa_qf_pack(ctx.h, W, ptr(d_x), ptr(d_can), None, None))   # no checksum wanted
    assert L.exa_qf_pack(ctx.h, 97, ptr(d_x), ptr(d_can), None, None) == L.EXA_ERR_ARG


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("layout", [0, 1])
def test_pack_unpack_hexahedra(E, layout):
    import exaconstit_amd.lib as L
    dev = hipref.Dev()
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    if layout:
        ctx.check(L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64))
    for W in (6, 9, 28, 36):
        _roundtrip(L, dev, ctx, layout, W, 8, E, seed=E + W)
    ctx.close()


@pytest.mark.parametrize("order,layout,E", [(2, 1, 70), (2, 0, 70)])
def test_pack_unpack_p2(order, layout, E):
    import exaconstit_amd.lib as L
    dev = hipref.Dev()
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, order, E)
    if layout:
        ctx.check(L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64))
    for W in (6, 9, 28):
        _roundtrip(L, dev, ctx, layout, W, 27, E, seed=W)
    ctx.close()


@pytest.mark.parametrize("order,Q", [(1, 5), (2, 14)])
def test_pack_unpack_tetrahedra(order, Q):
    import exaconstit_amd.lib as L
    dev = hipref.Dev()
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    E = 162
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, order, E, geometry=L.EXA_GEOM_TET)
    assert ctx.Q == Q
    for W in (6, 9, 28, 36):
        _roundtrip(L, dev, ctx, 0, W, Q, E, seed=W)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- cases
def _ref_toml(tmp_path, name, vis=(), extra="", tag=None):
    """an options file of tests/golden/refdata with absolute paths to its data files, optional extra Visualizations lines and tables"""
    text = open(os.path.join(REF, name + ".toml")).read()
    for fl in os.listdir(REF):
        if fl.endswith((".txt", ".ori")):
            text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    if vis:      # the given lines replace the keys of the same name inside the [Visualizations] table
        a = text.index("[Visualizations]") + len("[Visualizations]")
        b = text.index("[Solvers]")
        keys = {ln.split("=")[0].strip() for ln in vis}
        body = "\n".join(l for l in text[a:b].split("\n") if l.split("=")[0].strip() not in keys)
        text = text[:a] + "\n" + "\n".join("    " + l for l in vis) + body + text[b:]
    os.makedirs(str(tmp_path), exist_ok=True)
    p = os.path.join(str(tmp_path), (tag or name) + ".toml")
    open(p, "w").write(text + "\n" + extra)
    return p


def _gen_toml(tmp_path, tag, mesh=None, N=4, p=1, assembly="PA", integ="FULL", precond=None):
    """the generated N^3 cube or a file mesh, Voce FCC, the reference's grains and orientations, uniaxial tension"""
    if mesh:
        meshs = '    type = "other"\n    floc = "%s"\n    ref_ser = 0\n    p_refinement = %d\n' % (mesh, p)
    else:
        meshs = '    type = "auto"\n    ref_ser = 0\n    p_refinement = %d\n    [Mesh.Auto]\n        length = [1.0, 1.0, 1.0]\n        ncuts = [%d, %d, %d]\n' % (p, N, N, N)
    grains = os.path.join(str(tmp_path), "grains_%s.txt" % tag)
    os.makedirs(str(tmp_path), exist_ok=True)
    np.savetxt(grains, (np.arange(N ** 3) % 500 + 1).reshape(-1, 1), fmt="%d")
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
        grain_floc = "{grains}"
[BCs]
    essential_ids = [1, 2, 3, 4]
    essential_comps = [3, 1, 2, 3]
    essential_vals = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.000, 0.001]
[Model]
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
        iter = 25
        rel_tol = 5e-5
        abs_tol = 5e-10
    [Solvers.Krylov]
        iter = 2000
        rel_tol = 1e-7
        abs_tol = 1e-27
        solver = "PCG"
{('        preconditioner = "%s"' % precond + chr(10)) if precond else ''}[Mesh]
{meshs}'''
    path = os.path.join(str(tmp_path), tag + ".toml")
    open(path, "w").write(txt)
    return path


AVG_FILES = ("stress", "def_grad", "pl_work", "dp_tensor")


def _avg_bytes(out_dir):
    """contents of every avg_* / light-up / auto-dt text file of a run directory"""
    out = {}
    for f in sorted(os.listdir(str(out_dir))):
        p = os.path.join(str(out_dir), f)
        if os.path.isfile(p) and f.endswith(".txt"):
            out[f] = open(p, "rb").read()
    return out


def _steps(d, first, last):
    for ti in range(first, last + 1):
        assert d.step(ti), "Newton failed at step %d" % ti


def _final(L, d, path):
    """end state of a run: its final checkpoint (every field section and the header's clock), the averages and the solver history"""
    d.save_checkpoint(path)
    r = L.read_checkpoint(path)
    st = d.stats()
    return dict(ck=r, avgs=[d.avgs(w, n) for w, n in ((0, 6), (1, 9), (2, 1), (3, 6))], newton=list(st[0]), krylov=list(st[1]))


def _same_state(a, b, sections=FIELD_SECTIONS):
    for n in sections:
        assert np.array_equal(a["ck"][n].view(np.int64), b["ck"][n].view(np.int64)), "section %s differs" % n
    for k in ("steps_done", "time", "dt_class", "last_dt", "bc_index", "model_calls", "newton_cap", "newton_cap2"):
        assert a["ck"]["header"][k] == b["ck"]["header"][k], k
    assert a["newton"] == b["newton"] and a["krylov"] == b["krylov"]
    for x, y in zip(a["avgs"], b["avgs"]):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


def _full_and_resumed(L, toml, k, n, tmp_path, tag="", reader_env=None, writer_env=None, monkeypatch=None):
    """uninterrupted run of n steps | k steps, save, destroy, fresh driver, load, the rest.  Returns the two end states and output directories."""
    full_dir, cut_dir = tmp_path / ("full" + tag), tmp_path / ("cut" + tag)
    for d_ in (full_dir, cut_dir):
        os.makedirs(str(d_), exist_ok=True)

    def setenv(env):
        for key in ("EXA_QLAYOUT",):
            monkeypatch.delenv(key, raising=False) if monkeypatch else None
        for key, v in (env or {}).items():
            monkeypatch.setenv(key, v)
    setenv(reader_env)                      # the uninterrupted run is the reader's configuration
    d = L.Driver.from_toml(toml, out_dir=str(full_dir))
    _steps(d, 1, n)
    full = _final(L, d, str(full_dir / "final.ckpt"))
    d.close()
    setenv(writer_env)
    d = L.Driver.from_toml(toml, out_dir=str(cut_dir))
    _steps(d, 1, k)
    ck = str(cut_dir / "cut.ckpt")
    d.save_checkpoint(ck)
    assert not os.path.exists(ck + ".tmp")
    d.close()
    setenv(reader_env)
    d = L.Driver.from_toml(toml, out_dir=str(cut_dir))
    d.load_checkpoint(ck)
    assert L.checkpoint_info(ck)["steps_done"] == k
    _steps(d, k + 1, n)
    cut = _final(L, d, str(cut_dir / "final.ckpt"))
    d.close()
    return full, cut, full_dir, cut_dir


def _assert_same_files(full_dir, cut_dir):
    a, b = _avg_bytes(full_dir), _avg_bytes(cut_dir)
    assert sorted(a) == sorted(b) and a, (sorted(a), sorted(b))
    for f in a:
        assert a[f] == b[f], "file %s differs between the uninterrupted and the resumed run" % f


# ---------------------------------------------------------------------------------------------------------------- the file
def test_file_holds_the_drivers_state(tmp_path):
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path))
    _steps(d, 1, 4)
    ck = str(tmp_path / "s4.ckpt")
    d.save_checkpoint(ck)
    r = L.read_checkpoint(ck)
    info = L.checkpoint_info(ck)
    gid = d.element_fields()["GlobalElementId"]
    E, Q = len(gid), 8
    assert info["elements"] == 1000 and info["qpts_per_elem"] == Q and info["steps_done"] == 4 and info["nranks"] == 1 and info["bc_index"] == 0
    assert info["geometry"] == 0 and info["order"] == 1 and info["model"] == L.EXA_FCC_VOCE and info["nprops"] == 17 and info["nstatev"] == 28
    assert r["header"]["time"] == info["time"] == pytest.approx(np.loadtxt(os.path.join(REF, "custom_dt.txt"))[:4].sum(), rel=1e-15)
    for c in range(28):
        assert np.array_equal(r["matVars0"][gid, :, c].view(np.int64), d.qf_component(0, c).reshape(E, Q).view(np.int64)), c
    for c in range(6):
        assert np.array_equal(r["stress0"][gid, :, c].view(np.int64), d.qf_component(2, c).reshape(E, Q).view(np.int64)), c
    assert np.array_equal(r["avg_stress"], d.avgs(0, 6)) and r["avg_stress"].shape == (4, 6)
    st = d.stats()
    assert np.array_equal(r["solver_stats"][:, 0], st[0]) and np.array_equal(r["solver_stats"][:, 1], st[1]) and np.all(r["solver_stats"][:, 3] == 1)
    assert np.abs(r["stress0"]).max() > 0 and r["x_beg"].shape == (11 ** 3, 3) and np.abs(r["v_sol"]).max() > 0
    # slot 0 of the state satisfies the invariant of exa_state_normalize as stored (the loader does not touch this library's files)
    assert np.allclose(r["matVars0"][:, :, 0], np.abs(r["matVars0"][:, :, 14:26]).sum(axis=2), rtol=1e-12, atol=0.0)
    d.close()


# ---------------------------------------------------------------------------------------------------------------- resume is exact
@pytest.mark.parametrize("case,k,n", [("voce_ea_cs", 3, 6), ("voce_full_cyclic_cs", 8, 14), ("voce_full_cyclic_cs", 10, 14), ("voce_full_cyclic_cs", 11, 14),
                                      ("voce_full_cyclic_cs", 12, 14), ("mtsdd_bcc", 5, 9), ("mtsdd_full_auto", 2, 4)])
def test_resume_is_exact(tmp_path, case, k, n):
    """voce_ea_cs: velocity-gradient BCs + additional averages; voce_full_cyclic_cs: update_steps = [1, 11, ...], the boundary conditions change
    in step 11.  Cut before it (8, and 10: the resumed driver runs the changing step itself), exactly at it (11: the file is written by the step
    that changed them, entry 1 is in force and is applied again on load without that step's SolveInit) and after it (12); mtsdd_bcc: the
    tail-split controller is active; mtsdd_full_auto: Time.Auto."""
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, case)
    full, cut, fd, cd = _full_and_resumed(L, toml, k, n, tmp_path)
    if case == "voce_full_cyclic_cs":
        assert L.checkpoint_info(str(cd / "cut.ckpt"))["bc_index"] == (1 if k >= 11 else 0)
        assert full["ck"]["header"]["bc_index"] == cut["ck"]["header"]["bc_index"] == 1
    _same_state(full, cut)
    _assert_same_files(fd, cd)


def test_resume_in_a_fresh_process(tmp_path):
    """voce_pa: the second half runs in a child process under its own time limit, so nothing survives in process memory"""
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    k, n = 6, 12
    fd, cd = tmp_path / "full", tmp_path / "cut"
    os.makedirs(str(fd)); os.makedirs(str(cd))
    d = L.Driver.from_toml(toml, out_dir=str(fd))
    _steps(d, 1, n)
    full = _final(L, d, str(fd / "final.ckpt"))
    d.close()
    d = L.Driver.from_toml(toml, out_dir=str(cd))
    _steps(d, 1, k)
    d.save_checkpoint(str(cd / "cut.ckpt"))
    d.close()
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "checkpoint_worker.py"), toml, str(cd), str(cd / "cut.ckpt"), str(n),
                        str(cd / "final.ckpt")], capture_output=True, text=True, env=dict(os.environ, EXA_DETERMINISTIC="1"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    line = [l for l in r.stdout.split("\n") if l.startswith("STATS")][0][5:].split("|")
    assert [int(v) for v in line[0].split()] == full["newton"] and [int(v) for v in line[1].split()] == full["krylov"]
    a, b = full["ck"], L.read_checkpoint(str(cd / "final.ckpt"))
    for s in FIELD_SECTIONS + ("avg_stress", "solver_stats"):
        assert np.array_equal(a[s].ravel().view(np.int64 if a[s].dtype == np.float64 else np.int32), b[s].ravel().view(np.int64 if a[s].dtype == np.float64 else np.int32)), s
    _assert_same_files(fd, cd)


@pytest.mark.parametrize("kind", ["multigrid", "p2_bbar", "tet"])
def test_resume_is_exact_other_discretisations(tmp_path, kind):
    import exaconstit_amd.lib as L
    if kind == "multigrid":
        toml = _gen_toml(tmp_path, "mg", N=8, precond="multigrid")
    elif kind == "p2_bbar":
        toml = _gen_toml(tmp_path, "p2b", N=3, p=2, assembly="EA", integ="BBAR")
    else:
        mesh = T.write_mfem(str(tmp_path / "k3.mesh"), T.kuhn_cube(3, perturb=0.2, shuffle=True, seed=2))
        toml = _gen_toml(tmp_path, "tet", mesh=mesh, p=1)
    full, cut, fd, cd = _full_and_resumed(L, toml, 3, 6, tmp_path)
    _same_state(full, cut)
    _assert_same_files(fd, cd)


@pytest.mark.parametrize("aos_side", ["writer", "reader"])
def test_file_is_layout_free(tmp_path, monkeypatch, aos_side):
    """EXA_QLAYOUT=aos for the writer only / the reader only.  The file does not know the layout: loaded and saved again at once by a driver of
    the other layout it is the same file, byte for byte.  The existing tests promise agreement of the two layouts to round-off only
    (tests/test_gpu_parity.py, test_element_blocked_layout_matches_aos: 1e-12 relative per launch), not the same bits, so the resumed run is held
    to the bound the suite uses for runs that differ at round-off (test_partitioned_run_matches_single_rank): 1e-9 max|sigma|, equal Newton counts,
    against the uninterrupted run of the reader's layout."""
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    aos = {"EXA_QLAYOUT": "aos"}
    wenv, renv = (aos, None) if aos_side == "writer" else (None, aos)
    full, cut, fd, cd = _full_and_resumed(L, toml, 4, 8, tmp_path, reader_env=renv, writer_env=wenv, monkeypatch=monkeypatch)
    s0, s1 = full["avgs"][0], cut["avgs"][0]
    diff = np.abs(s0 - s1).max()
    print("layout %s: max |avg_stress difference| %.3e (max |sigma| %.3e)" % (aos_side, diff, np.abs(s0).max()))
    assert diff <= 1e-9 * np.abs(s0).max() and full["newton"] == cut["newton"]
    # reader's layout: load, save at once, compare the bytes
    for key in ("EXA_QLAYOUT",):
        monkeypatch.delenv(key, raising=False)
    for key, v in (renv or {}).items():
        monkeypatch.setenv(key, v)
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path / "again"), write_files=False)
    d.load_checkpoint(str(cd / "cut.ckpt"))
    d.save_checkpoint(str(tmp_path / "again.ckpt"))
    d.close()
    assert open(str(cd / "cut.ckpt"), "rb").read() == open(str(tmp_path / "again.ckpt"), "rb").read()


def test_resume_without_deterministic_mode(tmp_path, monkeypatch):
    """FP64 atomics: two uninterrupted runs differ by d (the spread of the code as it stands); the resumed run may differ from an uninterrupted one
    by 10 d with a floor of 1e-12 max|sigma| (three runs are compared where d saw two; the floor covers d = 0)."""
    import exaconstit_amd.lib as L
    monkeypatch.delenv("EXA_DETERMINISTIC")
    toml = _ref_toml(tmp_path, "voce_pa")
    k, n = 6, 12
    runs = []
    for i in range(2):
        d = L.Driver.from_toml(toml, out_dir=str(tmp_path / ("u%d" % i)), write_files=False)
        _steps(d, 1, n)
        runs.append(d.avgs(0, 6)); d.close()
    dspread = np.abs(runs[0] - runs[1]).max()
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    _steps(d, 1, k)
    d.save_checkpoint(str(tmp_path / "c.ckpt")); d.close()
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False, restart=str(tmp_path / "c.ckpt"))
    _steps(d, k + 1, n)
    s = d.avgs(0, 6); d.close()
    got = np.abs(s - runs[0]).max()
    tol = max(10.0 * dspread, 1e-12 * np.abs(runs[0]).max())
    print("non-deterministic: spread of two uninterrupted runs d = %.3e, resumed vs uninterrupted %.3e, allowed %.3e (max |sigma| %.3e)" % (dspread, got, tol, np.abs(runs[0]).max()))
    assert s.shape == runs[0].shape and got <= tol


# ---------------------------------------------------------------------------------------------------------------- output continuity
def _tree(d):
    out = []
    for base, _, files in os.walk(str(d)):
        for f in files:
            out.append(os.path.relpath(os.path.join(base, f), str(d)))
    return sorted(out)


def test_output_continuity_and_keep(tmp_path):
    """RunAll with [Checkpoint]: paraview, grain averages, texture and light-up on.  The interrupted run goes two steps past its last-but-one
    checkpoint before it is "killed" and restarts from the older file.  (The truncated .tmp it leaves behind cannot be picked up by anything -
    the library never searches for checkpoints, the user names one - so all it shows is that the resumed run's own write of that checkpoint
    goes through the same name and replaces it.)"""
    import exaconstit_amd.lib as L
    vis = ["paraview = true", "steps = 2", 'floc = "vis/run"', "grain_avgs = true", "texture = true", "light_up = true",
           "light_up_hkl = [[1,1,1],[2,0,0],[2,2,0]]", "light_up_dist_tol_deg = 15.0"]
    n = 8
    def toml_for(d_, nsteps, extra):
        t = _ref_toml(d_, "voce_pa", vis=vis, extra=extra)
        txt = open(t).read(); assert "nsteps = 40" in txt
        open(t, "w").write(txt.replace("nsteps = 40", "nsteps = %d" % nsteps, 1))
        return t
    ckpt = '[Checkpoint]\nwrite = true\nsteps = 2\nfloc = "ck"\nkeep = 2\n'
    fd, cd = tmp_path / "full", tmp_path / "cut"
    d = L.Driver.from_toml(toml_for(fd, n, ckpt), out_dir=str(fd))
    assert d.run() == n
    d.close()
    assert sorted(f for f in os.listdir(str(fd)) if f.endswith(".ckpt")) == ["ck_000006.ckpt", "ck_000008.ckpt"]      # keep = 2
    # interrupted: 6 steps (checkpoints at 2, 4, 6 -> 4 and 6 kept), "killed" while writing; restart from step 4's file
    d = L.Driver.from_toml(toml_for(cd, 6, ckpt), out_dir=str(cd))
    assert d.run() == 6
    d.close()
    assert sorted(f for f in os.listdir(str(cd)) if f.endswith(".ckpt")) == ["ck_000004.ckpt", "ck_000006.ckpt"]
    raw = open(str(cd / "ck_000006.ckpt"), "rb").read()
    open(str(cd / "ck_000008.ckpt.tmp"), "wb").write(raw[:len(raw) // 3])
    os.remove(str(cd / "ck_000006.ckpt"))
    os.makedirs(str(cd / "time"), exist_ok=True)
    d = L.Driver.from_toml(toml_for(cd, n, ckpt + 'restart_from = "%s"\n' % str(cd / "ck_000004.ckpt")), out_dir=str(cd))
    assert d.run() == n
    d.close()
    assert not os.path.exists(str(cd / "ck_000008.ckpt.tmp"))           # (the resumed run's own write of that checkpoint went through the name)
    skip = lambda t: [f for f in t if not f.startswith("time/") and not f.endswith(".toml")]  # noqa: E731
    assert skip(_tree(fd)) == skip(_tree(cd))
    for f in ("test_voce_pa_stress.txt", "lattice_strains.txt", "lattice_volumes.txt"):
        a, b = open(str(fd / f), "rb").read(), open(str(cd / f), "rb").read()
        assert a == b and len(a.strip().split(b"\n")) == n, f
    pvd = [f for f in _tree(cd) if f.endswith(".pvd")]
    assert len(pvd) == 1
    txt = open(str(cd / pvd[0])).read()
    assert txt == open(str(fd / pvd[0])).read() and txt.count("<DataSet") >= 5                     # cycles 0, 2, 4, 6, 8
    for f in _tree(fd):
        if f.startswith(("grain_avgs", "texture")) and f.endswith(".txt"):
            assert open(str(fd / f), "rb").read() == open(str(cd / f), "rb").read(), f
    assert L.read_checkpoint(str(fd / "ck_000008.ckpt"))["pvd_cycles"][:, 0].tolist() == [0, 2, 4, 6, 8]
    a, b = L.read_checkpoint(str(fd / "ck_000008.ckpt")), L.read_checkpoint(str(cd / "ck_000008.ckpt"))
    for s in FIELD_SECTIONS:
        assert np.array_equal(a[s].view(np.int64), b[s].view(np.int64)), s


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_load(tmp_path):
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    _steps(d, 1, 2)
    ck = str(tmp_path / "a.ckpt")
    d.save_checkpoint(ck)
    with pytest.raises(RuntimeError, match="freshly created driver"):
        d.load_checkpoint(ck)                                             # after steps
    d.close()

    def refused(path_toml, *words, file=ck):
        e = L.Driver.from_toml(path_toml, out_dir=str(tmp_path), write_files=False)
        with pytest.raises(RuntimeError) as x:
            e.load_checkpoint(file)
        e.close()
        for w in words:
            assert w in str(x.value), str(x.value)
        with pytest.raises(RuntimeError) as x:                            # the same through restart=
            L.Driver.from_toml(path_toml, out_dir=str(tmp_path), write_files=False, restart=file)
        for w in words:
            assert w in str(x.value), str(x.value)

    refused(_ref_toml(tmp_path, "voce_bcc"), "model id mismatch")
    t = open(toml).read(); assert "ncuts = [5, 5, 5]" in t
    other = str(tmp_path / "n4.toml"); open(other, "w").write(t.replace("ncuts = [5, 5, 5]", "ncuts = [4, 4, 4]"))
    refused(other, "global element count mismatch", "1000", "512")
    assert "prefinement = 1" in t
    p2 = str(tmp_path / "p2.toml"); open(p2, "w").write(t.replace("prefinement = 1", "p_refinement = 2"))
    refused(p2, "order mismatch")
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel(); props[3] *= 1.0 + 1e-12
    np.savetxt(str(tmp_path / "props2.txt"), props, fmt="%.17g")
    pp = str(tmp_path / "pp.toml"); open(pp, "w").write(t.replace(os.path.join(REF, "props_cp_voce.txt"), str(tmp_path / "props2.txt")))
    refused(pp, "property hash mismatch")
    grains = np.loadtxt(os.path.join(REF, "grains.txt")).astype(int).ravel(); grains[7] = grains[7] % 500 + 1
    np.savetxt(str(tmp_path / "grains2.txt"), grains.reshape(-1, 1), fmt="%d")
    gg = str(tmp_path / "gg.toml"); open(gg, "w").write(t.replace(os.path.join(REF, "grains.txt"), str(tmp_path / "grains2.txt")))
    refused(gg, "grain-map hash mismatch")
    raw = bytearray(open(ck, "rb").read())
    secs = L.checkpoint_info(ck)["sections"]
    for name in ("matVars0", "stress0", "x_beg", "avg_stress"):
        off, nb, _ = secs[name]
        bad = bytearray(raw); bad[off + nb // 2 + 3] ^= 0x04
        fp = str(tmp_path / "flip.ckpt"); open(fp, "wb").write(bytes(bad))
        refused(toml, "checksum mismatch in section '%s'" % name, file=fp)
    fp = str(tmp_path / "short.ckpt"); open(fp, "wb").write(bytes(raw[:secs["matVars0"][0] + 1000]))
    refused(toml, "truncated", "matVars0", file=fp)
    fp = str(tmp_path / "magic.ckpt"); open(fp, "wb").write(b"XX" + bytes(raw[2:]))
    refused(toml, "wrong magic", file=fp)
    # a refused load leaves the driver as it was created (nothing is taken over before every checksum is verified): it runs from the start ...
    off, nb, _ = secs["matVars0"]
    bad = bytearray(raw); bad[off + 8 * 5] ^= 0x80
    fp = str(tmp_path / "flip2.ckpt"); open(fp, "wb").write(bytes(bad))
    fresh = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    e = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    with pytest.raises(RuntimeError, match="checksum mismatch in section 'matVars0'"):
        e.load_checkpoint(fp)
    _steps(fresh, 1, 2); _steps(e, 1, 2)
    assert np.array_equal(fresh.avgs(0, 6).view(np.int64), e.avgs(0, 6).view(np.int64))
    for c in (0, 3, 27):
        assert np.array_equal(fresh.qf_component(0, c).view(np.int64), e.qf_component(0, c).view(np.int64))
    fresh.close(); e.close()
    # ... or takes the good file afterwards
    e = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    with pytest.raises(RuntimeError, match="checksum mismatch"):
        e.load_checkpoint(fp)
    e.load_checkpoint(ck)
    assert e.step(3)
    e.close()
    # a good file still loads after all of this, twice is refused
    e = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False, restart=ck)
    with pytest.raises(RuntimeError, match="freshly created driver"):
        e.load_checkpoint(ck)
    assert e.step(3)
    e.close()


def test_state_of_another_writer_is_normalised(tmp_path):
    """A file whose header names another writer goes through exa_state_normalize after the unpack (slot 0 = sum of |slots 14 ... 25|); this library's
    own files do not (test_resume_is_exact: they come back bit for bit)."""
    import struct
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    _steps(d, 1, 3)
    ck = str(tmp_path / "own.ckpt")
    d.save_checkpoint(ck)
    gid = d.element_fields()["GlobalElementId"]
    d.close()
    raw = bytearray(open(ck, "rb").read())
    info = L.checkpoint_info(ck)
    off, nb, _ = info["sections"]["matVars0"]
    mv = np.frombuffer(bytes(raw[off:off + nb]), "<f8").reshape(-1, 8, 28).copy()
    assert np.abs(mv[:, :, 0]).max() > 0
    mv[:, :, 0] = 0.0                                                      # what another code would leave there
    raw[off:off + nb] = mv.tobytes()
    entry = 256 + 48 * list(info["sections"]).index("matVars0")
    struct.pack_into("<Q", raw, entry + 40, int(mv.ravel().view(np.uint64).sum(dtype=np.uint64)))
    struct.pack_into("<I", raw, 144, 0)
    struct.pack_into("<Q", raw, 248, int(np.frombuffer(bytes(raw[:248]), "<u8").sum(dtype=np.uint64)))
    other = str(tmp_path / "other.ckpt"); open(other, "wb").write(bytes(raw))
    assert L.checkpoint_info(other)["writer"] == 0
    e = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False, restart=other)
    want = np.abs(mv[:, :, 14:26]).sum(axis=2)
    got = e.qf_component(0, 0).reshape(len(gid), 8)
    assert np.allclose(got, want[gid], rtol=1e-14, atol=0.0) and np.abs(got).max() > 0
    for c in (1, 5, 14, 27):
        assert np.array_equal(e.qf_component(0, c).reshape(len(gid), 8), mv[gid, :, c])
    assert e.step(4)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- several ranks
def _rank_threads(L, nranks, work):
    """work(rank, uid) on one thread per rank of an in-process loopback group"""
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    errors, out = [], [None] * nranks

    def run(r):
        try:
            out[r] = work(r, gid)
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
    th = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    assert all(not t.is_alive() for t in th), "a rank hung"
    assert not errors, errors
    L.exa_loopback_group_destroy(gid)
    return out


def _run_ranks(L, toml, nranks, out_dir, first, last, load=None, save_at=None, final=None):
    """steps first..last on nranks rank threads (optionally resuming from `load`); checkpoints: save_at = (step, path), final = path"""
    os.makedirs(str(out_dir), exist_ok=True)

    def work(r, uid):
        d = L.Driver.from_toml(toml, out_dir=str(out_dir), rank=r, nranks=nranks, uid=uid if nranks > 1 else None, write_files=(r == 0), restart=load)
        for ti in range(first, last + 1):
            assert d.step(ti), (r, ti)
            if save_at and ti == save_at[0]:
                d.save_checkpoint(save_at[1])
        if final:
            d.save_checkpoint(final)
        res = (d.avgs(0, 6), [list(x) for x in d.stats()])
        d.close()
        return res
    return _rank_threads(L, nranks, work)


@pytest.mark.parametrize("nranks", [2, 4])
def test_resume_same_rank_count(tmp_path, nranks):
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    k, n = 4, 8
    full = _run_ranks(L, toml, nranks, tmp_path / "full", 1, n, final=str(tmp_path / "full.ckpt"))
    _run_ranks(L, toml, nranks, tmp_path / "cut", 1, k, final=str(tmp_path / "cut.ckpt"))
    assert L.checkpoint_info(str(tmp_path / "cut.ckpt"))["nranks"] == nranks
    cut = _run_ranks(L, toml, nranks, tmp_path / "cut", k + 1, n, load=str(tmp_path / "cut.ckpt"), final=str(tmp_path / "cutfinal.ckpt"))
    for (s, st), (s2, st2) in zip(full, cut):
        assert np.array_equal(s.view(np.int64), s2.view(np.int64)) and st[0] == st2[0] and st[1] == st2[1]
    a, b = L.read_checkpoint(str(tmp_path / "full.ckpt")), L.read_checkpoint(str(tmp_path / "cutfinal.ckpt"))
    for s in FIELD_SECTIONS:
        assert np.array_equal(a[s].view(np.int64), b[s].view(np.int64)), s
    _assert_same_files(tmp_path / "full", tmp_path / "cut")


def _bytes_but_rank_count(path):
    b = bytearray(open(path, "rb").read())
    b[116:120] = b"\0\0\0\0"            # header: ranks that wrote the file (informational)
    b[248:256] = b"\0" * 8              # ... and the header checksum that covers it
    return bytes(b)


@pytest.mark.parametrize("writer,reader", [(1, 2), (1, 4), (4, 1)])
def test_resume_across_rank_counts(tmp_path, writer, reader):
    """The run resumed on another rank count is held to what the suite promises between rank counts (test_partitioned_run_matches_single_rank:
    1e-9 max|sigma|, equal Newton counts) against the uninterrupted run of the READER's rank count; the file itself is exact: loaded on 1, 2 and 4
    ranks and saved again at once it is the same file apart from the rank-count field."""
    import exaconstit_amd.lib as L
    toml = _ref_toml(tmp_path, "voce_pa")
    k, n = 3, 6
    ref = _run_ranks(L, toml, reader, tmp_path / "ref", 1, n)
    ck = str(tmp_path / "cut.ckpt")
    _run_ranks(L, toml, writer, tmp_path / "w", 1, k, final=ck)
    got = _run_ranks(L, toml, reader, tmp_path / "r", k + 1, n, load=ck)
    for (s, st), (s0, st0) in zip(got, ref):
        diff = np.abs(s - s0).max()
        print("writer %d reader %d: max |avg_stress difference| %.3e" % (writer, reader, diff))
        assert s.shape == s0.shape and diff < 1e-9 * np.abs(s0).max() and st[0] == st0[0]
    want = _bytes_but_rank_count(ck)
    for nr in (1, 2, 4):
        again = str(tmp_path / ("again%d.ckpt" % nr))
        _run_ranks(L, toml, nr, tmp_path / ("again%d" % nr), 1, 0, load=ck, final=again)
        assert L.checkpoint_info(again)["nranks"] == nr
        assert _bytes_but_rank_count(again) == want, "file re-saved by %d ranks differs" % nr


def test_executable_restart_two_rank_processes(tmp_path):
    """`mechanics -opt case.toml -restart file` with 2 rank processes: the run is cut by Checkpoint files of a 6-step run and resumed to 10 steps."""
    import exaconstit_amd.lib as L
    assert os.path.exists(EXE)
    ckpt = '[Checkpoint]\nwrite = true\nsteps = 3\n'
    def stage(d_, nsteps):
        t = _ref_toml(d_, "voce_pa", extra=ckpt)
        txt = open(t).read()
        open(t, "w").write(txt.replace("nsteps = 40", "nsteps = %d" % nsteps, 1))
        return t
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}

    def launch(cwd, toml, port, *args):
        ps = [subprocess.Popen(["timeout", "-k", "10", "600", EXE, "-opt", toml] + list(args), cwd=str(cwd),
                               env=dict(env, EXA_RANK=str(r), EXA_NRANKS="2", EXA_MASTER_PORT=str(port), EXA_DETERMINISTIC="1")) for r in range(2)]
        rcs = [p.wait(timeout=700) for p in ps]
        assert rcs == [0, 0], rcs
    fd, cd = tmp_path / "full", tmp_path / "cut"
    launch(fd, stage(fd, 10), 29561)
    launch(cd, stage(cd, 6), 29562)
    assert sorted(f for f in os.listdir(str(cd)) if f.endswith(".ckpt")) == ["checkpoint_000003.ckpt", "checkpoint_000006.ckpt"]
    assert L.checkpoint_info(str(cd / "checkpoint_000006.ckpt"))["nranks"] == 2
    launch(cd, stage(cd, 10), 29563, "-restart", str(cd / "checkpoint_000003.ckpt"))
    a, b = open(str(fd / "test_voce_pa_stress.txt"), "rb").read(), open(str(cd / "test_voce_pa_stress.txt"), "rb").read()
    assert a == b and len(a.strip().split(b"\n")) == 10
    x, y = L.read_checkpoint(str(fd / "checkpoint_000010.ckpt")), L.read_checkpoint(str(cd / "checkpoint_000010.ckpt"))
    for s in FIELD_SECTIONS + ("avg_stress", "solver_stats"):
        assert np.array_equal(x[s], y[s]), s
