"""Per-grain averages on the GPU: Driver.grain_averages() against numpy sums of the element_fields() rows of the same state for
crafted grain maps (Driver.set_grains), repeat calls, identities with the driver's volume averages, the per-step grain_avgs files of a run,
several loopback ranks and the executable on two rank processes."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
EXE = os.path.join(ROOT, "exaconstit_amd", "mechanics")
DTS = np.array([0.005, 0.1, 0.2])
ANGLES = ("MisorientationMean", "MisorientationMax", "GrainRotation")


def _props():
    return np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def quat_to_mat(q):
    x0, x1, x2, x3 = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([x0 * x0 + x1 * x1 - x2 * x2 - x3 * x3, 2 * (x1 * x2 - x0 * x3), 2 * (x1 * x3 + x0 * x2)], -1),
                     np.stack([2 * (x1 * x2 + x0 * x3), x0 * x0 - x1 * x1 + x2 * x2 - x3 * x3, 2 * (x2 * x3 - x0 * x1)], -1),
                     np.stack([2 * (x1 * x3 - x0 * x2), 2 * (x2 * x3 + x0 * x1), x0 * x0 - x1 * x1 - x2 * x2 + x3 * x3], -1)], -2)


def misori_deg(a, b):
    """2 atan2(|d_vec|, |d_0|) of d = conj(a) (x) b, degrees (rows of unit quaternions)"""
    d0 = (a * b).sum(-1)
    dv = a[..., :1] * b[..., 1:] - b[..., :1] * a[..., 1:] - np.cross(a[..., 1:], b[..., 1:])
    return np.degrees(2.0 * np.arctan2(np.linalg.norm(dv, axis=-1), np.abs(d0)))


def grains_numpy(f, qref):
    """the grain averages of DESIGN 4.7 from element_fields() rows; qref[g - 1] = unit reference orientation of grain g"""
    attr = f["attribute"].astype(np.int64)
    ids, inv = np.unique(attr, return_inverse=True)
    n = len(ids)
    V = f["ElementVolume"][:, 0]

    def vsum(x):
        """sum over each grain of V x, in extended precision: the reference is then closer to the exact sums than the kernel's blocked sums
        (a sequential double sum over the 6912 elements of a large grain errs by ~1e-14, which moves qbar, and so every angle, by ~1e-12 degrees)"""
        x = x.reshape(len(V), -1)
        out = np.zeros((n, x.shape[1]), np.longdouble)
        np.add.at(out, inv, V[:, None].astype(np.longdouble) * x)
        return out.astype(np.float64)
    vol = vsum(np.ones(len(V)))[:, 0]
    o = {"grain_id": ids, "n_elements": np.bincount(inv, minlength=n), "volume": vol, "volume_fraction": vol / V.sum()}
    s = vsum(f["Stress"]) / vol[:, None]
    o["Stress"] = s
    o["VonMisesStress"] = np.sqrt(0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2 + 6 * (s[:, 3:] ** 2).sum(1)))
    o["HydrostaticStress"] = s[:, :3].sum(1) / 3.0
    e = f["XtalElasticStrain"]
    T = np.stack([np.stack([e[:, 0], e[:, 5], e[:, 4]], -1), np.stack([e[:, 5], e[:, 1], e[:, 3]], -1), np.stack([e[:, 4], e[:, 3], e[:, 2]], -1)], -2)
    q = f["LatticeOrientation"]
    R = quat_to_mat(q)
    Ts = np.einsum("eij,ejk,elk->eil", R, T, R)
    es = np.stack([Ts[:, 0, 0], Ts[:, 1, 1], Ts[:, 2, 2], Ts[:, 1, 2], Ts[:, 0, 2], Ts[:, 0, 1]], -1)
    o["ElasticStrainSample"] = vsum(es) / vol[:, None]
    o["XtalElasticStrain"] = vsum(e) / vol[:, None]
    for k in ("EffPlasticStrain", "DpEff", "Hardness"):
        o[k] = vsum(f[k])[:, 0] / vol
    o["ShearRate"] = vsum(f["ShearRate"]) / vol[:, None]
    qr = qref[attr - 1]
    sgn = np.where((q * qr).sum(1) >= 0.0, 1.0, -1.0)
    qbar = _unit(vsum(sgn[:, None] * q))
    o["LatticeOrientation"] = qbar
    th = misori_deg(qbar[inv], q)
    o["MisorientationMean"] = vsum(th)[:, 0] / vol
    mx = np.zeros(n)
    np.maximum.at(mx, inv, th)
    o["MisorientationMax"] = mx
    o["GrainRotation"] = misori_deg(qbar, qref[ids - 1])
    # the scale of every column: the largest element value its sums add up (an average can cancel far below it)
    am = lambda x: np.abs(x).max(axis=0)   # noqa: E731
    sm = am(f["Stress"]).max()
    o["_scale"] = {"volume": vol.max(), "volume_fraction": 1.0, "Stress": am(f["Stress"]), "VonMisesStress": 3 * sm, "HydrostaticStress": sm,
                   "ElasticStrainSample": np.abs(e).max(), "XtalElasticStrain": am(e), "EffPlasticStrain": am(f["EffPlasticStrain"]),
                   "DpEff": am(f["DpEff"]), "Hardness": am(f["Hardness"]), "ShearRate": am(f["ShearRate"]), "LatticeOrientation": 1.0}
    return o


def _compare(got, ref, rel=1e-12):
    assert np.array_equal(got["grain_id"], ref["grain_id"])
    assert np.array_equal(got["n_elements"], ref["n_elements"])
    for k, r in ref.items():
        if k in ("grain_id", "n_elements", "_scale"):
            continue
        g = got[k]
        assert g.shape == r.shape, k
        if k in ANGLES:
            tol = 1e-12 + rel * np.abs(r)                                        # degrees
        else:
            tol = rel * (np.abs(r) + ref["_scale"][k])                           # relative to the value and to the scale of what was summed
        assert np.all(np.abs(g - r) <= tol), (k, np.abs(g - r).max(), np.abs(r).max())


def crafted_map(N, rng):
    """one grain of half the box (x < N/2), 50 single-element grains, about 200 grains of random sizes; ids non-contiguous with unused ids"""
    E = N ** 3
    x = np.arange(E) % N
    grain = np.zeros(E, np.int64)
    half = np.flatnonzero(x < N // 2)
    rest = rng.permutation(np.flatnonzero(x >= N // 2))
    cuts = np.sort(rng.choice(np.arange(1, len(rest) - 50), 199, replace=False))
    pieces = np.split(rest[50:], cuts)                                            # 200 grains of random sizes
    groups = [half] + [rest[i:i + 1] for i in range(50)] + [p for p in pieces if len(p)]
    ids = rng.choice(np.arange(1, 4 * len(groups)), len(groups), replace=False) + 1
    for gid, el in zip(ids, groups):
        grain[el] = gid
    G = int(4 * len(groups) + 7)                                                  # unused ids above the largest, too
    assert grain.min() >= 1
    return grain.astype(np.int32), G, ids, len(groups)


def _synthetic(N, grain, gq, **kw):
    import exaconstit_amd.lib as L
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS, **kw)
    d.set_grains(grain, gq)
    return d


def test_against_numpy_24():
    N = 24
    rng = np.random.default_rng(24)
    grain, G, ids, ng = crafted_map(N, rng)
    gq = rng.standard_normal((G, 4)) * rng.uniform(0.5, 2.0, (G, 1))            # not normalised: set_grains does
    qref = _unit(gq)
    d = _synthetic(N, grain, gq)
    # before the first step every element has its grain's orientation
    g0 = d.grain_averages()
    assert len(g0["grain_id"]) == ng and np.array_equal(g0["grain_id"], np.sort(ids))
    assert g0["GrainRotation"].max() < 1e-10 and g0["MisorientationMax"].max() < 1e-10
    assert np.allclose(g0["LatticeOrientation"], qref[g0["grain_id"] - 1], rtol=0, atol=1e-14)
    f0 = d.element_fields()
    assert np.array_equal(f0["attribute"], grain[f0["GlobalElementId"]])
    _compare(g0, grains_numpy(f0, qref))
    for ti in (1, 2):
        assert d.step(ti)
    got = d.grain_averages()
    f = d.element_fields()
    ref = grains_numpy(f, qref)
    _compare(got, ref)
    assert got["MisorientationMax"].max() > 0.0 and got["GrainRotation"].max() > 0.0      # the state has moved: the angles are not trivially 0
    # repeat calls: the same bits
    again = d.grain_averages()
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    # identities
    s_avg = d.avgs(0, 6)[-1]
    s_sum = (got["volume_fraction"][:, None] * got["Stress"]).sum(0)
    assert np.all(np.abs(s_sum - s_avg) <= 1e-12 * np.abs(s_avg).max()), (s_sum, s_avg)
    assert got["n_elements"].sum() == N ** 3 and abs(got["volume_fraction"].sum() - 1.0) < 1e-13
    single = got["n_elements"] == 1
    assert single.sum() >= 50 and got["MisorientationMax"][single].max() < 1e-10
    assert got["n_elements"].max() == N ** 3 // 2
    with pytest.raises(RuntimeError, match="before the first step"):
        d.set_grains(grain, gq)
    d.close()


def test_against_numpy_64():
    """512 grains of 8^3 elements at 64^3: every grain spans several 64-element chunks and the launches many blocks"""
    N = 64
    rng = np.random.default_rng(64)
    i = np.arange(N ** 3)
    x, y, z = i % N, (i // N) % N, i // (N * N)
    cell = (x // 8) + 8 * ((y // 8) + 8 * (z // 8))
    perm = rng.permutation(512) + 1
    grain = perm[cell].astype(np.int32)
    gq = _unit(rng.standard_normal((512, 4)))
    d = _synthetic(N, grain, gq)
    for ti in (1, 2):
        assert d.step(ti)
    got = d.grain_averages()
    _compare(got, grains_numpy(d.element_fields(), gq))
    assert len(got["grain_id"]) == 512 and np.all(got["n_elements"] == 512)
    again = d.grain_averages()
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    d.close()


def test_set_grains_refusals():
    import exaconstit_amd.lib as L
    N = 4
    quats = _unit(np.random.default_rng(1).standard_normal((N ** 3, 4)))
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS)
    # without the hook: one grain per element, q_ref = the element's initial orientation
    g = d.grain_averages()
    assert np.array_equal(g["grain_id"], np.arange(1, N ** 3 + 1)) and np.all(g["n_elements"] == 1)
    assert g["GrainRotation"].max() < 1e-10
    assert np.allclose(g["LatticeOrientation"], quats, rtol=0, atol=1e-14)
    ok = np.ones(N ** 3, np.int32)
    with pytest.raises(RuntimeError, match="1 .. G"):
        d.set_grains(np.full(N ** 3, 2, np.int32), quats[:1])
    with pytest.raises(RuntimeError, match="1 .. G"):
        d.set_grains(np.zeros(N ** 3, np.int32), quats[:1])
    with pytest.raises(RuntimeError, match="global element"):
        d.set_grains(ok[:-1], quats[:1])
    with pytest.raises(RuntimeError, match="zero"):
        d.set_grains(ok, np.zeros((1, 4)))
    d.set_grains(ok, quats[:1])
    g = d.grain_averages()
    assert np.array_equal(g["grain_id"], [1]) and g["n_elements"][0] == N ** 3 and g["MisorientationMax"][0] < 1e-10
    d.close()


def _stage(tmp_path, vis_lines, nsteps=None):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")) and not f.endswith("_stress.txt"):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines + ['avg_stress_fname = "test_voce_pa_stress.txt"']) + t[b:]
    assert "nsteps = 40" in t
    if nsteps is not None:
        t = t.replace("nsteps = 40", "nsteps = %d" % nsteps, 1)
    path = os.path.join(str(tmp_path), "voce_pa.toml")
    open(path, "w").write(t)
    return path


def _files(d, fname="grain_avgs"):
    return sorted(glob.glob(os.path.join(str(d), fname + "_*.txt")))


def test_driver_files(tmp_path):
    """voce_pa (125 grains of 8 elements on 10^3, 500 orientation rows) to its end with steps = 3: files at 3, 6, ..., 39 and 40"""
    import exaconstit_amd.lib as L
    toml = _stage(tmp_path, ["grain_avgs = true", "steps = 3"])
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=True)
    due = [ti for ti in range(1, 41) if ti % 3 == 0 or ti == 40]
    seen = {}
    for ti in range(1, 41):
        assert d.step(ti)
        if ti in due:
            seen[ti] = d.grain_averages()
    d.close()
    names = [os.path.basename(p) for p in _files(tmp_path)]
    assert names == ["grain_avgs_%06d.txt" % ti for ti in due]
    ori = _unit(np.loadtxt(os.path.join(REFDATA, "voce_quats.ori")).reshape(-1, 4))
    for ti in due:
        path = os.path.join(str(tmp_path), "grain_avgs_%06d.txt" % ti)
        head = open(path).readline().split()
        assert head[0] == "#" and len(head) == 47 and head[1] == "grain_id"
        got = L.read_grain_avgs(path)
        assert len(got["grain_id"]) == 125 and np.all(got["n_elements"] == 8)
        for k in got:
            assert np.array_equal(got[k], seen[ti][k]), (ti, k)                 # 17 significant digits: the same doubles
    # the reference orientations are the orientation file's rows of the grains
    g = seen[40]
    q = g["LatticeOrientation"]
    assert np.all(g["GrainRotation"] > 0) and np.all(g["GrainRotation"] < 10.0)
    assert np.allclose(np.abs((q * ori[g["grain_id"] - 1]).sum(1)), 1.0, atol=1e-2)
    # without the key: no files
    t2 = tmp_path / "off"
    t2.mkdir()
    toml = _stage(t2, ["steps = 1"], nsteps=2)
    d = L.Driver.from_toml(toml, out_dir=str(t2), write_files=True)
    assert d.run() == 2
    d.close()
    assert _files(t2) == []


def test_two_loopback_ranks_match_one():
    """12^3 synthetic mesh with grains of 5^3 elements offset by 2: the split of the box between the two ranks cuts through grains"""
    import exaconstit_amd.lib as L
    N = 12
    i = np.arange(N ** 3)
    x, y, z = i % N, (i // N) % N, i // (N * N)
    cell = ((x + 2) // 5) + 4 * (((y + 2) // 5) + 4 * ((z + 2) // 5))
    grain = (cell + 1).astype(np.int32)
    G = 64
    gq = _unit(np.random.default_rng(12).standard_normal((G, 4)))
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))

    def run(nranks):
        gid = (C.c_ubyte * 128)()
        assert L.exa_loopback_group_create(nranks, gid) == 0
        res, errors = [None] * nranks, []

        def work(r):
            try:
                d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS, rank=r, nranks=nranks, uid=gid)
                d.set_grains(grain, gq)
                for ti in (1, 2):
                    assert d.step(ti)
                f = d.element_fields()
                res[r] = (d.grain_averages(), set(f["attribute"].tolist()))
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

    one = run(1)[0][0]
    two = run(2)
    assert two[0][1] & two[1][1], "no grain is shared by the two ranks"
    for k in one:
        assert np.array_equal(two[0][0][k], two[1][0][k]), k                    # every rank sees the all-reduced values
    # the two partitions reduce the PCG dot products in another order: the converged states agree to round-off, not bit for bit
    one["_scale"] = {k: np.abs(v).max(axis=0) for k, v in one.items() if k not in ("grain_id", "n_elements") + ANGLES}
    _compare(two[0][0], one, rel=1e-10)


def _mpirun():
    for c in ("mpirun", "/opt/conda/bin/mpirun", "mpiexec"):
        p = shutil.which(c) or (c if os.path.exists(c) else None)
        if p:
            return p
    return None


def test_executable_two_ranks_ipc(tmp_path):
    """`mechanics -opt` on one rank and on two rank processes sharing the device through the ipc transport (reductions of 125 x 39 doubles)"""
    import exaconstit_amd.lib as L
    assert os.path.exists(EXE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir()
    d2.mkdir()
    lines = ["grain_avgs = true", "steps = 2", 'grain_avgs_fname = "gr"']
    _stage(d1, lines, nsteps=4)
    _stage(d2, lines, nsteps=4)
    r = subprocess.run([EXE, "-opt", "voce_pa.toml"], cwd=str(d1), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    env2 = dict(env, EXA_TRANSPORT="ipc", EXA_MASTER_PORT="29571")
    mpirun = _mpirun()
    if mpirun:
        r = subprocess.run([mpirun, "-np", "2", EXE, "-opt", "voce_pa.toml"], cwd=str(d2), env=env2, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "transport ipc" in r.stderr or "ipc" in r.stderr, r.stderr
    else:
        ps = [subprocess.Popen([EXE, "-opt", "voce_pa.toml"], cwd=str(d2), env=dict(env2, EXA_RANK=str(k), EXA_NRANKS="2")) for k in range(2)]
        assert all(p.wait(timeout=1200) == 0 for p in ps)
    f1, f2 = _files(d1, "gr"), _files(d2, "gr")
    assert [os.path.basename(p) for p in f1] == ["gr_000002.txt", "gr_000004.txt"] == [os.path.basename(p) for p in f2]
    for a, b in zip(f1, f2):
        ref = L.read_grain_avgs(a)
        ref["_scale"] = {k: np.abs(v).max(axis=0) for k, v in ref.items() if k not in ("grain_id", "n_elements") + ANGLES}
        _compare(L.read_grain_avgs(b), ref, rel=1e-10)
