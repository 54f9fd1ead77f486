"""Texture on the GPU: exa_texture_weights against a numpy restatement of the pole-figure and inverse-pole-figure binning on
crafted rows, a single orientation, the MRD normalisation, bitwise repeatability in any row order or split, Driver.pole_figures() against numpy
on element_fields(), one loopback rank against two, the per-step texture files of a run and the executable on two rank processes."""
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
NF = 37
FAMILIES = [(1, 1, 1), (2, 0, 0), (2, 2, 0), (3, 1, 1), (1, 2, 3)]
DIRS = [(0.0, 0.0, 1.0), (0.3, -0.5, 0.8)]
EDGE = 1e-9          # radians: a pole this close to a bin edge may land on either side
DTS = np.array([0.005, 0.1, 0.2])


def quat_to_mat(q):
    """R(q) of quat_to_mat (ecm_device.hpp), scalar first; crystal -> sample.  q (.., 4) -> (.., 3, 3)"""
    x0, x1, x2, x3 = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([x0 * x0 + x1 * x1 - x2 * x2 - x3 * x3, 2 * (x1 * x2 - x0 * x3), 2 * (x1 * x3 + x0 * x2)], -1),
                     np.stack([2 * (x1 * x2 + x0 * x3), x0 * x0 - x1 * x1 + x2 * x2 - x3 * x3, 2 * (x2 * x3 - x0 * x1)], -1),
                     np.stack([2 * (x1 * x3 - x0 * x2), 2 * (x2 * x3 + x0 * x1), x0 * x0 - x1 * x1 - x2 * x2 + x3 * x3], -1)], -2)


def cubic_rotations():
    """the 24 proper rotations of the cubic group: signed permutation matrices of determinant +1"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, p[i]] = s[i]
            if np.linalg.det(m) > 0:
                out.append(m)
    assert len(out) == 24
    return np.array(out)


def fiber_axes(hkl):
    """distinct axes of the cubic orbit of (h, k, l) / |(h, k, l)|, a direction and its negative once"""
    c = np.asarray(hkl, float) / np.linalg.norm(hkl)
    ax = []
    for m in cubic_rotations():
        a = m @ c
        lead = a[np.flatnonzero(a)[0]]
        a = a if lead > 0 else -a
        if not any(np.array_equal(a, b) for b in ax):
            ax.append(a)
    return np.array(ax)


def bins_numpy(p, res):
    """DESIGN 4.8 binning of poles p (.., 3): ring, sector and whether the pole lies within EDGE of a bin edge (or of the fold)"""
    p = np.array(p, float)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    flip = (z < 0) | ((z == 0) & ((y < 0) | ((y == 0) & (x < 0))))
    x, y, z = np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)
    na, nb = round(90 / res), round(360 / res)
    rho = np.hypot(x, y)
    a = np.arctan2(rho, z)
    b = np.where(rho > 0, np.arctan2(y, x), 0.0)
    b = np.where(b < 0, b + 2 * np.pi, b)
    r = np.radians(res)
    i = np.minimum(np.floor(np.degrees(a) / res).astype(int), na - 1)
    k = np.floor(np.degrees(b) / res).astype(int) % nb
    da = np.abs(a / r - np.rint(a / r)) * r                          # distance to the nearest ring edge
    db = np.abs(b / r - np.rint(b / r)) * r * np.maximum(np.sin(a), 1e-300)
    near = ((da < EDGE) & (a > EDGE) & (a < np.pi / 2 - EDGE)) | (db < EDGE) | (a < EDGE) | (np.abs(z) < EDGE)
    return i, k, near


def weights_numpy(rows, hkls, dirs, res):
    """W [set][n_alpha][n_beta] of the poles off the edges, the allowance [set][n_alpha][n_beta] (the weight of the near-edge poles that may
    land in that bin: their ring and sector +- 1, and the far side of the fold) and the total weight of the near-edge poles of each set"""
    V = rows[:, 0]
    R = quat_to_mat(rows[:, 27:31])
    na, nb = round(90 / res), round(360 / res)
    sets = []
    for h in hkls:
        A = fiber_axes(h)
        sets.append((np.einsum("eij,aj->eai", R, A), np.repeat(V[:, None] / len(A), len(A), 1)))
    S = cubic_rotations()
    for d in dirs:
        d = np.asarray(d, float) / np.linalg.norm(d)
        u = np.einsum("eij,i->ej", R, d)
        sets.append((np.einsum("kij,ej->eki", S, u), np.repeat(V[:, None] / 24.0, 24, 1)))
    W = np.zeros((len(sets), na, nb))
    allow = np.zeros_like(W)
    amb = np.zeros(len(sets))
    for s, (p, w) in enumerate(sets):
        i, k, near = bins_numpy(p, res)
        np.add.at(W[s], (i[~near], k[~near]), w[~near])
        amb[s] = w[near].sum()
        for ii, kk, ww, zz in zip(i[near], k[near], w[near], p[near][:, 2]):
            for di in (-1, 0, 1):
                for dk in (-1, 0, 1):
                    if 0 <= ii + di < na:
                        allow[s, ii + di, (kk + dk) % nb] += ww
                        if abs(zz) < EDGE:
                            allow[s, ii + di, (kk + dk + nb // 2) % nb] += ww
            if ii == 0:
                allow[s, 0, :] += ww
    return W, allow, amb


def random_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1)[:, None]


def crafted_rows(rng, E):
    rows = rng.standard_normal((E, NF))                                  # columns the analysis does not read
    rows[:, 0] = rng.uniform(0.5, 1.5, E) * 10.0 ** rng.uniform(-3, 0, E)
    rows[:, 27:31] = random_quats(rng, E)
    return rows


def _ctx(L, E):
    props = np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()
    return L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)


def kernel_counts(L, hipref, dev, rows, hkls, dirs, res, qlog2=None):
    import torch
    E = rows.shape[0]
    ctx = _ctx(L, E)
    if qlog2 is None:
        qlog2 = L.exa_texture_quantum_log2(float(rows[:, 0].max()), E)
    na, nb = L.texture_grid(res)
    d_rows = dev.up(np.ascontiguousarray(rows).ravel())
    d_out = torch.full(((len(hkls) + len(dirs)) * na * nb,), -7, dtype=torch.int64, device=dev.dev)
    L.texture_weights(ctx, hipref.ptr(d_rows), hkls, dirs, res, qlog2, hipref.ptr(d_out))
    dev.sync()
    out = d_out.cpu().numpy().reshape(-1, na, nb)
    ctx.close()
    return out


def mrd_of(W, res):
    import exaconstit_amd.lib as L
    sa = L.texture_cells(res)[2]
    W = np.asarray(W, float)
    return W / W.sum(axis=(1, 2), keepdims=True) * (2 * np.pi / sa)[None, :, None]


def assert_weights_close(got, W, allow, amb, rel=1e-9):
    """got / W: [set][n_alpha][n_beta] weights, compared as fractions of each set's total: W holds the poles off the edges, allow the weight
    of the near-edge poles that may land in each bin, amb [set] their total weight"""
    fg = got / got.sum(axis=(1, 2), keepdims=True)
    tot = W.sum(axis=(1, 2), keepdims=True) + amb[:, None, None]
    lo = W / tot * (1 - rel) - 1e-15
    hi = (W + allow) / tot * (1 + rel) + 1e-15
    bad = (fg < lo) | (fg > hi)
    assert not bad.any(), (np.argwhere(bad)[:5], fg[bad][:5], (W / tot)[bad][:5])


@pytest.mark.parametrize("E", [1000, 64 * 97 + 13])
def test_kernel_against_numpy(E):
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    rng = np.random.default_rng(E)
    rows = crafted_rows(rng, E)
    for res in (5.0, 2.0, 15.0):
        got = kernel_counts(L, hipref, dev, rows, FAMILIES, DIRS, res)
        assert got.min() >= 0
        W, allow, amb = weights_numpy(rows, FAMILIES, DIRS, res)
        assert_weights_close(got, W, allow, amb)
        if not allow.any():   # no pole near an edge: the MRD agrees everywhere
            m, ref = mrd_of(got, res), mrd_of(W, res)
            assert np.all(np.abs(m - ref) <= 1e-9 * np.abs(ref) + 1e-12), (res, np.abs(m - ref).max())


def _off_edge_quat(rng, res, margin=1e-4):
    """an orientation whose {200} poles and images of z all lie more than margin radians from every bin edge and from the equator"""
    for _ in range(1000):
        q = random_quats(rng, 1)[0]
        R = quat_to_mat(q)
        p = np.concatenate([fiber_axes((2, 0, 0)) @ R.T, cubic_rotations() @ (R.T @ np.array([0.0, 0.0, 1.0]))])
        p = np.where(p[:, 2:3] < 0, -p, p)
        a = np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2])
        b = np.arctan2(p[:, 1], p[:, 0])
        r = np.radians(res)
        da = np.abs(a / r - np.rint(a / r)) * r
        db = np.abs(b / r - np.rint(b / r)) * r
        if da.min() > margin and db.min() > margin and np.abs(p[:, 2]).min() > margin:
            return q
    raise AssertionError("no orientation off the bin edges")


def test_single_orientation():
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    rng = np.random.default_rng(11)
    res = 5.0
    q = _off_edge_quat(rng, res)
    E = 777
    rows = crafted_rows(rng, E)
    rows[:, 27:31] = q
    got = kernel_counts(L, hipref, dev, rows, [(2, 0, 0)], [(0, 0, 1)], res)
    pf = got[0] / got[0].sum()
    nz = np.argwhere(pf > 0)
    assert len(nz) == 3
    assert np.all(np.abs(pf[pf > 0] - 1.0 / 3.0) < 1e-12)
    R = quat_to_mat(q)
    i, k, near = bins_numpy((R @ fiber_axes((2, 0, 0)).T).T, res)
    assert not near.any()
    assert sorted(map(tuple, nz)) == sorted(zip(i.tolist(), k.tolist()))
    # inverse pole figure of z: the 24 images of u = R^T z, duplicates kept
    u = R.T @ np.array([0.0, 0.0, 1.0])
    i, k, near = bins_numpy(cubic_rotations() @ u, res)
    assert not near.any()
    want = np.zeros(got[1].shape)
    np.add.at(want, (i, k), 1.0 / 24.0)
    ipf = got[1] / got[1].sum()
    assert np.array_equal(ipf > 0, want > 0)
    assert np.all(np.abs(ipf - want) < 1e-12)


def test_normalisation_and_determinism():
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    rng = np.random.default_rng(5)
    E = 64 * 97 + 13
    rows = crafted_rows(rng, E)
    for res in (2.0, 5.0, 30.0):
        sa = L.texture_cells(res)[2]
        qlog2 = L.exa_texture_quantum_log2(float(rows[:, 0].max()), E)
        a = kernel_counts(L, hipref, dev, rows, FAMILIES, DIRS, res, qlog2)
        m = mrd_of(a, res)
        assert m.min() >= 0.0
        norm = (m * sa[None, :, None]).sum(axis=(1, 2)) / (2 * np.pi)
        assert np.all(np.abs(norm - 1.0) < 1e-12), norm
        b = kernel_counts(L, hipref, dev, rows, FAMILIES, DIRS, res, qlog2)
        assert np.array_equal(a, b)                                           # repeated launches: the same bits
        perm = rng.permutation(E)
        c = kernel_counts(L, hipref, dev, rows[perm], FAMILIES, DIRS, res, qlog2)
        assert np.array_equal(a, c)                                           # any row order: the same bits
        cut = 2345
        d = kernel_counts(L, hipref, dev, rows[:cut], FAMILIES, DIRS, res, qlog2) + kernel_counts(L, hipref, dev, rows[cut:], FAMILIES, DIRS, res, qlog2)
        assert np.array_equal(a, d)                                           # any split of the rows: integer sums
        assert np.array_equal(mrd_of(a, res), mrd_of(c, res))


def test_kernel_refusals():
    import torch

    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    rows = crafted_rows(np.random.default_rng(1), 64)
    ctx = _ctx(L, 64)
    d_rows = dev.up(rows.ravel())
    d_out = torch.zeros(20 * 8100, dtype=torch.int64, device=dev.dev)
    for hkls, dirs, res in (([], [], 5.0), (FAMILIES, DIRS, 7.0), (FAMILIES, DIRS, 1.0), (FAMILIES, [(0, 0, 0)], 5.0), ([(1, 1, 1)] * 17, [], 5.0),
                            ([], DIRS * 2, 5.0)):
        with pytest.raises(RuntimeError, match="exa_texture_weights"):
            L.texture_weights(ctx, hipref.ptr(d_rows), hkls, dirs, res, 0, hipref.ptr(d_out))
    dev.sync()
    ctx.close()


def _props():
    return np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()


def _rows_of(f):
    rows = np.zeros((len(f["ElementVolume"]), NF))
    rows[:, 0] = f["ElementVolume"][:, 0]
    rows[:, 27:31] = f["LatticeOrientation"]
    return rows


def _check_driver(pf, rows, hkls, dirs, res):
    W, allow, amb = weights_numpy(rows, hkls, dirs, res)
    got = np.concatenate([pf["pf"], pf["ipf"]]) * pf["solid_angle"][None, :, None]          # proportional to the weights
    assert_weights_close(got, W, allow, amb)
    if not allow.any():
        ref = mrd_of(W, res)
        m = np.concatenate([pf["pf"], pf["ipf"]])
        assert np.all(np.abs(m - ref) <= 1e-9 * np.abs(ref) + 1e-12)


def test_driver_against_numpy():
    import exaconstit_amd.lib as L
    N = 10
    quats = random_quats(np.random.default_rng(3), N ** 3)
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS)
    p0 = d.pole_figures()
    assert p0["pf"].shape == (3, 18, 72) and p0["ipf"].shape == (1, 18, 72)
    assert np.array_equal(p0["alpha_edges"], 5.0 * np.arange(19)) and np.array_equal(p0["beta_edges"], 5.0 * np.arange(73))
    _check_driver(p0, _rows_of(d.element_fields()), L.TEXTURE_HKL, L.TEXTURE_IPF_DIRS, 5.0)
    for ti in (1, 2):
        assert d.step(ti)
    f = d.element_fields()
    for hkls, dirs, res in ((L.TEXTURE_HKL, L.TEXTURE_IPF_DIRS, 5.0), (FAMILIES, DIRS + [(1, 0, 0)], 10.0), ([(1, 1, 1)], [], 3.0), ([], [(0, 1, 0)], 2.0)):
        pf = d.pole_figures(hkls, dirs, res)
        assert pf["pf"].shape[0] == len(hkls) and pf["ipf"].shape[0] == len(dirs)
        _check_driver(pf, _rows_of(f), hkls, dirs, res)
        again = d.pole_figures(hkls, dirs, res)
        assert np.array_equal(pf["pf"], again["pf"]) and np.array_equal(pf["ipf"], again["ipf"])
    d.close()


def test_driver_refusals():
    import exaconstit_amd.lib as L
    N = 4
    d = L.Driver.synthetic(N, _props(), random_quats(np.random.default_rng(2), N ** 3).ravel(), DTS)
    with pytest.raises(ValueError):
        d.pole_figures(res_deg=7.0)                                           # the grid is refused before the call
    with pytest.raises(RuntimeError, match="texture_ipf_dirs"):
        d.pole_figures(ipf_dirs=[(0, 0, 0)])
    with pytest.raises(RuntimeError, match="texture_hkl"):
        d.pole_figures(hkl=[(0, 0, 0)])
    with pytest.raises(RuntimeError):
        d.pole_figures(hkl=[], ipf_dirs=[])
    d.close()


def test_loopback_ranks():
    """one loopback rank and two: the same bits before the first step (the same rows, integer sums), the edge allowance after two steps"""
    import exaconstit_amd.lib as L
    N = 12
    quats = random_quats(np.random.default_rng(12), N ** 3)
    hkls, dirs = FAMILIES, DIRS

    def run(nranks):
        gid = (C.c_ubyte * 128)()
        assert L.exa_loopback_group_create(nranks, gid) == 0
        res, errors = [None] * nranks, []

        def work(r):
            try:
                d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS, rank=r, nranks=nranks, uid=gid)
                a = d.pole_figures(hkls, dirs, 5.0)
                for ti in (1, 2):
                    assert d.step(ti)
                b = d.pole_figures(hkls, dirs, 5.0)
                res[r] = (a, b, d.element_fields())
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

    one = run(1)[0]
    two = run(2)
    for k in ("pf", "ipf"):
        assert np.array_equal(two[0][0][k], two[1][0][k]) and np.array_equal(two[0][1][k], two[1][1][k])   # every rank: the all-reduced MRD
        assert np.array_equal(one[0][k], two[0][0][k])                                                   # before the first step: bitwise
    # after two steps the two solves differ at round-off: a pole near an edge may move
    W, allow, amb = weights_numpy(_rows_of(one[2]), hkls, dirs, 5.0)
    got = np.concatenate([two[0][1]["pf"], two[0][1]["ipf"]]) * two[0][1]["solid_angle"][None, :, None]
    assert_weights_close(got, W, allow, amb)
    if not allow.any():
        m1 = np.concatenate([one[1]["pf"], one[1]["ipf"]])
        m2 = np.concatenate([two[0][1]["pf"], two[0][1]["ipf"]])
        assert np.all(np.abs(m1 - m2) <= 1e-9 * np.abs(m1) + 1e-12)


def _stage(tmp_path, vis_lines, nsteps=None):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")) and not f.endswith("_stress.txt"):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines) + t[b:]
    assert "nsteps = 40" in t
    if nsteps is not None:
        t = t.replace("nsteps = 40", "nsteps = %d" % nsteps, 1)
    path = os.path.join(str(tmp_path), "voce_pa.toml")
    open(path, "w").write(t)
    return path


def _files(d, fname="texture"):
    return sorted(glob.glob(os.path.join(str(d), fname + "_*.txt")))


def test_driver_files(tmp_path, monkeypatch):
    """voce_pa (10^3 elements) for 5 steps with steps = 2: files at 0, 2, 4 and 5 that parse back to pole_figures(); without the keys none,
    and the avg_* files of the two runs are byte-identical (ordered sums, EXA_DETERMINISTIC=1: the default atomics differ at round-off
    from run to run whatever the options)"""
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir()
    off.mkdir()
    toml = _stage(on, ["texture = true", "steps = 2"], nsteps=5)
    d = L.Driver.from_toml(toml, out_dir=str(on), write_files=True)
    seen = {0: d.pole_figures()}
    for ti in range(1, 6):
        assert d.step(ti)
        seen[ti] = d.pole_figures()
    d.close()
    due = [0, 2, 4, 5]
    assert [os.path.basename(p) for p in _files(on)] == ["texture_%06d.txt" % ti for ti in due]
    for ti in due:
        path = os.path.join(str(on), "texture_%06d.txt" % ti)
        head = open(path).readline().split()
        assert head[:4] == ["#", "texture", "step", str(ti)] and head[6:] == ["res_deg", "5", "n_alpha", "18", "n_beta", "72"]
        got = L.read_texture(path)
        assert got["hkl"] == list(L.TEXTURE_HKL) and got["ipf_dirs"] == [(0.0, 0.0, 1.0)] and got["step"] == ti
        assert (got["time"] == 0.0) == (ti == 0)
        assert np.array_equal(got["pf"], seen[ti]["pf"]) and np.array_equal(got["ipf"], seen[ti]["ipf"])   # 17 significant digits: the same doubles
    assert not np.array_equal(seen[0]["pf"], seen[5]["pf"])                  # the texture has evolved
    toml = _stage(off, ["steps = 2"], nsteps=5)
    d = L.Driver.from_toml(toml, out_dir=str(off), write_files=True)
    for ti in range(1, 6):
        assert d.step(ti)
    d.close()
    assert _files(off) == []
    avg_on = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(on), "avg_*")))
    avg_off = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(off), "avg_*")))
    assert avg_on == avg_off and avg_on
    for f in avg_on:
        assert open(os.path.join(str(on), f), "rb").read() == open(os.path.join(str(off), f), "rb").read(), f


def _mpirun():
    for c in ("mpirun", "/opt/conda/bin/mpirun", "mpiexec"):
        p = shutil.which(c) or (c if os.path.exists(c) else None)
        if p:
            return p
    return None


def test_executable_two_ranks_ipc(tmp_path):
    """`mechanics -opt` on one rank and on two rank processes sharing the device (ipc transport): the same texture files within the edge
    allowance (at most a few poles of one element may cross an edge: the two solves differ at round-off)"""
    import exaconstit_amd.lib as L
    assert os.path.exists(EXE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir()
    d2.mkdir()
    lines = ["texture = true", "steps = 2", 'texture_fname = "tx"', "texture_ipf_dirs = [[0, 0, 1], [1, 0, 0]]"]
    _stage(d1, lines, nsteps=4)
    _stage(d2, lines, nsteps=4)
    r = subprocess.run([EXE, "-opt", "voce_pa.toml"], cwd=str(d1), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    env2 = dict(env, EXA_TRANSPORT="ipc", EXA_MASTER_PORT="29573")
    mpirun = _mpirun()
    if mpirun:
        r = subprocess.run([mpirun, "-np", "2", EXE, "-opt", "voce_pa.toml"], cwd=str(d2), env=env2, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, (r.stdout, r.stderr)
    else:
        ps = [subprocess.Popen([EXE, "-opt", "voce_pa.toml"], cwd=str(d2), env=dict(env2, EXA_RANK=str(k), EXA_NRANKS="2")) for k in range(2)]
        assert all(p.wait(timeout=1200) == 0 for p in ps)
    f1, f2 = _files(d1, "tx"), _files(d2, "tx")
    assert [os.path.basename(p) for p in f1] == ["tx_%06d.txt" % t for t in (0, 2, 4)] == [os.path.basename(p) for p in f2]
    sa = L.texture_cells(5.0)[2]
    for a, b in zip(f1, f2):
        ta, tb = L.read_texture(a), L.read_texture(b)
        assert ta["step"] == tb["step"] and ta["hkl"] == tb["hkl"] and ta["ipf_dirs"] == tb["ipf_dirs"]
        ma = np.concatenate([ta["pf"], ta["ipf"]])
        mb = np.concatenate([tb["pf"], tb["ipf"]])
        if ta["step"] == 0:
            assert np.array_equal(ma, mb)                                     # the initial rows are the same: the same bits
            continue
        fa, fb = ma * sa[None, :, None] / (2 * np.pi), mb * sa[None, :, None] / (2 * np.pi)
        diff = np.abs(fa - fb)
        bad = diff > 1e-9 * fa + 1e-15
        # one pole of one of the 1000 equal elements weighs at most 1 / 1000 of a set; allow two poles to cross an edge per set
        assert bad.sum(axis=(1, 2)).max() <= 4 and (diff[bad] <= 1.0 / 1000 * (1 + 1e-6)).all(), (bad.sum(), diff.max())
