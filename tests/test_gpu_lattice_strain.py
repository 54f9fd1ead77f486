"""Light-up analysis on the GPU: exa_lattice_strains against a numpy restatement of the lattice-strain math (include/exaconstit_hip.h), a pin of
the rotation convention, repeat launches, the driver's Driver.lattice_strains() and its per-step files (Visualizations.light_up_hkl), several
ranks and the executable."""
import ctypes as C
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from test_lattice_strain_host import fiber_axes_numpy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
EXE = os.path.join(ROOT, "exaconstit_amd", "mechanics")
FAMILIES = [(1, 1, 1), (2, 0, 0), (2, 2, 0), (3, 1, 1)]      # the example of calc_lattice_strain.py
NF = 37


def quat_to_mat(q):
    """R(q) of quat_to_mat (ecm_device.hpp) = ExaModel::Quat2RMat, scalar first; maps crystal vectors to sample vectors.  q (.., 4) -> (.., 3, 3)"""
    x0, x1, x2, x3 = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([x0 * x0 + x1 * x1 - x2 * x2 - x3 * x3, 2 * (x1 * x2 - x0 * x3), 2 * (x1 * x3 + x0 * x2)], -1),
                     np.stack([2 * (x1 * x2 + x0 * x3), x0 * x0 - x1 * x1 + x2 * x2 - x3 * x3, 2 * (x2 * x3 - x0 * x1)], -1),
                     np.stack([2 * (x1 * x3 - x0 * x2), 2 * (x2 * x3 + x0 * x1), x0 * x0 - x1 * x1 - x2 * x2 + x3 * x3], -1)], -2)


def quat_taking(d, s):
    """unit quaternion (scalar first) of the smallest rotation with R(q) d = s (unit vectors, d . s > -1)"""
    q = np.concatenate([[1.0 + np.dot(d, s)], np.cross(d, s)])
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    a0, av, b0, bv = a[0], a[1:], b[0], b[1:]
    return np.concatenate([[a0 * b0 - np.dot(av, bv)], a0 * bv + b0 * av + np.cross(av, bv)])


def quat_about(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])


def fibre_quat(rng, c, s, tilt_deg):
    """orientation whose crystal direction d, tilt_deg away from the axis c, lies along s, with a random twist about s"""
    c = np.asarray(c, float) / np.linalg.norm(c)
    perp = np.cross(c, rng.standard_normal(3))
    perp /= np.linalg.norm(perp)
    t = np.radians(tilt_deg)
    d = np.cos(t) * c + np.sin(t) * perp
    return quat_mul(quat_about(s, rng.uniform(0, 2 * np.pi)), quat_taking(d, s))


def random_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1)[:, None]


def lattice_numpy(rows, hkls, s, tol_deg):
    """rows (E, 37) -> strain (H,), volume fraction (H,), membership (H, E)"""
    s = np.asarray(s, float) / np.linalg.norm(s)
    V = rows[:, 0]
    R = quat_to_mat(rows[:, 27:31])
    u = np.einsum("eij,i->ej", R, s)                                  # R^T s
    e = rows[:, 31:37]
    T = np.stack([np.stack([e[:, 0], e[:, 5], e[:, 4]], -1), np.stack([e[:, 5], e[:, 1], e[:, 3]], -1), np.stack([e[:, 4], e[:, 3], e[:, 2]], -1)], -2)
    es = np.einsum("ei,eij,ej->e", u, T, u)
    ct = np.cos(np.radians(tol_deg))
    strain, vf, mem = [], [], []
    for hkl in hkls:
        m = np.abs(u @ fiber_axes_numpy(hkl).T).max(1) > ct
        vin = V[m].sum()
        strain.append((V[m] * es[m]).sum() / vin if vin > 0 else np.nan)
        vf.append(vin / V.sum())
        mem.append(m)
    return np.array(strain), np.array(vf), np.array(mem)


def synthetic_rows(rng, E, s, hkls, per_fibre=3):
    rows = np.zeros((E, NF))
    rows[:, 0] = rng.uniform(0.5, 1.5, E) * 10.0 ** rng.uniform(-3, 0, E)      # spread volumes: a changed membership changes the sums visibly
    rows[:, 27:31] = random_quats(rng, E)
    rows[:, 31:37] = rng.standard_normal((E, 6)) * 1e-3
    rows[:, 1:27] = rng.standard_normal((E, 26))                                # columns the analysis does not read
    k = 0
    for hkl in hkls:
        for _ in range(per_fibre):
            rows[k, 27:31] = fibre_quat(rng, hkl, s, rng.uniform(0.0, 4.0))
            k += 1
    return rows


def _kernel_run(L, hipref, dev, ctx, rows, hkls, s, tol_deg):
    axes = [L.cubic_fiber_axes(*h) for h in hkls]
    off = np.concatenate([[0], np.cumsum([len(a) for a in axes])]).astype(np.int32)
    ax = np.ascontiguousarray(np.concatenate(axes))
    sd = np.asarray(s, float) / np.linalg.norm(s)
    d_rows = dev.up(rows.ravel())
    d_out = dev.zeros(2 * len(hkls) + 1)
    ctx.check(L.exa_lattice_strains(ctx.h, hipref.ptr(d_rows), len(hkls), ax.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int)),
                                    sd.ctypes.data_as(C.POINTER(C.c_double)), float(np.cos(np.radians(tol_deg))), hipref.ptr(d_out), None), "exa_lattice_strains")
    dev.sync()
    return d_out.cpu().numpy()


def _ctx(L, E):
    props = np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()
    return L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)


def _sums_to_strains(out, H):
    vin = out[1:2 * H:2]
    strain = np.where(vin > 0, out[0:2 * H:2] / np.where(vin > 0, vin, 1.0), np.nan)
    return strain, vin / out[2 * H]


@pytest.mark.parametrize("E", [125, 1000])
@pytest.mark.parametrize("s", [(0, 0, 1), (0.3, -0.5, 0.8)])
def test_kernel_against_numpy(E, s):
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    hkls = FAMILIES + [(1, 2, 3)]
    sd = np.asarray(s, float) / np.linalg.norm(s)
    rng = np.random.default_rng(E + int(100 * s[0]))
    rows = synthetic_rows(rng, E, sd, hkls)
    ctx = _ctx(L, E)
    out = _kernel_run(L, hipref, dev, ctx, rows, hkls, s, 5.0)
    strain, vf = _sums_to_strains(out, len(hkls))
    ref_s, ref_f, mem = lattice_numpy(rows, hkls, s, 5.0)
    assert mem.sum(1).min() >= 3                                                # every fibre holds the rows placed in it
    assert abs(out[-1] - rows[:, 0].sum()) <= 1e-13 * rows[:, 0].sum()
    assert np.all(np.abs(vf - ref_f) <= 1e-13 * np.maximum(ref_f, 1e-300)), (vf, ref_f)      # identical in-fibre membership
    assert np.all(np.abs(strain - ref_s) <= 1e-13 * np.abs(ref_s) + 1e-13 * np.abs(rows[:, 31:37]).max()), (strain, ref_s)
    # the raw sums as well
    for j, m in enumerate(mem):
        V = rows[m, 0]
        assert abs(out[2 * j + 1] - V.sum()) <= 1e-13 * V.sum()
    ctx.close()


def test_convention_pin():
    """R(q) maps crystal to sample: a row whose R(q) takes crystal [111] onto sample z, with eps = alpha c c^T, has eps_111 = alpha, f_111 = 1 and
    lies outside the 200 fibre; the same for [100].  A transposed rotation or a vector-first quaternion fails this."""
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    z = np.array([0.0, 0.0, 1.0])
    alpha = 2.5e-3
    for c, inside, outside in (((1, 1, 1), 0, 1), ((1, 0, 0), 1, 0)):
        ch = np.asarray(c, float) / np.linalg.norm(c)
        q = quat_mul(quat_about(z, 0.7), quat_taking(ch, z))                    # R c = z, twisted about z
        assert np.allclose(quat_to_mat(q) @ ch, z, atol=1e-15)
        assert not np.allclose(quat_to_mat(q).T @ ch, z, atol=1e-3)             # the transposed map differs
        rows = np.zeros((1, NF))
        rows[0, 0] = 0.37
        rows[0, 27:31] = q
        T = alpha * np.outer(ch, ch)
        rows[0, 31:37] = [T[0, 0], T[1, 1], T[2, 2], T[1, 2], T[0, 2], T[0, 1]]
        ctx = _ctx(L, 1)
        out = _kernel_run(L, hipref, dev, ctx, rows, [(1, 1, 1), (2, 0, 0)], z, 5.0)
        strain, vf = _sums_to_strains(out, 2)
        assert vf[inside] == 1.0 and abs(strain[inside] - alpha) <= 1e-15, (c, strain, vf)
        assert vf[outside] == 0.0 and np.isnan(strain[outside]), (c, strain, vf)
        ctx.close()


def test_repeat_launches_same_bits():
    import exaconstit_amd.lib as L
    import hipref
    dev = hipref.Dev()
    rng = np.random.default_rng(9)
    E = 70001
    s = np.array([0.0, 0.6, 0.8])
    rows = synthetic_rows(rng, E, s, FAMILIES, per_fibre=50)
    ctx = _ctx(L, E)
    a = _kernel_run(L, hipref, dev, ctx, rows, FAMILIES, s, 5.0)
    b = _kernel_run(L, hipref, dev, ctx, rows, FAMILIES, s, 5.0)
    assert np.array_equal(a, b)
    ref_s, ref_f, _ = lattice_numpy(rows, FAMILIES, s, 5.0)
    strain, vf = _sums_to_strains(a, len(FAMILIES))
    assert np.allclose(vf, ref_f, rtol=1e-12, atol=0) and np.allclose(strain, ref_s, rtol=1e-11, atol=1e-16)
    ctx.close()


def _driver_numpy(f, hkls, s, tol):
    rows = np.zeros((f["ElementVolume"].shape[0], NF))
    rows[:, 0] = f["ElementVolume"][:, 0]
    rows[:, 27:31] = f["LatticeOrientation"]
    rows[:, 31:37] = f["XtalElasticStrain"]
    return lattice_numpy(rows, hkls, s, tol)


def _close(got, ref, tol):
    g, r = got["strain"], ref[0]
    assert np.array_equal(np.isnan(g), np.isnan(r))
    k = ~np.isnan(r)
    assert np.all(np.abs(g[k] - r[k]) <= tol * np.abs(r[k]).max()), (g, r)
    assert np.all(np.abs(got["volume_fraction"] - ref[1]) <= tol), (got["volume_fraction"], ref[1])


def test_driver_against_numpy():
    import exaconstit_amd.lib as L
    N = 12
    E = N ** 3
    rng = np.random.default_rng(21)
    z = np.array([0.0, 0.0, 1.0])
    quats = random_quats(rng, E)
    idx = rng.permutation(E)
    for e in idx[:200]:
        quats[e] = fibre_quat(rng, (1, 0, 0), z, rng.uniform(0.0, 3.0))
    for e in idx[200:400]:
        quats[e] = fibre_quat(rng, (1, 1, 1), z, rng.uniform(0.0, 3.0))
    props = np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()
    C11, C12, C44 = props[3], props[4], props[5]
    assert 3.0 < 2 * C44 / (C11 - C12) < 3.4                                  # Zener ratio of the props
    d = L.Driver.synthetic(N, props, quats.ravel(), np.array([0.005, 0.1, 0.2]))
    hkls = FAMILIES
    for ti in (1, 2, 3):
        assert d.step(ti)
        got = d.lattice_strains(hkls)
        ref = _driver_numpy(d.element_fields(), hkls, z, 5.0)
        _close(got, ref, 1e-12)
        assert got["volume_fraction"][0] > 0.1 and got["volume_fraction"][1] > 0.1
        if ti == 1:                                                             # elastic, z tension: <100> is the compliant direction
            assert got["strain"][1] > got["strain"][0] > 0, got["strain"]
        other = d.lattice_strains([(1, 1, 1)], s_dir=(1, 0, 1), tol_deg=10.0)   # any set of families and directions
        _close(other, _driver_numpy(d.element_fields(), [(1, 1, 1)], (1, 0, 1), 10.0), 1e-12)
    with pytest.raises(RuntimeError):
        d.lattice_strains([(0, 0, 0)])
    with pytest.raises(RuntimeError):
        d.lattice_strains([(1, 1, 1)], tol_deg=0.0)
    d.close()


def _stage(tmp_path, vis_lines, nsteps):
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


LIGHTUP = ["light_up = true", "light_up_hkl = [[1,1,1],[2,0,0],[2,2,0],[3,1,1]]", "light_up_dist_tol_deg = 15.0"]


def _read_rows(path):
    return np.atleast_2d(np.loadtxt(path))


def test_driver_files(tmp_path):
    import exaconstit_amd.lib as L
    toml = _stage(tmp_path, LIGHTUP, nsteps=3)
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=True)
    seen = []
    for ti in (1, 2, 3):
        assert d.step(ti)
        seen.append(d.lattice_strains(FAMILIES, tol_deg=15.0))
    d.close()
    S = _read_rows(os.path.join(str(tmp_path), "lattice_strains.txt"))
    F = _read_rows(os.path.join(str(tmp_path), "lattice_volumes.txt"))
    assert S.shape == (3, 4) and F.shape == (3, 4)
    for i, g in enumerate(seen):
        assert np.array_equal(np.isnan(S[i]), np.isnan(g["strain"]))
        k = ~np.isnan(g["strain"])
        assert np.allclose(S[i][k], g["strain"][k], rtol=1e-5, atol=0)          # append_row prints 6 significant digits
        assert np.allclose(F[i], g["volume_fraction"], rtol=1e-5, atol=0)
    assert np.array_equal(np.isnan(S), F == 0.0)                                 # nan exactly where a fibre is empty
    assert (F > 0).any()

    # light_up without light_up_hkl: no analysis, no files
    t2 = tmp_path / "off"
    t2.mkdir()
    toml = _stage(t2, ["light_up = true"], nsteps=2)
    d = L.Driver.from_toml(toml, out_dir=str(t2), write_files=True)
    assert d.run() == 2
    d.close()
    assert not os.path.exists(str(t2 / "lattice_strains.txt")) and not os.path.exists(str(t2 / "lattice_volumes.txt"))


def test_two_loopback_ranks_match_one(tmp_path):
    import exaconstit_amd.lib as L
    toml = _stage(tmp_path, LIGHTUP, nsteps=3)

    def run(nranks, out):
        os.makedirs(out, exist_ok=True)
        gid = (C.c_ubyte * 128)()
        assert L.exa_loopback_group_create(nranks, gid) == 0
        res, errors = [None] * nranks, []

        def work(r):
            try:
                d = L.Driver.from_toml(toml, out_dir=out, rank=r, nranks=nranks, uid=gid, write_files=True)
                assert d.run() == 3
                res[r] = (d.lattice_strains(FAMILIES, tol_deg=15.0), d.lattice_strains(FAMILIES, s_dir=(1, 1, 0), tol_deg=5.0))
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
    for k in range(2):
        a, b0, b1 = one[k], two[0][k], two[1][k]
        for key in ("strain", "volume_fraction"):
            assert np.array_equal(b0[key], b1[key], equal_nan=True)             # every rank sees the all-reduced values
            assert np.array_equal(np.isnan(a[key]), np.isnan(b0[key]))
            m = ~np.isnan(a[key])
            # the two partitions reduce the PCG dot products in another order, so their converged states agree to the round-off of the solve
            # (a few 1e-12 relative on these strains), not bit for bit
            assert np.all(np.abs(a[key][m] - b0[key][m]) <= 1e-10 * np.maximum(np.abs(a[key][m]), 1e-300)), (key, a[key], b0[key])
    for r in ("r1", "r2"):
        assert _read_rows(str(tmp_path / r / "lattice_strains.txt")).shape == (3, 4)
    assert np.allclose(_read_rows(str(tmp_path / "r1" / "lattice_volumes.txt")), _read_rows(str(tmp_path / "r2" / "lattice_volumes.txt")), rtol=1e-5, atol=0)


def test_executable_writes_lattice_files(tmp_path):
    assert os.path.exists(EXE)
    _stage(tmp_path, LIGHTUP + ['light_up_strain_fname = "ls.txt"', 'light_up_volume_fname = "lv.txt"'], nsteps=3)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE")}
    r = subprocess.run([EXE, "-opt", "voce_pa.toml"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    S = _read_rows(os.path.join(str(tmp_path), "ls.txt"))
    F = _read_rows(os.path.join(str(tmp_path), "lv.txt"))
    assert S.shape == (3, 4) and F.shape == (3, 4)
    assert np.array_equal(np.isnan(S), F == 0.0)
