"""The deterministic two-launch summary the in-situ analyses share (exaconstit_amd/csrc/analysis_device.hpp), at the sizes where it can go
wrong: exa_curvature_summary, exa_fip_summary, exa_lattice_strains (two families) and exa_texture_volume_max on made-up rows through the C ABI.
  E = 1, 63        less than one wave
  E = 20 000       79 partials: the reduce wave's stride-64 loop runs more than once, and the last block is partial
  E = 245 825      = 960 x 256 + 65: the block cap of 960 binds (1024 for the volume maximum: 961 blocks), so the grid-stride loop of the
                   partial launch runs more than once, and the last 64-element block is partial
The per-kernel tests of these entry points (test_gpu_lattice_curvature.py, test_gpu_fatigue.py, test_gpu_lattice_strain.py) stop at 25 blocks.

Tolerances are those of the per-kernel NumPy tests of the same entry points: curvature sums 1e-10 of the value (test_gpu_lattice_curvature.py), fatigue
sums 1e-12 (test_gpu_fatigue.py), lattice volumes 1e-13 and strains 1e-13 of the value plus 1e-13 of the largest strain component
(test_gpu_lattice_strain.py).  They hold at these sizes because every sum here is a tree: a lane adds at most 2 elements, the wave tree 6 levels,
the block 4 waves, the reduce wave at most 15 partials per lane and 6 levels - fewer than 35 roundings of 1.1e-16 on any path, and the sums
compared to a relative bound have terms of one sign (the FIP values are mostly positive: their sum is far from 0).  The reference sums are
math.fsum (exactly rounded), so the bound is spent on the GPU alone.  Maxima and the id of the largest FIP are compared exactly, and every entry
point is called twice on the same data: no atomics, the same bits."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import hipref
from hipref import ptr
from test_gpu_fatigue import summary7
from test_gpu_lattice_strain import lattice_numpy, random_quats

pytestmark = pytest.mark.gpu

REFDATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refdata")
SIZES = [1, 63, 20000, 960 * 256 + 65]
HKLS = [(1, 1, 1), (2, 0, 0)]
S_DIR = (0.3, -0.5, 0.8)
TOL_DEG = 15.0          # about 14 % and 10 % of random orientations lie in the two fibres


def _fsum_dot(a, b):
    return math.fsum((a * b).tolist())


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    """rows, curvature rows, FIP rows and ids of one size, on the host and on the device, with a context of that size; built once per size"""
    import exaconstit_amd.lib as L
    E = request.param
    rng = np.random.default_rng(1000 + E)
    rows = rng.standard_normal((E, 37))
    rows[:, 0] = rng.uniform(0.5, 1.5, E) * 10.0 ** rng.uniform(-3, 0, E)
    rows[:, 27:31] = random_quats(rng, E)
    rows[:, 31:37] = 1e-3 * rng.standard_normal((E, 6))
    curv = rng.standard_normal((E, 16))
    curv[:, 3], curv[:, 4], curv[:, 15] = rng.uniform(0, 10, E), rng.uniform(0, 2, E), 1e12 * rng.uniform(0, 1, E)      # GROD, KAM, GND density >= 0
    fip = rng.standard_normal((E, 6))
    fip[:, 0], fip[:, 2], fip[:, 4] = rng.uniform(-0.1, 1.0, E), rng.uniform(0, 1e-2, E), rng.uniform(0, 0.5, E)         # FIP (may be negative), ShearRange, AccumulatedSlip
    gid = rng.permutation(3 * E)[:E].astype(np.int64)                                                                     # ids in no order, with gaps
    if E >= 2:
        # the largest FIP twice: on an element of the first third and on the last element (the last, partial block), which carries the smaller id
        i1, i2 = E // 3, E - 1
        fip[i1, 0] = fip[i2, 0] = 1.5
        if gid[i2] > gid[i1]:
            gid[[i1, i2]] = gid[[i2, i1]]
    dev = hipref.Dev()
    props = np.loadtxt(os.path.join(REFDATA, "props_cp_voce.txt")).ravel()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    c = dict(L=L, E=E, ctx=ctx, dev=dev, rows=rows, curv=curv, fip=fip, gid=gid,
             d_rows=dev.up(rows.ravel()), d_curv=dev.up(curv.ravel()), d_fip=dev.up(fip.ravel()), d_gid=dev.up(gid))
    yield c
    ctx.close()


def _twice(c, n, call):
    """the entry point twice into fresh buffers: equal bits; returns the first result"""
    outs = []
    for _ in range(2):
        d_out = c["dev"].up(np.full(n, -7.25e300))
        c["ctx"].check(call(ptr(d_out)))
        c["dev"].sync()
        outs.append(d_out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), (outs[0], outs[1])
    return outs[0]


def test_curvature_summary(case):
    c = case
    L, V, cv = c["L"], c["rows"][:, 0], c["curv"]
    got = _twice(c, 7, lambda o: L.exa_curvature_summary(c["ctx"].h, ptr(c["d_rows"]), ptr(c["d_curv"]), o, None))
    ref = np.array([math.fsum(V.tolist()), _fsum_dot(V, cv[:, 3]), _fsum_dot(V, cv[:, 4]), _fsum_dot(V, cv[:, 15])])
    err = np.abs(got[:4] - ref)
    print(f"E={c['E']} curvature sums: {err / ref}")
    assert np.all(err <= 1e-10 * np.abs(ref)), (got, ref)
    assert np.array_equal(got[4:], [cv[:, 3].max(), cv[:, 4].max(), cv[:, 15].max()]), got


def test_fip_summary(case):
    c = case
    L, V, fip, gid = c["L"], c["rows"][:, 0], c["fip"], c["gid"]
    got = _twice(c, 7, lambda o: L.exa_fip_summary(c["ctx"].h, ptr(c["d_rows"]), ptr(c["d_fip"]), ptr(c["d_gid"]), o, None))
    ref7 = summary7(V, fip, gid)
    ref = np.array([math.fsum(V.tolist()), _fsum_dot(V, fip[:, 0]), _fsum_dot(V, fip[:, 4])])
    err = np.abs(got[:3] - ref)
    print(f"E={c['E']} fatigue sums: {err / np.abs(ref)}")
    assert np.all(err <= 1e-12 * np.abs(ref)), (got, ref)
    assert np.array_equal(got[3:6], ref7[3:6]), (got, ref7)
    assert got[6] == ref7[6], (got, ref7)
    if c["E"] >= 2:
        i1, i2 = c["E"] // 3, c["E"] - 1
        assert got[3] == 1.5 and got[6] == float(min(gid[i1], gid[i2])) == float(gid[i2])      # the tie went to the smaller id, met last
        # ... and with the two ids exchanged the smaller one is met first: "the later one wins" and "the earlier one wins" both fail one of the two
        gid2 = gid.copy()
        gid2[[i1, i2]] = gid[[i2, i1]]
        d_gid2 = c["dev"].up(gid2)
        got2 = _twice(c, 7, lambda o: L.exa_fip_summary(c["ctx"].h, ptr(c["d_rows"]), ptr(c["d_fip"]), ptr(d_gid2), o, None))
        assert got2[3] == 1.5 and got2[6] == float(gid2[i1]) == float(min(gid2[i1], gid2[i2])), (got2, gid2[i1], gid2[i2])
        assert np.array_equal(got2[:6], got[:6])


def test_lattice_strains(case):
    c = case
    L, rows, H = c["L"], c["rows"], len(HKLS)
    axes = [L.cubic_fiber_axes(*h) for h in HKLS]
    off = np.concatenate([[0], np.cumsum([len(a) for a in axes])]).astype(np.int32)
    ax = np.ascontiguousarray(np.concatenate(axes))
    sd = np.asarray(S_DIR, float) / np.linalg.norm(S_DIR)
    dp = C.POINTER(C.c_double)
    got = _twice(c, 2 * H + 1, lambda o: L.exa_lattice_strains(c["ctx"].h, ptr(c["d_rows"]), H, ax.ctypes.data_as(dp), off.ctypes.data_as(C.POINTER(C.c_int)),
                                                               sd.ctypes.data_as(dp), float(np.cos(np.radians(TOL_DEG))), o, None))
    ref_s, _, mem = lattice_numpy(rows, HKLS, S_DIR, TOL_DEG)
    vtot = math.fsum(rows[:, 0].tolist())
    assert abs(got[-1] - vtot) <= 1e-13 * vtot, (got[-1], vtot)
    if c["E"] >= 20000:
        assert mem.sum(1).min() >= 1000                                               # both fibres are populated
    for j, m in enumerate(mem):
        vin = math.fsum(rows[m, 0].tolist())
        assert abs(got[2 * j + 1] - vin) <= 1e-13 * vin, (j, got[2 * j + 1], vin)       # identical in-fibre membership
        if vin > 0:
            strain = got[2 * j] / got[2 * j + 1]
            print(f"E={c['E']} fibre {j}: {int(m.sum())} rows, strain error {abs(strain - ref_s[j]):.3e}")
            assert abs(strain - ref_s[j]) <= 1e-13 * abs(ref_s[j]) + 1e-13 * np.abs(rows[:, 31:37]).max(), (j, strain, ref_s[j])
        else:
            assert got[2 * j] == 0.0


def test_texture_volume_max(case):
    c = case
    L = c["L"]
    got = _twice(c, 1, lambda o: L.exa_texture_volume_max(c["ctx"].h, ptr(c["d_rows"]), o, None))
    assert got[0] == c["rows"][:, 0].max(), got
