"""Slip-system activity and the Fatemi-Socie fatigue indicator parameter on the GPU: exa_slip_accumulate / exa_fip_rows /
exa_fip_summary and Driver.slip_activity() against a NumPy restatement of the definitions (float64, vectorised over elements and systems) on
made-up rows, on stepped synthetic RVEs through load reversals, on several loopback ranks, a periodic cell, tetrahedra, and the files and
checkpoints of an options-file run.

Tolerance GPU vs NumPy: per accumulator plane (and per column of the evaluation) |d| <= 1e-12 x the largest magnitude of the plane for the six
calls of the ABI test - a sum of six terms with or without FMA contraction differs by a few ulp per term, three orders below that - and the same
bound times the number of accumulated steps in the driver tests.  The two quadrature layouts share every code path of these entry points (only
the [E][EXA_NFIELDS] rows are read), so the ABI tests run on one."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hipref
import tet_mesh_util as T
from hipref import ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
PLANES_111 = np.array([[1, 1, 1]] * 3 + [[-1, 1, 1]] * 3 + [[-1, -1, 1]] * 3 + [[1, -1, 1]] * 3, float)
DIRS_110 = np.array([[0, 1, -1], [-1, 0, 1], [1, -1, 0], [-1, 0, -1], [0, -1, 1], [1, 1, 0], [0, -1, -1], [1, 0, 1], [-1, 1, 0], [1, 0, -1], [0, 1, 1],
                     [-1, -1, 0]], float)
PLANES = ("SlipAccumulated", "SlipAbsolute", "SlipMin", "SlipMax", "NormalStressMax")
FIPCOLS = ("FIP", "FIPSystem", "ShearRange", "NormalStressMaxFIP", "AccumulatedSlip", "NetSlipMax")
K_FS, SIGMA_Y = 0.5, 0.2
REL = 1e-12
# 16 steps of 5e-4 and 4e-4 strain in turn (ten times the default rate; two sizes, so that a step accumulated with another step's dt shows) with the
# load reversed at steps 5 and 13: plastic from step 3 on, reversed yield in between
DTS16 = np.where(np.arange(16) % 2 == 0, 0.05, 0.04)
VZ = 1.0e-2
TIGHT = dict(newton=(50, 1e-12, 1e-14), krylov=(500, 1e-8, 1e-30))   # tests/test_gpu_lattice_curvature.py: states that agree to round-off between rank counts


def _props(name="props_cp_voce.txt"):
    return np.loadtxt(os.path.join(REFDATA, name)).ravel()


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


# ---- the definitions in NumPy -----------------------------------------------------------------------------------------------------------------

def quat_to_mat(q):
    """(E, 4) -> (E, 3, 3), crystal -> sample (ExaModel::Quat2RMat)"""
    x0, x1, x2, x3 = q.T
    return np.stack([np.stack([x0 * x0 + x1 * x1 - x2 * x2 - x3 * x3, 2 * (x1 * x2 - x0 * x3), 2 * (x1 * x3 + x0 * x2)], -1),
                     np.stack([2 * (x1 * x2 + x0 * x3), x0 * x0 - x1 * x1 + x2 * x2 - x3 * x3, 2 * (x2 * x3 - x0 * x1)], -1),
                     np.stack([2 * (x1 * x3 - x0 * x2), 2 * (x2 * x3 + x0 * x1), x0 * x0 - x1 * x1 - x2 * x2 + x3 * x3], -1)], 1)


def stress_tensor(s6):
    s = np.zeros((len(s6), 3, 3))
    s[:, 0, 0], s[:, 1, 1], s[:, 2, 2] = s6[:, 0], s6[:, 1], s6[:, 2]
    s[:, 1, 2] = s[:, 2, 1] = s6[:, 3]; s[:, 0, 2] = s[:, 2, 0] = s6[:, 4]; s[:, 0, 1] = s[:, 1, 0] = s6[:, 5]
    return s


def normal_stress(rows, planes):
    """sigma_n,a = n_a^T sigma n_a with n_a = R(q) m_a / |m_a|: (E, 12)"""
    m = planes / np.linalg.norm(planes, axis=1, keepdims=True)
    n = np.einsum("eij,aj->eai", quat_to_mat(rows[:, 27:31]), m)
    return np.einsum("eai,eij,eaj->ea", n, stress_tensor(rows[:, 4:10]), n)


class Acc:
    """the 60 accumulators of every element, zero at the start of a run"""

    def __init__(self, E, planes):
        self.planes = planes
        self.g, self.a, self.lo, self.hi, self.nm = (np.zeros((E, 12)) for _ in range(5))

    def step(self, rows, dt, reset=False):
        rate = rows[:, 15:27]
        sn = normal_stress(rows, self.planes)
        self.g = self.g + dt * rate
        self.a = self.a + dt * np.abs(rate)
        if reset:
            self.lo, self.hi, self.nm = self.g.copy(), self.g.copy(), sn
        else:
            self.lo, self.hi, self.nm = np.minimum(self.lo, self.g), np.maximum(self.hi, self.g), np.maximum(self.nm, sn)
        return self

    def planes60(self):
        return np.concatenate([self.g, self.a, self.lo, self.hi, self.nm], 1)          # (E, 60)

    def fip(self, k, sy):
        rng = 0.5 * (self.hi - self.lo)
        f = rng * (1.0 + k * self.nm / sy)
        a = np.argmax(f, axis=1)                                                          # the smallest index that attains the maximum
        e = np.arange(len(f))
        return np.stack([f[e, a], a.astype(float), rng[e, a], self.nm[e, a], self.a.sum(1), np.abs(self.g).max(1)], 1), f


def summary7(V, fip, gid):
    best = fip[:, 0].max()
    return np.array([V.sum(), V @ fip[:, 0], V @ fip[:, 4], best, fip[:, 2].max(), fip[:, 4].max(), float(gid[fip[:, 0] == best].min())])


def _close(got, ref, rel, what):
    """per column / plane: |d| <= rel x its largest magnitude"""
    worst = 0.0
    for c in range(ref.shape[1] if len(ref) else 0):
        scale = np.abs(ref[:, c]).max()
        err = np.abs(got[:, c] - ref[:, c]).max()
        worst = max(worst, err / max(scale, 1e-300))
        assert err <= rel * scale, (what, c, err, scale)
    print(f"{what}: worst |d| / scale = {worst:.3e} (bound {rel:.1e})")


def _close_fip(got, ref, f_all, rel, what):
    """the evaluation rows; the system (and with it the two columns that follow it) is compared where the two largest FIP_a differ by more than the bound"""
    top = np.sort(f_all, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 10 * rel * np.abs(f_all).max()
    assert np.array_equal(got[clear, 1], ref[clear, 1]), what
    cols = [0, 4, 5]
    _close(got[:, cols], ref[:, cols], rel, what + " FIP, AccumulatedSlip, NetSlipMax")
    _close(got[clear][:, [2, 3]], ref[clear][:, [2, 3]], rel, what + " ShearRange, NormalStressMax of the FIP system")


# ---- 1, 6, 9: the ABI ---------------------------------------------------------------------------------------------------------------------------

SENTINEL = -7.25e300


def made_up_rows(E, seed):
    """unit quaternions, stresses ~1e2, rates of both signs ~1e-3 with some exactly 0, volumes ~1"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((E, 37))
    r[:, 0] = rng.uniform(0.5, 1.5, E)
    r[:, 4:10] = 100.0 * rng.standard_normal((E, 6))
    r[:, 15:27] = 1e-3 * rng.standard_normal((E, 12)) * (rng.uniform(size=(E, 12)) > 0.2)
    r[:, 27:31] = _unit(rng.standard_normal((E, 4)))
    return r


def run_abi_sequence(L, ctx, rows_seq, dts, resets, planes, gid, k=K_FS, sy=SIGMA_Y):
    """one exa_slip_accumulate per entry of rows_seq on accumulators that start from zero inside a sentinel-filled buffer, then the evaluation
    and its summary: planar (60, E), padding (60, E_pad - E), fip rows (E, 6), summary (7,)"""
    dev = hipref.Dev()
    E = rows_seq[0].shape[0]
    n = L.slip_activity_sizes(E)
    Ep = n // 60
    assert Ep % 64 == 0 and 0 <= Ep - E < 64
    host = np.full((60, Ep), SENTINEL)
    host[:, :E] = 0.0
    d_acc = dev.up(host.ravel())
    nrm = np.ascontiguousarray(planes, dtype=np.float64)          # unnormalised: the entry point normalises
    for rows, dt, rs in zip(rows_seq, dts, resets):
        d_rows = dev.up(rows.ravel())
        ctx.check(L.exa_slip_accumulate(ctx.h, ptr(d_rows), nrm.ctypes.data_as(C.POINTER(C.c_double)), float(dt), int(rs), ptr(d_acc), None), "exa_slip_accumulate")
        dev.sync()
    d_fip, d_sum = dev.up(np.full(6 * E, SENTINEL)), dev.zeros(7)
    d_gid = dev.up(np.ascontiguousarray(gid, dtype=np.int64))
    d_rows = dev.up(rows_seq[-1].ravel())
    ctx.check(L.exa_fip_rows(ctx.h, ptr(d_acc), k, sy, ptr(d_fip), None), "exa_fip_rows")
    ctx.check(L.exa_fip_summary(ctx.h, ptr(d_rows), ptr(d_fip), ptr(d_gid), ptr(d_sum), None), "exa_fip_summary")
    dev.sync()
    a = d_acc.cpu().numpy().reshape(60, Ep)
    return a[:, :E].copy(), a[:, E:].copy(), d_fip.cpu().numpy().reshape(E, 6), d_sum.cpu().numpy()


def check_abi(L, ctx, rows_seq, dts, resets, planes, what):
    E = rows_seq[0].shape[0]
    gid = np.random.default_rng(4).permutation(3 * E)[:E].astype(np.int64)          # ids in no order, with gaps
    ref = Acc(E, planes)
    for rows, dt, rs in zip(rows_seq, dts, resets):
        ref.step(rows, dt, rs)
    rfip, f_all = ref.fip(K_FS, SIGMA_Y)
    got, pad, gfip, gsum = run_abi_sequence(L, ctx, rows_seq, dts, resets, planes, gid)
    again = run_abi_sequence(L, ctx, rows_seq, dts, resets, planes, gid)
    assert np.array_equal(got, again[0]) and np.array_equal(gfip, again[2]) and np.array_equal(gsum, again[3])   # no atomics: the same bits
    assert np.all(pad == SENTINEL), "lanes beyond E were written"
    for j, nm in enumerate(PLANES):
        _close(got[12 * j:12 * j + 12].T, ref.planes60()[:, 12 * j:12 * j + 12], REL, f"{what} {nm}")
    _close_fip(gfip, rfip, f_all, REL, what)
    rsum = summary7(rows_seq[-1][:, 0], rfip, gid)
    err = np.abs(gsum[:6] - rsum[:6])
    print(f"{what} summary: {err / np.abs(rsum[:6])}")
    assert np.all(err <= REL * np.abs(rsum[:6])), (gsum, rsum)
    assert gsum[6] == rsum[6]
    return ref, got, gfip


@pytest.mark.parametrize("E", [125, 64])
@pytest.mark.parametrize("xtal", ["fcc", "bcc"])
def test_kernels_against_numpy(E, xtal):
    """E = 125: one full block and one of 61 lanes; six calls with different dt, the window reset fused into the third"""
    import exaconstit_amd.lib as L
    planes = PLANES_111 if xtal == "fcc" else DIRS_110
    model = L.EXA_FCC_VOCE if xtal == "fcc" else L.EXA_BCC_VOCE
    assert np.abs(L.slip_plane_normals(model) - planes / np.linalg.norm(planes, axis=1, keepdims=True)).max() <= 2e-16
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, 1, E)
    rows_seq = [made_up_rows(E, 100 + i) for i in range(6)]
    dts = [0.1, 0.25, 0.05, 0.4, 0.3, 0.15]
    resets = [0, 0, 1, 0, 0, 0]
    ref, got, gfip = check_abi(L, ctx, rows_seq, dts, resets, planes, f"E={E} {xtal}")
    # the reset did something: without it the window is wider on most entries
    no = Acc(E, planes)
    for rows, dt in zip(rows_seq, dts):
        no.step(rows, dt)
    assert np.mean((no.hi - no.lo) > (ref.hi - ref.lo)) > 0.5
    # dt = 0 with reset: the reset alone, Gamma and A keep their bits
    one = run_abi_sequence(L, ctx, rows_seq[:2], dts[:2], [0, 0], planes, np.arange(E))
    two = run_abi_sequence(L, ctx, rows_seq[:2] + [rows_seq[2]], dts[:2] + [0.0], [0, 0, 1], planes, np.arange(E))
    assert np.array_equal(one[0][:24], two[0][:24])
    assert np.array_equal(two[0][24:36], two[0][:12]) and np.array_equal(two[0][36:48], two[0][:12])
    _close(two[0][48:60].T, normal_stress(rows_seq[2], planes), REL, "reset N_max")
    # refusals
    d = hipref.Dev()
    buf = d.zeros(L.slip_activity_sizes(E)); r = d.up(rows_seq[0].ravel()); o = d.zeros(6 * E)
    nrm = np.ascontiguousarray(planes)
    dp = C.POINTER(C.c_double)
    assert L.exa_slip_accumulate(ctx.h, ptr(r), nrm.ctypes.data_as(dp), -0.1, 0, ptr(buf), None) == L.EXA_ERR_ARG
    assert L.exa_slip_accumulate(ctx.h, ptr(r), np.zeros((12, 3)).ctypes.data_as(dp), 0.1, 0, ptr(buf), None) == L.EXA_ERR_ARG
    assert L.exa_fip_rows(ctx.h, ptr(buf), 0.5, 0.0, ptr(o), None) == L.EXA_ERR_ARG
    assert L.exa_fip_rows(ctx.h, ptr(buf), -0.5, 1.0, ptr(o), None) == L.EXA_ERR_ARG
    ctx.close()


@pytest.mark.parametrize("p", [1, 2])
def test_tetrahedra_rows_abi(tmp_path, p):
    """rows of one exa_element_fields call on a tetrahedron context at p = 1 and 2 (162 elements): the kernels read rows only"""
    import exaconstit_amd.lib as L
    from test_gpu_tetrahedra import _mesh_arrays
    dev = hipref.Dev()
    path = T.write_mfem(str(tmp_path / "k3.mesh"), T.kuhn_cube(3, perturb=0.3, shuffle=True, seed=5))
    E, NN, n, conn, X = _mesh_arrays(L, path, p)
    ctx = L.Context(L.EXA_FCC_VOCE, _props(), 298.0, p, E, geometry=L.EXA_GEOM_TET)
    Q = ctx.Q; P = E * Q
    xe = hipref.l_to_e({"E": E, "n": n, "NN": NN, "conn": conn}, X)
    d_xe, d_J = dev.up(xe), dev.zeros(9 * P)
    ctx.check(L.exa_jacobians(ctx.h, ptr(d_xe), ptr(d_J), None))
    rows_seq = []
    for i in range(3):
        rng = np.random.default_rng(40 + 10 * p + i)
        S = 100.0 * rng.standard_normal((P, 6))
        SV = rng.standard_normal((P, 28))
        SV[:, 14:26] *= 1e-3
        SV[:, 26] = rng.uniform(0.95, 1.05, P)
        d_out = dev.zeros(37 * E)
        d_S, d_SV = dev.up(S.ravel()), dev.up(SV.ravel())
        ctx.check(L.exa_element_fields(ctx.h, ptr(d_J), ptr(d_S), ptr(d_SV), ptr(d_xe), ptr(d_out), None), "exa_element_fields")
        dev.sync()
        rows_seq.append(d_out.cpu().numpy().reshape(E, 37))
    assert np.all(rows_seq[0][:, 0] > 0) and np.abs(np.linalg.norm(rows_seq[0][:, 27:31], axis=1) - 1).max() < 1e-14
    check_abi(L, ctx, rows_seq, [0.2, 0.1, 0.3], [0, 1, 0], PLANES_111, f"tet p={p}")
    ctx.close()


def test_no_scratch():
    import exaconstit_amd.lib as L
    assert L.fatigue_scratch_bytes() == [0, 0, 0, 0, 0]


# ---- 2, 3: the driver ---------------------------------------------------------------------------------------------------------------------------

def eight_grains(N):
    i = np.arange(N ** 3)
    x, y, z = i % N, (i // N) % N, i // (N * N)
    return (1 + (x >= N // 2) + 2 * (y >= N // 2) + 4 * (z >= N // 2)).astype(np.int32)


def _field_rows(f):
    import exaconstit_amd.lib as L
    r = np.zeros((len(f["GlobalElementId"]), 37))
    for k, (c0, n) in L.ELEMENT_FIELDS.items():
        r[:, c0:c0 + n] = f[k]
    return r


def _got60(sa):
    return np.concatenate([sa[k] for k in PLANES], 1)


def _gotfip(sa):
    return np.stack([sa[k] for k in FIPCOLS], 1)


def grains_numpy(V, fip0, attr):
    ids = np.unique(attr)
    return ids, np.array([V[attr == g].sum() for g in ids]), np.array([V[attr == g] @ fip0[attr == g] / V[attr == g].sum() for g in ids]), \
        np.array([fip0[attr == g].max() for g in ids])


def compare_driver(sa, ref, rows, nsteps, window_start, what):
    rel = REL * nsteps
    for j, nm in enumerate(PLANES):
        _close(sa[nm], ref.planes60()[:, 12 * j:12 * j + 12], rel, f"{what} {nm}")
    rfip, f_all = ref.fip(K_FS, SIGMA_Y)
    _close_fip(_gotfip(sa), rfip, f_all, rel, what)
    V, gid = rows[:, 0], sa["GlobalElementId"]
    r7 = summary7(V, rfip, gid)
    s = sa["summary"]
    want = dict(volume=r7[0], FIP_mean=r7[1] / r7[0], FIP_max=r7[3], AccumulatedSlip_mean=r7[2] / r7[0], AccumulatedSlip_max=r7[5], ShearRange_max=r7[4])
    for k, v in want.items():
        assert abs(s[k] - v) <= rel * abs(v), (what, k, s[k], v)
    assert s["FIP_max_element"] == int(r7[6]) and s["window_start_step"] == window_start, (what, s, r7[6])
    ids, vol, mean, mx = grains_numpy(V, rfip[:, 0], sa["attribute"])
    g = sa["grains"]
    assert np.array_equal(g["grain_id"], ids)
    for got, want_ in ((g["volume"], vol), (g["FIP_mean"], mean), (g["FIP_max"], mx)):
        assert np.all(np.abs(got - want_) <= rel * np.abs(want_).max()), what


def run_driver_against_numpy(d, planes, nsteps, dts, check_at, reset_after=None, plastic_by=None):
    """steps a driver, advancing the NumPy accumulators from element_fields() after every step; returns the evaluations by step"""
    f0 = d.element_fields()
    ref = Acc(len(f0["GlobalElementId"]), planes).step(_field_rows(f0), 0.0, True)      # before step 1: Gamma = 0 and the rows of the initial state
    out, pending, window, prev = {}, False, 0, None
    for ti in range(1, nsteps + 1):
        assert d.step(ti), f"Newton failed at step {ti}"
        rows = _field_rows(d.element_fields())
        ref.step(rows, dts[ti - 1], pending)
        if pending:
            window, pending = ti, False
        if plastic_by == ti:
            assert np.abs(rows[:, 15:27]).max() > 0.0                                       # the case cannot pass on zeros
        sa = d.slip_activity(k=K_FS, sigma_y=SIGMA_Y)
        assert np.all(sa["AccumulatedSlip"] >= (prev if prev is not None else 0.0))         # never decreases
        prev = sa["AccumulatedSlip"]
        # sum_a A_a >= max_a |Gamma_a|.  In exact arithmetic A_a >= |Gamma_a| term by term; Gamma_a and A_a are two separately rounded sums of up to 16
        # terms (1e-14 covers 16 x 2^-53 several times), and with one active system of one sign the two sides are equal up to that rounding
        assert np.all(sa["SlipAbsolute"].sum(1) >= np.abs(sa["SlipAccumulated"]).max(1) * (1 - 1e-14))
        if ti in check_at:
            compare_driver(sa, ref, rows, ti, window, f"step {ti}")
        out[ti] = sa
        if reset_after == ti:
            d.reset_fatigue_window(); pending = True
    return out, ref


@pytest.mark.parametrize("bcc", [False, True])
def test_driver_against_numpy(bcc):
    """5^3 elements in 8 grains, Voce, 16 steps through two load reversals; reset_fatigue_window() after step 8 takes effect with step 9"""
    import exaconstit_amd.lib as L
    N = 5
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    nsteps = 6 if bcc else 16
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:nsteps], vz=VZ, bcc=bcc, reversals=(5,) if bcc else (5, 13))
    with pytest.raises(RuntimeError, match="not on"):
        d.slip_activity(sigma_y=SIGMA_Y)
    d.set_grains(eight_grains(N), _unit(np.random.default_rng(11).standard_normal((8, 4))))
    d.enable_slip_activity()
    out, ref = run_driver_against_numpy(d, DIRS_110 if bcc else PLANES_111, nsteps, DTS16, check_at=(4, 6) if bcc else (4, 9, 12, 16),
                                        reset_after=None if bcc else 8, plastic_by=3)
    if not bcc:
        s9, s8, s16 = out[9], out[8], out[16]
        assert s8["summary"]["window_start_step"] == 0 and s9["summary"]["window_start_step"] == 9
        assert np.array_equal(s9["SlipMin"], s9["SlipAccumulated"]) and np.array_equal(s9["SlipMax"], s9["SlipAccumulated"]) and np.all(s9["ShearRange"] == 0.0)
        assert np.any(s16["ShearRange"] < s16["NetSlipMax"])                                # the window forgets the slip before the reset
        assert s16["ShearRange"].max() > 0.0 and s16["FIP"].max() > 0.0
        assert np.any(s16["SlipAbsolute"] > 1.5 * np.abs(s16["SlipAccumulated"]) + 1e-6)          # slip that reversed on its own system
    with pytest.raises(RuntimeError, match="sigma_y"):
        d.slip_activity(sigma_y=0.0)
    d.close()
    if not bcc:
        e = _stepped_driver(L)
        with pytest.raises(RuntimeError, match="before the first step"):
            e.enable_slip_activity()
        e.close()


def _stepped_driver(L):
    d = L.Driver.synthetic(2, _props(), _unit(np.random.default_rng(1).standard_normal((8, 4))).ravel(), np.array([0.005, 0.1]))
    assert d.step(1)
    return d


def _quat_of(R):
    """unit quaternion of a proper rotation matrix, the inverse of quat_to_mat (from the largest of the four components)"""
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1]]]) / 3.0
    w, v = np.linalg.eigh(K)
    return v[:, np.argmax(w)]


def _compatible_single_slip(a):
    """orientation in which slip on system a alone satisfies the face conditions: the sample axes are the principal axes of sym(s (x) m),
    z = (s + m) / sqrt 2 (Schmid factor 1/2), x = (s - m) / sqrt 2, y = m x s, so that gamma s (x) m plus a uniform lattice spin is the diagonal
    velocity gradient diag(-gamma/2, 0, gamma/2) - planes x = 0, y = 0, z = 0 stay planes, the stress stays uniaxial and the field uniform"""
    sd, m = DIRS_110[a] / np.sqrt(2.0), PLANES_111[a] / np.sqrt(3.0)
    R = np.stack([(sd - m) / np.sqrt(2.0), np.cross(m, sd), (sd + m) / np.sqrt(2.0)])       # rows: the sample axes in crystal components
    return _quat_of(R), R


@pytest.mark.parametrize("case", ["generic", "single_slip"])
def test_single_crystal_signs(case):
    """one grain, 4^3, pulled along z: every active system slips in the sense of its resolved shear stress s^T sigma m (sample frame).  In a generic
    orientation the face conditions (planes x = 0, y = 0, z = 0 stay planes) force several systems on every element and the field is not uniform, so
    the agreement on the FIP system is checked in the orientation in which one system alone is compatible with them (_compatible_single_slip:
    Schmid factor 0.5 against 0.469 for the next, a rate ratio of 0.04 at the power-law exponent 50)"""
    import exaconstit_amd.lib as L
    N = 4
    SYS = 3
    if case == "generic":
        q = _unit(np.array([[0.9, 0.1, -0.3, 0.25]]))
    else:
        q1, R1 = _compatible_single_slip(SYS)
        q = q1[None, :]
        assert np.abs(quat_to_mat(q)[0] - R1).max() < 1e-14 and abs(np.linalg.det(R1) - 1.0) < 1e-15
    quats = np.repeat(q, N ** 3, axis=0)
    d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:4], vz=VZ)
    d.set_grains(np.ones(N ** 3, np.int32), q)
    d.enable_slip_activity()
    for ti in range(1, 5):
        assert d.step(ti)
    f = d.element_fields()
    rows = _field_rows(f)
    R = quat_to_mat(rows[:, 27:31])
    s = np.einsum("eij,aj->eai", R, DIRS_110 / np.linalg.norm(DIRS_110, axis=1, keepdims=True))
    m = np.einsum("eij,aj->eai", R, PLANES_111 / np.linalg.norm(PLANES_111, axis=1, keepdims=True))
    tau = np.einsum("eai,eij,eaj->ea", s, stress_tensor(rows[:, 4:10]), m)
    g = rows[:, 15:27]
    active = np.abs(g) > 1e-6 * np.abs(g).max()
    assert np.all(active.sum(1) >= 1) and np.array_equal(np.sign(g[active]), np.sign(tau[active]))
    sa = d.slip_activity(k=K_FS, sigma_y=SIGMA_Y)
    d.close()
    print(case, "active systems per element:", sorted(set(active.sum(1).tolist())), "FIP systems:", sorted(set(sa["FIPSystem"].tolist())))
    if case == "single_slip":
        gid = sa["GlobalElementId"]
        z = gid // (N * N)
        inner = (z >= 1) & (z <= N - 2) & (gid % N >= 1) & ((gid // N) % N >= 1)          # away from the faces x = 0, y = 0, z = 0 and z = 1 that carry conditions
        assert inner.sum() == 18 and len(set(sa["FIPSystem"][inner].tolist())) == 1, sa["FIPSystem"][inner]
        assert int(sa["FIPSystem"][inner][0]) == SYS
        assert np.all(np.argmax(np.abs(tau[inner]), axis=1) == SYS)                          # ... and it is the system of the largest resolved shear stress


def test_commit_paths_give_the_same_bits(monkeypatch):
    """step(ti) against step(ti, commit=False) + commit_step(): one accumulation per committed step on either path"""
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    N = 4
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    res = []
    for split in (False, True):
        d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:6], vz=VZ, reversals=(4,))
        d.enable_slip_activity()
        for ti in range(1, 7):
            if split:
                assert d.step(ti, commit=False)
                d.commit_step()
            else:
                assert d.step(ti)
            if ti == 3:
                d.reset_fatigue_window()
        res.append(d.slip_activity(k=K_FS, sigma_y=SIGMA_Y))
        d.close()
    a, b = res
    assert a["SlipAbsolute"].max() > 0.0 and a["summary"]["window_start_step"] == 4
    for k in a:
        assert (a[k] == b[k]) if k == "summary" else all(np.array_equal(a[k][j], b[k][j]) for j in a[k]) if k == "grains" else np.array_equal(a[k], b[k]), k


# ---- 4: ranks ---------------------------------------------------------------------------------------------------------------------------------

def _run_ranks(L, N, nranks):
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    quats = _unit(np.random.default_rng(5).standard_normal((N ** 3, 4)))
    res, errors = [None] * nranks, []

    def work(r):
        try:
            d = L.Driver.synthetic(N, _props(), quats.ravel(), DTS16[:6], vz=VZ, rank=r, nranks=nranks, uid=gid, reversals=(4,), **TIGHT)
            d.set_grains(eight_grains(N), _unit(np.random.default_rng(11).standard_normal((8, 4))))
            d.enable_slip_activity()
            for ti in range(1, 7):
                assert d.step(ti)
                if ti == 2:
                    d.reset_fatigue_window()
            res[r] = d.slip_activity(k=K_FS, sigma_y=SIGMA_Y)
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


@pytest.fixture(scope="module")
def one_rank_6():
    import exaconstit_amd.lib as L
    return _run_ranks(L, 6, 1)[0]


@pytest.mark.parametrize("nranks", [2, 8])
def test_loopback_ranks_match_one(one_rank_6, nranks):
    """6^3 on 2 and 8 loopback ranks against one rank, rows matched by GlobalElementId: 1e-9 of the column maximum, the suite's bound for runs
    that differ at round-off"""
    import exaconstit_amd.lib as L
    one = one_rank_6
    many = _run_ranks(L, 6, nranks)
    gids = np.concatenate([r["GlobalElementId"] for r in many])
    assert np.array_equal(np.sort(gids), np.arange(216))
    o1, om = np.argsort(one["GlobalElementId"]), np.argsort(gids)
    rel = 1e-9
    _close(np.concatenate([_got60(r) for r in many])[om], _got60(one)[o1], rel, f"{nranks} ranks planes")
    a, b = _gotfip(one)[o1], np.concatenate([_gotfip(r) for r in many])[om]
    # all six columns; the system and the two columns that belong to it where the two largest FIP_a of the one-rank run are further apart than the bound
    f_all = 0.5 * (one["SlipMax"] - one["SlipMin"])[o1] * (1.0 + K_FS * one["NormalStressMax"][o1] / SIGMA_Y)
    _close_fip(b, a, f_all, rel, f"{nranks} ranks")
    for r in many:
        assert r["summary"] == many[0]["summary"]                                         # every rank sees the combined values
        assert all(np.array_equal(r["grains"][k], many[0]["grains"][k]) for k in r["grains"])
    s1, sm = one["summary"], many[0]["summary"]
    for k in ("volume", "FIP_mean", "FIP_max", "AccumulatedSlip_mean", "AccumulatedSlip_max", "ShearRange_max"):
        assert abs(sm[k] - s1[k]) <= rel * abs(s1[k]), (k, sm[k], s1[k])
    assert sm["window_start_step"] == s1["window_start_step"] == 3
    top = np.sort(a[:, 0])
    if top[-1] - top[-2] > rel * top[-1]:
        assert sm["FIP_max_element"] == s1["FIP_max_element"]
    g1, gm = one["grains"], many[0]["grains"]
    assert np.array_equal(g1["grain_id"], gm["grain_id"]) and len(g1["grain_id"]) == 8
    for k in ("volume", "FIP_mean", "FIP_max"):
        assert np.all(np.abs(gm[k] - g1[k]) <= rel * np.abs(g1[k]).max()), k


# ---- 5: periodic cell ---------------------------------------------------------------------------------------------------------------------------

def test_periodic_cell(tmp_path):
    """4^3 periodic cell whose macroscopic velocity gradient is reversed after step 4 (4 + 4 steps), against NumPy as above"""
    import exaconstit_amd.lib as L
    from test_gpu_periodic import _toml, LMAC, DTS
    N = 4
    toml = _toml(tmp_path, "fat", eight_grains(N), N=N, vgrad=(LMAC, -LMAC), update_steps=(1, 5))
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False)
    d.enable_slip_activity()
    out, _ = run_driver_against_numpy(d, PLANES_111, 8, DTS, check_at=(4, 8))
    assert out[8]["SlipAbsolute"].max() > 0.0
    d.close()


# ---- 7, 8: options-file runs ------------------------------------------------------------------------------------------------------------------

def _cyclic_toml(tmp_path, tag, vis_lines, extra=""):
    """voce_full_cyclic.toml on 5^3 elements, 16 steps, the load reversed at steps 5 and 13"""
    txt = open(os.path.join(REFDATA, "voce_full_cyclic.toml")).read()
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt"):
        txt = txt.replace('"%s"' % fl, '"%s"' % os.path.join(REFDATA, fl))
    a, b = txt.index("[BCs]"), txt.index("[Model]")
    vals = ", ".join("[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, %s]" % v for v in ("0.001", "-0.001", "0.001"))
    txt = txt[:a] + ("[BCs]\n    changing_ess_bcs = true\n    update_steps = [1, 5, 13]\n    essential_ids = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]\n"
                     "    essential_comps = [[3, 1, 2, 3], [3, 1, 2, 3], [3, 1, 2, 3]]\n    essential_vals = [%s]\n" % vals) + txt[b:]
    a, b = txt.index("[Visualizations]"), txt.index("[Solvers]")
    txt = txt[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines + ['avg_stress_fname = "avg_stress.txt"']) + txt[b:]
    for x, y in (("ref_ser = 1", "ref_ser = 0"), ("t_final = 7.0", "t_final = 1.6")):
        assert x in txt
        txt = txt.replace(x, y, 1)
    path = os.path.join(str(tmp_path), tag + ".toml")
    open(path, "w").write(txt + extra)
    return path


FAT_ON = ["fatigue = true", "fatigue_sigma_y = %r" % SIGMA_Y, "fatigue_cycle_steps = 8"]
NEW_ARRAYS = ("FIP", "ShearRange", "AccumulatedSlip", "SlipAccumulated")


def test_options_file_run(tmp_path, monkeypatch):
    import exaconstit_amd.lib as L
    from test_gpu_lattice_curvature import _cell_array_names
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    on, off, tw = tmp_path / "on", tmp_path / "off", tmp_path / "twin"
    for p in (on, off, tw):
        p.mkdir()
    d = L.Driver.from_toml(_cyclic_toml(on, "on", FAT_ON + ["paraview = true", "steps = 8"]), out_dir=str(on))
    assert d.run() == 16
    d.close()
    t = L.read_fatigue(str(on / "fatigue.txt"))
    assert np.array_equal(t["step"], [8, 16]) and np.array_equal(t["window_start_step"], [0, 9])
    # a Python-driven twin: the same accumulation, the reset asked for after the evaluation of step 8
    e = L.Driver.from_toml(_cyclic_toml(tw, "twin", FAT_ON[:2]), out_dir=str(tw), write_files=False)
    evals = {}
    for ti in range(1, 17):
        assert e.step(ti)
        if ti in (8, 16):
            evals[ti] = e.slip_activity(k=0.5, sigma_y=SIGMA_Y)
        if ti == 8:
            e.reset_fatigue_window()
    e.close()
    for i, ti in enumerate((8, 16)):
        s = evals[ti]["summary"]
        for k in ("FIP_mean", "FIP_max", "FIP_max_element", "AccumulatedSlip_mean", "AccumulatedSlip_max", "ShearRange_max", "window_start_step"):
            assert t[k][i] == s[k], (ti, k, t[k][i], s[k])                                    # 17 significant digits: the same doubles
    for ti in (8, 16):
        g = L.read_fatigue_grains(str(on / ("fatigue_grains_%06d.txt" % ti)))
        for k in g:
            assert np.array_equal(g[k], evals[ti]["grains"][k]), (ti, k)
    names = _cell_array_names(str(on / "results" / "exaconstit"), 16)
    assert all(k in names for k in NEW_ARRAYS) and names["SlipAccumulated"] == "12" and names["FIP"] is None
    assert all(k in _cell_array_names(str(on / "results" / "exaconstit"), 0) for k in NEW_ARRAYS)
    from test_gpu_element_fields import _read_cycle
    c16 = _read_cycle(str(on / "results" / "exaconstit"), 16)
    assert np.array_equal(np.asarray(c16["GlobalElementId"]).ravel(), evals[16]["GlobalElementId"])
    assert np.array_equal(np.asarray(c16["FIP"]).ravel(), evals[16]["FIP"]) and np.array_equal(np.asarray(c16["SlipAccumulated"]).reshape(-1, 12), evals[16]["SlipAccumulated"])
    # the key off: no array, no file
    d = L.Driver.from_toml(_cyclic_toml(off, "off", ["fatigue = false", "paraview = true", "steps = 8"]), out_dir=str(off))
    assert d.run() == 16
    d.close()
    assert not any(k in _cell_array_names(str(off / "results" / "exaconstit"), 16) for k in NEW_ARRAYS)
    assert not [f for f in os.listdir(str(off)) if f.startswith("fatigue")]


def test_auto_time_stepping_accumulates_the_solved_dt(tmp_path):
    """[Time.Auto]: the step is accumulated with the dt it was solved with, not with the proposal for the next step that the controller has formed
    by the time the step is committed.  The dts are restated here from the controller's rule (dt_next = dt x NR.iter x dt_scale / Newton iterations,
    capped by the time left) so that they are exact doubles, and checked against auto_dt_out.txt (12 digits)"""
    import exaconstit_amd.lib as L
    t_final, dt_min, scale, nr_iter = 3.0, 0.01, 0.333333, 25
    auto = "[Time]\n    [Time.Auto]\n        dt_start = 0.1\n        dt_min = %r\n        dt_scale = %r\n        t_final = %r\n" % (dt_min, scale, t_final)
    toml = _cyclic_toml(tmp_path, "auto", FAT_ON[:2])
    txt = open(toml).read()
    assert txt.count("[Time]\n") == 1
    a, b = txt.index("[BCs]"), txt.index("[Model]")                                        # Time.Auto takes no changing boundary conditions: one load direction
    txt = txt[:a] + ("[BCs]\n    essential_ids = [1, 2, 3, 4]\n    essential_comps = [3, 1, 2, 3]\n"
                     "    essential_vals = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.001]\n") + txt[b:]
    open(toml, "w").write(txt.replace("[Time]\n", auto, 1))
    d = L.Driver.from_toml(toml, out_dir=str(tmp_path))
    f0 = d.element_fields()
    ref = Acc(len(f0["GlobalElementId"]), PLANES_111).step(_field_rows(f0), 0.0, True)
    dt, time, used = 0.1, 0.0, []
    for ti in range(1, 40):
        dt_real = min(dt, t_final - time)
        time += dt_real
        assert d.step(ti), f"Newton failed at step {ti}"
        it = int(d.stats()[0][-1])
        written = np.loadtxt(str(tmp_path / "auto_dt_out.txt"), ndmin=1)
        assert len(written) == ti
        for _ in range(3):                                                                     # up to two cut-backs by dt_scale when Newton failed at the proposal
            if abs(written[-1] - dt_real) <= 1e-11 * dt_real:
                break
            time -= dt_real
            dt_real = max(dt_real * scale, dt_min)
            time += dt_real
        assert abs(written[-1] - dt_real) <= 1e-11 * dt_real, (ti, written, dt_real)
        used.append(dt_real)
        rows = _field_rows(d.element_fields())
        ref.step(rows, dt_real)
        dt = max(dt_real * ((nr_iter * scale) / max(1, it)), dt_min)
        if abs(time - t_final) <= abs(1e-3 * dt_real):
            break
    print("auto dts:", used)
    assert 3 <= len(used) <= 12 and max(used) > 1.5 * min(used)                                # steps of different sizes
    sa = d.slip_activity(k=K_FS, sigma_y=SIGMA_Y)
    assert sa["SlipAbsolute"].max() > 0.0
    compare_driver(sa, ref, rows, len(used), 0, "Time.Auto")
    d.close()


def test_checkpoint_continues_the_accumulators(tmp_path, monkeypatch):
    import exaconstit_amd.lib as L
    monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    ck = '[Checkpoint]\n    write = true\n    steps = 8\n    keep = 4\n'
    full, res, off, par = tmp_path / "full", tmp_path / "resumed", tmp_path / "off", tmp_path / "parent"
    for p in (full, res, off, par):
        p.mkdir()
    toml = _cyclic_toml(tmp_path, "on", FAT_ON, ck)
    d = L.Driver.from_toml(toml, out_dir=str(full))
    assert d.run() == 16
    a = d.slip_activity(k=0.5, sigma_y=SIGMA_Y)
    d.close()
    c8 = str(full / "checkpoint_000008.ckpt")
    info = L.checkpoint_info(c8)
    assert info["version"] == 1 and info["steps_done"] == 8 and info["elements"] == 125
    assert info["sections"]["slip_activity"][1] == 480 * 125 and info["sections"]["fatigue_window"][1] == 16 and info["sections"]["fatigue_rows"][1] == 72
    raw = open(c8, "rb").read()
    w = np.frombuffer(raw, np.int64, 2, info["sections"]["fatigue_window"][0])
    assert list(w) == [0, 1]                                                                  # the reset asked for after the evaluation of step 8 waits for step 9
    e = L.Driver.from_toml(toml, out_dir=str(res), restart=c8)
    assert open(str(res / "fatigue.txt")).read() == "".join(open(str(full / "fatigue.txt")).read().splitlines(True)[:2])   # rewritten from the stored rows
    assert e.run() == 16
    b = e.slip_activity(k=0.5, sigma_y=SIGMA_Y)
    e.close()
    assert a["SlipAbsolute"].max() > 0.0
    for k in a:
        assert (a[k] == b[k]) if k == "summary" else all(np.array_equal(a[k][j], b[k][j]) for j in a[k]) if k == "grains" else np.array_equal(a[k], b[k]), k
    assert open(str(res / "fatigue.txt")).read() == open(str(full / "fatigue.txt")).read()
    assert open(str(res / "fatigue_grains_000016.txt")).read() == open(str(full / "fatigue_grains_000016.txt")).read()
    # the feature off: the sections of the parent configuration, nothing else
    t_off, t_par = _cyclic_toml(tmp_path, "off", ["fatigue = false"], ck), _cyclic_toml(tmp_path, "parent", [], ck)
    for t, o in ((t_off, off), (t_par, par)):
        x = L.Driver.from_toml(t, out_dir=str(o))
        assert x.run() == 16
        x.close()
    i_off, i_par = L.checkpoint_info(str(off / "checkpoint_000008.ckpt")), L.checkpoint_info(str(par / "checkpoint_000008.ckpt"))
    assert list(i_off["sections"]) == list(i_par["sections"]) and not any("fatigue" in k or "slip" in k for k in i_off["sections"])
    assert open(str(off / "checkpoint_000008.ckpt"), "rb").read() == open(str(par / "checkpoint_000008.ckpt"), "rb").read()
    assert set(info["sections"]) - set(i_par["sections"]) == {"slip_activity", "fatigue_window", "fatigue_rows"}
    # refusals and the ignored sections
    with pytest.raises(RuntimeError, match="slip_activity"):
        L.Driver.from_toml(toml, out_dir=str(tmp_path), write_files=False, restart=str(par / "checkpoint_000008.ckpt"))
    x = L.Driver.from_toml(t_par, out_dir=str(tmp_path), write_files=False, restart=c8)   # the feature off: the sections are ignored
    assert x.step(9)
    with pytest.raises(RuntimeError, match="not on"):
        x.slip_activity(sigma_y=SIGMA_Y)
    x.close()
