"""The constitutive kernels (ecm_device.hpp) against the live oracle OFF the load history every other comparison runs (hipref.velocity_field:
monotonic, nearly isochoric uniaxial tension at 1e-3 /s from the virgin state).  The inputs are the load paths of hipref.load_path and the
edited state of the `state` case; tests/test_offpath_inputs_host.py asserts on the oracle alone that they reach the following code, which
no other test runs:
  rotation  lattice-rotation increments of 0.02, 0.05, 0.2 and 0.5 rad in one step under tension, then a pure spin (D = 0) of 0.02 rad: the
            large-angle branches of exp_map (th2 >= 1e-4) and of the quaternion update, i.e. sincos_s and the closed forms sin th / th,
            (1 - cos th) / th^2, (th - sin th) / th^3; the two-sweep Gauss-Seidel Newton step (jac_solve) with coupling blocks of size |W| dt up to
            0.5 instead of the 1e-4 its comment argues for; on the pure spin |dev D| is the jitter alone and the scale is the cap 1e6 dt;
  hold      exactly zero velocity, then 1e-12, 1e-7, 1e-5 and 1e-3 of the tension rate: `dnorm < EPS_SQRT * adots_ref` (scale by the reference
            slip rate) on the first three steps (four for Kocks-Mecking), the `s1 > 1e6 dt` cap on the rest; few evaluations per solve, the
            stress relaxing;
  reversal  elastic unloading, the zero crossing and reverse yield: every point ends with a slip system whose rate has the opposite sign to
            its begin-of-step rate (copysign sites, hardening update from rates of the other sign);
  shear     simple shear from the virgin state: D and W of equal size, other slip systems than tension's;
  volume    relative volume 1.009 then 0.97 ... 0.978: vNew = vOld exp(dkk dt), bulkNew, eNew = eint - delv pOld with a pressure of tens of GPa-units;
  rate      strain-rate jumps over four decades (0.1 ... 1000 times 1e-3 /s): the drag-limited and athermal-threshold windows of km_gdot;
  state     the last tension step from a begin-of-step state with relative volume 0.97 / 1.03 and internal energy for 200 K / 450 K / 300 K:
            tK = tK0 + eNew dtde, which feeds c_e of the Kocks-Mecking kinds, is otherwise one number in every test.
Each (path, model) case compares, at every step and from the oracle's begin-of-step state, (a) the reference-layout entry exa_model_setup
and (b) the default product path (element-blocked layout, exa_model_setup_lvec and exa_model_setup_lvec_records on a compact-tangent
context) with the oracle: status 0; stress, the six state slot groups and the tangent within bound; the record launch equal to the
tangent-writing one (1e-13) and its action equal to the action from that launch's tangent (1e-12).

Bounds.  The project's are 1e-9 (stress), 1e-8 (each slot group), 1e-7 (tangent).  Where ten times the reference's own convergence noise (the
oracle against itself at a hundredth of the solver tolerance, worst step of the path, offpath.bounds) is larger, that is the bound: for the
Voce models on `hold` only (stress 4.4e-7, slip rates 3.3e-5, tangent 2.5e-6: a relaxing point's answer depends on where in the tolerance
ball the solve stopped); for the Kocks-Mecking models, whose property table asks for 1e-8, on every path by factors of 1 ... 20 for stress,
slots 0-2, 14-25 and the tangent, and on `hold` by orders of magnitude (stress 1.6e-3, slip rates 0.7: there the comparison says little
beyond "converged to the same relaxation", and the record says so).  profiles/offpath_checks.txt holds every bound beside what was measured.

Evaluation counts (state slot 3): on every path but `rotation` equal to the oracle's at >= 99.9 % of the points of a model's pooled paths and
never more than one apart (_nfev_check of test_gpu_parity.py).  On `rotation` the approximate Newton step is outside the regime its comment
argues for: convergence, the bounds and "no point at the limit of 200" are asserted, the two histograms printed, equality is not.

Also here: the finite-difference test of the tangent (test_gpu_point_fixtures.py) on the last step of `reversal` and on the 0.2 rad step of
`rotation`, where "the tangent eliminates the rotation block exactly" is put to the test; `rotation` and `reversal` through the order-2
instantiation; and the rotation arithmetic on its own (exa_selftest_rot_math) against extended precision.

Found ("Off the tension path"; figures in profiles/offpath_checks.txt):
  * exp_map: b = (1 - cos th) / th^2 cancelled just above the branch point; entries of Tr were off by 27 ulp of 1 (5.9e-15) at th = 0.01
    (bound 4).  Fixed in the large-angle branch, which the tension path never takes: b = a^2 / (1 + cos th) while cos th > 0.  sincos_s: 1.5 ulp.
  * rotation: every point converges, within the bounds; the counts equal the oracle's at all but 4 or 5 of 1944 point updates of a Voce
    model, where they differ by up to 35 (bcc_voce) and 6 (fcc_voce), at points with 40 to 100 evaluations.  The oracle's own counts move
    under a last-bit perturbation of its Jacobians there too (by 25 on one step of bcc_voce, by 1 for fcc_voce), so round-off is one
    possible cause; the two-sweep step, which the Voce kinds keep, is the other, and which it is has not been settled (a Voce build with
    ECM_GS_SWEEPS=4 on this path would).  Not asserted, as planned; the histograms are in the record and in DESIGN.md.
  * test_offpath_evaluation_counts_pooled failed for fcc_kmdd (46 of 10800 point updates unequal, by up to 19 either way) and bcc_kmdd (7, by
    up to 4): on the steps with dt >= 1 s (shear at dt = 2 and 5, the volume steps, 1e-4 /s at dt = 4), at points whose oracle count is
    12 ... 57, with stress, state and tangent inside the bounds and the same counts in both layouts, while the oracle's counts are steady
    under last-bit perturbations on these paths (asserted by the host module).  A build with four Gauss-Seidel sweeps in the Newton step
    (ECM_GS_SWEEPS=4) agreed everywhere: the two-sweep step was the cause.  Fixed for the Kocks-Mecking kinds: the sweeps go on until one
    changes x_r by less than 1e-6 (ecm_device.hpp jac_solve, ADAPT).  The Voce kinds met the criterion and keep two sweeps."""
import numpy as np
import pytest

import hipref
import offpath as O
from hipref import ptr, rel_l2
from test_gpu_parity import _aos_to_eb64, _eb64_to_aos, _nfev_check

pytestmark = pytest.mark.gpu

MODELS = [c[0] for c in O.CASES]
NSTART = len(hipref.PATH_START_DTS)
P2_CASES = [(path, model) for path in ("rotation", "reversal") for model in ("fcc_voce", "bcc_kmdd")]

_gpu = {}


def _worst(dicts):
    return {q: max(d[q] for d in dicts) for q in O.QUANTITIES}


def _gpu_run(orc, path, model):
    """both launches at every step of one (path, model), from the oracle's begin-of-step state: per step the status, the differences from the
    oracle (offpath.differences), the evaluation counts, and the record launch's agreement with the tangent-writing one.  Cached."""
    key = (path, model)
    if key in _gpu:
        return _gpu[key]
    import torch
    import exaconstit_amd.lib as L
    r = O.run(orc, path, model)
    rve, props, P = r["rve"], r["props"], r["P"]
    E, Q, NN = rve["E"], rve["Q"], rve["NN"]
    lib_model = O.CASE[model][4]
    dev = hipref.Dev()
    ca = L.Context(lib_model, props, 298.0, 1, E)
    cb = L.Context(lib_model, props, 298.0, 1, E, assembly=L.EXA_ASSEMBLY_PA)
    d_conn = torch.from_numpy(rve["conn"].astype(np.int32)).to(dev.dev)
    cb.check(L.exa_set_quadrature_layout(cb.h, L.EXA_QLAYOUT_EB64)); cb.check(L.exa_set_connectivity(cb.h, ptr(d_conn), NN))
    cb.check(L.exa_set_tangent_form(cb.h, L.EXA_TANGENT_DEV5_BULK))
    sz = lambda w: int(L.exa_qf_size(cb.h, w))
    xg = np.random.default_rng(5).standard_normal(3 * NN)
    mask = (np.random.default_rng(6).random(3 * NN) < 0.1).astype(np.uint8)
    d_xg, d_mask = dev.up(xg), dev.up(mask)
    out = []
    for s in r["steps"]:
        dt = float(s["dt"])
        res = dict(k=s["k"], dt=dt)
        # (a) reference layout, E-vector velocity, the oracle's Jacobians
        d = [dev.up(np.array(a)) for a in (s["J"], s["vel_e"], s["s0"], s["sv0"])]
        o = [dev.zeros(6 * P), dev.zeros(28 * P), dev.zeros(36 * P)]
        ca.check(L.exa_model_setup(ca.h, dt, *[ptr(t) for t in d], *[ptr(t) for t in o], None))
        res["status_a"] = ca.check(L.exa_model_status(ca.h, None))
        a_s1, a_sv1, a_cm = [t.cpu().numpy() for t in o]
        res["a"] = O.differences(a_s1, a_sv1, a_cm, s["s1"], s["sv1"], s["cm"])
        res["nfev_a"] = a_sv1.reshape(P, 28)[:, 3].copy()
        # (b) element-blocked layout, L-vector coordinates and velocity: the tangent-writing launch, then the record launch
        d_s0 = dev.up(_aos_to_eb64(s["s0"], E, Q, 6)); d_sv0 = dev.up(_aos_to_eb64(s["sv0"], E, Q, 28))
        d_s1 = dev.zeros(sz(6)); d_sv1 = dev.zeros(sz(28)); d_cm = dev.zeros(sz(36)); d_J = dev.zeros(sz(9))
        d_x = dev.up(np.array(s["x"])); d_v = dev.up(np.array(s["v"]))
        cb.check(L.exa_model_setup_lvec(cb.h, dt, ptr(d_x), ptr(d_v), ptr(d_s0), ptr(d_sv0), ptr(d_s1), ptr(d_sv1), ptr(d_cm), ptr(d_J), None))
        res["status_b"] = cb.check(L.exa_model_status(cb.h, None))
        res["J"] = rel_l2(_eb64_to_aos(d_J, E, Q, 9).cpu().numpy().ravel(), s["J"])
        b_sv1 = _eb64_to_aos(d_sv1, E, Q, 28).cpu().numpy()
        res["b"] = O.differences(_eb64_to_aos(d_s1, E, Q, 6).cpu().numpy(), b_sv1, _eb64_to_aos(d_cm, E, Q, 36).cpu().numpy(), s["s1"], s["sv1"], s["cm"])
        res["nfev_b"] = b_sv1[:, 3].copy()
        cb.check(L.exa_grad_set_coords(cb.h, ptr(d_x)))
        cb.check(L.exa_grad_setup(cb.h, dt, ptr(d_J), ptr(d_cm), None))
        d_kf = dev.zeros(3 * NN); cb.check(L.exa_grad_apply_lvec(cb.h, ptr(d_xg), ptr(d_kf), ptr(d_mask), None))
        r_s1 = dev.zeros(sz(6)); r_sv1 = dev.zeros(sz(28)); r_J = dev.zeros(sz(9))
        cb.check(L.exa_model_setup_lvec_records(cb.h, dt, ptr(d_x), ptr(d_v), ptr(d_s0), ptr(d_sv0), ptr(r_s1), ptr(r_sv1), ptr(r_J), None))
        res["status_r"] = cb.check(L.exa_model_status(cb.h, None))
        d_kr = dev.zeros(3 * NN); cb.check(L.exa_grad_apply_lvec(cb.h, ptr(d_xg), ptr(d_kr), ptr(d_mask), None))
        res["rec_J"] = bool(torch.equal(r_J, d_J))
        res["rec_stress"] = rel_l2(r_s1.cpu().numpy(), d_s1.cpu().numpy()); res["rec_state"] = rel_l2(r_sv1.cpu().numpy(), d_sv1.cpu().numpy())
        res["rec_action"] = rel_l2(d_kr.cpu().numpy(), d_kf.cpu().numpy())
        res["nfev_ref"] = s["sv1"].reshape(P, 28)[:, 3].copy()
        out.append(res)
    ca.close(); cb.close()
    _gpu[key] = out
    return out


def _count_line(tag, got, ref):
    d = np.abs(got - ref)
    return f"evaluation counts {tag}: equal at {int((d == 0).sum())} of {d.size} point updates, largest difference {int(d.max())}"


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("path", O.PATHS)
def test_offpath_matches_oracle(oracle, path, model):
    r = O.run(oracle, path, model)
    noise = O.run_noise(r); bound = O.bounds(noise)
    g = _gpu_run(oracle, path, model)
    wa, wb = _worst([s["a"] for s in g]), _worst([s["b"] for s in g])
    ref = np.concatenate([s["nfev_ref"] for s in g]); na = np.concatenate([s["nfev_a"] for s in g]); nb = np.concatenate([s["nfev_b"] for s in g])
    lines = [f"reference noise: {O.fmt(noise)}", f"bound: {O.fmt(bound)}",
             f"exa_model_setup, worst step: {O.fmt(wa)}", f"exa_model_setup_lvec, worst step: {O.fmt(wb)}",
             f"record launch against the tangent-writing one, worst step: stress {max(s['rec_stress'] for s in g):.2e}, state {max(s['rec_state'] for s in g):.2e}, "
             f"action {max(s['rec_action'] for s in g):.2e}; Jacobians against the oracle's {max(s['J'] for s in g):.2e}",
             f"failed points: exa_model_setup {sum(s['status_a'] for s in g)}, exa_model_setup_lvec {sum(s['status_b'] for s in g)}, records {sum(s['status_r'] for s in g)}",
             _count_line("exa_model_setup", na, ref), _count_line("exa_model_setup_lvec", nb, ref)]
    if path == "rotation":
        spin = slice(NSTART * r["P"], None)
        lines += [f"spin steps, evaluation counts (count:points) oracle: {O.histogram(ref[spin])}",
                  f"spin steps, evaluation counts (count:points) exa_model_setup: {O.histogram(na[spin])}",
                  f"spin steps, evaluation counts (count:points) exa_model_setup_lvec: {O.histogram(nb[spin])}"]
    for s in g:
        lines.append(f"step {s['k']} dt {s['dt']:g}: exa_model_setup {O.fmt(s['a'])}")
    for ln in lines:
        print(f"{path} {model}: {ln}")
    O.record(f"gpu {path} {model}", lines)
    for s in g:
        assert s["status_a"] == 0 and s["status_b"] == 0 and s["status_r"] == 0, (path, model, s["k"])
        assert s["J"] < 1e-13, (path, model, s["k"])
        for q in O.QUANTITIES:
            assert s["a"][q] <= bound[q], (path, model, s["k"], "exa_model_setup", q, s["a"][q], bound[q])
            assert s["b"][q] <= bound[q], (path, model, s["k"], "exa_model_setup_lvec", q, s["b"][q], bound[q])
        assert s["rec_J"] and s["rec_stress"] < 1e-13 and s["rec_state"] < 1e-13, (path, model, s["k"])
        assert s["rec_action"] < 1e-12, (path, model, s["k"])
    assert max(na.max(), nb.max()) < O.NFEV_LIMIT, (path, model)      # (agreement of the counts with the oracle's: the pooled test below)


@pytest.mark.parametrize("model", MODELS)
def test_offpath_evaluation_counts_pooled(oracle, model):
    """state slot 3 over one model's paths but `rotation`, both launches: _nfev_check (equal at >= 99.9 %, never more than one apart)"""
    g = [s for path in O.PATHS if path != "rotation" for s in _gpu_run(oracle, path, model)]
    ref = np.concatenate([s["nfev_ref"] for s in g])
    assert ref.max() > 10
    for tag in ("nfev_a", "nfev_b"):
        got = np.concatenate([s[tag] for s in g])
        line = _count_line(tag, got, ref)
        print(f"{model}: {line}")
        O.record(f"gpu pooled counts {model} {tag}", [line])
        _nfev_check(got, ref, (model, tag))


def _gpu_update(L, ctx, dev, dt, J, vel_e, s0, sv0, P):
    d = [dev.up(np.array(a)) for a in (J, vel_e, s0, sv0)]
    o = [dev.zeros(6 * P), dev.zeros(28 * P), dev.zeros(36 * P)]
    ctx.check(L.exa_model_setup(ctx.h, float(dt), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(o[0]), ptr(o[1]), ptr(o[2]), None))
    assert ctx.check(L.exa_model_status(ctx.h, None)) == 0
    return [t.cpu().numpy() for t in o]


@pytest.mark.parametrize("model", ["fcc_voce", "bcc_kmdd"])
@pytest.mark.parametrize("path,step", [("reversal", -1), ("rotation", NSTART + 2)], ids=["reversal_last", "rotation_0p2rad"])
def test_gpu_tangent_is_the_derivative_of_the_gpu_stress_update(oracle, path, step, model):
    """test_gpu_point_fixtures.py's central differences (same five isochoric directions, steps, bounds and quantile rule) after reverse yield
    and on a step that turns the lattice by 0.2 rad: a symmetric trace-free dL changes neither spin nor volume, so tangent * (dt dL) must
    equal the stress difference - with the rotation block eliminated exactly, whatever the size of the rotation."""
    import exaconstit_amd.lib as L
    r = O.run(oracle, path, model)
    s = r["steps"][step]
    if path == "rotation":
        assert abs(np.linalg.norm(s["W"]) / np.sqrt(2.0) * s["dt"] - 0.2) < 1e-12
    rve, P = r["rve"], r["P"]
    E = rve["E"]
    dev = hipref.Dev()
    ctx = L.Context(O.CASE[model][4], r["props"], 298.0, 1, E)
    dt = s["dt"]
    vel = s["vel_e"].reshape(E, 3, 8); xe = s["xe"].reshape(E, 3, 8)
    _, _, cm = _gpu_update(L, ctx, dev, dt, s["J"], s["vel_e"], s["s0"], s["sv0"], P)
    C6 = cm.reshape(P, 6, 6).transpose(0, 2, 1)
    h = 1.0e-7 if "kmdd" not in model else 1.0e-6
    worst = 0.0; errs = []
    for v in ((1, -1, 0, 0, 0, 0), (1, 1, -2, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1)):
        v = np.array(v, dtype=np.float64)
        dL = h * np.array([[v[0], v[5] / 2, v[4] / 2], [v[5] / 2, v[1], v[3] / 2], [v[4] / 2, v[3] / 2, v[2]]])
        dv = np.einsum("ij,ejn->ein", dL, xe)
        sp, _, _ = _gpu_update(L, ctx, dev, dt, s["J"], (vel + dv).ravel(), s["s0"], s["sv0"], P)
        sm, _, _ = _gpu_update(L, ctx, dev, dt, s["J"], (vel - dv).ravel(), s["s0"], s["sv0"], P)
        fd = (sp - sm).reshape(P, 6) / (2.0 * h * dt)
        tan = np.einsum("pij,j->pi", C6, v)
        err = np.linalg.norm(tan - fd, axis=1) / np.linalg.norm(fd, axis=1)
        worst = max(worst, err.max()); errs.append(err)
    errs = np.concatenate(errs)
    line = f"tangent against central differences: worst point {worst:.3e}, quantiles 0.5 / 0.9 / 0.99 {np.quantile(errs, 0.5):.3e} / {np.quantile(errs, 0.9):.3e} / {np.quantile(errs, 0.99):.3e}"
    print(f"{path} step {s['k']} {model}: {line}")
    O.record(f"gpu tangent {path} step {s['k']} {model}", [line])
    ctx.close()
    if "kmdd" not in model:
        assert worst < 2.0e-5, (path, model, worst)
    else:
        assert np.quantile(errs, 0.9) < 1.0e-4, (path, model, np.quantile(errs, [0.5, 0.9, 0.99]))


@pytest.mark.parametrize("path,model", P2_CASES)
def test_offpath_p2_matches_oracle(oracle, path, model):
    """`rotation` and `reversal` through the order-2 instantiation (model_kernels_p2.hip; 8 elements of 27 points), the entry of
    test_model_setup_p2_matches_oracle, every output and every step"""
    import exaconstit_amd.lib as L
    r = O.run(oracle, path, model, p=2)
    noise = O.run_noise(r); bound = O.bounds(noise)
    rve, P = r["rve"], r["P"]
    dev = hipref.Dev()
    ctx = L.Context(O.CASE[model][4], r["props"], 298.0, 2, rve["E"])
    diffs, status, got, ref = [], [], [], []
    for s in r["steps"]:
        assert s["nf"] == 0 and s["sv1"].reshape(P, 28)[:, 3].max() <= 150, (path, model, s["k"])      # the host module's conditions, on this mesh
        d = [dev.up(np.array(a)) for a in (s["J"], s["vel_e"], s["s0"], s["sv0"])]; o = [dev.zeros(6 * P), dev.zeros(28 * P), dev.zeros(36 * P)]
        ctx.check(L.exa_model_setup(ctx.h, float(s["dt"]), *[ptr(t) for t in d], *[ptr(t) for t in o], None))
        status.append(ctx.check(L.exa_model_status(ctx.h, None)))
        s1, sv1, cm = [t.cpu().numpy() for t in o]
        diffs.append(O.differences(s1, sv1, cm, s["s1"], s["sv1"], s["cm"]))
        got.append(sv1.reshape(P, 28)[:, 3].copy()); ref.append(s["sv1"].reshape(P, 28)[:, 3].copy())
    ctx.close()
    got = np.concatenate(got); ref = np.concatenate(ref)
    lines = [f"reference noise: {O.fmt(noise)}", f"bound: {O.fmt(bound)}", f"exa_model_setup at p = 2, worst step: {O.fmt(_worst(diffs))}",
             f"failed points {sum(status)}", _count_line("exa_model_setup at p = 2", got, ref)]
    if path == "rotation":
        lines += [f"spin steps, evaluation counts (count:points) oracle: {O.histogram(ref[NSTART * P:])}",
                  f"spin steps, evaluation counts (count:points) exa_model_setup at p = 2: {O.histogram(got[NSTART * P:])}"]
    for ln in lines:
        print(f"p2 {path} {model}: {ln}")
    O.record(f"gpu p2 {path} {model}", lines)
    assert sum(status) == 0
    for k, df in enumerate(diffs):
        for q in O.QUANTITIES:
            assert df[q] <= bound[q], (path, model, k, q, df[q], bound[q])
    assert got.max() < O.NFEV_LIMIT
    if path != "rotation":
        assert np.abs(got - ref).max() <= 1


# ---- the rotation arithmetic on its own --------------------------------------------------------------------------------------------------
LD = np.longdouble


def _rot_math(x):
    """exa_selftest_rot_math on a float64 array: (sine, cosine) of every entry, and for every whole triple A (T, 3, 3) and Tr (T, 3, 3)"""
    import torch
    import exaconstit_amd.lib as L
    n = len(x); nt = n // 3
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    d_o = torch.zeros(2 * n + 18 * nt, dtype=torch.float64, device="cuda")
    assert L.exa_selftest_rot_math(ptr(d_x), ptr(d_o), n, None) == 0
    torch.cuda.synchronize()
    o = d_o.cpu().numpy()
    m = o[2 * n:].reshape(nt, 2, 3, 3)
    return o[0:2 * n:2], o[1:2 * n:2], m[:, 0], m[:, 1]


def test_rotation_sincos():
    """sincos_s against the extended-precision library routines: at most 2 ulp of the larger of |sin|, |cos| (its comment claims about 1) over
    [-10, 10], log-uniformly over [1e-2, 1e5] (the range the comment claims) and at k pi/2 +- 2^-j, where the reduced argument cancels"""
    assert np.finfo(LD).eps < 2e-19, "needs an extended-precision long double"
    rng = np.random.default_rng(11)
    pio2 = LD(2) * np.arctan(LD(1))
    ks = np.concatenate([np.arange(0, 24), [100, 1000, 10000, 40000, 60000, 63661]]).astype(LD)
    near = np.array([s * (k * pio2 + t * LD(2) ** -j) for k in ks for j in range(1, 53, 3) for t in (-1, 1) for s in (-1, 1)]).astype(np.float64)
    x = np.concatenate([rng.uniform(-10.0, 10.0, 200000), 10.0 ** rng.uniform(-2.0, 5.0, 200000), -(10.0 ** rng.uniform(-2.0, 5.0, 20000)), near,
                        [0.0, 1e-2, 1e5, -1e5, 1e-300]])
    sn, cs, _, _ = _rot_math(x)
    rs, rc = np.sin(x.astype(LD)), np.cos(x.astype(LD))
    ulp = np.spacing(np.maximum(np.abs(rs), np.abs(rc)).astype(np.float64))
    es = np.abs((sn.astype(LD) - rs)).astype(np.float64) / ulp; ec = np.abs((cs.astype(LD) - rc)).astype(np.float64) / ulp
    line = f"sincos_s on {len(x)} arguments: worst sine {es.max():.3f} ulp at x = {x[es.argmax()]:.17g}, worst cosine {ec.max():.3f} ulp at x = {x[ec.argmax()]:.17g}"
    print(line); O.record("gpu rotation arithmetic sincos", [line])
    assert es.max() <= 2.0 and ec.max() <= 2.0


def _exp_map_reference(xi):
    """A = I + a K + b K^2, Tr = I - b K + c K^2 (K = hat xi; a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3) in mpmath at 40
    digits where it is installed, else in long double from forms without cancellation (b from the half angle, c from its series below 0.5)"""
    xi = np.asarray(xi, dtype=np.float64)
    A = np.zeros((len(xi), 3, 3), dtype=LD); Tr = np.zeros((len(xi), 3, 3), dtype=LD)
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    for i, (x, y, z) in enumerate(xi):
        if mp is not None:
            mp.mp.dps = 40
            x, y, z = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z)); one = mp.mpf(1)
            th2 = x * x + y * y + z * z; th = mp.sqrt(th2)
            a = mp.sin(th) / th; b = (one - mp.cos(th)) / th2; c = (th - mp.sin(th)) / (th2 * th)
            cv = lambda v: LD(mp.nstr(v, 30))
        else:
            x, y, z = LD(x), LD(y), LD(z); one = LD(1)
            th2 = x * x + y * y + z * z; th = np.sqrt(th2)
            a = np.sin(th) / th; b = LD(2) * np.sin(th / 2) ** 2 / th2
            if th < 0.5:
                c = LD(0); term = one / LD(6)
                for k in range(14):
                    c += term; term *= -th2 / LD((2 * k + 4) * (2 * k + 5))
            else:
                c = (th - np.sin(th)) / (th2 * th)
            cv = lambda v: v
        K = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
        v = (x, y, z)
        for r in range(3):
            for s in range(3):
                k2 = v[r] * v[s] - (th2 if r == s else 0)
                e = one if r == s else 0 * one
                A[i, r, s] = cv(e + a * K[r][s] + b * k2); Tr[i, r, s] = cv(e - b * K[r][s] + c * k2)
    return A, Tr


def test_rotation_exp_map():
    """exp_map's A and Tr against the closed forms in extended precision, 4 ulp of 1 per entry, for rotation vectors of length 1e-3 ... 3 rad
    and on either side of the branch point th2 = 1e-4 (lengths 0.01 (1 -+ d), d = 1e-6 ... 1e-9: series below, sincos_s above); the step
    across the branch point equals the reference's step to the same bound; A A^T = I to 1e-15"""
    rng = np.random.default_rng(12)
    tol = 4.0 * np.finfo(np.float64).eps
    u = rng.standard_normal((1500, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    xi = u * (10.0 ** rng.uniform(-3.0, np.log10(3.0), 1500))[:, None]
    ub = rng.standard_normal((60, 3)); ub /= np.linalg.norm(ub, axis=1, keepdims=True)
    ds = np.repeat([1e-6, 1e-7, 1e-8, 1e-9], 15)
    below = ub * (0.01 * (1.0 - ds))[:, None]; above = ub * (0.01 * (1.0 + ds))[:, None]
    th2 = lambda v: v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    assert np.all(th2(below) < 1e-4 * (1 - 1e-10)) and np.all(th2(above) > 1e-4 * (1 + 1e-10))      # far enough that no rounding of th2 changes the side
    allv = np.concatenate([xi, below, above])
    assert th2(allv).min() < 1.1e-6 and th2(allv).max() > 8.0
    _, _, A, Tr = _rot_math(allv.ravel())
    rA, rTr = _exp_map_reference(allv)
    eA = np.abs(A.astype(LD) - rA).astype(np.float64); eT = np.abs(Tr.astype(LD) - rTr).astype(np.float64)
    nb = len(xi); na = nb + len(below)
    stepA = np.abs((A[na:].astype(LD) - A[nb:na].astype(LD)) - (rA[na:] - rA[nb:na])).astype(np.float64)
    stepT = np.abs((Tr[na:].astype(LD) - Tr[nb:na].astype(LD)) - (rTr[na:] - rTr[nb:na])).astype(np.float64)
    AL = A.astype(LD)
    orth = np.abs(np.einsum("tij,tkj->tik", AL, AL) - np.eye(3, dtype=LD)).astype(np.float64)
    eps = np.finfo(np.float64).eps
    lines = [f"exp_map on {len(allv)} rotation vectors: worst entry of A {eA.max() / eps:.2f} ulp of 1 (length {np.linalg.norm(allv[eA.max(axis=(1, 2)).argmax()]):.3g}), "
             f"of Tr {eT.max() / eps:.2f} ulp of 1 (length {np.linalg.norm(allv[eT.max(axis=(1, 2)).argmax()]):.3g})",
             f"across th2 = 1e-4: step of A against the reference's step {stepA.max() / eps:.2f} ulp of 1, of Tr {stepT.max() / eps:.2f}; "
             f"worst entry beside the branch point A {eA[nb:].max() / eps:.2f}, Tr {eT[nb:].max() / eps:.2f} ulp of 1",
             f"A A^T - I: worst entry {orth.max():.3e}"]
    for ln in lines:
        print(ln)
    O.record("gpu rotation arithmetic exp_map", lines)
    assert eA.max() <= tol and eT.max() <= tol
    assert stepA.max() <= tol and stepT.max() <= tol
    assert orth.max() <= 1e-15
