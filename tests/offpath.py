"""The oracle's side of the off-path constitutive tests, shared by tests/test_offpath_inputs_host.py (which asserts on the oracle alone that
the inputs reach what they were built for) and tests/test_gpu_offpath_constitutive.py (which compares the kernels with it).  One oracle
run per (path, model, order): computed on first use, read-only afterwards.

A run is a list of step records.  Both sides of the GPU comparison continue from the oracle's state, so a record holds everything one
launch needs (coordinates, velocity, Jacobians, begin-of-step stress and state) and everything it is compared with (end-of-step stress,
state, tangent, velocity gradient), plus the reference's own convergence noise: the same step solved again by the oracle from the same
begin-of-step state with the property table's solver tolerance divided by 100, and the rel-L2 distance of the two answers per quantity."""
import ctypes as C
import os

import numpy as np

import hipref
from hipref import rel_l2
from test_gpu_parity import CASES      # (name, oracle xtal, oracle kin, props, lib model id); importing that module needs no GPU

RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "offpath_checks.txt")
CASE = {c[0]: c for c in CASES}
PROPS_FILE = {"voce": "props_cp_voce.txt", "vocenl": "props_cp_vocenl.txt", "mts": "props_cp_mts.txt"}
PATHS = hipref.PATH_NAMES + ("state",)
IND_VOL, IND_EINT, IND_TOL = 26, 27, 2     # state slots; index of the solver tolerance in every property table (host_tables.cpp exa_fill_mat_params)
# state slot groups of _check_model_setup (test_gpu_parity.py) in slot numbers: slot 3, the evaluation count, has its own criterion
GROUPS = (("slots 0-2", (0, 1, 2)), ("slots 4-8", (4, 5, 6, 7, 8)), ("slots 9-12", (9, 10, 11, 12)), ("slot 13", (13,)),
          ("slots 14-25", tuple(range(14, 26))), ("slots 26-27", (26, 27)))
QUANTITIES = ("stress",) + tuple(g[0] for g in GROUPS) + ("tangent",)
PROJECT_BOUND = dict({"stress": 1e-9, "tangent": 1e-7}, **{g[0]: 1e-8 for g in GROUPS})
NFEV_LIMIT = 200                           # evaluation limit of the local solver, both sides


def record(key, lines):
    """profiles/high_order_checks.txt's convention: with EXA_WRITE_RECORDS=1 the lines replace the block '[key]' of profiles/offpath_checks.txt;
    without the variable a test run leaves the committed record alone"""
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


def fmt(d):
    """the QUANTITIES of a dict on one line"""
    return ", ".join(f"{q} {d[q]:.2e}" for q in QUANTITIES)


def props(orc, pkey):
    return np.loadtxt(orc.REFDATA + "/" + PROPS_FILE[pkey]).ravel()


def gam_w(pr, kin, state):
    """reference slip rate the solver scales by, per point: a property of the Voce tables; gam_wo / sqrt(dislocation density, slot 13) for Kocks-Mecking"""
    P = state.reshape(-1, 28).shape[0]
    return np.full(P, pr[8]) if kin != 2 else pr[12] / np.sqrt(state.reshape(-1, 28)[:, 13])


def temperature_constants(pr):
    """tK0, dtde as the library derives them (host_tables.cpp exa_fill_mat_params): cvav is entry 1, the cold energy the last entry"""
    dtde = 1.0 / pr[1]
    return -pr[-1] * dtde, dtde


def mesh(orc, p=1):
    """p = 1: 27 elements (one partial 64-element block), 216 points; p = 2: 8 elements, 216 points"""
    return hipref.make_rve(orc, 3, distort=0.2) if p == 1 else hipref.make_rve(orc, 2, p=2, distort=0.1)


def edit_state(sv, pr, volume=True, energy=True):
    """the begin-of-step state of the `state` case: relative volume 0.97 at the even points and 1.03 at the odd ones; internal energy such
    that tK0 + eint dtde is 200 K at the points 0 mod 3, 450 K at 1 mod 3 and unchanged at the rest"""
    s = np.array(sv).reshape(-1, 28)
    i = np.arange(s.shape[0])
    if volume:
        s[:, IND_VOL] = np.where(i % 2 == 0, 0.97, 1.03)
    if energy:
        tK0, dtde = temperature_constants(pr)
        s[i % 3 == 0, IND_EINT] = (200.0 - tK0) / dtde
        s[i % 3 == 1, IND_EINT] = (450.0 - tK0) / dtde
    return s.ravel()


def oracle_step(orc, xtal, kin, pr, rve, dt, J, vel_e, s0, sv0):
    """orc_model_setup on one step: (failed points, stress, state, tangent, velocity gradient)"""
    for a in (pr, J, vel_e, s0, sv0):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    P = rve["E"] * rve["Q"]
    s1 = np.zeros(6 * P); sv1 = np.zeros(28 * P); cm = np.zeros(36 * P); vg = np.zeros(9 * P)
    nf = orc.lib().orc_model_setup(xtal, kin, orc._p(pr), len(pr), rve["Q"], rve["E"], rve["n"], 28, C.c_double(dt), C.c_double(298.0), orc._p(J),
                                   orc._p(rve["G"]), orc._p(vel_e), orc._p(s0), orc._p(sv0), orc._p(s1), orc._p(sv1), orc._p(cm), orc._p(vg), 1, 0, 0)
    return nf, s1, sv1, cm, vg


def differences(s1, sv1, cm, r_s1, r_sv1, r_cm):
    """rel-L2 of (stress, the six slot groups, tangent) against the r_ side, keyed by QUANTITIES"""
    a = np.asarray(sv1).reshape(-1, 28); b = np.asarray(r_sv1).reshape(-1, 28)
    out = {"stress": rel_l2(s1, r_s1), "tangent": rel_l2(cm, r_cm)}
    for name, cols in GROUPS:
        out[name] = rel_l2(a[:, list(cols)], b[:, list(cols)])
    return out


def bounds(noise):
    """per quantity: the project's bound, or ten times the reference's own convergence noise where that is larger (the GPU iterate and the
    oracle's are two independent points inside the solver's tolerance ball, and the norm runs over a few hundred points)"""
    return {q: max(PROJECT_BOUND[q], 10.0 * noise[q]) for q in QUANTITIES}


def initial_state(orc, xtal, kin, pr, rve, quats):
    P = rve["E"] * rve["Q"]
    hist = np.zeros(26); orc.lib().orc_hist_init(xtal, kin, orc._p(pr), len(pr), orc._p(hist))
    sv0 = np.tile(np.concatenate([hist, [1.0, 0.0]]), P).reshape(P, 28)
    sv0[:, 9:13] = np.repeat(quats, rve["Q"], axis=0)
    return sv0.ravel()


_runs = {}


def run(orc, path, model, p=1):
    """the step records of one (path, model, order)"""
    key = (path, model, p)
    if key in _runs:
        return _runs[key]
    _, xtal, kin, pkey, _ = CASE[model]
    pr = props(orc, pkey)
    tight = pr.copy(); tight[IND_TOL] = pr[IND_TOL] / 100.0
    rve = mesh(orc, p)
    E, Q, P = rve["E"], rve["Q"], rve["E"] * rve["Q"]
    steps = hipref.load_path("reversal")[:len(hipref.PATH_START_DTS)] if path == "state" else hipref.load_path(path)
    rng = np.random.default_rng(20241021 + PATHS.index(path))
    sv0 = initial_state(orc, xtal, kin, pr, rve, hipref.random_quats(E))
    s0 = np.zeros(6 * P)
    x = rve["X"].copy()
    recs = []
    for k, (D, W, dt) in enumerate(steps):
        x, v = hipref.path_step(rve, x, D, W, dt, rng)
        xe = hipref.l_to_e(rve, x); vel_e = hipref.l_to_e(rve, v)
        J = np.zeros(9 * P); orc.lib().orc_jacobians(p, E, orc._p(xe), orc._p(J))
        if path == "state" and k == len(steps) - 1:
            sv_plain = sv0
            sv0 = edit_state(sv0, pr)
        nf, s1, sv1, cm, vg = oracle_step(orc, xtal, kin, pr, rve, dt, J, vel_e, s0, sv0)
        nf2, t_s1, t_sv1, t_cm, _ = oracle_step(orc, xtal, kin, tight, rve, dt, J, vel_e, s0, sv0)
        rec = dict(k=k, D=D, W=W, dt=dt, x=x, v=v, xe=xe, vel_e=vel_e, J=J, s0=s0, sv0=sv0, nf=nf, nf_tight=nf2, s1=s1, sv1=sv1, cm=cm, vg=vg,
                   noise=differences(t_s1, t_sv1, t_cm, s1, sv1, cm))
        if path == "state" and k == len(steps) - 1:
            rec["sv0_plain"] = sv_plain
        for a in rec.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        recs.append(rec)
        s0, sv0 = s1, sv1
    _runs[key] = dict(rve=rve, props=pr, xtal=xtal, kin=kin, steps=recs, P=P)
    return _runs[key]


def perturbed_steps(orc, r, trials=3, seed=3):
    """every step of a run solved again by the oracle with its Jacobians perturbed in the last bit (relative 1e-15, normal): per step
    (failed points summed over the trials, largest evaluation count, largest difference of a count from the unperturbed run's).  A kernel
    differs from the oracle by that much at least, so an input is only as good as the oracle is steady on it."""
    rng = np.random.default_rng(seed)
    out = []
    for s in r["steps"]:
        base = s["sv1"].reshape(-1, 28)[:, 3]
        nf = mx = df = 0
        for _ in range(trials):
            J = np.array(s["J"]) * (1.0 + 1e-15 * rng.standard_normal(s["J"].shape))
            o = oracle_step(orc, r["xtal"], r["kin"], r["props"], r["rve"], s["dt"], J, np.array(s["vel_e"]), np.array(s["s0"]), np.array(s["sv0"]))
            c = o[2].reshape(-1, 28)[:, 3]
            nf += o[0]; mx = max(mx, int(c.max())); df = max(df, int(np.abs(c - base).max()))
        out.append((nf, mx, df))
    return out


def run_noise(r):
    """worst noise of a run per quantity, over its steps: the figure the bound of the whole path is derived from"""
    return {q: max(rec["noise"][q] for rec in r["steps"]) for q in QUANTITIES}


def histogram(counts):
    """evaluation counts as 'count:points' pairs"""
    v, n = np.unique(np.asarray(counts).astype(np.int64), return_counts=True)
    return " ".join(f"{a}:{b}" for a, b in zip(v, n))


def rotation_angle(q0, q1):
    """angle of the rotation between two fields of unit quaternions (P, 4), rad"""
    q0 = np.asarray(q0); q1 = np.asarray(q1)
    sgn = np.where(np.sum(q0 * q1, axis=1) < 0, -1.0, 1.0)      # q and -q are the same rotation
    chord = np.linalg.norm(q1 - sgn[:, None] * q0, axis=1)     # 2 sin(angle / 4): the quaternions are angle / 2 apart on the unit sphere
    return 4.0 * np.arcsin(np.minimum(0.5 * chord, 1.0))
