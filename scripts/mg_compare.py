"""Identity against multigrid PCG preconditioning (Solvers.Krylov.preconditioner = "multigrid", exaconstit_amd/csrc/host/multigrid.hpp) on the
synthetic FCC Voce RVE, both in one invocation, at each --n: three steps through first yield (0.01 %, 0.03 %, 0.06 % z-strain), the
tolerances of BASELINE config 1 (Newton 5e-5, PCG rel 1e-7, 1000-iteration cap).  Prints one JSON document:
  per case and preconditioner: per step wall ms, Newton and Krylov iterations; the worst residual reduction reached; PCG ms per iteration;
  multigrid only: hierarchy set-up ms (last Newton iteration), V-cycle ms, levels and the lmax estimates.
--periodic: the same three-step run on a periodic cell under L = diag(0, 0, 1e-3) ("periodic cells"); --free with it: uniaxial
stress, xx and yy free - the control block of the preconditioner is then reported as control_dofs; --kinds picks the
preconditioners (identity, jacobi, multigrid).
--order 2: the same run at p = 2 ("p = 2"; N^3 elements are (2 N + 1)^3 nodes): identity against multigrid, and the multigrid run twice -
level 1 and the fine diagonal read off the point records ("multigrid") and probed ("multigrid_probe") - in one invocation; --degree lists the
Chebyshev degrees of the smoother (one multigrid entry per degree beyond the first, "multigrid_deg<k>").
--bbar: the same run under the B-bar integrator with element assembly ("B-bar"), at --order 1 or 2; --order 2 --bbar --n 64 is the
shape of BASELINE config 5.  --dts replaces the three time steps (s; 1e-3 /s of z-strain rate), e.g. six steps of 0.1 to the same end strain.
    python scripts/mg_compare.py --n 64 128 > profiles/mg_compare.json
    python scripts/mg_compare.py --order 2 --bbar --n 32 64 > profiles/mg_bbar_compare.json
    python scripts/mg_compare.py --order 2 --n 32 64 > profiles/mg_p2_compare.json
    python scripts/mg_compare.py --periodic --free --n 64 128"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(L, N, kind, dts, props, quats, periodic=False, free=False, order=1, degree=2, from_records=True, bbar=False):
    d = L.Driver.synthetic(N, props, quats, dts, assembly=1 if bbar else 0, order=order, bbar=bbar)
    if periodic:
        d.set_periodic(np.diag([0.0, 0.0, 1.0e-3]), np.diag([1, 1, 0]) if free else None)
    if kind != "identity":
        d.set_preconditioner(kind, degree=degree, periodic=periodic, p2=order == 2, bbar=bbar) if kind == "multigrid" else d.set_preconditioner(kind)
        if kind == "multigrid" and order == 2:
            d.set_mg_p2_build(from_records)
    steps = []
    worst = 0.0
    setups = []
    for ti in range(1, len(dts) + 1):
        t0 = time.perf_counter()
        ok = d.step(ti)
        wall = (time.perf_counter() - t0) * 1e3
        newton, krylov, _ = d.stats()
        dg = d.diagnostics()
        worst = max(worst, dg["pcg_last_reduction"], dg["pcg_worst_capped_reduction"])
        steps.append(dict(step=ti, converged=bool(ok), wall_ms=round(wall, 2), newton=int(newton[-1]), krylov=int(krylov[-1])))
        if kind == "multigrid":
            setups.append(d.mg_info()["setup_ms"])
    tm = d.timers()
    out = dict(steps=steps, krylov_total=int(sum(s["krylov"] for s in steps)), pcg_not_converged=d.diagnostics()["pcg_not_converged"],
               worst_residual_reduction_reached=worst, pcg_ms_per_iter=tm["krylov_ms"] / max(tm["krylov_iters"], 1),
               wall_ms_total=round(sum(s["wall_ms"] for s in steps), 2))
    if kind == "multigrid":
        info = d.mg_info()
        out.update(levels=info["levels"], setup_ms_per_newton_iter=float(np.mean(setups)), vcycle_ms=info["vcycle_ms"],
                   lmax=[float(v) for v in info["lmax"]], periodic=info["periodic"], control_dofs=info["control_dofs"], degree=info["degree"],
                   order=info["order"], level1_build=info["level1_build"], bbar=info["bbar"])
    d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--periodic", action="store_true", help="a periodic cell under L = diag(0, 0, 1e-3) instead of the prescribed faces")
    ap.add_argument("--free", action="store_true", help="with --periodic: xx and yy free (uniaxial stress)")
    ap.add_argument("--kinds", nargs="+", default=["identity", "multigrid"], choices=["identity", "jacobi", "multigrid"])
    ap.add_argument("--order", type=int, default=1, choices=[1, 2], help="polynomial order of the mesh")
    ap.add_argument("--degree", type=int, nargs="+", default=[2], help="Chebyshev degree(s) of the multigrid smoother")
    ap.add_argument("--dts", type=float, nargs="+", default=[0.1, 0.2, 0.3], help="time steps of the schedule")
    ap.add_argument("--bbar", action="store_true", help="the B-bar integrator with element assembly (multigrid: mg_bbar)")
    a = ap.parse_args()
    if a.free and not a.periodic:
        ap.error("--free needs --periodic")
    if a.bbar and a.periodic:
        ap.error("--bbar has no periodic multigrid")
    if a.order == 2 and a.periodic:
        ap.error("--order 2 has no periodic multigrid")
    import exaconstit_amd.lib as L
    import hipref
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    if min(a.dts) <= 0.0:
        ap.error("--dts: positive time steps")
    dts = np.array(a.dts, dtype=np.float64)
    res = dict(schedule=dict(dts=dts.tolist(), vz=1e-3, newton_rel=5e-5, krylov_rel=1e-7, krylov_iter=1000, periodic=a.periodic, free_xx_yy=a.free, order=a.order,
                             integ_model="BBAR" if a.bbar else "FULL", assembly="EA" if a.bbar else "PA"),
               cases={})
    for N in a.n:
        quats = hipref.random_quats(N ** 3, seed=16)
        case = res["cases"][str(N)] = {}
        for k in a.kinds:
            case[k] = run(L, N, k, dts, props, quats, a.periodic, a.free, a.order, a.degree[0], bbar=a.bbar)
            if k != "multigrid":
                continue
            if a.order == 2:
                case["multigrid_probe"] = run(L, N, k, dts, props, quats, order=2, degree=a.degree[0], from_records=False, bbar=a.bbar)
            for dg in a.degree[1:]:
                case["multigrid_deg%d" % dg] = run(L, N, k, dts, props, quats, a.periodic, a.free, a.order, dg, bbar=a.bbar)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
