"""GMRES against PCG, and the fused Gram-Schmidt kernels against modified Gram-Schmidt, in one invocation.  Prints one JSON document:
  kernels: per --n and column i = 8, 24, 49 the time of one orthogonalisation with its normalisation (exa_gmres_ortho_bench: device events around
           back-to-back repetitions) under one classical pass ("never"), two ("always": what the criterion asks for on the operators tried so far),
           "ifneeded" on data for which the criterion does not ask for the second pass (one pass plus the four launches that leave at once) and
           "mgs", the vector passes of the byte model of DESIGN 4.16 and the fraction of 8 TB/s they amount to; gate: at the largest n, i = 24,
           two fused passes take less time than mgs;
  solves:  three steps through first yield (0.01 %, 0.03 %, 0.06 % z-strain) under the reference settings (Newton 5e-5, Krylov rel 1e-7, cap 1000),
           PCG against GMRES(50), each under identity, Jacobi and multigrid: Krylov iterations per step, solves at the cap, the worst reduction
           reached, wall time, Krylov ms per iteration.
    python scripts/gmres_compare.py --n 64 128 > profiles/gmres_compare.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK = 8.0e12
CHUNK_NOTE = "w is read once per chunk of basis vectors"


def passes(i, mode, chunk):
    """vector passes of 8 n bytes of one orthogonalisation of column i and its normalisation (no preconditioner pass)"""
    k = i + 1
    one = (k + -(-k // chunk)) + (k + 2)            # multi-dot: k vectors + w per chunk; multi-axpy: k vectors, w read and written
    if mode in ("never", "ifneeded"):                # ifneeded as timed here: the second pass is enqueued and not taken
        return one + 2
    if mode == "always":
        return 2 * one + 2
    return 5 * k + 2                                 # mgs: per vector a dot (2) and an axpy (3)


def kernels(L, N, reps):
    n = 3 * (N + 1) ** 3
    out = {}
    for col in (8, 24, 49):
        row = {}
        for mode in ("never", "ifneeded", "always", "mgs"):
            ms = L.gmres_ortho_bench(n, col, mode, reps)
            p = passes(col, mode, L.GMRES_MULTIDOT_CHUNK)
            row[mode] = dict(ms=round(ms, 4), model_passes=p, model_gb=round(p * 8.0 * n / 1e9, 3), fraction_of_8TBs=round(p * 8.0 * n / (ms * 1e-3) / PEAK, 3))
        row["mgs_over_two_fused_passes"] = round(row["mgs"]["ms"] / row["always"]["ms"], 2)
        row["mgs_over_one_fused_pass"] = round(row["mgs"]["ms"] / row["never"]["ms"], 2)
        row["untaken_second_pass_ms"] = round(row["ifneeded"]["ms"] - row["never"]["ms"], 4)
        out["column %d" % col] = row
    return out


def solve(L, N, solver, kind, dts, props, quats):
    d = L.Driver.synthetic(N, props, quats, dts, assembly=0)
    if kind != "identity":
        d.set_preconditioner(kind)
    if solver == "gmres":
        d.set_krylov("gmres", kdim=50)
    steps = []
    worst = 0.0
    for ti in range(1, len(dts) + 1):
        t0 = time.perf_counter()
        ok = d.step(ti)
        wall = (time.perf_counter() - t0) * 1e3
        newton, krylov, _ = d.stats()
        dg = d.diagnostics()
        worst = max(worst, dg["pcg_last_reduction"], dg["pcg_worst_capped_reduction"])
        steps.append(dict(step=ti, converged=bool(ok), wall_ms=round(wall, 2), newton=int(newton[-1]), krylov=int(krylov[-1])))
    tm, dg, info = d.timers(), d.diagnostics(), d.krylov_info()
    out = dict(steps=steps, krylov_total=int(sum(s["krylov"] for s in steps)), solves_at_the_cap=dg["pcg_not_converged"], worst_residual_reduction_reached=worst,
               krylov_ms_per_iter=round(tm["krylov_ms"] / max(tm["krylov_iters"], 1), 4), wall_ms_total=round(sum(s["wall_ms"] for s in steps), 2))
    if solver == "gmres":
        out.update(restarts=info["restarts"], second_passes=info["reorth_passes"], basis_gb=round(info["basis_bytes"] / 1e9, 3))
    d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-solves", action="store_true")
    a = ap.parse_args()
    import exaconstit_amd.lib as L
    import hipref
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    dts = np.array([0.1, 0.2, 0.3])
    res = dict(build_id=L.exa_build_id().decode(), kernel_build_id=L.exa_kernel_build_id().decode(), multidot_chunk=L.GMRES_MULTIDOT_CHUNK, kdim=50,
               byte_model="passes of 8 n bytes per orthogonalisation and normalisation; " + CHUNK_NOTE, kernels={}, solves={},
               schedule=dict(dts=dts.tolist(), vz=1e-3, newton_rel=5e-5, krylov_rel=1e-7, krylov_iter=1000))
    for N in a.n:
        res["kernels"][str(N)] = kernels(L, N, a.reps)
    big = res["kernels"][str(max(a.n))]["column 24"]
    res["gate"] = dict(n=max(a.n), column=24, two_fused_passes_ms=big["always"]["ms"], mgs_ms=big["mgs"]["ms"], met=bool(big["always"]["ms"] < big["mgs"]["ms"]))
    if not a.no_solves:
        for N in a.n:
            quats = hipref.random_quats(N ** 3, seed=16)
            case = res["solves"][str(N)] = {}
            for kind in ("identity", "jacobi", "multigrid"):
                for solver in ("pcg", "gmres"):
                    case["%s %s" % (solver, kind)] = solve(L, N, solver, kind, dts, props, quats)
                    print("%d %s %s done" % (N, solver, kind), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
