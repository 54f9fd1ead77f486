"""Cost of the nine fluctuation solves of the homogenised tangent: the batched route at 1, 2, 3 columns per pass over the record
stream against the columns one by one through PCGSolver::Solve, at 64^3 and 128^3 (Voce FCC, one orientation per element, periodic under the velocity
gradient of tests/test_gpu_periodic.py, after one solved step).

A solve is cut off at a fixed iteration count (rel_tol far below reach), once at `--lo` and once at `--hi` iterations; the difference of the two
wall times over 9 (hi - lo) is the time of ONE column-iteration with everything else an evaluation does (gradient set-up, the two raw actions,
the true residuals, the contraction) subtracted out.  Each figure is the median of `--reps` such pairs.  A converged evaluation (the Krylov
options of the run) gives the iteration counts.  Writes profiles/macro_tangent_bench.json.

    python scripts/macro_tangent_bench.py [--sizes 64 128] [--reps 3] [--lo 16] [--hi 80]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
LMAC = np.array([[1.0e-3, 2.0e-4, -1.0e-4], [-3.0e-4, -5.0e-4, 4.0e-4], [5.0e-4, -2.0e-4, -5.0e-4]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lo", type=int, default=16)
    ap.add_argument("--hi", type=int, default=80)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "macro_tangent_bench.json"))
    a = ap.parse_args()
    import torch

    import exaconstit_amd.lib as L
    import hipref
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    dts = np.loadtxt(os.path.join(REF, "custom_dt.txt")).ravel()
    rows = []
    for N in a.sizes:
        d = L.Driver.synthetic(N, props, hipref.random_quats(N ** 3).ravel(), dts[:1], krylov=(2000, 1e-8, 1e-30))
        d.set_periodic(LMAC)
        assert d.step(1)

        def timed(batched, iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mt = d.macro_tangent(rel_tol=1e-30, max_iter=iters, batched=batched)
            torch.cuda.synchronize()
            assert all(int(i) == iters for i in mt["iters"]), mt["iters"]
            return 1e3 * (time.perf_counter() - t0)

        def per_column_iteration(batched):
            timed(batched, a.lo)      # warm-up: allocations, the captured PCG chunk
            v = [(timed(batched, a.hi) - timed(batched, a.lo)) / (9.0 * (a.hi - a.lo)) for _ in range(a.reps)]
            return statistics.median(v), min(v), max(v)

        row = dict(N=N, dofs=int(3 * (N + 1) ** 3), route={})
        for nch in (1, 2, 3):
            d.set_tangent_route(nch, True)
            med, lo, hi = per_column_iteration(True)
            row["route"]["batched_nch%d" % nch] = dict(ms_per_column_iteration=med, min=lo, max=hi)
        med, lo, hi = per_column_iteration(False)
        row["route"]["one_by_one"] = dict(ms_per_column_iteration=med, min=lo, max=hi)
        d.set_tangent_route(0, True)
        for name, batched in (("batched", True), ("one_by_one", False)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            mt = d.macro_tangent(batched=batched)
            torch.cuda.synchronize()
            row["converged_" + name] = dict(ms=1e3 * (time.perf_counter() - t0), iters=[int(i) for i in mt["iters"]], true_rel_max=float(mt["true_rel"].max()), nch=mt["nch"])
        rows.append(row)
        print(json.dumps(row))
        d.close()
    out = dict(what="ms per column-iteration of the nine tangent solves: (wall(hi) - wall(lo)) / (9 (hi - lo)), median of reps", lo=a.lo, hi=a.hi, reps=a.reps,
               device=torch.cuda.get_device_name(0), build_id=L.exa_build_id().decode(), kernel_build_id=L.exa_kernel_build_id().decode(), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
