#!/usr/bin/env python
"""Cost of periodic boundary conditions in a PCG iteration on one GPU: fixed-length PCG (Driver.bench_pcg) on the kinematically driven
plastic state of bench.py, with the face conditions and after Driver.set_periodic, at 16^3, 64^3 and 128^3 elements (p = 1, partial assembly,
Voce FCC).  A periodic action is followed by one more launch (k_periodic_sum over the surface dofs), so the difference should be a few
microseconds per iteration, visible where the iteration itself is short.  Not a gate: writes profiles/periodic_pcg.json with the library's
kernel_build_id.

    python scripts/periodic_compare.py [--sizes 16 64 128] [--iters 200] [--reps 3] [--out profiles/periodic_pcg.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PREP_DTS = [0.005, 0.195, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]      # the schedule bench.py drives the state with
LMAC = np.array([[1.0e-3, 2.0e-4, -1.0e-4], [-3.0e-4, -5.0e-4, 4.0e-4], [5.0e-4, -2.0e-4, -5.0e-4]])


def measure(L, N, props, periodic, iters, reps):
    rng = np.random.default_rng(20240928)
    quats = rng.standard_normal((N ** 3, 4)); quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    d = L.Driver.synthetic(N, props, quats.ravel(), np.array(PREP_DTS), krylov=(1000, 1e-7, 1e-27))
    if periodic:
        d.set_periodic(LMAC)
    d.bench_prepare(PREP_DTS)
    d.bench_pcg(max(2, iters // 10))
    us = []
    for _ in range(reps):
        pc = d.bench_pcg(iters)
        us.append(1e3 * pc["pcg_ms"] / max(pc["iters"], 1))
    info = d.periodic_info()
    d.close()
    return dict(us_per_iter=sorted(us), median_us=float(np.median(us)), groups=info["groups"] if periodic else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_pcg.json"))
    args = ap.parse_args()
    import exaconstit_amd.lib as L
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rows = []
    for N in args.sizes:
        a = measure(L, N, props, False, args.iters, args.reps)
        b = measure(L, N, props, True, args.iters, args.reps)
        rows.append(dict(N=N, elements=N ** 3, surface_dofs_summed=3 * sum(k * v for k, v in b["groups"].items()), face_conditions=a, periodic=b,
                         extra_us_per_iter=b["median_us"] - a["median_us"]))
        print("N = %3d: %.2f us / iteration with the face conditions, %.2f us periodic (%+.2f us)" % (N, a["median_us"], b["median_us"], rows[-1]["extra_us_per_iter"]))
    out = dict(what="fixed-length PCG on one GPU, p = 1 partial assembly, FCC Voce, kinematically driven plastic state; median of %d repetitions of %d iterations"
                    % (args.reps, args.iters), kernel_build_id=L.exa_kernel_build_id().decode(), build_id=L.exa_build_id().decode(),
               ids="kernel_build_id covers the PCG and action kernels (the counter passes' translation units); periodic_kernels.hip is covered by build_id",
               sizes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
