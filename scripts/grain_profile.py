"""Cost of the per-grain averages (Driver.grain_averages) on the synthetic FCC Voce RVE at --n (p = 1, one GPU) for one grain
layout given through Driver.set_grains, on the initial state (the cost does not depend on the values):
  one       one grain of the whole mesh
  cubes     cubic grains of --cube^3 elements (4096 grains at n = 128, cube = 8)
  element   one grain per element
Prints one JSON line: the wall ms of every timed call.  A call is one exa_element_fields launch, both exa_grain_sums passes (all levels), the
all-reduces and the copies back; run it under `rocprofv3 --kernel-trace --stats` for the kernel times.
    python scripts/grain_profile.py --n 128 --layout cubes"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--layout", choices=("one", "cubes", "element"), default="cubes")
    ap.add_argument("--cube", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import exaconstit_amd.lib as L
    N = a.n
    E = N ** 3
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rng = np.random.default_rng(1)
    quats = rng.standard_normal((E, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    d = L.Driver.synthetic(N, props, quats.ravel(), np.array([0.005]))
    i = np.arange(E)
    if a.layout == "one":
        grain = np.ones(E, np.int32)
    elif a.layout == "element":
        grain = (i + 1).astype(np.int32)
    else:
        m = N // a.cube
        x, y, z = i % N, (i // N) % N, i // (N * N)
        grain = (1 + (x // a.cube) + m * ((y // a.cube) + m * (z // a.cube))).astype(np.int32)
    G = int(grain.max())
    gq = rng.standard_normal((G, 4))
    d.set_grains(grain, gq)
    for _ in range(3):                      # warm-up; the first call builds the plan
        g = d.grain_averages()
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        g = d.grain_averages()
        walls.append((time.perf_counter() - t0) * 1e3)
    d.close()
    print(json.dumps(dict(N=N, E=E, layout=a.layout, grains=int(len(g["grain_id"])), wall_ms=[round(w, 3) for w in walls],
                          wall_ms_median=round(float(np.median(walls)), 3))))


if __name__ == "__main__":
    main()
