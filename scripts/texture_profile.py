"""Cost of the texture analysis (Driver.pole_figures) on the synthetic FCC Voce RVE at --n (p = 1, one GPU), initial state with
random orientations (a uniform texture: the LDS counters see the least contention), for the default sets: pole figures {111} {200} {220} and
the inverse pole figure of z at --res degrees.
Prints one JSON line: the wall ms of every timed call.  A call is one exa_element_fields launch, exa_texture_volume_max, exa_texture_weights,
the all-reduces (no-ops on one rank), the copy back and the MRD on the host; run it under `rocprofv3 --kernel-trace --stats` for the kernel times.
    python scripts/texture_profile.py --n 128"""
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
    ap.add_argument("--res", type=float, default=5.0)
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
    for _ in range(3):                      # warm-up
        p = d.pole_figures(res_deg=a.res)
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        p = d.pole_figures(res_deg=a.res)
        walls.append((time.perf_counter() - t0) * 1e3)
    d.close()
    m = np.concatenate([p["pf"], p["ipf"]])
    print(json.dumps(dict(N=N, E=E, res_deg=a.res, sets=int(m.shape[0]), mrd_min=round(float(m.min()), 4), mrd_max=round(float(m.max()), 4),
                          wall_ms=[round(w, 3) for w in walls], wall_ms_median=round(float(np.median(walls)), 3))))


if __name__ == "__main__":
    main()
