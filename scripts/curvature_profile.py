"""Cost of the lattice-curvature analysis (Driver.lattice_curvature) on the synthetic FCC Voce RVE at --n (p = 1, one GPU) with
cubic grains of --cube^3 elements (4096 grains at n = 128, cube = 8), on the initial state (the cost does not depend on the values).
  1. the three entry points of the C ABI on the driver-sized problem with hand-built rows, each between device events, --reps calls after 3 warm-up
     calls (exa_curvature_nodal holds two launches, exa_curvature_summary two; run under `rocprofv3 --kernel-trace --stats` for every kernel
     on its own, the element-field launch of the driver calls included), and exa_element_fields - the launch the analysis follows - on a
     context of the driver's kind, timed the same way in the same process;
  2. the wall ms of Driver.lattice_curvature(): the element-field launch, pass 1 of the grain sums, the launches above and the copies back.
Prints one JSON line.
    python scripts/curvature_profile.py --n 128"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hex_mesh(N):
    n1 = N + 1
    e = np.arange(N ** 3, dtype=np.int64)
    ex, ey, ez = e % N, (e // N) % N, e // (N * N)
    off = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    conn = np.stack([(ex + o[0]) + n1 * ((ey + o[1]) + n1 * (ez + o[2])) for o in off], -1).astype(np.int32)
    n = np.arange(n1 ** 3, dtype=np.int64)
    X = np.stack([n % n1, (n // n1) % n1, n // (n1 * n1)], -1).astype(float) / N
    return conn, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--cube", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import exaconstit_amd.lib as L
    N = a.n
    E = N ** 3
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rng = np.random.default_rng(1)
    i = np.arange(E)
    m = N // a.cube
    x, y, z = i % N, (i // N) % N, i // (N * N)
    grain = (1 + (x // a.cube) + m * ((y // a.cube) + m * (z // a.cube))).astype(np.int32)
    G = int(grain.max())
    gq = rng.standard_normal((G, 4))
    gq /= np.linalg.norm(gq, axis=1, keepdims=True)
    dev = torch.device("cuda:0")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())                           # noqa: E731
    # -- 1. the entry points between device events
    conn, X = hex_mesh(N)
    NN = len(X)
    q = gq[grain - 1] + 1e-3 * rng.standard_normal((E, 4))             # a small spread about the grain orientation
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rows = np.zeros((E, L.EXA_NFIELDS))
    rows[:, 0] = 1.0 / E
    rows[:, 27:31] = q
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    d_conn = up(conn.ravel())
    ctx.check(L.exa_set_connectivity(ctx.h, ptr(d_conn), NN))
    work, planes = L.curvature_sizes(E)
    d_rows, d_g, d_qb = up(rows.ravel()), up(grain), up(gq.ravel())
    d_xe = up(X[conn].transpose(0, 2, 1).ravel())
    zeros = lambda k: torch.zeros(int(k), dtype=torch.float64, device=dev)   # noqa: E731
    d_work, d_nodal, d_out, d_sum = zeros(work), zeros(planes * NN), zeros(L.EXA_NCURV * E), zeros(7)
    calls = {
        "exa_curvature_nodal": lambda: L.exa_curvature_nodal(ctx.h, ptr(d_rows), ptr(d_g), G, ptr(d_qb), ptr(d_work), ptr(d_nodal), None),
        "exa_curvature_elements": lambda: L.exa_curvature_elements(ctx.h, ptr(d_rows), ptr(d_g), G, ptr(d_qb), ptr(d_work), ptr(d_nodal), ptr(d_xe), 2.5e-7,
                                                                   ptr(d_out), None),
        "exa_curvature_summary": lambda: L.exa_curvature_summary(ctx.h, ptr(d_rows), ptr(d_out), ptr(d_sum), None),
    }
    ev_ms = {k: [] for k in calls}
    for rep in range(3 + a.reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.check(f())
            e1.record()
            e1.synchronize()
            if rep >= 3:
                ev_ms[k].append(e0.elapsed_time(e1))
    summary = d_sum.cpu().numpy().tolist()
    # the yardstick, in the same process: the element-field launch the analysis follows, on a context of the driver's kind (EB64 layout, det J
    # from the node coordinates) with random stress and state of the same sizes - its time does not depend on the values
    fctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    fctx.check(L.exa_set_quadrature_layout(fctx.h, L.EXA_QLAYOUT_EB64))
    d_s = torch.rand(int(L.exa_qf_size(fctx.h, 6)), dtype=torch.float64, device=dev)
    d_sv = torch.rand(int(L.exa_qf_size(fctx.h, 28)), dtype=torch.float64, device=dev) + 0.5
    d_f = zeros(L.EXA_NFIELDS * E)
    field_ms = []
    for rep in range(3 + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fctx.check(L.exa_element_fields(fctx.h, None, ptr(d_s), ptr(d_sv), ptr(d_xe), ptr(d_f), None))
        e1.record()
        e1.synchronize()
        if rep >= 3:
            field_ms.append(e0.elapsed_time(e1))
    fctx.close()
    del d_s, d_sv, d_f
    ctx.close()
    del d_rows, d_g, d_qb, d_xe, d_work, d_nodal, d_out, d_conn
    torch.cuda.empty_cache()
    # -- 2. the driver call
    quats = rng.standard_normal((E, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    d = L.Driver.synthetic(N, props, quats.ravel(), np.array([0.005]))
    d.set_grains(grain, gq)
    for _ in range(3):                      # warm-up; the first call builds the grain plan and the node -> element table
        c = d.lattice_curvature(burgers=2.5e-7)
    walls = []
    for _ in range(10):
        t0 = time.perf_counter()
        c = d.lattice_curvature(burgers=2.5e-7)
        walls.append((time.perf_counter() - t0) * 1e3)
    d.close()
    med = lambda v: round(float(np.median(v)), 4)   # noqa: E731
    print(json.dumps(dict(N=N, E=E, NN=NN, grains=G, reps=a.reps, event_ms_median={k: med(v) for k, v in ev_ms.items()},
                          event_ms_min={k: round(min(v), 4) for k, v in ev_ms.items()}, element_fields_ms_median=med(field_ms),
                          element_fields_ms_min=round(min(field_ms), 4), abi_summary=summary,
                          driver_wall_ms=[round(w, 3) for w in walls], driver_wall_ms_median=med(walls), driver_grod_max=c["summary"]["GROD_max"])))


if __name__ == "__main__":
    main()
