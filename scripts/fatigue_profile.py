"""Cost of the slip-activity accumulators and the FIP evaluation at --n (p = 1, one GPU) with cubic grains of --cube^3 elements
(4096 grains at n = 128, cube = 8), on made-up rows (the cost does not depend on the values).
  1. the entry points of the C ABI between device events, --reps calls after 3 warm-up calls: exa_slip_accumulate without and with the fused
     window reset, exa_fip_rows, exa_fip_summary (two launches; run under `rocprofv3 --kernel-trace --stats` in a run of its own for every kernel),
     and exa_element_fields - the launch the accumulation follows in every committed step - on a context of the driver's kind, timed the same
     way in the same process;
  2. the wall ms of Driver.slip_activity() on the initial state of a synthetic driver: the element-field launch, the launches above, the copies
     back and the per-grain sums on the host.
Prints one JSON line.
    python scripts/fatigue_profile.py --n 128"""
import argparse
import ctypes as C
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
    ap.add_argument("--cube", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-driver", action="store_true", help="part 1 only (the run under the kernel trace)")
    a = ap.parse_args()
    import torch
    import exaconstit_amd.lib as L
    N = a.n
    E = N ** 3
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())                           # noqa: E731
    zeros = lambda k: torch.zeros(int(k), dtype=torch.float64, device=dev)   # noqa: E731
    # -- 1. the entry points between device events
    rows = rng.standard_normal((E, L.EXA_NFIELDS))
    rows[:, 0] = 1.0 / E
    rows[:, 15:27] *= 1e-3
    rows[:, 27:31] /= np.linalg.norm(rows[:, 27:31], axis=1, keepdims=True)
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    d_rows = up(rows.ravel())
    del rows
    d_acc, d_fip, d_sum = zeros(L.slip_activity_sizes(E)), zeros(L.EXA_NFIP * E), zeros(7)
    d_gid = up(np.arange(E, dtype=np.int64))
    nrm = L.slip_plane_normals(L.EXA_FCC_VOCE)
    pn = nrm.ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "exa_slip_accumulate": lambda: L.exa_slip_accumulate(ctx.h, ptr(d_rows), pn, 0.1, 0, ptr(d_acc), None),
        "exa_slip_accumulate_reset": lambda: L.exa_slip_accumulate(ctx.h, ptr(d_rows), pn, 0.1, 1, ptr(d_acc), None),
        "exa_fip_rows": lambda: L.exa_fip_rows(ctx.h, ptr(d_acc), 0.5, 100.0, ptr(d_fip), None),
        "exa_fip_summary": lambda: L.exa_fip_summary(ctx.h, ptr(d_rows), ptr(d_fip), ptr(d_gid), ptr(d_sum), None),
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
    # the yardstick, in the same process: the element-field launch on a context of the driver's kind (EB64 layout, det J from the node coordinates)
    fctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    fctx.check(L.exa_set_quadrature_layout(fctx.h, L.EXA_QLAYOUT_EB64))
    d_s = torch.rand(int(L.exa_qf_size(fctx.h, 6)), dtype=torch.float64, device=dev)
    d_sv = torch.rand(int(L.exa_qf_size(fctx.h, 28)), dtype=torch.float64, device=dev) + 0.5
    d_xe = torch.rand(24 * E, dtype=torch.float64, device=dev)
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
    ctx.close()
    del d_s, d_sv, d_f, d_xe, d_rows, d_acc, d_fip, d_gid
    torch.cuda.empty_cache()
    med = lambda v: round(float(np.median(v)), 4)   # noqa: E731
    out = dict(N=N, E=E, reps=a.reps, build_id=L.exa_build_id().decode(), event_ms_median={k: med(v) for k, v in ev_ms.items()},
               event_ms_min={k: round(min(v), 4) for k, v in ev_ms.items()}, element_fields_ms_median=med(field_ms),
               element_fields_ms_min=round(min(field_ms), 4), abi_summary=summary,
               accumulate_over_element_fields=round(float(np.median(ev_ms["exa_slip_accumulate"]) / np.median(field_ms)), 3),
               accumulate_line_bytes=int(E * (L.EXA_NFIELDS * 8 + 2 * L.EXA_NSLIPACC * 8)))
    out["accumulate_TB_per_s"] = round(out["accumulate_line_bytes"] / (np.median(ev_ms["exa_slip_accumulate"]) * 1e-3) / 1e12, 3)
    # -- 2. the driver call
    if not a.no_driver:
        i = np.arange(E)
        m = N // a.cube
        x, y, z = i % N, (i // N) % N, i // (N * N)
        grain = (1 + (x // a.cube) + m * ((y // a.cube) + m * (z // a.cube))).astype(np.int32)
        G = int(grain.max())
        gq = rng.standard_normal((G, 4))
        gq /= np.linalg.norm(gq, axis=1, keepdims=True)
        quats = rng.standard_normal((E, 4))
        quats /= np.linalg.norm(quats, axis=1, keepdims=True)
        d = L.Driver.synthetic(N, props, quats.ravel(), np.array([0.005]))
        d.set_grains(grain, gq)
        d.enable_slip_activity()
        for _ in range(2):
            c = d.slip_activity(sigma_y=100.0)
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            c = d.slip_activity(sigma_y=100.0)
            walls.append((time.perf_counter() - t0) * 1e3)
        d.close()
        out.update(grains=G, driver_wall_ms=[round(w, 3) for w in walls], driver_wall_ms_median=med(walls), driver_grains=len(c["grains"]["grain_id"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
