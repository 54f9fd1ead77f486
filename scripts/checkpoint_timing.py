#!/usr/bin/env python3
"""What a checkpoint costs next to a step: for N^3 synthetic FCC-Voce RVEs on one GPU
  - device time of exa_qf_pack / exa_qf_unpack of the state (28) and stress (6) fields in the driver's element-blocked layout (hip events),
  - wall time of Driver.save_checkpoint and Driver.load_checkpoint (file in a scratch directory, removed afterwards),
  - wall time of the load steps of the same run.
usage: checkpoint_timing.py [--sizes 64 128] [--steps 3] [--out profiles/checkpoint_timing.json] [--dir /tmp]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DTS = [0.005, 0.195, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]   # the first steps of the reference schedule (bench.py)


def pack_times(L, torch, props, N, reps=5):
    E = N ** 3
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, 1, E)
    ctx.check(L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64))
    out = {}
    cks = torch.zeros(1, dtype=torch.int64, device="cuda")
    for W in (28, 6):
        src = torch.rand(int(L.exa_qf_size(ctx.h, W)), dtype=torch.float64, device="cuda")
        can = torch.empty(W * 8 * E, dtype=torch.float64, device="cuda")
        for name, fn, a, b in (("pack", L.exa_qf_pack, src, can), ("unpack", L.exa_qf_unpack, can, src)):
            times = []
            for _ in range(reps + 1):      # the first launch loads the code object
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(fn(ctx.h, W, a.data_ptr(), b.data_ptr(), cks.data_ptr(), None))
                e1.record(); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            best = min(times[1:])
            gb = 2 * 8.0 * W * 8 * E / 1e9
            out["%s_%d" % (name, W)] = {"ms": best, "GB_moved": gb, "TB_per_s": gb / best}
        del src, can
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_timing.json"))
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    import torch
    import exaconstit_amd.lib as L
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rows = []
    for N in args.sizes:
        row = {"N": N, "elements": N ** 3, "points": 8 * N ** 3}
        row["kernels"] = pack_times(L, torch, props, N)
        rng = np.random.default_rng(20240928)
        quats = rng.standard_normal((N ** 3, 4)); quats /= np.linalg.norm(quats, axis=1, keepdims=True)
        d = L.Driver.synthetic(N, props, quats.ravel(), np.array(DTS[:args.steps + 1]))
        walls = []
        for ti in range(1, args.steps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            assert d.step(ti)
            torch.cuda.synchronize(); walls.append(time.perf_counter() - t0)
        row["step_wall_s"] = walls
        tmp = tempfile.mkdtemp(dir=args.dir)
        try:
            path = os.path.join(tmp, "t.ckpt")
            saves = []
            for _ in range(2):
                t0 = time.perf_counter(); d.save_checkpoint(path); saves.append(time.perf_counter() - t0)
            row["save_wall_s"] = saves
            row["file_GB"] = os.path.getsize(path) / 1e9
            d.close()
            d = L.Driver.synthetic(N, props, quats.ravel(), np.array(DTS[:args.steps + 1]))
            t0 = time.perf_counter(); d.load_checkpoint(path); row["load_wall_s"] = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            assert d.step(args.steps + 1)
            torch.cuda.synchronize(); row["step_after_load_wall_s"] = time.perf_counter() - t0
            d.close()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"build_id": L.exa_build_id().decode(), "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
