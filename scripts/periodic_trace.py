#!/usr/bin/env python
"""Launch budget of periodic boundary conditions, asserted on the GPU: a kernel trace (rocprofv3 --kernel-trace --stats, in a run of its own)
of a fixed-length periodic PCG solve at 16^3 on one rank must show five launches per iteration - the four of the one-rank loop plus
k_periodic_sum - and k_periodic_sum must have no private segment, in the trace and in the loaded code object.  Writes the figures to
profiles/periodic_trace.txt; exits non-zero when an assertion fails.

    python scripts/periodic_trace.py [--iters 320] [--out profiles/periodic_trace.txt]
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def child(iters):
    """the traced program: plain stream launches (no graph replay), one solve of exactly `iters` iterations"""
    import numpy as np
    import exaconstit_amd.lib as L
    from periodic_compare import LMAC, PREP_DTS
    N = 16
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    rng = np.random.default_rng(1)
    q = rng.standard_normal((N ** 3, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    d = L.Driver.synthetic(N, props, q.ravel(), np.array(PREP_DTS), krylov=(1000, 1e-7, 1e-27))
    d.set_periodic(LMAC)
    d.bench_prepare(PREP_DTS)
    pc = d.bench_pcg(iters)
    print("child: iterations", pc["iters"], "groups", d.periodic_info()["groups"], "scratch_bytes", L.exa_periodic_sum_scratch_bytes(),
          "build", L.exa_build_id().decode(), L.exa_kernel_build_id().decode())
    assert pc["iters"] == iters
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_trace.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.iters)
    tmp = tempfile.mkdtemp(prefix="periodic_trace_")
    env = dict(os.environ, EXA_PCG_GRAPH="0")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "pcg", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    tail = [ln for ln in r.stdout.splitlines() if ln.startswith("child:")]
    if r.returncode != 0 or not tail:
        print(r.stdout[-3000:])
        raise SystemExit("the traced run failed (exit %d)" % r.returncode)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written under " + tmp
    rows = list(csv.DictReader(open(files[0])))
    short = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0].strip()      # noqa: E731
    calls = Counter(short(r_["Kernel_Name"]) for r_ in rows)
    K = args.iters
    print("kernel calls:", dict(calls))
    step1 = [k for k in calls if k.startswith("k_cg_step1")]
    assert len(step1) == 1 and calls[step1[0]] == K, (step1, [calls[k] for k in step1])
    per_iter = sorted(k for k, c in calls.items() if c >= K)
    psum = [k for k in calls if k.startswith("k_periodic_sum")]
    col = "Scratch_Size" if "Scratch_Size" in rows[0] else "Private_Segment_Size"
    scratch = sorted({int(r_[col]) for r_ in rows if short(r_["Kernel_Name"]).startswith("k_periodic_sum")})
    lines = ["kernel trace of one periodic PCG solve, 16^3 elements, one rank, %d iterations, stream launches (rocprofv3 --kernel-trace --stats)" % K,
             tail[-1],
             "kernels launched at least once per iteration (%d): %s" % (len(per_iter), ", ".join("%s x %d" % (k, calls[k]) for k in per_iter)),
             "  (the action kernel also runs once before the loop and %d times in the bench's back-to-back action timing; k_periodic_sum also follows the" % K,
             "   residual and the first action)",
             "k_periodic_sum: %d launches, %s of its dispatches: %s" % (calls[psum[0]] if psum else 0, col, scratch),
             "launches per iteration: %d" % len(per_iter)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    assert len(psum) == 1 and K <= calls[psum[0]] <= K + 4, calls
    assert len(per_iter) == 5 and psum[0] in per_iter, per_iter
    assert scratch == [0], scratch
    assert "scratch_bytes 0 " in tail[-1], tail[-1]
    print("ok: five launches per iteration, k_periodic_sum without scratch")


if __name__ == "__main__":
    main()
