#!/bin/bash
# run on the GPU box: the judged profile set of round 5 -> gpurun_out/r04_*  (copy the summaries into profiles/ afterwards)
#   1. rocprofv3 --kernel-trace --marker-trace --stats of the default bench command (real-solve state): region summary, kernel stats, bench line
#   2. FETCH_SIZE / WRITE_SIZE passes per crystal model (separate passes, kinematic state: the counters serialise every dispatch) -> per-model
#      traffic json, stamped with the library's kernel build id (bench.py refuses a file of another build)
#   3. SQ counters of the three constitutive kernels, FP64 instruction counts of the Voce kernel (stamped as well)
export EXA_BENCH_FULL=1     # every bench.py run below is the --full one: the blocks and the dispatch sequence it reads come from it
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
T=r05
KID=$(python -c "import exaconstit_amd.lib as L; print(L.exa_kernel_build_id().decode())")
CMD="env EXA_BENCH_SOLVE_STEPS_TOTAL=14 python bench.py --steps ${STEPS:-100} --warmup 5 --pcg-iters 100 --no-cpu-baseline"
rocprofv3 --kernel-trace --marker-trace --stats --output-format csv -d gpurun_out/${T}_trace -- $CMD > gpurun_out/${T}_trace.log 2>&1
python scripts/region_summary.py gpurun_out/${T}_trace gpurun_out/${T}_region_summary.csv
cp $(ls gpurun_out/${T}_trace/*/*kernel_stats.csv | head -1) gpurun_out/${T}_kernel_stats.csv 2>/dev/null
grep '^{"metric"' gpurun_out/${T}_trace.log > gpurun_out/${T}_bench_under_rocprof.json
export EXA_BENCH_SOLVE_STEPS=0
for m in fcc_voce bcc_kmdd fcc_kmdd; do
  for c in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $c --output-format csv -d gpurun_out/${T}_${m}_pmc_$c -- python bench.py --model $m --steps 3 --warmup 1 --pcg-iters 20 --no-cpu-baseline > gpurun_out/${T}_${m}_pmc_$c.log 2>&1
  done
done
python - <<PY
import collections, csv, glob, json, statistics
def traffic(tag, key):
    med = {}; grid = {}
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        vals = collections.defaultdict(list)
        for f in glob.glob(f"gpurun_out/{tag}_pmc_{c}/*/*counter_collection.csv"):
            for r in csv.DictReader(open(f)):
                if r["Counter_Name"] == c and key in r["Kernel_Name"]:
                    vals[r["Kernel_Name"]].append(float(r["Counter_Value"])); grid[r["Kernel_Name"]] = float(r["Grid_Size"])
        for k, v in vals.items():
            v = v[len(v) // 2:]
            hi = [x for x in v if x >= 0.5 * (max(v) + min(v))]      # capped launch and tail launch share a name: the large cluster is the main launch
            med[(c, k)] = statistics.median(hi)
    ks = [k for (c, k) in med if c == "FETCH_SIZE"]
    if not ks:
        return None
    k = max(ks, key=lambda k: grid[k] * 1e12 + med[("FETCH_SIZE", k)])
    return (2 * med[("FETCH_SIZE", k)] + med.get(("WRITE_SIZE", k), 0.0)) * 1024 / grid[k], k
out = {"k_model_setup": {}}
# instantiations: 8 = Voce with the exponent 49 compiled in, 7 = athermal-threshold Kocks-Mecking p = q = 1 (BCC), 6 = Kocks-Mecking p = q = 1 (FCC)
for m, key in (("fcc_voce", "k_model_setup<8"), ("bcc_kmdd", "k_model_setup<7"), ("fcc_kmdd", "k_model_setup<6")):
    t = traffic("${T}_" + m, key); out["k_model_setup"][m] = t[0] if t else None
t = traffic("${T}_fcc_voce", "k_grad_apply_p1")
if t: out["k_grad_apply_p1"] = t[0] / 8.0      # one thread per element, 8 points
json.dump({"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes (scripts/profile_round5.sh), bench.py --solve-steps 0 at 128^3, per kernel instantiation",
           "correction": "gfx950: traffic = 2*FETCH_SIZE*1024 + WRITE_SIZE*1024 (MI355X_MICROARCH.md HBM section); the x2 over-corrects 8-byte strided loads by ~15 %",
           "kernel_build_id": "$KID", "bytes_per_qpt": out}, open("gpurun_out/${T}_pmc_traffic.json", "w"), indent=1)
print(out)
PY
for m in fcc_voce bcc_kmdd fcc_kmdd; do MODEL=$m bash scripts/pmc_model.sh ${T}_sq_$m > gpurun_out/${T}_sq_$m.txt 2>&1; done
bash scripts/pmc_flops.sh ${T} > gpurun_out/${T}_pmc_flops.out 2>&1
python - <<PY
import json
d = json.load(open("gpurun_out/${T}_pmc_flops.json")); d["kernel_build_id"] = "$KID"; json.dump(d, open("gpurun_out/${T}_pmc_flops.json", "w"), indent=1)
PY
rm -rf gpurun_out/${T}_*_pmc_FETCH_SIZE gpurun_out/${T}_*_pmc_WRITE_SIZE gpurun_out/${T}_sq_fcc_kmdd gpurun_out/${T}_sq_fcc_voce gpurun_out/${T}_sq_bcc_kmdd gpurun_out/${T}_pmc_flops gpurun_out/${T}_trace/*/*marker* 2>/dev/null
cat gpurun_out/${T}_sq_fcc_voce.txt gpurun_out/${T}_sq_bcc_kmdd.txt gpurun_out/${T}_sq_fcc_kmdd.txt; tail -1 gpurun_out/${T}_pmc_flops.out; cat gpurun_out/${T}_pmc_traffic.json
