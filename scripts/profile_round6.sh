#!/bin/bash
# run on the GPU box: the judged evidence set of round 6 -> gpurun_out/r06_*  (scripts/collect_round6.py copies the summaries into profiles/ and REFUSES a record of another
# kernel build).  Every file is produced by ONE library build: each JSON carries library.kernel_build_id, the counter files are stamped with it.
#   1. rocprofv3 --kernel-trace --marker-trace --stats of the default bench command (real-solve state, adapter_route block included): region summary, kernel stats, bench line
#   2. bench records: driver form (--steps 20 --warmup 5), BCC / FCC Kocks-Mecking at 128^3, 64^3 (identity and true Jacobi), 128^3 true Jacobi, config-5 rates
#   3. FETCH_SIZE / WRITE_SIZE passes per crystal model (kinematic state) + the staged AOS launch of the adapter route + the p = 2 kernels -> traffic json
#   4. SQ counters of the constitutive kernels (element-blocked record launch per model, staged AOS launch, p = 2 launch), FP64 instruction counts of the Voce kernel
export EXA_BENCH_FULL=1     # every bench.py run below is the --full one: the blocks and the dispatch sequence it reads come from it
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
T=r06
KID=$(python -c "import exaconstit_amd.lib as L; print(L.exa_kernel_build_id().decode())")
echo "kernel build id $KID" > gpurun_out/${T}_build_id.txt
CMD="env EXA_BENCH_SOLVE_STEPS_TOTAL=14 python bench.py --steps ${STEPS:-100} --warmup 5 --pcg-iters 100 --no-cpu-baseline"
rocprofv3 --kernel-trace --marker-trace --stats --output-format csv -d gpurun_out/${T}_trace -- $CMD > gpurun_out/${T}_trace.log 2>&1
python scripts/region_summary.py gpurun_out/${T}_trace gpurun_out/${T}_region_summary.csv
cp $(ls gpurun_out/${T}_trace/*/*kernel_stats.csv | head -1) gpurun_out/${T}_kernel_stats.csv 2>/dev/null
grep '^{"metric"' gpurun_out/${T}_trace.log > gpurun_out/${T}_bench_under_rocprof.json
rm -rf gpurun_out/${T}_trace/*/*marker* gpurun_out/${T}_trace/*/*kernel_trace.csv 2>/dev/null
# ---- 3. traffic
export EXA_BENCH_SOLVE_STEPS=0
for m in fcc_voce bcc_kmdd fcc_kmdd; do
  for c in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $c --output-format csv -d gpurun_out/${T}_${m}_pmc_$c -- python bench.py --model $m --steps 3 --warmup 1 --pcg-iters 20 --no-cpu-baseline --no-adapter-route > gpurun_out/${T}_${m}_pmc_$c.log 2>&1
  done
done
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --output-format csv -d gpurun_out/${T}_adapter_pmc_$c -- python scripts/adapter_route.py --steps 3 --iters 3 > gpurun_out/${T}_adapter_pmc_$c.log 2>&1
  rocprofv3 --pmc $c --output-format csv -d gpurun_out/${T}_config5_pmc_$c -- python scripts/bench_config5.py 32 > gpurun_out/${T}_config5_pmc_$c.log 2>&1
done
unset EXA_BENCH_SOLVE_STEPS
python - <<PY
import collections, csv, glob, json, statistics
def traffic(tag, key, per=1.0):
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
    return (2 * med[("FETCH_SIZE", k)] + med.get(("WRITE_SIZE", k), 0.0)) * 1024 / (grid[k] * per)
out = {"k_model_setup": {}}
# instantiations of the record launch: 8 = Voce with the exponent 49 compiled in, 7 = athermal-threshold Kocks-Mecking p = q = 1 (BCC), 6 = Kocks-Mecking p = q = 1 (FCC)
for m, key in (("fcc_voce", "k_model_setup<8, true, 8, true, true"), ("bcc_kmdd", "k_model_setup<7, true, 8, true, true"), ("fcc_kmdd", "k_model_setup<6, true, 8, true, true")):
    out["k_model_setup"][m] = traffic("${T}_" + m, key)
t = traffic("${T}_fcc_voce", "k_grad_apply_p1", 8.0)
if t: out["k_grad_apply_p1"] = t      # one thread per element, 8 points
ad = {"k_model_setup_staged_aos_evec": traffic("${T}_adapter", "k_model_setup<8, false, 8, false, false, true"), "k_model_setup_staged_aos_lvec": traffic("${T}_adapter", "k_model_setup<8, true, 8, false, false, true"),
      "k_model_setup_staged_aos_lvec_records": traffic("${T}_adapter", "k_model_setup<8, true, 8, false, true, true"),
      "k_grad_apply_p1_evec_compact_geo": traffic("${T}_adapter", "k_grad_apply_p1<false, false, false, false, true, true", 8.0), "k_grad_setup_pa": traffic("${T}_adapter", "k_grad_setup_pa", 8.0)}
c5 = {"k_model_setup_p2_vg_records": traffic("${T}_config5", "k_model_setup<8, false, 27, true, true"), "k_geom_p2": traffic("${T}_config5", "k_geom_p2", 27.0),
      "k_mf_apply_p2": traffic("${T}_config5", "k_mf_apply_p2", 27.0), "k_residual_p2": traffic("${T}_config5", "k_residual_p2", 27.0)}
json.dump({"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes (scripts/profile_round6.sh), bench.py --solve-steps 0 at 128^3 per kernel instantiation; adapter route: scripts/adapter_route.py at 128^3; config 5: scripts/bench_config5.py at 32^3 p = 2",
           "correction": "gfx950: traffic = 2*FETCH_SIZE*1024 + WRITE_SIZE*1024 (MI355X_MICROARCH.md HBM section); the x2 over-corrects 8-byte strided loads by ~15 %",
           "kernel_build_id": "$KID", "bytes_per_qpt": out, "adapter_route_bytes_per_qpt": ad, "config5_bytes_per_qpt": c5}, open("gpurun_out/${T}_pmc_traffic.json", "w"), indent=1)
print(out, ad, c5)
PY
# ---- 4. SQ counters and FP64 counts
for m in fcc_voce bcc_kmdd fcc_kmdd; do MODEL=$m bash scripts/pmc_model.sh ${T}_sq_$m > gpurun_out/${T}_sq_$m.txt 2>&1; done
bash scripts/pmc_kernel.sh ${T}_sq_adapter "false, 8, false, false, true" python scripts/adapter_route.py --steps 5 --iters 2 > gpurun_out/${T}_sq_adapter_staged.txt 2>&1
for k in "k_model_setup" "k_geom_p2" "k_mf_apply_p2" "k_residual_p2"; do echo "== $k"; bash scripts/pmc_kernel.sh ${T}_sq_c5 "$k" python scripts/bench_config5.py 32 2>&1 | tail -3; done > gpurun_out/${T}_sq_config5.txt 2>&1
bash scripts/pmc_flops.sh ${T} > gpurun_out/${T}_pmc_flops.out 2>&1
python - <<PY
import json
d = json.load(open("gpurun_out/${T}_pmc_flops.json")); d["kernel_build_id"] = "$KID"; json.dump(d, open("gpurun_out/${T}_pmc_flops.json", "w"), indent=1)
PY
# ---- 2. bench records (after the counter passes: bench.py fills roofline.traffic from profiles/*_pmc_traffic.json of THIS kernel build)
unset EXA_BENCH_SOLVE_STEPS
cp gpurun_out/${T}_pmc_traffic.json profiles/${T}_pmc_traffic.json
bash scripts/bench_records_round6.sh
for f in gpurun_out/${T}_sq_*.txt; do sed -i "1i kernel_build_id $KID" $f; done
rm -rf gpurun_out/${T}_*_pmc_FETCH_SIZE gpurun_out/${T}_*_pmc_WRITE_SIZE gpurun_out/${T}_sq_fcc_kmdd gpurun_out/${T}_sq_fcc_voce gpurun_out/${T}_sq_bcc_kmdd gpurun_out/${T}_pmc_flops gpurun_out/${T}_sq_adapter_trace gpurun_out/${T}_sq_c5_trace gpurun_out/${T}_trace 2>/dev/null
cat gpurun_out/${T}_sq_fcc_voce.txt gpurun_out/${T}_sq_bcc_kmdd.txt gpurun_out/${T}_sq_adapter_staged.txt gpurun_out/${T}_sq_config5.txt; tail -1 gpurun_out/${T}_pmc_flops.out; cat gpurun_out/${T}_pmc_traffic.json
