#!/bin/bash
# run on the GPU box: the judged profile set of round 3 -> gpurun_out/r03_*  (copy the summaries into profiles/ afterwards)
#   1. scripts/profile_round.sh r03: kernel + marker trace of the default bench command, region summary, FETCH/WRITE passes (fcc_voce)
#   2. FETCH/WRITE passes of the BCC Kocks-Mecking launch (BASELINE config 3) -> per-model traffic json
#   3. SQ counters of both constitutive kernels, FP64 instruction counts of the Voce kernel
export EXA_BENCH_FULL=1     # every bench.py run below is the --full one: the blocks and the dispatch sequence it reads come from it
cd $GRAFT_REPO_ROOT
STEPS=${STEPS:-100} bash scripts/profile_round.sh r03
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --output-format csv -d gpurun_out/r03km_pmc_$c -- python bench.py --model bcc_kmdd --steps 3 --warmup 1 --pcg-iters 10 --no-cpu-baseline > gpurun_out/r03km_pmc_$c.log 2>&1
  rocprofv3 --pmc $c --output-format csv -d gpurun_out/r03kf_pmc_$c -- python bench.py --model fcc_kmdd --steps 3 --warmup 1 --pcg-iters 10 --no-cpu-baseline > gpurun_out/r03kf_pmc_$c.log 2>&1
done
python - <<'PY'
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
            # a capped launch and its tail launch share the kernel name (Kocks-Mecking): keep the cluster of the large values = the main launch
            hi = [x for x in v if x >= 0.5 * (max(v) + min(v))]
            med[(c, k)] = statistics.median(hi)
    ks = [k for (c, k) in med if c == "FETCH_SIZE"]
    if not ks:
        return None
    k = max(ks, key=lambda k: grid[k] * 1e12 + med[("FETCH_SIZE", k)])      # the full-size launch, not the tail launch
    return (2 * med[("FETCH_SIZE", k)] + med.get(("WRITE_SIZE", k), 0.0)) * 1024 / grid[k], k
out = {"k_model_setup": {}}
t = traffic("r03", "k_model_setup<0");   out["k_model_setup"]["fcc_voce"] = t[0] if t else None
# Kocks-Mecking sets with p = q = 1 run the KIN_PQ1 instantiations (ecm_device.hpp): 7 = athermal-threshold (BCC), 6 = FCC
t = traffic("r03km", "k_model_setup<7"); out["k_model_setup"]["bcc_kmdd"] = t[0] if t else None
t = traffic("r03kf", "k_model_setup<6"); out["k_model_setup"]["fcc_kmdd"] = t[0] if t else None
t = traffic("r03", "k_grad_apply_p1")
if t: out["k_grad_apply_p1"] = t[0] / 8.0      # one thread per element, 8 points
json.dump({"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes (scripts/profile_round3.sh), bench.py at 128^3, per kernel instantiation",
           "correction": "gfx950: traffic = 2*FETCH_SIZE*1024 + WRITE_SIZE*1024 (MI355X_MICROARCH.md HBM section); the x2 over-corrects 8-byte strided loads by ~15 %",
           "bytes_per_qpt": out}, open("gpurun_out/r03_pmc_traffic.json", "w"), indent=1)
print(out)
PY
MODEL=fcc_voce bash scripts/pmc_model.sh r03_sq_fcc_voce > gpurun_out/r03_sq_fcc_voce.txt 2>&1
MODEL=bcc_kmdd bash scripts/pmc_model.sh r03_sq_bcc_kmdd > gpurun_out/r03_sq_bcc_kmdd.txt 2>&1
MODEL=fcc_kmdd bash scripts/pmc_model.sh r03_sq_fcc_kmdd > gpurun_out/r03_sq_fcc_kmdd.txt 2>&1
bash scripts/pmc_flops.sh r03 > gpurun_out/r03_pmc_flops.out 2>&1
rm -rf gpurun_out/r03_pmc_FETCH_SIZE gpurun_out/r03_pmc_WRITE_SIZE gpurun_out/r03km_pmc_FETCH_SIZE gpurun_out/r03km_pmc_WRITE_SIZE gpurun_out/r03kf_pmc_FETCH_SIZE gpurun_out/r03kf_pmc_WRITE_SIZE gpurun_out/r03_sq_fcc_kmdd gpurun_out/r03_sq_fcc_voce gpurun_out/r03_sq_bcc_kmdd gpurun_out/r03_pmc_flops
cat gpurun_out/r03_sq_fcc_voce.txt gpurun_out/r03_sq_bcc_kmdd.txt gpurun_out/r03_sq_fcc_kmdd.txt; tail -1 gpurun_out/r03_pmc_flops.out
