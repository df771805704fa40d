#!/bin/bash
# Round-6 round-end evidence (run on the GPU box: gpurun -- 'bash tools/r6_final.sh'): the GPU test suite, rocprofv3 kernel stats of the bench configs (each under its own
# timeout) WITH the per-dispatch trace filtered to full decode steps (the pin-model launches of bench.py's correctness gate carry the same kernel name: VERDICT r5 weak 11),
# a separate PMC pass (FETCH_SIZE only, no tracing) for roofline.traffic, phase stamps of the final kernel, the default bench line at --steps 50 and --steps 200.
# Results: gpurun_out/final/ -> copy to profiles/.
TAG=r06
R=${GRAFT_REPO_ROOT:-/root/repo}; O=$R/gpurun_out/final; mkdir -p $O
cd $R
if [ "${1:-all}" != "noprof" ]; then
timeout 1500 python -m pytest tests -q -m gpu -x 2>&1 | tail -5 > $O/${TAG}_gpu_tests.txt; cat $O/${TAG}_gpu_tests.txt
fi
cd /tmp && export TMPDIR=/tmp
run() { # name, bench args...
  n=$1; shift
  timeout 400 rocprofv3 --kernel-trace --stats -d $O/$n -o out --output-format csv -- python $R/bench.py --no-extra --no-cpu "$@" > $O/${TAG}_bench_${n}_under_rocprof.json 2> $O/$n.err
  cp $O/$n/out_kernel_stats.csv $O/${TAG}_bench_${n}_kernel_stats.csv 2>/dev/null
  python3 - <<PY
import csv, glob, json
rows = []
for f in glob.glob("$O/$n/*kernel_trace.csv"): rows += list(csv.DictReader(open(f)))
ps = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "exl3_pstep_kernel" in r.get("Kernel_Name", "")]
if ps:
    import statistics
    big = [d for d in ps if d > 0.5 * max(ps)]          # full decode steps (the pin model of the correctness gate is one layer: ~ 70 us)
    json.dump({"kernel": "exl3_pstep_kernel", "dispatches": len(ps), "full_step_dispatches": len(big), "full_step_avg_us": round(sum(big) / len(big), 2),
               "full_step_median_us": round(statistics.median(big), 2), "pin_model_dispatches": len(ps) - len(big),
               "note": "per-dispatch durations of the kernel trace; full steps = dispatches longer than half the longest (the one-layer pin model of bench.py's logits gate runs the same kernel)"},
              open("$O/${TAG}_bench_${n}_pstep_full_steps.json", "w"), indent=1)
    print("$n: pstep full steps", len(big), "avg us", round(sum(big) / len(big), 2))
PY
  rm -rf $O/$n
}
run bs1 --no-prefill --steps 50
run bs1_launch_per_op --pipeline fx --no-prefill --steps 20
run 1b_persistent --model llama-3.2-1b --no-prefill --steps 50
run bs1_attention --attention --no-prefill --steps 20
run bs1_3inst --codebook 3inst --no-prefill --steps 20
run prefill --steps 5 --full
# PMC passes: eager launches (one dispatch record per kernel), FETCH_SIZE in KiB, x2 on gfx950 for wide coalesced reads (MI355X_MICROARCH.md)
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc -o out --output-format csv -- python $R/bench.py --no-extra --no-cpu --no-prefill --steps 3 --warmup 1 --no-graph --pipeline fx > $O/pmc.log 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_p8 -o out --output-format csv -- python $R/bench.py --no-extra --no-cpu --no-prefill --steps 3 --warmup 1 --no-graph > $O/pmc_p8.log 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_p1 -o out --output-format csv -- python $R/bench.py --no-extra --no-cpu --no-prefill --steps 3 --warmup 1 --no-graph --model llama-3.2-1b > $O/pmc_p1.log 2>&1
python3 - <<PY
import csv, glob, json
def rows_of(d):
    rows = []
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    return rows
rows = rows_of("$O/pmc")
g = [r for r in rows if ("exl3_gemv4_kernel" in r.get("Kernel_Name", "") or "exl3_gemv2_kernel" in r.get("Kernel_Name", "")) and r.get("Counter_Name") == "FETCH_SIZE"]
out = {}
if g:
    per = sum(float(r["Counter_Value"]) for r in g) / len(g) * 1024 * 2
    ko = None
    try:
        kr = [r for r in csv.DictReader(open("$O/${TAG}_bench_bs1_launch_per_op_kernel_stats.csv")) if "exl3_gemv4_kernel" in r["Name"] or "exl3_gemv2_kernel" in r["Name"]]
        calls = sum(int(r["Calls"]) for r in kr); tot = sum(float(r["TotalDurationNs"]) for r in kr)
        ko = {"avg_launch_us": round(tot / calls / 1e3, 3), "calls": calls, "source": "profiles/${TAG}_bench_bs1_launch_per_op_kernel_stats.csv"}
    except Exception as e:
        print("kernel-only figure unavailable:", e)
    out = {"kernel": "exl3_gemv4_kernel<4,2,1,*> (all GEMV launches of the decode step, Llama-3.1-8B 4bpw mul1, bs=1, fx pipeline)", "fetch_bytes_per_launch": int(per),
           "launches_sampled": len(g), "collected": "${TAG}, tools/r6_final.sh", "kernel_only": ko, "method": "rocprofv3 --pmc FETCH_SIZE (own pass, no tracing) on bench.py --steps 3 --warmup 1 --no-graph; FETCH_SIZE is KiB and reads 1/2 of a wide coalesced stream on gfx950 (MI355X_MICROARCH.md, HBM section): x1024 x2 applied; average over all GEMV dispatches (includes the activation / residual-accumulator reads and scale vectors)"}
    print("traffic bytes/launch", int(per), "over", len(g))
else:
    print("no PMC rows (fx)", len(rows))
ps = {}
for model, d in (("llama-3.1-8b", "$O/pmc_p8"), ("llama-3.2-1b", "$O/pmc_p1")):
    r_ = [r for r in rows_of(d) if "exl3_pstep_kernel" in r.get("Kernel_Name", "") and r.get("Counter_Name") == "FETCH_SIZE"]
    if r_:
        vals = sorted(float(r["Counter_Value"]) for r in r_)
        big = [v for v in vals if v > 0.5 * vals[-1]]          # full steps only (the pin model's launches fetch one layer)
        per = sum(big) / len(big) * 1024 * 2
        ps[model] = {"fetch_bytes_per_launch": int(per), "launches_sampled": len(big), "collected": "${TAG}, tools/r6_final.sh",
                     "method": "rocprofv3 --pmc FETCH_SIZE (own pass) on bench.py --no-graph --steps 3 --warmup 1; x1024 x2 as above; one dispatch = one decode step (full steps only: the one-layer pin-model launches of the logits gate are excluded)"}
        print("persistent step", model, "fetch bytes / launch", int(per), "over", len(big))
    else:
        print("no PMC rows for the persistent step", model)
out["persistent_step"] = ps
json.dump(out, open("$O/traffic.json", "w"), indent=1)
PY
rm -rf $O/pmc $O/pmc_p8 $O/pmc_p1
cd $R
# phase stamps of the final kernel (C++ harness)
export LD_LIBRARY_PATH=$R/exllamav3_amd:$LD_LIBRARY_PATH
H_SPIN_LIMIT=20000 timeout 90 tools/bin/pstep_harness 1b 0 1 "3" $O/s_1b.bin 2>&1 | grep -o '"best".*' | cut -c1-220
H_SPIN_LIMIT=20000 timeout 90 tools/bin/pstep_harness 8b 0 1 "3" $O/s_8b.bin 2>&1 | grep -o '"best".*' | cut -c1-220
python3 tools/pstep_stamps.py $O/s_1b.bin 16 $O/${TAG}_stamps_1b.json > $O/${TAG}_stamps_1b.txt; python3 tools/pstep_stamps.py $O/s_8b.bin 32 $O/${TAG}_stamps_8b.json > $O/${TAG}_stamps_8b.txt
python3 tools/pstep_stragglers.py $O/s_8b.bin 32 > $O/${TAG}_stragglers_8b.txt; rm -f $O/s_1b.bin $O/s_8b.bin
for r in 1 2 3; do for m in 8b 1b; do H_SPIN_LIMIT=20000 timeout 120 tools/bin/pstep_harness $m 0 2 "3" 2>/dev/null | grep -o '"best".*' | cut -c1-220; done; done > $O/${TAG}_harness_final.txt
timeout 600 python bench.py --full > $O/${TAG}_bench_final.json 2> $O/final.err; tail -c 300 $O/final.err
timeout 300 python bench.py --no-extra --no-cpu --no-prefill --steps 200 --warmup 20 > $O/${TAG}_bench_steps200.json 2>> $O/final.err
STEP=persistent timeout 300 python tools/bench_decode_ctx.py > $O/${TAG}_decode_ctx.txt 2>&1
ls $O; for f in $O/${TAG}_bench_*_under_rocprof.json $O/${TAG}_bench_final.json $O/${TAG}_bench_steps200.json; do echo $f; grep "^{" $f | cut -c1-200; done
