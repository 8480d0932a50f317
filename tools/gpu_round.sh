#!/bin/bash
# One gpurun call of the round: GPU tests, then the bench lines (default config =
# the judged one, then configs 2/3).  Usage: tools/gpu_round.sh <tag> [what...]
set -u
TAG="${1:-r02a}"; shift || true
WHAT="${*:-tests bench bench23}"
OUT="gpurun_out/$TAG"; mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
    tests)   timeout 900 python -m pytest tests -m gpu -x -q --timeout 300 -o faulthandler_timeout=240 > "$OUT/pytest.log" 2>&1; echo "pytest rc=$?" | tee -a "$OUT/pytest.log"; tail -15 "$OUT/pytest.log";;
    bench)   timeout 900 python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_iqn_lstm.json" 2> "$OUT/bench_iqn_lstm.err"; echo "bench rc=$?"; tail -c 1500 "$OUT/bench_iqn_lstm.err"; head -c 6000 "$OUT/bench_iqn_lstm.json";;
    bench23) for c in rainbow_iqn dqn_uniform; do timeout 600 python bench.py --full --config $c --steps 50 --warmup 10 > "$OUT/bench_$c.json" 2> "$OUT/bench_$c.err"; echo "bench $c rc=$?"; tail -c 800 "$OUT/bench_$c.err"; head -c 5000 "$OUT/bench_$c.json"; done;;
    ctests)  timeout 600 python -m pytest tests/test_conv_in_gpu.py tests/test_fused_gpu.py tests/test_models_gpu.py -x -q --timeout 300 > "$OUT/pytest_conv.log" 2>&1; echo "pytest conv rc=$?"; tail -25 "$OUT/pytest_conv.log";;
    cprobe)  timeout 300 python tools/conv_in_probe.py > "$OUT/conv_in_probe.jsonl" 2> "$OUT/conv_in_probe.err"; echo "cprobe rc=$?"; cat "$OUT/conv_in_probe.jsonl"; tail -3 "$OUT/conv_in_probe.err";;
    benchq)  timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/bench_quick.json" 2> "$OUT/bench_quick.err"; echo "benchq rc=$?"; tail -c 600 "$OUT/bench_quick.err"; python - "$OUT/bench_quick.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("ms/step", d["ms_per_step"], d["step_ms"], "value", d["value"])
for k in d["roofline_all"]["kernels"][:12]:
    print(k["kernel"], k["launches_per_step"], k["avg_us"], k["ms_per_step"], k["frac_of_hbm_peak"])
PY
    ;;
    cpmc)    R="$(pwd)"; export TMPDIR=/tmp
             (cd /tmp && timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d "$R/$OUT/cpmc" -o c -- python "$R/tools/conv_in_probe.py" all 42496 > "$R/$OUT/cpmc_probe.jsonl" 2> "$R/$OUT/cpmc_probe.err"); echo "cpmc rc=$?"
             python - "$OUT" <<'PY'
import csv, glob, os, sys, collections, json
out = sys.argv[1]
f = glob.glob(os.path.join(out, "cpmc", "**", "*counter_collection.csv"), recursive=True)
if not f:
    print("no counter csv"); print(open(os.path.join(out, "cpmc_probe.err")).read()[-1500:]); sys.exit(0)
acc = collections.defaultdict(lambda: collections.defaultdict(float)); calls = collections.Counter(); dur = collections.Counter(); seen = set()
for r in csv.DictReader(open(f[0])):
    n = r["Kernel_Name"]
    if not ("conv" in n.lower() or "igemm" in n): continue
    n = n.split("(")[0][:70]
    acc[n][r["Counter_Name"]] += float(r["Counter_Value"])
    if r["Dispatch_Id"] not in seen:
        seen.add(r["Dispatch_Id"]); calls[n] += 1; dur[n] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
res = {}
for n, c in acc.items():
    mf, gui = c.get("SQ_VALU_MFMA_BUSY_CYCLES", 0), c.get("GRBM_GUI_ACTIVE", 0)
    res[n] = {"dispatches": calls[n], "avg_ms_under_counters": round(dur[n] / max(calls[n], 1), 4), "SQ_VALU_MFMA_BUSY_CYCLES": mf,
              "SQ_BUSY_CYCLES": c.get("SQ_BUSY_CYCLES", 0), "GRBM_GUI_ACTIVE": gui, "mfma_busy_per_gui_active_cycle": round(mf / gui, 2) if gui else None}
print(json.dumps(res, indent=1)); json.dump(res, open(os.path.join(out, "conv_mfma_util.json"), "w"), indent=1)
PY
             find "$OUT/cpmc" -name "*.csv" -size +1M -delete; find "$OUT/cpmc" -name "*.db" -delete;;
    probe)   timeout 300 python tools/convert_probe.py > "$OUT/convert_probe.jsonl" 2> "$OUT/convert_probe.err"; echo "probe rc=$?"; cat "$OUT/convert_probe.jsonl"; tail -3 "$OUT/convert_probe.err";;
    prof)    R="$(pwd)"; export TMPDIR=/tmp; (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/stats" -o bench -- python "$R/bench.py" --steps 5 --warmup 2 --no-cpu-baseline --profile-steps 0 > "$R/$OUT/bench_under_rocprof.json" 2> "$R/$OUT/bench_under_rocprof.err"); echo "prof rc=$?"; python tools/summarize_prof.py "$OUT" > "$OUT/summary.txt" 2>&1; head -60 "$OUT/summary.txt"; find "$OUT" -name "*kernel_trace.csv" -delete; find "$OUT" -name "*.db" -delete;;
    gprobe)  for nt in 1 2; do PROBE_SIZE=1000000 PROBE_NT=$nt PROBE_ITERS=10 timeout 300 python tools/gather_probe.py >> "$OUT/gather_probe.jsonl" 2>> "$OUT/gather_probe.err"; done; echo "gprobe rc=$?"; cat "$OUT/gather_probe.jsonl";;
    overlap) timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --train-arg overlap_acting=true > "$OUT/bench_overlap.json" 2> "$OUT/bench_overlap.err"; echo "overlap rc=$?"; tail -c 600 "$OUT/bench_overlap.err"; head -c 1500 "$OUT/bench_overlap.json"; echo;;
    dedup)   timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --frame-dedup > "$OUT/bench_dedup.json" 2> "$OUT/bench_dedup.err"; echo "dedup rc=$?"; tail -c 600 "$OUT/bench_dedup.err"; head -c 2500 "$OUT/bench_dedup.json"; echo;;
    tests1)  timeout 600 python -m pytest tests/test_multirank_gpu.py -x -q --timeout 300 -o faulthandler_timeout=240 > "$OUT/pytest_multirank.log" 2>&1; echo "pytest multirank rc=$?"; tail -40 "$OUT/pytest_multirank.log";;
    find)    timeout 900 python bench.py --steps 10 --warmup 3 --no-cpu-baseline --profile-steps 0 --miopen-find > "$OUT/bench_miopen_find.json" 2> "$OUT/bench_miopen_find.err"; echo "find rc=$?"; tail -c 400 "$OUT/bench_miopen_find.err"; head -c 700 "$OUT/bench_miopen_find.json"; echo;;
    actprobe) R="$(pwd)"; export TMPDIR=/tmp; (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/act_stats" -o act -- python "$R/tools/acting_probe.py" 200 > "$R/$OUT/acting_probe.json" 2> "$R/$OUT/acting_probe.err"); echo "actprobe rc=$?"; cat "$OUT/acting_probe.json"; python - "$OUT" <<'PY'
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/act_stats/**/*kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(f[0]))) if f else []
steps = 230.0
print("%8s %9s %9s  %s" % ("calls/st", "us/step", "avg_us", "kernel"))
for r in rows[:45]:
    print("%8.2f %9.2f %9.2f  %s" % (int(r["Calls"]) / steps, float(r["TotalDurationNs"]) / 1e3 / steps, float(r["AverageNs"]) / 1e3, r["Name"][:110]))
print("total us/step", sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / steps)
PY
      find "$OUT" -name "*kernel_trace.csv" -delete; find "$OUT" -name "*.db" -delete;;
    pmc)     R="$(pwd)"; export TMPDIR=/tmp
             for C in FETCH_SIZE WRITE_SIZE; do
               (cd /tmp && PROBE_SIZE=1000000 PROBE_ITERS=3 PROBE_NT=1 timeout 400 rocprofv3 --pmc $C --kernel-trace --output-format csv -d "$R/$OUT/pmc_$C" -o probe -- python "$R/tools/gather_probe.py" > "$R/$OUT/probe_$C.log" 2>&1)
               (cd /tmp && timeout 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d "$R/$OUT/pmcc_$C" -o probe -- python "$R/tools/convert_probe.py" 62464 default > "$R/$OUT/cprobe_$C.log" 2>&1)
             done
             python - "$OUT" <<'PY'
import csv, glob, json, sys, collections
out = sys.argv[1]
res = {}
for tag, pat in (("gather", "pmc_"), ("convert", "pmcc_")):
    for cname in ("FETCH_SIZE", "WRITE_SIZE"):
        files = glob.glob("%s/%s%s/**/*counter_collection.csv" % (out, pat, cname), recursive=True)
        acc = collections.defaultdict(list)
        for f in files:
            for r in csv.DictReader(open(f)):
                if r.get("Counter_Name") == cname:
                    acc[r.get("Kernel_Name", "")[:60]].append(float(r["Counter_Value"]))
        for k, v in acc.items():
            if ("k_gather_rows_v1" in k and tag == "gather") or ("k_frames_to_f32_nhwc4" in k and tag == "convert"):
                v = sorted(v)
                res.setdefault(tag, {})[cname] = {"kernel": k, "launches": len(v), "median_KiB": v[len(v) // 2], "min_KiB": v[0], "max_KiB": v[-1]}
for tag, algo in (("gather", 2.0 * 122 * 512 * 28224), ("convert", 62464 * 28224 * 5.0)):
    if tag in res and "FETCH_SIZE" in res[tag] and "WRITE_SIZE" in res[tag]:
        fetch = res[tag]["FETCH_SIZE"]["median_KiB"] * 1024 * 2      # gfx950: FETCH_SIZE counts 64 B per 128 B request (MI355X_MICROARCH.md, HBM)
        write = res[tag]["WRITE_SIZE"]["median_KiB"] * 1024
        res[tag]["hbm_bytes_per_launch"] = fetch + write
        res[tag]["fetch_bytes_corrected"] = fetch
        res[tag]["write_bytes"] = write
        res[tag]["algorithmic_bytes_per_launch"] = algo
        res[tag]["traffic_over_algorithmic"] = (fetch + write) / algo
json.dump(res, open(out + "/pmc_traffic.json", "w"), indent=1)
print(json.dumps(res, indent=1))
PY
             find "$OUT" -name "*kernel_trace.csv" -delete; find "$OUT" -name "*counter_collection.csv" -size +1M -delete; find "$OUT" -name "*.db" -delete;;
    dist1)   BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29577 bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --profile-steps 0 > "$OUT/bench_rccl_forced_world1.json" 2> "$OUT/bench_rccl_forced_world1.err"; echo "dist1 rc=$?"; tail -c 500 "$OUT/bench_rccl_forced_world1.err"; head -c 600 "$OUT/bench_rccl_forced_world1.json"; echo;;
    selflaunch) BENCH_FORCE_DIST=1 timeout 600 python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --profile-steps 0 > "$OUT/bench_selflaunch_world1.json" 2> "$OUT/bench_selflaunch_world1.err"; echo "selflaunch rc=$?"; tail -c 500 "$OUT/bench_selflaunch_world1.err"; head -c 1500 "$OUT/bench_selflaunch_world1.json"; echo
             timeout 900 python bench.py --full --gpus 2 --share-gpu --steps 5 --warmup 2 --no-cpu-baseline --profile-steps 0 > "$OUT/bench_gpus2_shared_gloo.json" 2> "$OUT/bench_gpus2_shared_gloo.err"; echo "gpus2 rc=$?"; tail -c 800 "$OUT/bench_gpus2_shared_gloo.err"; python - "$OUT/bench_gpus2_shared_gloo.json" <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    print({k: d[k] for k in ("value", "learner_steps_per_sec", "n_gpus", "ms_per_step", "scaling", "rccl")}); print("weak:", d.get("weak"))
except Exception as e:
    print("no json line:", e)
PY
    ;;
    lstm)    timeout 900 python -m pytest tests/test_lstm_gpu.py -x -q --timeout 300 -k "lstm or persistent" > "$OUT/pytest_lstm.log" 2>&1; echo "pytest lstm rc=$?"; tail -15 "$OUT/pytest_lstm.log"
             timeout 300 python tools/lstm_probe.py > "$OUT/lstm_probe.jsonl" 2> "$OUT/lstm_probe.err"; echo "lstm probe rc=$?"; cat "$OUT/lstm_probe.jsonl"; tail -3 "$OUT/lstm_probe.err";;
    acttrace) R="$(pwd)"; export TMPDIR=/tmp; (cd /tmp && timeout 600 rocprofv3 --kernel-trace --output-format csv -d "$R/$OUT/act_trace" -o act -- python "$R/tools/acting_probe.py" 60 > "$R/$OUT/acting_probe_trace.json" 2> "$R/$OUT/acting_probe_trace.err"); echo "acttrace rc=$?"; cat "$OUT/acting_probe_trace.json"; python - "$OUT" <<'PY'
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/act_trace/**/*kernel_trace.csv", recursive=True)
rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
names = [r["Kernel_Name"] for r in rows]
# one steady-state vector step = from one k_episode_track to the next, near the end of the acting loop
idx = [i for i, n in enumerate(names) if ("k_actor_pre" in n or "k_episode_track" in n)]
a, b = idx[-12], idx[-11]
print("kernels in one acting vector step:", b - a)
t0 = int(rows[a]["Start_Timestamp"])
for r in rows[a:b]:
    print("%8.1f %7.1f  %s" % ((int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"][:120]))
print("step span us", (int(rows[b]["Start_Timestamp"]) - t0) / 1e3)
PY
      find "$OUT" -name "*kernel_trace.csv" -delete; find "$OUT" -name "*.db" -delete;;
    fast)    timeout 900 python -m pytest tests/test_fast_acting_gpu.py tests/test_train_loop_gpu.py tests/test_ingest_paths_gpu.py tests/test_replay_gpu.py -x -q --timeout 300 > "$OUT/pytest_fast.log" 2>&1; echo "pytest fast rc=$?"; tail -25 "$OUT/pytest_fast.log";;
    gemm3)   timeout 600 python tools/gemm3_probe.py ${GEMM3_SPECS:-} > "$OUT/gemm3_probe.jsonl" 2> "$OUT/gemm3_probe.err"; echo "gemm3 probe rc=$?"; cat "$OUT/gemm3_probe.jsonl"; tail -5 "$OUT/gemm3_probe.err";;
    g3pmc)   R="$(pwd)"; export TMPDIR=/tmp; i=0
             for grp in "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_LDS" "SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM" "SQ_LDS_UNALIGNED_STALL SQ_LDS_ADDR_CONFLICT SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_ACTIVE_INST_MISC"; do
               i=$((i+1)); (cd /tmp && timeout 200 rocprofv3 --pmc $grp --kernel-trace --output-format csv -d "$R/$OUT/g3pmc$i" -o c -- python "$R/tools/gemm3_probe.py" ${GEMM3_SPECS:-nt:655360x1024x512} > "$R/$OUT/g3pmc$i.jsonl" 2> "$R/$OUT/g3pmc$i.err"); echo "g3pmc pass $i rc=$?"
             done
             python - "$OUT" <<'PY'
import csv, glob, os, sys, collections, json
out = sys.argv[1]
res = collections.defaultdict(dict)
for f in glob.glob(os.path.join(out, "g3pmc*", "**", "*counter_collection.csv"), recursive=True):
    acc = collections.defaultdict(lambda: collections.defaultdict(float)); n_disp = collections.Counter(); seen = set(); dur = collections.Counter()
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        if "k_gemm3<" not in n and "Cijk" not in n: continue
        n = n.split("(")[0][:60]
        acc[n][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Dispatch_Id"] not in seen:
            seen.add(r["Dispatch_Id"]); n_disp[n] += 1; dur[n] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    for n, c in acc.items():
        for k, v in c.items(): res[n][k] = v / n_disp[n]
        res[n]["avg_ms_under_counters"] = round(dur[n] / n_disp[n], 4); res[n]["dispatches"] = n_disp[n]
print(json.dumps(res, indent=1)); json.dump(res, open(os.path.join(out, "gemm3_pmc.json"), "w"), indent=1)
PY
             find "$OUT" -path "*g3pmc*" -name "*.csv" -size +1M -delete; find "$OUT" -path "*g3pmc*" -name "*.db" -delete; tail -3 "$OUT"/g3pmc*.err | tail -20;;
    gemmshapes) BENCH_GEMM_SHAPES="$OUT/gemm_shapes.jsonl" timeout 600 python bench.py --steps 3 --warmup 2 --no-cpu-baseline --profile-steps 1 > "$OUT/bench_gemmshapes.json" 2> "$OUT/bench_gemmshapes.err"; echo "gemmshapes rc=$?"; tail -3 "$OUT/bench_gemmshapes.err"; cat "$OUT/gemm_shapes.jsonl";;
    conv3)   timeout 300 python tools/conv3_probe.py > "$OUT/conv3_probe.jsonl" 2> "$OUT/conv3_probe.err"; echo "conv3 probe rc=$?"; cat "$OUT/conv3_probe.jsonl"; tail -3 "$OUT/conv3_probe.err"
             R="$(pwd)"; export TMPDIR=/tmp; (cd /tmp && timeout 200 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES --kernel-trace --output-format csv -d "$R/$OUT/c3pmc" -o c -- python "$R/tools/conv3_probe.py" > /dev/null 2> "$R/$OUT/c3pmc.err"); echo "c3pmc rc=$?"
             python - "$OUT" <<'PY'
import csv, glob, os, sys, collections, json
out = sys.argv[1]
res = {}
for f in glob.glob(os.path.join(out, "c3pmc", "**", "*counter_collection.csv"), recursive=True):
    acc = collections.defaultdict(lambda: collections.defaultdict(float)); n_disp = collections.Counter(); seen = set(); dur = collections.Counter()
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        if "k_conv3_fwd" not in n and "igemm_fwd" not in n: continue
        n = n.split("(")[0][:50] + " grid " + r.get("Grid_Size", "?")
        acc[n][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Dispatch_Id"] not in seen:
            seen.add(r["Dispatch_Id"]); n_disp[n] += 1; dur[n] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    for n, c in acc.items():
        d = {k: v / n_disp[n] for k, v in c.items()}
        d["avg_ms_under_counters"] = round(dur[n] / n_disp[n], 4); d["dispatches"] = n_disp[n]
        if d.get("GRBM_GUI_ACTIVE"):
            d["mfma_busy_fraction"] = round(d.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) / (d["GRBM_GUI_ACTIVE"] * 128), 3)
            d["clock_GHz"] = round(d["GRBM_GUI_ACTIVE"] / 8 / d["avg_ms_under_counters"] / 1e6, 3)
        res[n] = d
print(json.dumps(res, indent=1)); json.dump(res, open(os.path.join(out, "conv3_pmc.json"), "w"), indent=1)
PY
             find "$OUT" -path "*c3pmc*" -name "*.csv" -size +1M -delete; find "$OUT" -path "*c3pmc*" -name "*.db" -delete;;
    f32pipe) MIRL_GEMM3=0 MIRL_CONV1_BF16=0 MIRL_CONV3=0 timeout 600 python bench.py --steps 10 --warmup 3 --no-cpu-baseline --profile-steps 0 > "$OUT/bench_f32_pipe_only.json" 2> "$OUT/bench_f32_pipe_only.err"; echo "f32pipe rc=$?"; head -c 700 "$OUT/bench_f32_pipe_only.json"; echo;;
    noact)   timeout 600 python bench.py --full --steps 20 --warmup 5 --no-acting --no-cpu-baseline > "$OUT/bench_noacting.json" 2> "$OUT/bench_noacting.err"; echo "noact rc=$?"; head -c 3000 "$OUT/bench_noacting.json";;
  esac
done
