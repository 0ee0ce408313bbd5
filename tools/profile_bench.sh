#!/bin/bash
# One command (run on the GPU box from the repo root) that regenerates the profiler evidence bench.py cites:
#   gpurun_out/<tag>_bench.json               the un-profiled JSON line of bench.py
#   gpurun_out/<tag>_bench_kernel_stats.csv   rocprofv3 --kernel-trace --stats of the same bench.py command (our kernels only)
#   gpurun_out/<tag>_bench_trace_gemv.txt     percentiles of the GEMV / GEMM / floor / empty dispatches of that trace
#   gpurun_out/pmc_traffic.json               HBM/fabric bytes per launch from separate --pmc passes (kernel-trace only)
#   gpurun_out/<tag>_gemv_decomposition.txt   tools/kbench_stamps decompose (un-profiled) + the same under rocprofv3
#   gpurun_out/bench_rocprof.json             average / calls / min of the two headline kernels from that summary, stamped with the
#                                             commit (EETQ_HEAD, passed in: the GPU box has no .git) and the kernel-source hash
# Copy the files you want judged into profiles/ (pmc_traffic.json and bench_rocprof.json keep their names; bench.py reads
# them from there and reports whether the kernel sources still hash to the value they were measured at).
# usage: EETQ_HEAD=$(git rev-parse --short HEAD) tools/profile_bench.sh [tag] [bench args...]
set -u
TAG=${1:-rXX}
shift || true
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
OUT=$ROOT/gpurun_out
mkdir -p "$OUT"
export TMPDIR=/tmp
PY=${PYTHON:-python}

echo "== 1. un-profiled bench line" >&2
$PY bench.py --full "$@" > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" || echo "bench.py failed" >&2

echo "== 2. rocprofv3 --kernel-trace --stats of the same command" >&2
rm -rf /tmp/prof_bench
( cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -- $PY "$ROOT/bench.py" --full "$@" --no-cpu-baseline --no-config5 --no-config4 --no-power-check \
    > "$OUT/${TAG}_bench_under_rocprof.json" 2> "$OUT/${TAG}_rocprof.err" ) || echo "rocprofv3 stats run failed" >&2
STATS=$(find /tmp/prof_bench -name '*kernel_stats.csv' | head -1)
if [ -n "$STATS" ]; then
    # our kernels only, name column cut to 120 characters (torch's template names run to kilobytes)
    $PY - "$STATS" > "$OUT/${TAG}_bench_kernel_stats.csv" <<'PYEOF'
import csv, sys
rows = list(csv.reader(open(sys.argv[1])))
w = csv.writer(sys.stdout)
w.writerow(rows[0])
for r in rows[1:]:
    if "eetq" in r[0]:
        w.writerow([r[0][:120]] + r[1:])
PYEOF
fi
if [ -s "$OUT/${TAG}_bench_kernel_stats.csv" ]; then
    $PY - "$OUT/${TAG}_bench_kernel_stats.csv" "profiles/${TAG}_bench_kernel_stats.csv" "$OUT/${TAG}_bench_under_rocprof.json" "$OUT/${TAG}_bench.json" > "$OUT/bench_rocprof.json" <<'PYEOF'
import csv, json, os, sys, time
sys.path.insert(0, os.getcwd())
import bench
doc = {"file": sys.argv[2], "head": os.environ.get("EETQ_HEAD", "unknown"), "kernel_src_sha16": bench.kernel_source_sha16(),
       "date": time.strftime("%Y-%m-%d"), "how": "rocprofv3 --kernel-trace --stats -- python bench.py (tools/profile_bench.sh)"}
for r in csv.DictReader(open(sys.argv[1])):
    # (the headline GEMV is the plain K = 4096 projection: its minimal-argument entry, gemv_plain_kernel, since round 7)
    for key, pat in (("gemv", "gemv_plain_kernelILi16ELi4E"), ("gemv", "gemv_kernelILi1ELi16ELi4ELb1ELb1E"), ("gemm_m1024", "gemm_tile_kernelILi0ELi2ELb0E")):
        if pat in r["Name"] and key not in doc:
            doc[key] = {"avg_us": round(float(r["AverageNs"]) / 1e3, 3), "calls": int(r["Calls"]),
                        "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
# The profiled process's OWN chain step (bench.py's timed region while rocprofv3 was attached) next to the tool's average, and
# the un-profiled chain of step 1 of this script: avg_us must not exceed chain_us_same_process (a chain step is the kernel plus
# the inter-dispatch gap); profiler_offset_us = what the attached tool adds to a step.
def chain(path):
    try:
        line = [l for l in open(path).read().splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        return {"gemv": d["roofline"]["kernel_us"], "gemm_m1024": d["secondary"]["ms_per_step"] * 1e3}
    except Exception as e:
        return {}
prof, plain = chain(sys.argv[3]), chain(sys.argv[4])
# median of the traced dispatches (the mean carries the cold first launches and the warm-up at unsettled clocks: M = 1024 GEMM mean
# 35.92 / median 35.48 / max 68.6 us in the r05 run): the figure to hold against the chain step
import glob
med = {}
for f in glob.glob("/tmp/prof_bench/**/*kernel_trace.csv", recursive=True):
    durs = {"gemv": [], "gemm_m1024": []}
    for r in csv.DictReader(open(f)):
        for key, pat in (("gemv", "gemv_plain_kernelILi16ELi4E"), ("gemv", "gemv_kernelILi1ELi16ELi4ELb1ELb1E"), ("gemm_m1024", "gemm_tile_kernelILi0ELi2ELb0E")):
            if pat in r.get("Kernel_Name", ""):
                durs[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, v in durs.items():
        if v:
            v.sort()
            med[key] = round(v[len(v) // 2], 3)
for key in ("gemv", "gemm_m1024"):
    if key in doc and key in med:
        doc[key]["median_us"] = med[key]
for key in ("gemv", "gemm_m1024"):
    if key in doc and key in prof:
        doc[key]["chain_us_same_process"] = round(prof[key], 3)
        if key in plain:
            doc[key]["chain_us_unprofiled"] = round(plain[key], 3)
            doc[key]["profiler_offset_us"] = round(prof[key] - plain[key], 3)
        doc[key]["avg_le_chain_same_process"] = bool(doc[key]["avg_us"] <= prof[key] * 1.005)
        if "median_us" in doc[key]:
            doc[key]["median_le_chain_same_process"] = bool(doc[key]["median_us"] <= prof[key] * 1.005)
print(json.dumps(doc, indent=1))
PYEOF
fi
TRACE=$(find /tmp/prof_bench -name '*kernel_trace.csv' | head -1)
[ -n "$TRACE" ] && $PY tools/trace_durations.py /tmp/prof_bench | grep -i "eetq\|gemv\|gemm\|stream_read\|empty" > "$OUT/${TAG}_bench_trace_gemv.txt"

echo "== 3. PMC passes (separate runs, --kernel-trace only) on tools/kbench gemm1" >&2
if [ -x tools/kbench ]; then
    for pass in "FETCH_SIZE" "TCC_EA0_RDREQ_sum TCC_HIT_sum TCC_MISS_sum" "WRITE_SIZE" "TCC_EA0_WRREQ_sum" "TCP_TCC_READ_REQ_sum" "TCC_REQ_sum TCC_READ_sum"; do
        d=/tmp/prof_pmc_$(echo $pass | tr ' ' '_')
        rm -rf $d
        ( cd /tmp && rocprofv3 --pmc $pass --kernel-trace --output-format csv -d $d -- "$ROOT/tools/kbench" gemm1 > /dev/null 2>> "$OUT/${TAG}_rocprof.err" ) \
            || echo "pmc pass '$pass' failed" >&2
    done
    $PY - > "$OUT/pmc_traffic.json" <<'PYEOF'
import csv, glob, json, os, sys, time
sys.path.insert(0, os.getcwd())
import bench
def mean_counter(counter, kern):
    v = []
    for f in glob.glob("/tmp/prof_pmc_*/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter and kern in r["Kernel_Name"]:
                v.append(float(r["Counter_Value"]))
    return sum(v) / len(v) if v else None
doc = {"source": "rocprofv3 --pmc on tools/kbench gemm1 via tools/profile_bench.sh (%s, MI355X): separate --pmc passes with "
                 "--kernel-trace only; 20 dispatches per kernel, mean per dispatch" % time.strftime("%Y-%m-%d"),
       "head": os.environ.get("EETQ_HEAD", "unknown"), "kernel_src_sha16": bench.kernel_source_sha16()}
for key, kern in (("gemv", "gemv_kernel"), ("gemm_m1024", "gemm_tile_kernel")):
    rd, fs = mean_counter("TCC_EA0_RDREQ_sum", kern), mean_counter("FETCH_SIZE", kern)
    wr, ws = mean_counter("TCC_EA0_WRREQ_sum", kern), mean_counter("WRITE_SIZE", kern)
    hit, miss = mean_counter("TCC_HIT_sum", kern), mean_counter("TCC_MISS_sum", kern)
    # gfx950: a 16 B/lane stream's requests are 128 B each; FETCH_SIZE (KiB) reports half the bytes of such a stream
    # (MI355X_MICROARCH.md, HBM section) -> doubled.  The two must agree; the request count is the one reported.
    doc[key + "_hbm_bytes_per_launch"] = int(rd * 128) if rd else (int(fs * 1024 * 2) if fs else None)
    # CU <- L2 read requests (the LDS-DMA and vector loads of all CUs): x 128 B = what the kernel pulls out of the L2s
    l1 = mean_counter("TCP_TCC_READ_REQ_sum", kern)
    l2rd = mean_counter("TCC_READ_sum", kern)
    doc[key + "_l2_to_cu_bytes_per_launch"] = int(l1 * 128) if l1 else (int(l2rd * 128) if l2rd else None)
    doc[key + "_raw"] = {"TCC_EA0_RDREQ_sum": rd, "FETCH_SIZE_KiB": fs, "FETCH_SIZE_x2_bytes": fs * 2048 if fs else None,
                         "TCC_EA0_WRREQ_sum": wr, "WRITE_SIZE_KiB": ws, "TCC_HIT_sum": hit, "TCC_MISS_sum": miss,
                         "TCP_TCC_READ_REQ_sum": l1, "TCC_READ_sum": l2rd, "TCC_REQ_sum": mean_counter("TCC_REQ_sum", kern)}
print(json.dumps(doc, indent=1))
PYEOF
fi

echo "== 3b. SQ / GRBM counters of the two headline kernels (their own --pmc passes, kernel-trace only)" >&2
if [ -x tools/kbench ]; then
    rm -rf /tmp/prof_sq1 /tmp/prof_sq2
    ( cd /tmp && rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE \
        --kernel-trace --output-format csv -d /tmp/prof_sq1 -- "$ROOT/tools/kbench" gemm1 > /dev/null 2>> "$OUT/${TAG}_rocprof.err" ) || echo "sq pass 1 failed" >&2
    ( cd /tmp && rocprofv3 --pmc GRBM_GUI_ACTIVE GRBM_COUNT SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VALU_MFMA_MOPS_F16 \
        --kernel-trace --output-format csv -d /tmp/prof_sq2 -- "$ROOT/tools/kbench" gemm1 > /dev/null 2>> "$OUT/${TAG}_rocprof.err" ) || echo "sq pass 2 failed" >&2
    { echo "# rocprofv3 --pmc (two passes, kernel-trace only) on tools/kbench gemm1, head ${EETQ_HEAD:-unknown}; mean per dispatch"; \
      $PY tools/pmc_summary.py /tmp/prof_sq1; $PY tools/pmc_summary.py /tmp/prof_sq2; } > "$OUT/${TAG}_pmc_sq.txt" 2>&1
fi

echo "== 4. GEMV decomposition (device-clock stamps), un-profiled and under the kernel trace" >&2
if [ -x tools/kbench_stamps ]; then
    ./tools/kbench_stamps decompose > "$OUT/${TAG}_gemv_decomposition.txt" 2>&1
    rm -rf /tmp/prof_dec
    ( cd /tmp && rocprofv3 --kernel-trace --output-format csv -d /tmp/prof_dec -- "$ROOT/tools/kbench_stamps" decompose > /tmp/dec_under.txt 2>&1 )
    { echo; echo "# the same run under rocprofv3 --kernel-trace: the tool's own begin->end per dispatch"; \
      $PY tools/trace_durations.py /tmp/prof_dec; echo "# (kbench's own lines while the tool was attached)"; grep -v "^device" /tmp/dec_under.txt; } \
        >> "$OUT/${TAG}_gemv_decomposition.txt" 2>&1
fi
echo "== 5. the un-profiled bench line again, now citing THIS run's sidecars" >&2
# bench.py reads profiles/bench_rocprof.json and profiles/pmc_traffic.json: on the GPU box's scratch copy they are still the
# previous run's, so step 1's line cites a stale rocprof average.  Put the fresh sidecars in place and print the line again.
if [ -s "$OUT/bench_rocprof.json" ]; then
    cp "$OUT/bench_rocprof.json" profiles/bench_rocprof.json
    [ -s "$OUT/pmc_traffic.json" ] && cp "$OUT/pmc_traffic.json" profiles/pmc_traffic.json
    [ -s "$OUT/${TAG}_bench_kernel_stats.csv" ] && cp "$OUT/${TAG}_bench_kernel_stats.csv" "profiles/${TAG}_bench_kernel_stats.csv"
    $PY bench.py --full "$@" > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" || echo "bench.py (second line) failed" >&2
fi
echo "done: $(ls $OUT | tr '\n' ' ')" >&2
