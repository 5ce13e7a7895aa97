#!/bin/bash
# Per-kernel times and hardware counters of the fp32 and 16-bit MSDeformAttn kernels at the config #2 encoder shape
# (tools/bench_msda_h16.py as the workload).  One rocprofv3 run for the kernel trace, then ONE run per counter (counters are
# never collected together with a trace).  Output: <out>/kernel_stats.csv and <out>/pmc_<COUNTER>.csv + <out>/pmc_summary.txt
# usage: tools/pmc_msda_h16.sh <out-dir> [COUNTER ...]
set -o pipefail
out=${1:-profiles/msda_h16_counters}; shift
counters=${@:-SQ_INSTS_VALU SQ_WAVES SQ_INSTS_VMEM_RD SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum}
mkdir -p "$out"
tmp=$(mktemp -d)
# a step that ends with ANY non-zero status ends the script: nothing more is started on a GPU after a failed step
stop() { if [ "$1" -ne 0 ]; then echo "stopping: exit status $1 ($2)"; tail -5 "$3" 2>/dev/null; exit $1; fi; }
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/kt" -- python tools/bench_msda_h16.py --launches 50 --rounds 1 > "$out/kernel_trace.log" 2>&1
rc=$?; stop $rc "kernel trace" "$out/kernel_trace.log"
f=$(find "$tmp/kt" -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && grep -E "Name|msda|k_scatter|k_gv|k_sel" "$f" > "$out/kernel_stats.csv"
: > "$out/pmc_summary.txt"
for c in $counters; do
  timeout -k 10 240 rocprofv3 --pmc $c --output-format csv -d "$tmp/pmc_$c" -- python tools/bench_msda_h16.py --launches 10 --rounds 1 > "$out/pmc_$c.log" 2>&1
  rc=$?; stop $rc "counter $c" "$out/pmc_$c.log"
  f=$(find "$tmp/pmc_$c" -name "*counter_collection.csv" | head -1)
  if [ -z "$f" ]; then echo "$c: no counter file written" >> "$out/pmc_summary.txt"; continue; fi
  python - "$f" >> "$out/pmc_summary.txt" <<'PY'
import collections, csv, re, sys
acc = collections.defaultdict(list)
for row in csv.DictReader(open(sys.argv[1])):
    k = row["Kernel_Name"]
    m = re.search(r"(msda_fwd_fast<8>|msda_fwd_h16<[^>]*>|msda_bwd_gather_row<8, false>|msda_bwd_gather_h16<[^>]*>)", k)
    if m:
        acc[(row["Counter_Name"], m.group(1))].append(float(row["Counter_Value"]))
for (c, k), v in sorted(acc.items()):
    print(f"{c:34s} {k:52s} avg {sum(v) / len(v):16.1f}  n={len(v)}")
PY
  rm -f "$out/pmc_$c.log"
done
rm -rf "$tmp"
cat "$out/pmc_summary.txt"
