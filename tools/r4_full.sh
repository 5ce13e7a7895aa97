#!/bin/bash
# full GPU test suite + the default bench line with its --full legs (round-4 checkpoints): logs into the directory $O
cd $GRAFT_REPO_ROOT
: "${O:?set O to the log directory}"; mkdir -p "$O"
tag=${1:-a}
timeout -k 10 900 python3 -m pytest tests -m gpu -x -q > $O/full_gpu_$tag.log 2>&1; echo "pytest rc=$?" >> $O/full_gpu_$tag.log
tail -4 $O/full_gpu_$tag.log
timeout -k 10 600 python3 bench.py --full > $O/bench_$tag.json 2> $O/bench_$tag.err; echo "bench rc=$?"
python3 - <<PY
import json
l=json.load(open("$O/bench_$tag.json"))
print({k:l[k] for k in ("value","ms_per_step")}, l.get("b1"), l.get("roofline"), l.get("roofline_trained_like_offsets"))
PY
