#!/bin/bash
# The last two records of the round, made AFTER profiles/traffic_stamp.json is in place (the bench prints `traffic` only when the stamp's
# source hash matches): the contract line alone under rocprofv3, and the default bench.py run.
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out/r5}  # where the records go
mkdir -p "$OUT"
( cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" &&
  rocprofv3 --kernel-trace --stats -d "$OUT/contract_line" -o b --output-format csv -- python bench.py --steps 20 --warmup 5 --no-extras --no-cpu-baseline > "$OUT/contract_line.json" 2> "$OUT/contract_line.err"
  python tools/prof_summary.py "$OUT/contract_line/b_kernel_stats.csv" > "$OUT/contract_line_kernel_stats.txt"; cat "$OUT/contract_line_kernel_stats.txt"; tail -c 700 "$OUT/contract_line.json" )
python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"; tail -c 300 "$OUT/bench_final.json"; wc -c "$OUT/bench_final.json"
