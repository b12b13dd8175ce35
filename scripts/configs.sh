#!/bin/bash
# GPU-box: one bench line per BASELINE config (c1 as committed, c2 headline,
# c3, c4, c5 on one GPU) with their CPU baselines (bench.py --full), into
# $BENCH_OUT/TAG_configs.jsonl (BENCH_OUT: default bench_out/)
set -eu
TAG=${1:-r05}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
D=${BENCH_OUT:-bench_out}
mkdir -p $D
O=$D/${TAG}_configs.jsonl
: > $O
for cfg in c2_committed c2 c3 c4 c5; do
  echo "== $cfg"
  timeout -k 10 400 python3 bench.py --full --config $cfg > $D/${TAG}_$cfg.log 2> $D/${TAG}_$cfg.err
  grep '^{' $D/${TAG}_$cfg.log | tail -1 >> $O
  tail -c 300 $O
done
