#!/bin/bash
# GPU-box: the round-end sequence the driver runs, in order and bounded:
# smoke(), the default bench with every leg (N=1, --full), then the driver's
# plain command.
# usage: scripts/final_check.sh TAG  (writes $BENCH_OUT/TAG_*; BENCH_OUT: default bench_out/)
set -eu
TAG=${1:-final}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
D=${BENCH_OUT:-bench_out}
mkdir -p $D
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > $D/${TAG}_smoke.log 2>&1
timeout -k 10 400 python3 bench.py --full > $D/${TAG}_bench_default.json 2> $D/${TAG}_bench_default.err
timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 > $D/${TAG}_bench_driver.json 2> $D/${TAG}_bench_driver.err
echo done
