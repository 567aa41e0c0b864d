#!/bin/bash
# Iteration check: every GPU test, one bench line (no CPU baseline), a kernel-trace profile.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > $OUT/t.log 2>&1
rc=$?; tail -3 $OUT/t.log; [ $rc = 0 ] || exit $rc
timeout -k 10 200 python bench.py --full --no-cpu-baseline > $OUT/b.json 2>$OUT/b.err
rc=$?; tail -1 $OUT/b.json | cut -c1-700; [ $rc = 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/prof.log 2>&1
