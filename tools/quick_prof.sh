#!/bin/bash
# taco/postnet parity tests, then a kernel-trace profile of a short bench run ($OUT/qprof)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/qprof
timeout -k 10 300 python3 -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_parity.py -m gpu \
  -k "${TESTS:-postnet or tacotron2 or c5}" > $OUT/qprof_t.log 2>&1 || { tail -30 $OUT/qprof_t.log; exit 1; }
tail -2 $OUT/qprof_t.log
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/qprof -o run --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --r1-steps 0 --f32-steps 0 > $OUT/qprof.log 2>&1
ls $OUT/qprof/run_kernel_stats.csv > /dev/null && tail -1 $OUT/qprof.log | cut -c1-300
