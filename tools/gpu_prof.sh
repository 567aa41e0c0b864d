#!/bin/bash
# kernel-trace profile of a short bench run -> $OUT/prof (the tool segfaults at process exit
# after writing its outputs; that is expected and the last step here)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/prof
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/prof.log 2>&1
ls $OUT/prof/run_kernel_stats.csv > /dev/null
