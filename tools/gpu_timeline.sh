#!/bin/bash
# kernel + memory-copy trace of a short bench run, then the GPU timeline of its last step
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace -d $OUT/tl -o run --output-format csv -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --r1-steps 0 --f32-steps 0 > $OUT/tl.log 2>&1 &&
kt=$(find $OUT/tl -name "*kernel_trace.csv" | head -1) && mc=$(find $OUT/tl -name "*memory_copy_trace.csv" | head -1) &&
python tools/timeline.py "$kt" $mc > $OUT/timeline.txt 2>&1
rc=$?
tail -5 $OUT/timeline.txt
exit $rc
