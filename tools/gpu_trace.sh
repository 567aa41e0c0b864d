#!/bin/bash
# persistent decoder phase trace (TTS_PTRACE) of one bench step, summarised by tools/ptrace.py
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
TTSHIP_LIB=$PWD/tools/var/lib_trace.so TTS_PTRACE=$OUT/pt.bin timeout -k 10 150 python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --f32-steps 0 --r1-steps 0 > $OUT/pt.json 2>$OUT/pt.err &&
python tools/ptrace.py $OUT/pt.bin > $OUT/pt.txt 2>&1
rc=$?
cat $OUT/pt.txt
exit $rc
