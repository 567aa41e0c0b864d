#!/bin/bash
# GPU tests, one bench line without the CPU baseline, and the persistent decoder phase trace
# (TTS_PTRACE, tools/ptrace.py) of one bench step.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > $OUT/t.log 2>&1; rc=$?; tail -2 $OUT/t.log; [ $rc = 0 ] || exit $rc
timeout -k 10 200 python bench.py --full --no-cpu-baseline --f32-steps 0 > $OUT/b.json 2>$OUT/b.err || exit 1
python -c "import json; d=json.load(open('$OUT/b.json')); print(d['ms_per_step'], d['decoder_step_us'], d['roofline']['launches'])"
TTSHIP_LIB=$PWD/tools/var/lib_trace.so TTS_PTRACE=$OUT/pt.bin timeout -k 10 150 python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --f32-steps 0 > /dev/null 2>$OUT/pt.err && python tools/ptrace.py $OUT/pt.bin | head -14
