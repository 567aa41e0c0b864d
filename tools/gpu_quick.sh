set -o pipefail
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread -k "tacotron2 or smoke or encoder or synth" > $OUT/t.log 2>&1; rc=$?; tail -5 $OUT/t.log; [ $rc = 0 ] || exit $rc
timeout -k 10 120 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > $OUT/b.json 2>$OUT/b.err && tail -1 $OUT/b.json | cut -c1-600
TTSHIP_LIB=$PWD/tools/var/lib_trace.so TTS_PTRACE=$OUT/pt.bin timeout -k 10 120 python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2>>$OUT/b.err && python tools/ptrace.py $OUT/pt.bin
