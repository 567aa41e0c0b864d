#!/bin/bash
# fused ConvTranspose + C = 48 stack (TTS_CT_FUSE) A/B: vocoder parity tests, bit-identity of the
# C2 batch's waveforms between the two modes, kernel times under rocprofv3
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
export TMPDIR=/tmp
out=$OUT/ct_ab.txt
: > $out
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_parity.py -m gpu -k "mbmelgan or melgan or c2 or synthesizer_mean_var" >> $out 2>&1 || { cat $out; exit 1; }
TTS_CT_FUSE=0 timeout -k 10 200 python tools/voc_dump.py $OUT/w0.npy --bench >> $out 2>&1 &&
TTS_CT_FUSE=1 timeout -k 10 200 python tools/voc_dump.py $OUT/w1.npy --bench >> $out 2>&1 &&
python -c "import numpy as np; a=np.load('$OUT/w0.npy'); b=np.load('$OUT/w1.npy'); print('bit-identical', np.array_equal(a,b), 'max diff', float(np.abs(a-b).max()))" >> $out 2>&1 || { cat $out; exit 1; }
rm -f $OUT/w0.npy $OUT/w1.npy
for f in 0 1 0 1; do
  rm -rf $OUT/ctp
  TTS_CT_FUSE=$f timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $OUT/ctp -o run --output-format csv -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --r1-steps 0 --f32-steps 0 > $OUT/ctp.log 2>&1 || { cat $out; exit 1; }
  echo "== TTS_CT_FUSE=$f" >> $out
  grep -h -E "resstack_x3|conv_x3_kernel<3, 4, 2, 2" $(find $OUT/ctp -name "*kernel_stats.csv") | cut -c1-160 >> $out
done
cat $out
