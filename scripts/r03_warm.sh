#!/bin/bash
set -u
OUT=${1:-gpurun_out/r03_warm}
mkdir -p $OUT
Q="--no-aux --no-cfgA --no-parity --no-cpu-baseline"
for V in 1 0 1 0; do
  ASR_WARM_BPTT=$V timeout 120 python bench.py --full --steps 20 --warmup 5 $Q > $OUT/b256_warm${V}_$RANDOM.json 2>> $OUT/err.log
done
python - <<PY
import json, glob
for p in sorted(glob.glob('$OUT/b*.json')):
    d = json.load(open(p)); k = d['kernels']
    print('%-28s %.3f ms/step fwd %.1f bwd %.1f' % (p.split('/')[-1], d['ms_per_step'], k['lstm_fwd']['avg_us'], k['lstm_bwd']['avg_us']))
PY
