#!/bin/bash
set -u
OUT=${1:-gpurun_out/r03_wgrad}
mkdir -p $OUT
timeout 900 python -m pytest tests/test_gpu_ops.py tests/test_gpu_configs.py tests/test_gpu_model.py -q -x -m gpu -k "conv or cfgC or vgg" > $OUT/tests.log 2>&1
tail -4 $OUT/tests.log
for V in 1 0; do
ASR_CONV_WGRAD_TR=$V timeout 400 python bench.py --full --steps 5 --warmup 2 --no-cfgA --no-parity --no-cpu-baseline --aux cfgC --aux-steps 6 > $OUT/aux$V.json 2> $OUT/aux$V.err
python - <<PY
import json
d = json.load(open('$OUT/aux$V.json'))
e = d['cfgC']
print('wgrad_tr=$V cfgC %.2f ms' % e['ms_per_step'], {k: round(v['avg_us']) for k, v in e.get('kernels', {}).items()})
PY
done
