#!/bin/bash
# round 4 evidence run: the driver's sequence (full -m gpu suite, smoke, default bench) + driver-settings bench line +
# kernel trace / timeline of the headline + PMC HBM traffic (headline and 5x512 B=32) + kernel traces of cfg C / cfg D
set -u
OUT=${1:-gpurun_out/r04_final}
mkdir -p $OUT
export TMPDIR=/tmp
( time timeout 1500 python -m pytest tests -m gpu -q > $OUT/gpu_tests.txt 2>&1 ) 2> $OUT/gpu_tests.time
tail -3 $OUT/gpu_tests.txt | cut -c1-300; grep real $OUT/gpu_tests.time
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | tee $OUT/smoke.txt
( time timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench20.out 2> $OUT/bench20.err ) 2> $OUT/bench20.time
echo "bench20 rc=$? $(grep real $OUT/bench20.time)"; cp bench_full.json $OUT/bench20_full.json
( time timeout 900 python bench.py --full > $OUT/bench_default.out 2> $OUT/bench_default.err ) 2> $OUT/bench_default.time
echo "bench default rc=$? $(grep real $OUT/bench_default.time)"; cp bench_full.json $OUT/bench_default_full.json
tail -1 $OUT/bench_default.out | wc -c
# kernel trace + timeline of the headline
rocprofv3 --kernel-trace --stats -d $OUT/trace -o bench -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-parity --no-cfgA --no-aux > $OUT/bench_trace.log 2>&1
DB=$(find $OUT/trace -name '*.db' | head -1)
python scripts/rocpd_stats.py "$DB" $OUT/stats.md > /dev/null
python scripts/rocpd_timeline.py "$DB" $OUT/timeline.md > /dev/null
head -5 $OUT/timeline.md; head -8 $OUT/stats.md | cut -c1-160
rm -rf $OUT/trace
bash scripts/r04_pmc.sh $OUT/pmc > $OUT/pmc.log 2>&1
bash scripts/r04_pmc.sh $OUT/pmc512 "--units 512 --batch 32" > $OUT/pmc512.log 2>&1
grep "lstm_fwd\|lstm_bwd\|optimizer" $OUT/pmc/*.txt $OUT/pmc512/*.txt | cut -c1-220
bash scripts/r02_trace_cfgC.sh $OUT/cfgC > $OUT/cfgC.log 2>&1
bash scripts/r02_trace_cfgD.sh $OUT/cfgD > $OUT/cfgD.log 2>&1
ls $OUT
