#!/bin/bash
# One GPU-box visit: GPU tests, the default bench, and a rocprofv3 kernel trace of the same bench.
# usage (on the GPU machine): [OUT=dir] bash tools/gpu_round.sh TAG [pytest-args]
set -o pipefail
TAG=${1:-r02}
OUT=${OUT:-out}   # where the logs, bench lines and traces go
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
python -m pytest tests -m gpu -x -q ${@:2} > $OUT/${TAG}_tests.log 2>&1
echo "tests rc=$?" | tee -a $OUT/${TAG}_tests.log
tail -5 $OUT/${TAG}_tests.log
python bench.py --steps 10 --warmup 3 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo "bench rc=$?"; tail -3 $OUT/${TAG}_bench.err; cut -c1-600 $OUT/${TAG}_bench.json
rm -rf $OUT/${TAG}_prof
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o ${TAG} --output-format csv -- python bench.py --steps 5 --warmup 3 --no-cpu-baseline --profile-steps 0 > $OUT/${TAG}_profbench.json 2> $OUT/${TAG}_profbench.err
echo "prof rc=$?"
MS=$(python -c "import json;print(json.load(open('$OUT/${TAG}_profbench.json'))['ms_per_step'])")
python tools/prof_summary.py $OUT/${TAG}_prof ${TAG} 5 $MS
mkdir -p $OUT/profiles_${TAG} && cp profiles/${TAG}_* $OUT/profiles_${TAG}/
# keep the merged-back payload small: drop the raw trace
find $OUT/${TAG}_prof -name "*_kernel_trace.csv" -delete
head -12 profiles/${TAG}_timed_region.txt
