#!/bin/bash
# C2 (conformer-CTC) bench + kernel trace.  usage (on the GPU machine): [OUT=dir] bash tools/gpu_c2.sh TAG
set -o pipefail
TAG=${1:-r02_c2}
OUT=${OUT:-out}   # where the logs, bench lines and traces go
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
python bench.py --config C2 --steps 10 --warmup 3 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo "bench rc=$?"; tail -3 $OUT/${TAG}_bench.err; cut -c1-400 $OUT/${TAG}_bench.json
rm -rf $OUT/${TAG}_prof
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o ${TAG} --output-format csv -- python bench.py --config C2 --steps 5 --warmup 3 --no-cpu-baseline --profile-steps 0 > $OUT/${TAG}_profbench.json 2> $OUT/${TAG}_profbench.err
echo "prof rc=$?"
MS=$(python -c "import json;print(json.load(open('$OUT/${TAG}_profbench.json'))['ms_per_step'])")
python tools/prof_summary.py $OUT/${TAG}_prof ${TAG} 5 $MS
mkdir -p $OUT/profiles_${TAG} && cp profiles/${TAG}_* $OUT/profiles_${TAG}/
find $OUT/${TAG}_prof -name "*_kernel_trace.csv" -delete
head -40 profiles/${TAG}_timed_region.txt | cut -c1-200
