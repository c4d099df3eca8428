#!/bin/bash
# rocprof of the bench + per-entry table (on the GPU machine): [OUT=dir] bash tools/gpu_r04c.sh TAG
set -o pipefail
TAG=${1:-r04c}
OUT=${OUT:-out}   # where the logs, bench lines and traces go
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $OUT
python bench.py --steps 10 --warmup 6 --full --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python - <<PY
import json
d = json.load(open("$OUT/${TAG}_bench.json"))
print("ms/step", round(d["ms_per_step"], 2), d["config"]["gemm_paths"], d["roofline"]["kernel"], d["roofline"]["frac"])
for k in d["roofline"]["kernels"][:45]:
    print("%-30s %7.1f /step %7.3f ms  %s %s" % (k["entry"], k["launches_per_step"], k["ms_per_step"],
          ("hbm %.2f" % k["frac_hbm"]) if "frac_hbm" in k else "", ("mfma %.2f" % k["frac_mfma"]) if "frac_mfma" in k else ""))
PY
rm -rf $OUT/${TAG}_prof
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o ${TAG} --output-format csv -- python bench.py --steps 5 --warmup 6 --no-cpu-baseline --profile-steps 0 > $OUT/${TAG}_profbench.json 2> $OUT/${TAG}_profbench.err
MS=$(python -c "import json;print(json.load(open('$OUT/${TAG}_profbench.json'))['ms_per_step'])")
python tools/prof_summary.py $OUT/${TAG}_prof ${TAG} 5 $MS
mkdir -p $OUT/profiles_${TAG} && cp profiles/${TAG}_* $OUT/profiles_${TAG}/
find $OUT/${TAG}_prof -name "*_kernel_trace.csv" -delete
head -10 profiles/${TAG}_timed_region.txt
