#!/bin/bash
# Everything profiles/<tag>_* is made from, in one run on the GPU box (the full bench line and the profiling logs go to OUT):
#   bash tools/profile_all.sh r02 <output directory>
TAG=${1:-r02}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${2:?usage: bash tools/profile_all.sh <tag> <output directory>}
mkdir -p "$OUT"
python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
bash $R/tools/profile_bench.sh $TAG > "$OUT/prof_$TAG.log" 2>&1
bash $R/tools/profile_legacy.sh $TAG > "$OUT/prof_${TAG}_legacy.log" 2>&1
bash $R/tools/pmc_legacy.sh > "$OUT/pmc_legacy.log" 2>&1
tail -3 "$OUT/prof_$TAG.log"
