#!/bin/bash
# Headline evidence on one build: sort probe, rocprofv3 trace + PMC passes (tools/gpu_profile.sh), then
# the bench line reading that profile's bench_pmc json. TAG names the files.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}  # where the logs and result lines go
export OUT
mkdir -p "$OUT"
TAG=${TAG:-r06}
CONFIG=${CONFIG:-groupby}
timeout -k 10 120 python tools/sort_probe.py 100000000 10 > $OUT/${TAG}_sort_probe.log 2>&1 || exit 3
grep sort $OUT/${TAG}_sort_probe.log
CONFIG=$CONFIG TAG=$TAG STEPS=${PSTEPS:-10} bash tools/gpu_profile.sh > $OUT/${TAG}_profile_$CONFIG.log 2>&1 || { tail -20 $OUT/${TAG}_profile_$CONFIG.log; exit 4; }
head -12 $OUT/prof_${TAG}_$CONFIG.txt | cut -c1-160
mkdir -p bench_pmc && cp $OUT/pmc_$CONFIG.json bench_pmc/pmc_$CONFIG.json
timeout -k 10 600 python -u bench.py --full --config $CONFIG --steps ${STEPS:-20} --warmup 3 > $OUT/${TAG}_bench_$CONFIG.json 2> $OUT/${TAG}_bench_$CONFIG.err || { tail -20 $OUT/${TAG}_bench_$CONFIG.err; exit 5; }
cut -c1-2500 $OUT/${TAG}_bench_$CONFIG.json
