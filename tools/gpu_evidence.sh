#!/bin/bash
# Per-config evidence on one build: rocprofv3 trace + PMC passes (tools/gpu_profile.sh), the bench_pmc
# json the line reads, then the bench line itself (STEPS_<config> timed steps, CPU baseline on).
# usage: TAG=r06_vNN CONFIGS="topn timeseries" tools/gpu_evidence.sh
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}  # where the logs and result lines go
export OUT
mkdir -p "$OUT" bench_pmc
TAG=${TAG:-r06}
for cfg in ${CONFIGS:-topn}; do
  case $cfg in topn*|timeseries|filtered) steps=100 ;; *) steps=20 ;; esac
  CONFIG=$cfg TAG=$TAG STEPS=10 timeout -k 10 900 bash tools/gpu_profile.sh > $OUT/${TAG}_profile_$cfg.log 2>&1 || { echo "profile $cfg failed"; tail -20 $OUT/${TAG}_profile_$cfg.log; exit 4; }
  head -14 $OUT/prof_${TAG}_$cfg.txt | cut -c1-150
  cp $OUT/prof_trace/trace_kernel_stats.csv $OUT/${TAG}_kernel_stats_$cfg.csv
  cp $OUT/pmc_$cfg.json bench_pmc/pmc_$cfg.json
  timeout -k 10 600 python -u bench.py --full --config $cfg --steps $steps --warmup 5 > $OUT/${TAG}_bench_$cfg.json 2> $OUT/${TAG}_bench_$cfg.err || { echo "bench $cfg failed"; tail -20 $OUT/${TAG}_bench_$cfg.err; exit 5; }
  cut -c1-400 $OUT/${TAG}_bench_$cfg.json
done
