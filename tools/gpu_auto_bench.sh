set -u
cd "${GRAFT_REPO_ROOT}"
OUT=${OUT:-bench_out}  # where the logs and result lines go
export OUT
mkdir -p "$OUT"
timeout -k 10 400 python -u bench.py --full --steps 10 --warmup 2 --long-encoding auto > $OUT/bench_auto_topn.json 2> $OUT/bench_auto_topn.err || { tail -20 $OUT/bench_auto_topn.err; exit 4; }
cat $OUT/bench_auto_topn.json
timeout -k 10 400 python -u bench.py --full --steps 10 --warmup 2 --config timeseries --long-encoding auto > $OUT/bench_auto_ts.json 2> $OUT/bench_auto_ts.err || { tail -20 $OUT/bench_auto_ts.err; exit 5; }
cat $OUT/bench_auto_ts.json
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d $OUT/prof_auto -o trace -- python3 bench.py --steps 10 --warmup 2 --no-cpu-baseline --long-encoding auto > $OUT/prof_auto.log 2>&1 || { tail -20 $OUT/prof_auto.log; exit 6; }
echo done
