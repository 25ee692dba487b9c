#!/bin/bash
# One GPU session: parity tests, smoke, short bench. Each GPU step has its own time limit; a fault,
# abort or timeout (any exit status other than 0/1 from pytest) ends the session.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}  # where the logs and result lines go
export OUT
mkdir -p "$OUT"
STEPS=${STEPS:-10}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc" >> $OUT/pytest_gpu.log
tail -5 $OUT/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/smoke.log; exit 3; }
tail -1 $OUT/smoke.log
timeout -k 10 900 python -u bench.py --full --steps "$STEPS" --warmup 2 ${BENCH_ARGS:-} > $OUT/bench.log 2> $OUT/bench.err || { echo "bench failed"; tail -20 $OUT/bench.err; exit 4; }
cat $OUT/bench.log
