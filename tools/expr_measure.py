"""The cost of a derived column, measured on one basic-schema segment (recorded, not a gate: nothing answered
an expression before).

One segment of ROWS rows with two LZ4 long columns, a = sumLongSequential and b = maxLongUniform, and a stored
twin ab = a * b. Medians of 5:
  build_ms            dg_segment_derive_column of `a * b` (the decode of a and b + one 8-byte store per row), the
                      column dropped between the builds
  first query         total_ms of doubleSum(a * b), ALL granularity, no filter, on a segment without the column
                      (dg_metrics of the query call; the build before it is the line above), and its wall time
                      with the build
  steady query        total_ms of the same query once the column is there
  stored twin         total_ms of doubleSum(ab) over the stored LZ4 column, same commit

usage: python tools/expr_measure.py [ROWS] [OUT_FILE]
"""
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
Q = importlib.import_module("incubator-druid_amd.query")
R = importlib.import_module("incubator-druid_amd.runners")
S = importlib.import_module("incubator-druid_amd.segment")
V = importlib.import_module("incubator-druid_amd.virtual")
W = importlib.import_module("incubator-druid_amd.writer")
DG = importlib.import_module("incubator-druid_amd.datagen")

FULL = (0, 1 << 40)
EXPR = "sumLongSequential * maxLongUniform"


def query(agg):
    return Q.TimeseriesQuery(intervals=[FULL], aggregations=[agg])


def run(seg, q):
    stats = R.RunStats()
    t0 = time.perf_counter()
    res = R.run_timeseries([seg], q, stats)
    wall = (time.perf_counter() - t0) * 1e3
    return res[0].value["s"], stats, wall


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    med = statistics.median
    emit(f"derived column `a * b` over two LZ4 long columns, one segment of {rows} rows; medians of 5")
    with tempfile.TemporaryDirectory() as tmp:
        spec = DG.basic_columns(rows, 9999, dims=["dimSequential"], metrics=["sumLongSequential", "maxLongUniform"])
        spec.metrics["ab"] = ("long", spec.metrics["sumLongSequential"][1] * spec.metrics["maxLongUniform"][1])
        path = W.write_segment(os.path.join(tmp, "seg"), spec, lz4_mode="fast")
        seg = S.GpuSegment(path)
        q_expr = query({"type": "doubleSum", "name": "s", "expression": EXPR})
        q_twin = query(Q.double_sum("s", "ab"))
        want = float(np.sum(spec.metrics["ab"][1].astype(np.float64)))  # (exact: far below 2^53)
        prog = V.compile_for_segments(Q.parse_expression(EXPR), None, [seg])
        builds = []
        for _ in range(5):
            info = seg.derive(prog.digest(), prog.ops, prog.inputs, 1)
            assert info["built"] == 1
            builds.append(info)
            seg.drop_derived()
        firsts = []
        for _ in range(5):
            v, stats, wall = run(seg, q_expr)
            assert v == want and stats.derived_built == 1
            firsts.append((stats.calls[-1]["total_ms"], stats.derived_build_ms, wall))
            seg.drop_derived()
        run(seg, q_expr)
        steady = []
        for _ in range(5):
            v, stats, wall = run(seg, q_expr)
            assert v == want and (stats.derived_built, stats.derived_reused) == (0, 1)
            steady.append((stats.calls[-1]["total_ms"], wall))
        twin = []
        for _ in range(6):
            v, stats, wall = run(seg, q_twin)
            assert v == want
            twin.append((stats.calls[-1]["total_ms"], wall))
        twin = twin[1:]
        emit("measure | ms")
        emit(f"build_ms of the derived column ({builds[0]['device_bytes']} bytes of HBM) | {med(b['build_ms'] for b in builds):.3f}")
        emit(f"first query: total_ms of the query call | {med(f[0] for f in firsts):.3f}")
        emit(f"first query: build_ms inside it | {med(f[1] for f in firsts):.3f}")
        emit(f"first query: host wall with the build | {med(f[2] for f in firsts):.3f}")
        emit(f"steady query over the derived column: total_ms | {med(s[0] for s in steady):.3f}")
        emit(f"steady query over the derived column: host wall | {med(s[1] for s in steady):.3f}")
        emit(f"doubleSum over the stored LZ4 twin: total_ms | {med(t[0] for t in twin):.3f}")
        emit(f"doubleSum over the stored LZ4 twin: host wall | {med(t[1] for t in twin):.3f}")
        seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
