"""topN over a LONG column measured on one basic-schema segment (recorded, not a gate: nothing answered this
query on the GPU before).

Query: topN by longSum(sumLongSequential), threshold 10 (per-segment threshold 1,000), with
doubleSum(sumFloatNormal) beside it, ALL granularity, no filter, output type LONG, over
  maxLongUniform   501 distinct values
  longDistinct     one value per row (a seeded permutation of the row numbers, times 7; added to the basic
                   columns here, the basic schema has no such LONG column)
Per column the segment is attached afresh. The first call builds the column's encoding and its bin index
(dg_segment_numeric_dim_info: build_ms, cardinality, bytes; wall clock of the whole first call). Then one
warm-up call and the medians of 5 further calls' dg_metrics (total_ms, aggregate_ms) and wall clock.
Alongside, the only route there was before: dg_groupby_run_dims over the same column and aggregators, every
group fetched, and the top 1,000 by the metric picked on the host (numpy argpartition + sort): its first call
on a fresh attach, then the median wall clock of 5 calls after a warm-up, split into query and fetch + top-K.

usage: python tools/topn_numeric_measure.py [ROWS] [OUT_FILE]
"""
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
N = importlib.import_module("incubator-druid_amd._native")
Q = importlib.import_module("incubator-druid_amd.query")
R = importlib.import_module("incubator-druid_amd.runners")
S = importlib.import_module("incubator-druid_amd.segment")
DG = importlib.import_module("incubator-druid_amd.datagen")
W = importlib.import_module("incubator-druid_amd.writer")

FULL = (0, 1 << 40)
METRIC = "sumLongSequential"


def aggs():
    return [Q.long_sum(METRIC), Q.double_sum("sumFloatNormal")]


def topn(seg, col):
    q = Q.TopNQuery(intervals=[FULL], dimension={"type": "default", "dimension": col, "outputType": "LONG"},
                    metric=METRIC, threshold=10, aggregations=aggs())
    stats = R.RunStats()
    t0 = time.perf_counter()
    raw = R.topn_raw([seg], q, stats)
    wall = (time.perf_counter() - t0) * 1e3
    return stats.calls[0], wall, int(raw.cnt[0]), int(raw.cut_ties[0])


def groupby_route(seg, col, k=1000):
    q = Q.GroupByQuery(intervals=[FULL], dimensions=[{"type": "default", "dimension": col, "outputType": "LONG"}],
                       aggregations=aggs())
    t0 = time.perf_counter()
    res = R.groupby_run([seg], q)
    t1 = time.perf_counter()
    part = res.fetch()
    m = np.asarray(part.aggs[0])
    k = min(k, len(m))
    top = np.argpartition(-m, k - 1)[:k] if k < len(m) else np.arange(len(m))
    top = top[np.argsort(-m[top], kind="stable")]
    t2 = time.perf_counter()
    groups = len(part)
    res.release()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, groups, len(top)


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    med = statistics.median
    emit(f"topN over a LONG column, one segment of {rows} rows, by longSum({METRIC}) + doubleSum, threshold 10 "
         f"(1000 per segment), ALL granularity, no filter; median of 5 calls after a warm-up")
    with tempfile.TemporaryDirectory() as tmp:
        spec = DG.basic_columns(rows, 9999, dims=["dimSequential"], metrics=["maxLongUniform", METRIC, "sumFloatNormal"])
        spec.metrics["longDistinct"] = ("long", np.random.default_rng(7).permutation(rows).astype(np.int64) * 7)
        path = W.write_segment(os.path.join(tmp, "seg"), spec, lz4_mode="fast")
        emit("topN column | cardinality | first call wall ms | encoding build_ms | encoding bytes | index bytes | "
             "steady total_ms | aggregate_ms | wall ms | entries | cut ties")
        for col in ("maxLongUniform", "longDistinct"):
            seg = S.GpuSegment(path)  # attached afresh: the first call builds the encoding and the bin index
            before = seg.device_bytes()
            _, wall, _, _ = topn(seg, col)
            info = seg.numeric_dim_info(col)
            index_bytes = seg.device_bytes() - before - info["device_bytes"]
            topn(seg, col)
            steady = [topn(seg, col) for _ in range(5)]
            emit(f"{col} | {info['cardinality']} | {wall:.1f} | {info['build_ms']:.3f} | {info['device_bytes']} | "
                 f"{index_bytes} | {med(s[0]['total_ms'] for s in steady):.3f} | "
                 f"{med(s[0]['aggregate_ms'] for s in steady):.3f} | {med(s[1] for s in steady):.3f} | "
                 f"{steady[-1][2]} | {steady[-1][3]}")
            seg.close()
        emit("groupBy route column | groups | first call wall ms (query + fetch + top-K) | steady query ms | "
             "fetch + host top-K ms | total wall ms")
        for col in ("maxLongUniform", "longDistinct"):
            seg = S.GpuSegment(path)
            first = groupby_route(seg, col)
            groupby_route(seg, col)
            steady = [groupby_route(seg, col) for _ in range(5)]
            emit(f"{col} | {first[2]} | {first[0] + first[1]:.1f} | {med(s[0] for s in steady):.3f} | "
                 f"{med(s[1] for s in steady):.3f} | {med(s[0] + s[1] for s in steady):.3f}")
            seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
