"""ORDER BY a post-aggregator on the device, measured (recorded, not a gate).

Query: groupBy ... ORDER BY avg DESC LIMIT 100 with avg = ds / rows (an arithmetic post-aggregator over a doubleSum
and the count). Two results:

  shape A   the tests' shape: three 40,000-row basic segments grouped by (dimZipf, dimSequential), filtered to
            dimSequential in [0, 300): 13,757 groups
  large     one basic segment grouped by (dimUniform, dimHyperUnique), about one group per row (the grouping of
            tools/post_measure.py, the largest result the benchmark's fixture schema gives at that row count)

Per result the medians of 5 calls after a warm-up, each on a fresh result of the same grouping:

  eval_ms              DEVICE time of k_post_eval (dg_result_post_aggregate's out_ms)
  having_ms, sort_ms   DEVICE times of dg_result_post_process (dg_post_info)
  call ms              HOST wall time of GroupByResult.apply_post_process (both calls, spec building included)
  fetch ms             HOST wall time of fetching the 100 groups left

Beside it the only route to the same answer without the device step, in the same process at BASELINE_ROWS (a size at
which it finishes in under a minute): fetch of every group, then merge_groupby -> postprocess_groupby on the host
(post-aggregators computed per row, the sort, the cut). Host wall time, one run.

usage: python tools/post_agg_measure.py [ROWS] [BASELINE_ROWS] [OUT_FILE]
"""
import importlib
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
Q = importlib.import_module("incubator-druid_amd.query")
R = importlib.import_module("incubator-druid_amd.runners")
S = importlib.import_module("incubator-druid_amd.segment")
DG = importlib.import_module("incubator-druid_amd.datagen")

FULL = (0, 1 << 42)
AVG = {"type": "arithmetic", "name": "avg", "fn": "/", "fields": [{"type": "fieldAccess", "fieldName": "ds"},
                                                                 {"type": "fieldAccess", "fieldName": "rows"}]}
ORDER = {"type": "default", "columns": [{"dimension": "avg", "direction": "descending"}], "limit": 100}


def query(dims, flt=None, ordered=True):
    return Q.GroupByQuery(intervals=[FULL], granularity="all", dimensions=list(dims), filter=flt,
                          aggregations=[Q.count("rows"), Q.double_sum("ds", "sumFloatNormal")],
                          postAggregations=[AVG], limitSpec=ORDER if ordered else None)


def device_route(segs, q, calls=5):
    infos, evals, walls, fetch_ms, left = [], [], [], 0.0, 0
    for k in range(calls + 1):
        res = R.groupby_run(segs, q)
        try:
            t0 = time.perf_counter()
            assert res.apply_post_process() and res.post_programs
            wall = (time.perf_counter() - t0) * 1e3
            if k:
                infos.append(res.post_info)
                evals.append(res.post_aggregate_ms)
                walls.append(wall)
            if k == calls:
                t0 = time.perf_counter()
                left = len(res.fetch())
                fetch_ms = (time.perf_counter() - t0) * 1e3
        finally:
            res.release()
    med = lambda f: statistics.median(i[f] for i in infos)
    return dict(groups_in=infos[-1]["groups_in"], kept=infos[-1]["groups_kept"], eval_ms=statistics.median(evals),
                having_ms=med("having_ms"), sort_ms=med("sort_ms"), call_ms=statistics.median(walls), fetch_ms=fetch_ms, left=left)


def host_route(segs, q):
    res = R.groupby_run(segs, q)
    try:
        t0 = time.perf_counter()
        part = res.fetch()
        t1 = time.perf_counter()
        rows = R.merge_groupby(q, [part])
        t2 = time.perf_counter()
    finally:
        res.release()
    return dict(groups=len(part), fetch_ms=(t1 - t0) * 1e3, post_ms=(t2 - t1) * 1e3, rows=len(rows))


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
    base_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit("command: python tools/post_agg_measure.py %d %d" % (rows, base_rows))
    emit("groupBy ORDER BY avg DESC LIMIT 100, avg = ds / rows (arithmetic post-aggregator); medians of 5 calls after a warm-up")
    head = "result | groups in | kept | eval_ms (device) | having_ms (device) | sort_ms (device) | call ms (host wall) | fetch ms (host wall)"
    with tempfile.TemporaryDirectory() as tmp:
        paths = DG.write_basic_dataset(os.path.join(tmp, "a"), 3, 40_000, bitmap="concise", compression="lz4", lz4_mode="fast")
        segs = [S.GpuSegment(p) for p in paths]
        flt = Q.BoundDimFilter("dimSequential", "0", "300", upperStrict=True, ordering="numeric")
        emit(head)
        m = device_route(segs, query(("dimZipf", "dimSequential"), flt))
        emit(f"shape A | {m['groups_in']} | {m['kept']} | {m['eval_ms']:.4f} | {m['having_ms']:.4f} | {m['sort_ms']:.4f} | "
             f"{m['call_ms']:.3f} | {m['fetch_ms']:.2f}")
        h = host_route(segs, query(("dimZipf", "dimSequential"), flt))
        emit(f"shape A without the device step (host wall, one run): fetch of {h['groups']} groups {h['fetch_ms']:.1f} ms, "
             f"merge_groupby + postprocess_groupby {h['post_ms']:.1f} ms, {h['rows']} rows returned")
        for s in segs:
            s.close()
        dims = ("dimUniform", "dimHyperUnique")
        for label, n in (("large", rows), ("large at the baseline's size", base_rows)):
            path = DG.write_basic_segment(os.path.join(tmp, f"s{n}"), n, lz4_mode="fast", dims=list(dims),
                                          metrics=["sumLongSequential", "sumFloatNormal"])
            seg = S.GpuSegment(path)
            m = device_route([seg], query(dims))
            emit(f"{label} ({n} rows) | {m['groups_in']} | {m['kept']} | {m['eval_ms']:.4f} | {m['having_ms']:.4f} | "
                 f"{m['sort_ms']:.4f} | {m['call_ms']:.3f} | {m['fetch_ms']:.2f}")
            if n == base_rows:
                h = host_route([seg], query(dims))
                emit(f"the same without the device step (host wall, one run): fetch of {h['groups']} groups {h['fetch_ms']:.1f} ms, "
                     f"merge_groupby + postprocess_groupby {h['post_ms']:.1f} ms, {h['rows']} rows returned")
            seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
