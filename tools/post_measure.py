"""groupBy post-processing on the device measured on one basic-schema segment (recorded, not a gate).

One segment grouped by (dimUniform, dimHyperUnique), about one group per row, with longSum + doubleSum.
Queries: ORDER BY longSum DESC LIMIT 100; the same with a having that keeps about 1 % of the groups
(greaterThan on the longSum); that having alone. Per query the medians of 5 dg_result_post_process calls
after a warm-up, each on a fresh result of the same grouping:

  having_ms, sort_ms   DEVICE times (GPU timestamps around the having pass + compaction, and around the
                       word loads + radix sorts + gather: dg_post_info)
  call ms              HOST wall time of GroupByResult.apply_post_process (spec building, the call, its
                       single synchronisation)
  fetch ms             HOST wall time of fetching what is left

The baseline is the route without the device step, measured in the same process on a smaller segment (the
group count is printed; the route must finish in under a minute): fetch of every group, then merge_groupby
-> postprocess_groupby over the rows. It is host wall time. The copy bandwidth of
dg_debug_probe(DG_PROBE_COPY) from the same process is printed so the sort passes can be read against it.

usage: python tools/post_measure.py [ROWS] [BASELINE_ROWS] [OUT_FILE]
"""
import ctypes
import importlib
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
N = importlib.import_module("incubator-druid_amd._native")
Q = importlib.import_module("incubator-druid_amd.query")
R = importlib.import_module("incubator-druid_amd.runners")
S = importlib.import_module("incubator-druid_amd.segment")
DG = importlib.import_module("incubator-druid_amd.datagen")

DIMS = ["dimUniform", "dimHyperUnique"]
FULL = (0, 1 << 42)
ORDER = {"type": "default", "columns": [{"dimension": "ls", "direction": "descending"}], "limit": 100}
HAVING = {"type": "greaterThan", "aggregation": "ls", "value": 9899}  # sumLongSequential = row % 10000: about 1 %
CASES = [("ORDER BY ls DESC LIMIT 100", ORDER, None), ("the same + having ~1 %", ORDER, HAVING), ("having alone", None, HAVING)]


def copy_gbs(n_bytes=1 << 30, iters=10):
    ms = ctypes.c_double()
    N.check(N.lib().dg_debug_probe(0, 0, n_bytes, iters, ctypes.byref(ms)))
    return 2 * n_bytes / (ms.value / 1e3) / 1e9


def query(spec, having):
    return Q.GroupByQuery(intervals=[FULL], granularity="all", dimensions=list(DIMS),
                          aggregations=[Q.long_sum("ls", "sumLongSequential"), Q.double_sum("ds", "sumFloatNormal")],
                          limitSpec=spec, having=having)


def device_route(seg, q, calls=5):
    infos, walls, fetch_ms, left = [], [], 0.0, 0
    for k in range(calls + 1):
        res = R.groupby_run([seg], q)
        try:
            t0 = time.perf_counter()
            assert res.apply_post_process()
            wall = (time.perf_counter() - t0) * 1e3
            if k:
                infos.append(res.post_info)
                walls.append(wall)
            if k == calls:
                t0 = time.perf_counter()
                left = len(res.fetch())
                fetch_ms = (time.perf_counter() - t0) * 1e3
        finally:
            res.release()
    med = lambda f: statistics.median(i[f] for i in infos)
    return dict(groups_in=infos[-1]["groups_in"], after=infos[-1]["groups_after_having"], kept=infos[-1]["groups_kept"],
                having_ms=med("having_ms"), sort_ms=med("sort_ms"), call_ms=statistics.median(walls), fetch_ms=fetch_ms,
                left=left)


def host_route(seg, q):
    """Fetch of all groups + merge_groupby -> postprocess_groupby: one run (seconds), host wall times."""
    res = R.groupby_run([seg], q)
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

    emit(f"groupBy post-processing, one segment of {rows} rows grouped by ({', '.join(DIMS)}), longSum + doubleSum")
    emit(f"copy probe (dg_debug_probe DG_PROBE_COPY, 1 GiB read + 1 GiB written): {copy_gbs():.0f} GB/s")
    with tempfile.TemporaryDirectory() as tmp:
        for label, n in (("device step", rows), ("device step at the baseline's size", base_rows)):
            t0 = time.perf_counter()
            path = DG.write_basic_segment(os.path.join(tmp, f"s{n}"), n, lz4_mode="fast", dims=DIMS,
                                          metrics=["sumLongSequential", "sumFloatNormal"])
            seg = S.GpuSegment(path)
            emit(f"-- {label}: {n} rows written and attached in {time.perf_counter() - t0:.1f} s")
            emit("query | groups in | after having | kept | having_ms (device) | sort_ms (device) | call ms (host wall) | "
                 "fetch ms (host wall)")
            for name, spec, having in CASES:
                m = device_route(seg, query(spec, having))
                emit(f"{name} | {m['groups_in']} | {m['after']} | {m['kept']} | {m['having_ms']:.3f} | {m['sort_ms']:.3f} | "
                     f"{m['call_ms']:.3f} | {m['fetch_ms']:.2f}")
            if n == base_rows:
                emit(f"-- baseline, the route without the device step at {n} rows (host wall times, one run each)")
                emit("query | groups fetched | fetch ms | merge_groupby + postprocess_groupby ms | rows returned")
                for name, spec, having in CASES:
                    h = host_route(seg, query(spec, having))
                    emit(f"{name} | {h['groups']} | {h['fetch_ms']:.1f} | {h['post_ms']:.1f} | {h['rows']}")
            seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
