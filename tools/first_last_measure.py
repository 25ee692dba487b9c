"""The first / last aggregators measured on one basic-schema segment (recorded, not a gate; no speed is claimed).

Queries: timeseries over ALL, topN on dimSequential (threshold 10, ordered by the aggregator), groupBy on
dimUniform. Each in two variants: (a) longMax(sumLongSequential), the nearest route the engine had before
these aggregators (this variant also runs on the commit before them), (b) longLast(sumLongSequential).
Per case the medians of 5 calls after a warm-up of dg_metrics total_ms / decode_ms / aggregate_ms and the
call's bytes_read; the key column's scratch is 8 B per row of the segment. The device time of k_fl_keys and
k_fl_resolve comes from a kernel trace of the same script (rocprofv3 --kernel-trace --stats -d DIR -o NAME
-- python tools/first_last_measure.py ROWS): --append-kernels adds the k_fl_* dispatches of the trace's
database (DIR/NAME_results.db) to a recorded output, per kernel and grid size.

usage: python tools/first_last_measure.py [ROWS] [OUT_FILE]
       python tools/first_last_measure.py --append-kernels TRACE_DB OUT_FILE
"""
import importlib
import os
import statistics
import sys
import tempfile
import time


def append_kernels(db, out_path):
    import sqlite3
    rows = sqlite3.connect(db).execute(
        "select name, duration, grid_x from kernels where name like '%k_fl_%' order by start").fetchall()
    by = {}
    for name, dur, grid in rows:
        by.setdefault((name.split("(")[0], grid), []).append(dur)
    with open(out_path, "a") as f:
        f.write("kernel trace of the same script (rocprofv3 --kernel-trace): kernel | grid threads | dispatches | "
                "median ns | min ns | max ns\n")
        for (name, grid), d in by.items():
            f.write(f"{name} | {grid} | {len(d)} | {statistics.median(d):.0f} | {min(d)} | {max(d)}\n")


if len(sys.argv) > 1 and sys.argv[1] == "--append-kernels":
    append_kernels(sys.argv[2], sys.argv[3])
    sys.exit(0)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
Q = importlib.import_module("incubator-druid_amd.query")
R = importlib.import_module("incubator-druid_amd.runners")
S = importlib.import_module("incubator-druid_amd.segment")
DG = importlib.import_module("incubator-druid_amd.datagen")

FULL = ["1970-01-01/2100-01-01"]
FIELD = "sumLongSequential"


def queries(agg):
    return [("timeseries ALL", Q.TimeseriesQuery(intervals=FULL, granularity="all", aggregations=[agg])),
            ("topN dimSequential", Q.TopNQuery(intervals=FULL, granularity="all", dimension="dimSequential", metric="m",
                                               threshold=10, aggregations=[agg])),
            ("groupBy dimUniform", Q.GroupByQuery(intervals=FULL, granularity="all", dimensions=["dimUniform"],
                                                  aggregations=[agg]))]


def measure(seg, q, calls=5):
    runs = []
    for k in range(calls + 1):
        stats = R.RunStats()
        R.run_query(q, [seg], stats)
        if k:
            runs.append(stats.calls[0])
    med = {f: statistics.median(r[f] for r in runs) for f in ("total_ms", "decode_ms", "aggregate_ms")}
    med["bytes_read"] = runs[-1]["bytes_read"]
    return med


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    variants = [("a: longMax", Q.long_max("m", FIELD))]
    if hasattr(Q, "long_last"):
        variants.append(("b: longLast", Q.long_last("m", FIELD)))
    emit(f"first / last aggregators, one segment of {rows} rows; medians of 5 calls after a warm-up")
    emit(f"key column scratch of a longLast call: {8 * rows} bytes (8 B per row)")
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        path = DG.write_basic_segment(os.path.join(tmp, "seg"), rows, lz4_mode="fast",
                                      dims=["dimSequential", "dimUniform"], metrics=[FIELD])
        seg = S.GpuSegment(path)
        emit(f"written and attached in {time.perf_counter() - t0:.1f} s")
        emit("query | variant | total_ms | decode_ms | aggregate_ms | bytes_read")
        for (name, qa), *rest in zip(queries(variants[0][1]), *[queries(v[1]) for v in variants[1:]]):
            for (vname, _), (_, q) in zip(variants, [(name, qa)] + rest):
                m = measure(seg, q)
                emit(f"{name} | {vname} | {m['total_ms']:.3f} | {m['decode_ms']:.3f} | {m['aggregate_ms']:.3f} | {m['bytes_read']}")
        seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
