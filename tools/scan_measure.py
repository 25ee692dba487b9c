"""The scan query measured on one basic-schema segment per bitmap format (recorded, not a gate).

Columns __time, dimSequential, dimSequentialHalfNull (string), sumLongSequential (long), sumFloatNormal
(double): 32 result bytes per row. Cases: unfiltered, a 1 % filter (dimSequential in 10 of its 1,000
values), a 50 % filter (dimSequentialHalfNull is null), unfiltered with limit 1000. Per case the medians
of 5 dg_rows_run calls after a warm-up (dg_metrics total_ms / decode_ms / aggregate_ms), the gather rate
kept rows x 32 B / aggregate_ms beside the copy bandwidth dg_debug_probe(DG_PROBE_COPY) measures in the same
process, and the time to fetch the whole result to the host. The limit-1000 call must read the first block
of every column only: its bytes_read is printed beside the unlimited call's and checked.

usage: python tools/scan_measure.py [ROWS] [OUT_FILE]
"""
import ctypes
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

COLUMNS = ["__time", "dimSequential", "dimSequentialHalfNull", "sumLongSequential", "sumFloatNormal"]
ROW_BYTES = 8 + 4 + 4 + 8 + 8
FULL = (0, 1 << 40)


def copy_gbs(n_bytes=1 << 30, iters=10):
    ms = ctypes.c_double()
    N.check(N.lib().dg_debug_probe(0, 0, n_bytes, iters, ctypes.byref(ms)))
    return 2 * n_bytes / (ms.value / 1e3) / 1e9


def measure(seg, flt, limit, calls=5):
    q = Q.ScanQuery(intervals=[FULL], columns=COLUMNS, filter=flt, limit=limit)
    runs = []
    kept = fetch_ms = 0
    for k in range(calls + 1):
        stats = R.RunStats()
        rs = R.scan_rows([seg], COLUMNS, q, q.row_limit, stats)
        kept = rs.rows(0)
        if k == calls:  # the whole result to the host, column by column
            t0 = time.perf_counter()
            got = [rs.fetch(0, c) for c in range(len(COLUMNS))]
            fetch_ms = (time.perf_counter() - t0) * 1e3
            assert all(len(v) == kept for v, _ in got)
        rs.close()
        if k:
            runs.append(stats.calls[0])
    med = {f: statistics.median(r[f] for r in runs) for f in ("total_ms", "decode_ms", "aggregate_ms", "bitmap_ms")}
    med.update(kept=kept, fetch_ms=fetch_ms, bytes_read=runs[-1]["bytes_read"], selected=runs[-1]["selected_rows"])
    return med


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"scan query, one segment of {rows} rows, columns {', '.join(COLUMNS)} ({ROW_BYTES} result bytes per row)")
    emit(f"copy probe (dg_debug_probe DG_PROBE_COPY, 1 GiB read + 1 GiB written): {copy_gbs():.0f} GB/s")
    cases = [("unfiltered", None, 0),
             ("1 % filter", Q.InDimFilter("dimSequential", [str(v) for v in range(100, 1000, 90)]), 0),
             ("50 % filter", Q.SelectorDimFilter("dimSequentialHalfNull", None), 0),
             ("unfiltered, limit 1000", None, 1000)]
    with tempfile.TemporaryDirectory() as tmp:
        for bitmap in ("concise", "roaring"):
            t0 = time.perf_counter()
            path = DG.write_basic_segment(os.path.join(tmp, bitmap), rows, bitmap=bitmap, lz4_mode="fast",
                                          dims=COLUMNS[1:3], metrics=COLUMNS[3:])
            seg = S.GpuSegment(path)
            emit(f"-- {bitmap}: written and attached in {time.perf_counter() - t0:.1f} s, "
                 f"{seg.device_bytes() / 1e6:.0f} MB resident")
            emit("case | kept rows | total_ms | bitmap_ms | decode_ms | aggregate_ms | gather GB/s | bytes_read | fetch ms (GB/s)")
            full_bytes = None
            for name, flt, limit in cases:
                m = measure(seg, flt, limit)
                gbs = m["kept"] * ROW_BYTES / (m["aggregate_ms"] / 1e3) / 1e9 if m["aggregate_ms"] > 0 else float("nan")
                fgbs = m["kept"] * ROW_BYTES / (m["fetch_ms"] / 1e3) / 1e9 if m["fetch_ms"] > 0 else float("nan")
                emit(f"{name} | {m['kept']} | {m['total_ms']:.3f} | {m['bitmap_ms']:.3f} | {m['decode_ms']:.3f} | "
                     f"{m['aggregate_ms']:.3f} | {gbs:.0f} | {m['bytes_read']} | {m['fetch_ms']:.1f} ({fgbs:.2f})")
                if limit == 0 and flt is None:
                    full_bytes = m["bytes_read"]
                if limit:
                    # the first block of each column: 1 of 1,526 blocks of an 8-byte column at 12.5 M rows
                    blocks8 = -(-rows // 8192)
                    ok = blocks8 < 8 or m["bytes_read"] * min(blocks8 // 4, 100) < full_bytes
                    emit(f"limit {limit}: bytes_read {m['bytes_read']} of {full_bytes} unlimited "
                         f"({'first blocks only' if ok else 'MORE THAN THE FIRST BLOCKS'})")
                    assert ok
            seg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
