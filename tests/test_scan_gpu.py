"""GPU suite of the scan query (dg_rows_run, the rowset, the host layer).

Expected values are the reference's own (tests/golden/scan_kats.json, transcribed from ScanQueryRunnerTest),
rows this file generates, or the oracle's reading of the same segment bytes (O.OracleSegment.numeric /
time / ids / multi / dictionary, O.filter_mask); never the engine's. Values are compared bit for bit.
"""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FULL = (0, 1 << 40)
LAYOUTS = [("concise", "lz4"), ("roaring", "lz4"), ("concise", "uncompressed"), ("roaring", "none")]


@pytest.fixture(scope="module")
def M():
    class Mods:
        R = importlib.import_module("incubator-druid_amd.runners")
        N = importlib.import_module("incubator-druid_amd._native")
        S = importlib.import_module("incubator-druid_amd.segment")
        I = importlib.import_module("incubator-druid_amd.incremental")
        W = importlib.import_module("incubator-druid_amd.writer")
        Q = importlib.import_module("incubator-druid_amd.query")
    return Mods


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def scan_arrays(M, segs, columns, flt=None, interval=FULL, limit=0, cancel=None):
    """One native call: (rows kept per segment, per segment {column: (values, offsets)}, metrics)."""
    q = M.Q.ScanQuery(intervals=[interval], columns=list(columns), filter=flt, limit=limit)
    stats = M.R.RunStats()
    rs = M.R.scan_rows(segs, list(columns), q, q.row_limit, stats, cancel)
    try:
        rows = [rs.rows(s) for s in range(len(segs))]
        assert rs.rows(-1) == sum(rows)
        cols = [{c: rs.fetch(s, k) for k, c in enumerate(columns)} for s in range(len(segs))]
    finally:
        rs.close()
    return rows, cols, stats.calls[0]


def oracle_rows(O, o, flt, interval=FULL):
    mask = np.ones(o.num_rows, bool) if flt is None else O.filter_mask(o, flt.optimize()).copy()
    t = o.time()
    mask &= (t >= interval[0]) & (t < interval[1])
    return np.nonzero(mask)[0]


def oracle_column(O, o, name, rows):
    """(values, offsets) of the given rows as the rowset holds them."""
    kind = o.column_kind(name)
    if kind == O.OR_MISSING:
        return None, None
    if kind == O.OR_STRING:
        if o.is_multi(name):
            off, vals = o.multi(name)
            lens = (off[1:] - off[:-1])[rows]
            out_off = np.zeros(len(rows) + 1, np.int64)
            out_off[1:] = np.cumsum(lens)
            parts = [vals[off[r]:off[r + 1]] for r in rows]
            return (np.concatenate(parts) if parts else np.zeros(0, np.int32)).astype(np.int32), out_off
        return o.ids(name)[rows], None
    as_type = {O.OR_LONG: "long", O.OR_FLOAT: "float", O.OR_DOUBLE: "double"}[kind]
    return o.numeric(name, as_type)[rows], None


def check_against_oracle(M, O, g, o, columns, flt=None, interval=FULL, limit=0):
    rows, cols, m = scan_arrays(M, g, columns, flt, interval, limit)
    left = limit if limit > 0 else None
    selected = scanned = 0
    for s, os_ in enumerate(o):
        sel = oracle_rows(O, os_, flt, interval)
        if left is None or left > 0:
            selected += len(sel)
            scanned += os_.num_rows
        keep = sel if left is None else sel[:left]
        if left is not None:
            left -= len(keep)
        assert rows[s] == len(keep), (s, rows, len(keep))
        for c in columns:
            want_v, want_o = oracle_column(O, os_, c, keep)
            got_v, got_o = cols[s][c]
            if want_v is None:
                assert got_v is None
                continue
            assert got_v.dtype == want_v.dtype and np.array_equal(_bits(got_v), _bits(want_v)), (s, c)
            assert (got_o is None) == (want_o is None) and (want_o is None or np.array_equal(got_o, want_o)), (s, c)
    assert m["selected_rows"] == selected and m["segment_rows"] == scanned, (m, selected, scanned)
    return rows, m


# ----------------------------------------------------------------------------------------------
# 1. reference KATs on the TestIndex sample segments
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample_segs(M, sample_dirs):
    segs = {k: M.S.GpuSegment(p) for k, p in sample_dirs.items()}
    yield segs
    for s in segs.values():
        s.close()


def test_reference_kats(M, sample_segs):
    with open(os.path.join(GOLDEN, "scan_kats.json")) as f:
        kats = json.load(f)
    ran = 0
    for case in kats["cases"]:
        compacted = case["query"].get("resultFormat") == "compactedList"
        for layout, seg in sample_segs.items():
            for q in (case["query"], M.Q.query_from_json(case["query"]).to_json()):
                got = M.R.run_query(q, [seg])
                if not case["events"]:
                    assert got == [], (case["name"], layout)
                    continue
                assert len(got) == 1 and got[0].segmentId == seg.identifier and got[0].columns == case["columns"]
                want = case["events"]
                if compacted:
                    want = [[e[c] for c in case["columns"]] for e in want]
                assert got[0].events == want, (case["name"], case["legacy"], layout)
                assert got[0].to_json()["events"] == want
            ran += 1
    assert ran == 20 * 6


@pytest.mark.parametrize("legacy", [False, True])
def test_full_on_select(M, O, sample_dirs, sample_segs, legacy):
    """testFullOnSelect's shape (every column, limit 3 and none) against the oracle's reading of the same
    segment: the sample segment does not carry every TestIndex metric."""
    Q, R = M.Q, M.R
    for layout, seg in sample_segs.items():
        o = O.OracleSegment(sample_dirs[layout])
        want_cols = ["timestamp" if legacy else "__time", "market", "quality", "qualityNumericString", "placement",
                     "partial_null_column"]
        for limit in (3, 0):
            q = Q.ScanQuery(intervals=["2011-01-12/2011-01-14"], limit=limit, legacy=legacy)
            got = R.run_query(q, [seg])
            assert len(got) == 1
            cols = got[0].columns
            assert cols[:6] == want_cols and sorted(cols[6:]) == sorted(c for c in o.columns() if c not in want_cols
                                                                        and c != "__time")
            rows = oracle_rows(O, o, None, (Q.parse_time("2011-01-12"), Q.parse_time("2011-01-14")))
            rows = rows[:limit] if limit else rows
            assert len(got[0].events) == len(rows) == (3 if limit else 26)
            for c in cols:
                if c == "timestamp":
                    want = [Q.format_time(int(t)) for t in o.time()[rows]]
                elif o.column_kind(c) == O.OR_STRING:
                    d = o.dictionary(c)
                    want = [d[i] for i in o.ids(c)[rows]]
                else:
                    kind = {O.OR_LONG: "long", O.OR_FLOAT: "float", O.OR_DOUBLE: "double"}[o.column_kind(c)]
                    want = o.numeric(c, kind)[rows].astype(np.float64 if kind != "long" else np.int64).tolist()
                assert [e[c] for e in got[0].events] == want, (layout, c)


# ----------------------------------------------------------------------------------------------
# 2. every layout of the basic schema: all columns, bit-equal
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basic(M, O, basic_dirs):
    out = {k: ([M.S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]) for k, paths in basic_dirs.items()}
    yield out
    for g, _ in out.values():
        for s in g:
            s.close()


def _basic_filters(Q):
    return [None, Q.SelectorDimFilter("dimZipf", "3"),
            Q.BoundDimFilter("sumLongSequential", "100", "5000", False, True, "numeric"),  # a row post-filter
            Q.NotDimFilter(Q.SelectorDimFilter("dimSequentialHalfNull", None))]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_basic_all_columns(M, O, basic, layout):
    g, o = basic[layout]
    columns = ["__time"] + [c for c in o[0].columns() if c != "__time"] + ["no_such_column"]
    for flt in _basic_filters(M.Q):
        rows, m = check_against_oracle(M, O, g, o, columns, flt)
        assert sum(rows) > 0 and m["bytes_read"] > 0


def test_limits_over_three_segments(M, O, basic):
    g, o = basic[("concise", "lz4")]
    Q = M.Q
    flt = Q.SelectorDimFilter("dimZipf", "2")
    cols = ["__time", "dimUniform", "sumFloatNormal"]
    sel = [len(oracle_rows(O, x, flt)) for x in o]
    assert min(sel) > 100
    for limit in (1, 37, sel[0] - 1, sel[0] + sel[1] + 5, sum(sel), sum(sel) + 9):
        rows, m = check_against_oracle(M, O, g, o, cols, flt, limit=limit)
        assert sum(rows) == min(limit, sum(sel))
    # exhausted inside the first segment: the others are not scanned
    rows, m = check_against_oracle(M, O, g, o, cols, flt, limit=50)
    assert rows == [50, 0, 0] and m["segment_rows"] == g[0].num_rows and m["selected_rows"] == sel[0]
    # exhausted exactly at a segment's end: the next segment contributes nothing and is not scanned
    rows, m = check_against_oracle(M, O, g, o, cols, flt, limit=sel[0])
    assert rows == [sel[0], 0, 0] and m["segment_rows"] == g[0].num_rows
    rows, m = check_against_oracle(M, O, g, o, cols, None, limit=g[0].num_rows)  # the unfiltered path
    assert rows == [g[0].num_rows, 0, 0] and m["segment_rows"] == g[0].num_rows
    # only the blocks holding kept rows are decoded
    _, m_all = check_against_oracle(M, O, g, o, cols, None)
    _, m_3 = check_against_oracle(M, O, g, o, cols, None, limit=3)
    _, m_f3 = check_against_oracle(M, O, g, o, cols, flt, limit=3)
    assert 0 < m_3["bytes_read"] < m_all["bytes_read"] / 3, (m_3["bytes_read"], m_all["bytes_read"])
    assert m_f3["bytes_read"] < m_all["bytes_read"] / 3


def test_intervals(M, O, basic, monkeypatch):
    g, o = basic[("roaring", "lz4")]
    Q = M.Q
    cols = ["__time", "dimSequential", "maxLongUniform"]
    t = o[0].time()
    inside = (123_457, 654_321)  # starts and ends inside blocks; whole __time blocks lie within
    for flt in (None, Q.SelectorDimFilter("dimZipf", "1")):
        rows, m_skip = check_against_oracle(M, O, g, o, cols, flt, inside)
        assert 0 < rows[0] < g[0].num_rows
        monkeypatch.setenv("DG_NO_TIME_SKIP", "1")
        _, m_all = check_against_oracle(M, O, g, o, cols, flt, inside)
        monkeypatch.delenv("DG_NO_TIME_SKIP")
        assert m_skip["bytes_read"] < m_all["bytes_read"]  # covered __time blocks stay undecoded
        check_against_oracle(M, O, g, o, cols, flt, inside, limit=777)
    gap = np.nonzero(np.diff(t) > 1)[0][0]
    for empty in ((2_000_000, 3_000_000), (int(t[gap]) + 1, int(t[gap + 1]))):
        rows, m = check_against_oracle(M, O, g[:1], o[:1], cols, None, empty)
        assert rows == [0]
    q = Q.ScanQuery(intervals=[(2_000_000, 3_000_000)], columns=cols)
    assert M.R.run_query(q, g) == []


# ----------------------------------------------------------------------------------------------
# 3. the compaction: row counts, selections, limits around words and tiles
# ----------------------------------------------------------------------------------------------
def _pattern_spec(W, n, tile):
    r = np.arange(n)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "one": r == min(n - 1, 4321), "last": r == n - 1,
            "e64": r % 64 == 0, "gap": (r < tile) | (r >= 2 * tile), "mod3": r % 3 == 0}
    dims = {k: W.encode_strings(np.where(v, "1", "0").tolist()) for k, v in pats.items()}
    return W.SegmentSpec(timestamps=r.astype(np.int64) + 1000, dims=dims,
                         metrics={"v": ("long", r.astype(np.int64) * 7 - 3), "x": ("double", r / 3.0),
                                  "f": ("float", (r % 1000).astype(np.float32) / 7)}), pats


def _check_generated(got, want_rows):
    v, x, f, t = (got[c][0] for c in ("v", "x", "f", "__time"))
    r = want_rows
    assert np.array_equal(v, r.astype(np.int64) * 7 - 3) and np.array_equal(t, r.astype(np.int64) + 1000)
    assert np.array_equal(_bits(x), _bits(r / 3.0))
    assert np.array_equal(_bits(f), _bits((r % 1000).astype(np.float32) / 7))


def test_row_counts(M, tmp_path):
    """Segments of 1, 63, 64, 65, tile - 1, tile, tile + 1 and 2 tile + 17 rows in one call."""
    W, Q, S = M.W, M.Q, M.S
    tile = M.N.ROWS_TILE_ROWS
    sizes = [1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 17]
    segs, pats = [], []
    for i, n in enumerate(sizes):
        spec, p = _pattern_spec(W, n, tile)
        segs.append(S.GpuSegment(W.write_segment(str(tmp_path / f"s{i}"), spec, bitmap="roaring" if i % 2 else "concise",
                                                 lz4_mode="fast")))
        pats.append(p)
    cols = ["v", "x", "f", "__time"]
    # NOT: the bits past the last row of the last bitset word are set by the complement and are not rows
    cases = [(None, lambda p: p["all"]), (Q.NotDimFilter(Q.SelectorDimFilter("mod3", "1")), lambda p: ~p["mod3"]),
             (Q.NotDimFilter(Q.SelectorDimFilter("all", "0")), lambda p: p["all"]),
             (Q.SelectorDimFilter("last", "1"), lambda p: p["last"])]
    for flt, want in cases:
        rows, got, m = scan_arrays(M, segs, cols, flt)
        for s, n in enumerate(sizes):
            r = np.nonzero(want(pats[s]))[0]
            assert rows[s] == len(r), (flt, n)
            _check_generated(got[s], r)
        assert m["segment_rows"] == sum(sizes)
    for s in segs:
        s.close()


def test_selections_and_limits(M, tmp_path):
    W, Q, S = M.W, M.Q, M.S
    tile = M.N.ROWS_TILE_ROWS
    n = 3 * tile + 5
    spec, pats = _pattern_spec(W, n, tile)
    seg = S.GpuSegment(W.write_segment(str(tmp_path / "p"), spec, lz4_mode="fast"))
    cols = ["v", "x", "f", "__time"]
    for name in ("none", "all", "one", "last", "e64", "gap", "mod3"):
        want = np.nonzero(pats[name])[0]
        count = len(want)
        limits = {0, 1, count, count + 3, max(count - 1, 1)}
        if name == "mod3":
            limits |= {50, 11}           # cut inside a word
        if name in ("all", "gap"):
            limits |= {tile, tile + 1, tile - 1, 2 * tile}  # at and around a tile edge
        for limit in sorted(limits):
            rows, got, m = scan_arrays(M, [seg], cols, Q.SelectorDimFilter(name, "1"), limit=limit)
            r = want[:limit] if limit else want
            assert rows == [len(r)] and m["selected_rows"] == count, (name, limit)
            _check_generated(got[0], r)
    seg.close()


# ----------------------------------------------------------------------------------------------
# 4. codecs: id widths, DELTA / TABLE longs, LZF; kept rows straddling their block boundaries
# ----------------------------------------------------------------------------------------------
def _codec_spec(W, n, seed):
    rng = np.random.default_rng(seed)
    return W.SegmentSpec(
        timestamps=np.sort(rng.integers(10_000, 10_000 + 3_600_000, n)).astype(np.int64),
        dims={"a": W.encode_int_strings(rng.integers(0, 300, n)), "b": W.encode_int_strings(rng.zipf(1.3, n) % 50)},
        metrics={"delta": ("long", 1_000_000 + rng.integers(0, 5000, n)), "table": ("long", rng.integers(0, 9, n) * 1111),
                 "wide": ("long", rng.integers(-(1 << 62), 1 << 62, n)), "x": ("double", rng.normal(3, 1, n)),
                 "f": ("float", rng.normal(3, 1, n).astype(np.float32))})


@pytest.mark.parametrize("variant", ["w3_lz4", "w4_lz4", "w3_uncompressed", "auto_lz4", "auto_none", "lzf", "lzf_v1"])
def test_codecs(M, O, tmp_path, variant):
    W, Q = M.W, M.Q
    n = 70_000  # several blocks of every width: 8-byte values 8192 per block, ids 16384 or more
    kw = {"w3_lz4": dict(id_bytes=3), "w4_lz4": dict(id_bytes=4), "w3_uncompressed": dict(id_bytes=3, compression="uncompressed"),
          "auto_lz4": dict(long_encoding="auto"), "auto_none": dict(long_encoding="auto", compression="none"),
          "lzf": dict(compression="lzf"), "lzf_v1": dict(compression="lzf_v1")}[variant]
    if "compression" not in kw or kw["compression"] == "lz4":
        kw["lz4_mode"] = "fast"
    p = W.write_segment(str(tmp_path / "s"), _codec_spec(W, n, 21), bitmap="roaring", **kw)
    g, o = [M.S.GpuSegment(p)], [O.OracleSegment(p)]
    cols = ["__time", "a", "b", "delta", "table", "wide", "x", "f"]
    check_against_oracle(M, O, g, o, cols, None)
    check_against_oracle(M, O, g, o, cols, Q.InDimFilter("b", ["1", "2", "40"]))       # sparse, across every block
    rows, m = check_against_oracle(M, O, g, o, cols, Q.BoundDimFilter("a", "100", "200", False, True), limit=9000)
    t = o[0].time()
    check_against_oracle(M, O, g, o, cols, None, (int(t[8000]), int(t[17000])))      # straddles block edges
    g[0].close()


# ----------------------------------------------------------------------------------------------
# 5. multi-value columns
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("legacy_mv,comp", [(False, "lz4"), (True, "lz4"), (False, "uncompressed")])
def test_multi_value(M, O, tmp_path, legacy_mv, comp):
    W, Q, R = M.W, M.Q, M.R
    rng = np.random.default_rng(5)
    n = 14_000
    lens = rng.choice([0, 1, 1, 2, 3, 7], n)
    lens[:3] = [0, 1, 4]
    rows_v = [[f"v{x:03d}" for x in rng.integers(0, 300, k)] for k in lens]  # 300 values: 2-byte ids,
    assert sum(len(r) for r in rows_v) > 32768                               # lists cross the value-block edge
    spec = W.SegmentSpec(timestamps=np.arange(n, dtype=np.int64), dims={"mv": W.encode_multi_strings(rows_v),
                                                                        "k": W.encode_int_strings(np.arange(n) % 5)},
                         metrics={"v": ("long", np.arange(n, dtype=np.int64))})
    p = W.write_segment(str(tmp_path / "mv"), spec, compression=comp, lz4_mode="fast", legacy_multi_value=legacy_mv)
    g, o = [M.S.GpuSegment(p)], [O.OracleSegment(p)]
    assert o[0].is_multi("mv")
    for flt, limit in ((None, 0), (Q.SelectorDimFilter("k", "3"), 0), (None, 5), (Q.SelectorDimFilter("k", "0"), 1234),
                       (Q.SelectorDimFilter("mv", "v007"), 0)):
        check_against_oracle(M, O, g, o, ["v", "mv", "k"], flt, limit=limit)
    # a page that starts mid-result: offsets are relative to the page
    q = Q.ScanQuery(intervals=[FULL], columns=["mv", "v"])
    rs = R.scan_rows(g, ["mv", "v"], q, None)
    off, vals = o[0].multi("mv")
    assert rs.column_info(0, 0) == (M.N.COL_STRING, True, len(vals)) and rs.column_info(0, 1) == (M.N.COL_LONG, False, n)
    for start, count in ((5000, 301), (n - 1, 1), (0, 1), (7, 0)):
        ids, po = rs.fetch(0, 0, start, count)
        assert po[0] == 0 and np.array_equal(po, off[start:start + count + 1].astype(np.int64) - off[start])
        assert np.array_equal(ids, vals[off[start]:off[start + count]])
    with pytest.raises(M.N.DruidGpuError) as e:  # a multi-value column needs out_offsets
        M.N.check(M.N.lib().dg_rowset_fetch(rs.handle, 0, 0, 0, 1, np.zeros(16, np.int32).ctypes.data, None))
    assert e.value.code == M.N.ERR_ARG
    rs.close()
    # the events: null for the (stored) empty row, the value for one element, the list otherwise
    got = R.run_query(Q.ScanQuery(intervals=[FULL], columns=["mv"], limit=3), g)
    assert [e["mv"] for e in got[0].events] == [None, sorted(rows_v[1])[0], sorted(rows_v[2])]
    g[0].close()


# ----------------------------------------------------------------------------------------------
# 6. paging, incremental segments, refusals, interleaving
# ----------------------------------------------------------------------------------------------
def test_paging(M, O, basic):
    g, o = basic[("concise", "uncompressed")]
    Q, R = M.Q, M.R
    flt = Q.SelectorDimFilter("dimZipf", "5")
    cols = ["__time", "dimSequentialHalfNull", "sumFloatNormal"]
    whole = R.run_query(Q.ScanQuery(intervals=[FULL], columns=cols, filter=flt, batchSize=1 << 20), g)
    assert [b.segmentId for b in whole] == [s.identifier for s in g]
    sel = [oracle_rows(O, x, flt) for x in o]
    for b, s, x in zip(whole, sel, o):
        d = x.dictionary("dimSequentialHalfNull")
        assert [e["__time"] for e in b.events] == x.time()[s].tolist()
        assert [e["dimSequentialHalfNull"] for e in b.events] == [d[i] for i in x.ids("dimSequentialHalfNull")[s]]
        assert [e["sumFloatNormal"] for e in b.events] == x.numeric("sumFloatNormal", "double")[s].tolist()
    for bs, limit in ((7, 60), (1, 9), (7, len(sel[0]) + 10)):
        got = R.run_query(Q.ScanQuery(intervals=[FULL], columns=cols, filter=flt, batchSize=bs, limit=limit), g)
        assert all(0 < len(b.events) <= bs for b in got)
        flat = [(b.segmentId, e) for b in got for e in b.events]
        assert flat == [(b.segmentId, e) for b in whole for e in b.events][:limit]
        ids = [b.segmentId for b in got]
        assert ids == sorted(ids, key=[s.identifier for s in g].index)  # no batch spans segments, order kept
    cl = R.run_query(Q.ScanQuery(intervals=[FULL], columns=cols, filter=flt, resultFormat="compactedList", limit=5), g)
    assert cl[0].events == [[e[c] for c in cols] for e in whole[0].events[:5]]


def test_incremental_segment(M):
    Q, R, I = M.Q, M.R, M.I
    idx = I.IncrementalIndex(["d", "mv"], [("n", "longSum", "n"), ("x", "doubleSum", "x"), ("f", "floatSum", "f")],
                             rollup=False, interval=(0, 100_000))
    rng = np.random.default_rng(3)
    rows = []
    for i in range(700):
        ev = {"d": [None, "a", "b", "c"][i % 4], "mv": [[], ["q"], ["q", "p"], ["z", "p", "p"]][i % 4],
              "n": int(rng.integers(-50, 50)), "x": float(rng.normal()), "f": float(np.float32(rng.normal()))}
        rows.append((100 + i, ev))
        idx.add(100 + i, ev)
    seg = idx.to_segment()
    q = Q.ScanQuery(intervals=[(0, 100_000)])
    got = R.run_query(q, [seg])
    assert len(got) == 1 and got[0].columns == ["__time", "d", "mv", "n", "x", "f"]
    want = [{"__time": t, "d": e["d"], "mv": (None if not e["mv"] else e["mv"][0] if len(e["mv"]) == 1 else sorted(e["mv"])),
             "n": e["n"], "x": e["x"], "f": e["f"]} for t, e in rows]
    assert got[0].events == want
    got = R.run_query(Q.ScanQuery(intervals=[(150, 100_000)], filter=Q.SelectorDimFilter("d", "b"), limit=20,
                                  columns=["n", "d"]), [seg])
    assert got[0].events == [{"n": e["n"], "d": "b"} for t, e in rows if t >= 150 and e["d"] == "b"][:20]
    seg.close()


def test_refusals_and_errors(M, O, basic, tmp_path):
    g, o = basic[("concise", "lz4")]
    Q, R, N = M.Q, M.R, M.N
    # a column the segments lack: null in every row
    got = R.run_query(Q.ScanQuery(intervals=[FULL], columns=["nope", "rows"], limit=4), g)
    assert got[0].events == [{"nope": None, "rows": 1}] * 4
    # bad fetch ranges
    q = Q.ScanQuery(intervals=[FULL], columns=["rows"], limit=10)
    rs = R.scan_rows(g, ["rows"], q, 10)
    buf = np.zeros(64, np.int64)
    for seg, col, start, count in ((3, 0, 0, 1), (-1, 0, 0, 1), (0, 1, 0, 1), (0, -1, 0, 1), (0, 0, -1, 1), (0, 0, 0, 11),
                                   (0, 0, 10, 1), (0, 0, 5, -1), (1, 0, 0, 1)):
        with pytest.raises(N.DruidGpuError) as e:
            N.check(N.lib().dg_rowset_fetch(rs.handle, seg, col, start, count, buf.ctypes.data, None))
        assert e.value.code == N.ERR_ARG, (seg, col, start, count)
    assert rs.rows(0) == 10 and rs.rows(1) == 0 and np.array_equal(rs.fetch(0, 0, 2, 8)[0], np.ones(8, np.int64))
    rs.close()
    # a complex column
    import struct
    p = M.W.write_segment(str(tmp_path / "cx"), M.W.SegmentSpec(timestamps=np.arange(10, dtype=np.int64),
                                                                 metrics={"v": ("long", np.arange(10))}))
    meta = open(os.path.join(p, "meta.smoosh")).read().splitlines()
    desc = json.dumps({"valueType": "COMPLEX", "hasMultipleValues": False,
                       "parts": [{"type": "complex", "typeName": "hyperUnique"}]}).encode()
    blob = struct.pack(">i", len(desc)) + desc + b"\0" * 16
    size = os.path.getsize(os.path.join(p, "00000.smoosh"))
    with open(os.path.join(p, "00000.smoosh"), "ab") as f:
        f.write(blob)
    with open(os.path.join(p, "meta.smoosh"), "w") as f:
        head = meta[0].split(",")
        f.write(",".join(head) + "\n" + "\n".join(meta[1:] + [f"uniques,0,{size},{size + len(blob)}"]) + "\n")
    cx = M.S.GpuSegment(p)
    assert cx.column_type("uniques") == N.COL_UNSUPPORTED
    with pytest.raises(N.UnsupportedQuery):
        R.run_query(Q.ScanQuery(intervals=[FULL], columns=["v", "uniques"]), [cx])
    with pytest.raises(N.UnsupportedQuery):
        R.run_query(Q.ScanQuery(intervals=[FULL]), [cx])  # the default list names it too
    assert R.run_query(Q.ScanQuery(intervals=[FULL], columns=["v"], limit=2), [cx])[0].events == [{"v": 0}, {"v": 1}]
    cx.close()
    # cancel set before the call: interrupted, and the next scan is exact
    flag = ctypes.c_int32(1)
    with pytest.raises(N.QueryInterrupted) as e:
        scan_arrays(M, g, ["rows", "dimZipf"], Q.SelectorDimFilter("dimZipf", "2"), cancel=flag)
    assert e.value.code == N.ERR_INTERRUPTED
    check_against_oracle(M, O, g, o, ["rows", "dimZipf", "__time"], Q.SelectorDimFilter("dimZipf", "2"))


def test_interleaved_with_aggregating_queries(M, O, basic):
    """Scratch reuse: a timeseries and a groupBy give the same results before and after scans."""
    from compare import assert_results
    g, o = basic[("roaring", "lz4")]
    Q, R = M.Q, M.R
    flt = Q.SelectorDimFilter("dimZipf", "4")
    aggs = [Q.count("n"), Q.long_sum("s", "sumLongSequential"), Q.double_sum("d", "sumFloatNormal")]
    qs = [Q.TimeseriesQuery(intervals=[FULL], granularity="minute", aggregations=aggs, filter=flt),
          Q.GroupByQuery(intervals=[FULL], dimensions=["dimZipf", "dimSequentialHalfNull"], aggregations=aggs)]
    want = [O.run(q, o) for q in qs]
    for q, w in zip(qs, want):
        assert_results(q, R.run_query(q, g), w)
    cols = ["__time"] + [c for c in o[0].columns() if c != "__time"]
    check_against_oracle(M, O, g, o, cols, flt)
    check_against_oracle(M, O, g, o, cols, None, limit=12345)
    for q, w in zip(qs, want):
        assert_results(q, R.run_query(q, g), w)
    check_against_oracle(M, O, g, o, cols, flt, (100_000, 900_000))
