"""GPU suite of the search query (dg_search_run + the host layer).

Expected values are the reference's own (tests/golden/search_kats.json, transcribed from its search
tests) or numpy over rows this file generates / the oracle decodes (O.OracleSegment.ids / multi /
time, O.filter_mask); never the engine's.
"""
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FULL = ["1970-01-01T00:00:00.000Z/2020-01-01T00:00:00.000Z"]
FORMATS = [("concise", "lz4"), ("roaring", "lz4"), ("concise", "uncompressed"), ("roaring", "none")]


@pytest.fixture(scope="module")
def mods():
    class M:
        R = importlib.import_module("incubator-druid_amd.runners")
        N = importlib.import_module("incubator-druid_amd._native")
        S = importlib.import_module("incubator-druid_amd.segment")
        I = importlib.import_module("incubator-druid_amd.incremental")
        W = importlib.import_module("incubator-druid_amd.writer")
        Q = importlib.import_module("incubator-druid_amd.query")
    return M


@pytest.fixture(scope="module")
def search_kats():
    with open(os.path.join(GOLDEN, "search_kats.json")) as f:
        return json.load(f)


def _triples(results):
    return sorted((h["dimension"], h["value"], h["count"]) for r in results for h in r.value)


def _query(Q, case, kats, strategy, **over):
    return Q.SearchQuery(intervals=[case.get("intervals", kats["intervals"])],
                         searchDimensions=case.get("searchDimensions", []), query=case["query"],
                         sort=case.get("sort", "lexicographic"), filter=case.get("filter"),
                         context={"searchStrategy": strategy}, **over)


# ----------------------------------------------------------------------------------------------
# 1. reference KATs
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample_segs(mods, sample_dirs):
    segs = {k: mods.S.GpuSegment(p) for k, p in sample_dirs.items()}
    yield segs
    for s in segs.values():
        s.close()


@pytest.fixture(scope="module")
def placementish_segs(mods, tmp_path_factory):
    """The TestIndex sample rows with the multi-value dimension placementish (TSV column 8, values
    separated by \\u0001), as make_sample_segment.py writes the other string dimensions."""
    W, Q = mods.W, mods.Q
    rows = [line.rstrip("\n").split("\t") for line in open(os.path.join(GOLDEN, "druid.sample.numeric.tsv"),
                                                             encoding="utf-8")]
    rows = [r + [""] * (11 - len(r)) for r in rows]
    rows.sort(key=lambda r: (Q.parse_time(r[0]), r[1], r[2]))
    ts = np.array([Q.parse_time(r[0]) for r in rows], dtype=np.int64)
    dims = {}
    for name, col in (("market", 1), ("quality", 2), ("qualityNumericString", 6), ("placement", 7)):
        dims[name] = W.encode_strings([r[col] or None for r in rows])
    dims["placementish"] = W.encode_multi_strings([r[8].split("\u0001") for r in rows])
    dims["partial_null_column"] = W.encode_strings([r[10] or None for r in rows])
    spec = W.SegmentSpec(timestamps=ts, dims=dims,
                         metrics={"index": ("double", np.array([float(r[9]) for r in rows]))},
                         interval=(Q.parse_time("2011-01-12"), Q.parse_time("2011-05-01")))
    base = tmp_path_factory.mktemp("placementish")
    segs = {}
    for bitmap, comp in FORMATS:
        segs[(bitmap, comp)] = mods.S.GpuSegment(W.write_segment(str(base / f"{bitmap}_{comp}"), spec, bitmap=bitmap,
                                                                 compression=comp))
    yield segs
    for s in segs.values():
        s.close()


@pytest.mark.parametrize("strategy", ["useIndexes", "cursorOnly"])
def test_reference_kats(mods, search_kats, sample_segs, placementish_segs, strategy):
    Q, R = mods.Q, mods.R
    ts = Q.parse_time(search_kats["timestamp"])
    ran = 0
    for case in search_kats["runner"]:
        pool = sample_segs if case["segment"] == "sample" else placementish_segs
        for layout, seg in pool.items():
            q = _query(Q, case, search_kats, strategy)
            got = R.run_query(q, [seg])
            assert len(got) == 1 and got[0].timestamp == ts, (case["name"], layout)
            want = sorted(tuple(h) for h in case["hits"])
            assert _triples(got) == want, (case["name"], layout, strategy)
            if case.get("ordered"):
                assert [(h["dimension"], h["value"], h["count"]) for h in got[0].value] == \
                    [tuple(h) for h in case["hits"]], (case["name"], layout)
            # the JSON form runs the same
            assert _triples(R.run_query(q.to_json(), [seg])) == want
            ran += 1
    assert ran >= 6 * 14 + 4 * 4


def test_reference_with_case_kats(mods, search_kats, tmp_path):
    """SearchQueryRunnerWithCaseTest: its rows as an in-memory index (no bitmaps: the cursor plan) and
    persisted (the index plan), under both strategies."""
    Q, R, I, W, S, N = mods.Q, mods.R, mods.I, mods.W, mods.S, mods.N
    wc = search_kats["with_case"]
    idx = I.IncrementalIndex(["market", "quality", "placement", "placementish"], [("rows", "count", None)],
                             rollup=False, interval=(Q.parse_time("2011-01-12"), Q.parse_time("2011-01-14")))
    for t, m, ql, p, pi in wc["rows"]:
        idx.add(Q.parse_time(t), {"market": m, "quality": ql, "placement": p, "placementish": pi})
    segs = [("rows", idx.to_segment())]
    for bitmap, comp in (("concise", "lz4"), ("roaring", "uncompressed")):
        segs.append((bitmap, S.GpuSegment(W.write_segment(str(tmp_path / bitmap), idx.to_spec(), bitmap=bitmap,
                                                          compression=comp))))
    for kind, seg in segs:
        for strategy in ("useIndexes", "cursorOnly"):
            for case in wc["cases"]:
                q = _query(Q, case, search_kats, strategy)
                got = R.run_query(q, [seg])
                assert len(got) == 1 and got[0].timestamp == Q.parse_time("2011-01-12")
                found = {}
                for h in got[0].value:
                    found.setdefault(h["dimension"], []).append(h["value"])
                    assert h["count"] >= 1
                want = {d: sorted(v) for d, v in case["expected"].items() if v}
                assert {d: sorted(v) for d, v in found.items()} == want, (kind, strategy, case["name"])
        # which plan ran: an in-memory index has no bitmap index
        q = _query(Q, wc["cases"][0], search_kats, "useIndexes")
        _, plans = R.search_counts([seg], q, ["market"], [[np.array([0], np.int32)]])
        assert plans[0][0] == (N.SEARCH_PLAN_CURSOR if kind == "rows" else N.SEARCH_PLAN_INDEX)
    for _, seg in segs:
        seg.close()


# ----------------------------------------------------------------------------------------------
# expected counts from decoded rows
# ----------------------------------------------------------------------------------------------
def _expected(ids_of_row, card, mask, accepted, offsets=None, index_plan=True):
    """Counts of the accepted ids over the rows `mask` selects. Single-value: ids_of_row[r]. Multi-value
    (offsets given): the index plan counts a row once per distinct value, the cursor plan every occurrence."""
    if offsets is None:
        return np.bincount(ids_of_row[mask], minlength=card)[accepted]
    n = len(offsets) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    keep = mask[rows]
    r, v = rows[keep], ids_of_row[keep].astype(np.int64)
    if index_plan:
        v = np.unique(r * card + v) % card
    return np.bincount(v, minlength=card)[accepted]


def _time_mask(times, interval):
    return (times >= interval[0]) & (times < interval[1])


# ----------------------------------------------------------------------------------------------
# 2. parity on the basic schema
# ----------------------------------------------------------------------------------------------
PARITY_DIMS = ["dimZipf", "dimSequential", "dimSequentialHalfNull", "dimUniform", "dimMissing"]
PARITY_SPECS = [{"type": "contains", "value": "7", "caseSensitive": True},
                {"type": "fragment", "values": ["1", "2"], "caseSensitive": True},
                {"type": "regex", "pattern": "^[12].*5$"},
                {"type": "all"}]
PARITY_INTERVALS = [(0, 2_000_000_000), (250_123, 700_457), (2_000_000, 3_000_000)]


def _parity_filters(Q):
    return [None,
            Q.InDimFilter("dimZipf", ["1", "2", "3", "17"]),
            Q.OrDimFilter([Q.SelectorDimFilter("dimSequential", "12"),
                           Q.NotDimFilter(Q.BoundDimFilter("dimSequentialHalfNull", "2", "7"))]),
            Q.BoundDimFilter("sumLongSequential", "100", "7000", ordering="numeric")]


@pytest.mark.parametrize("layout", [("concise", "lz4"), ("roaring", "lz4"), ("concise", "uncompressed"),
                                    ("roaring", "none")])
def test_parity_basic(mods, O, basic_dirs, layout):
    Q, R, N, S = mods.Q, mods.R, mods.N, mods.S
    paths = basic_dirs[layout]
    segs = [S.GpuSegment(p) for p in paths]
    osegs = [O.OracleSegment(p) for p in paths]
    filters = _parity_filters(Q)
    calls = 0
    for fi, flt in enumerate(filters):
        fmasks = [O.filter_mask(o, flt.optimize() if flt is not None else None) for o in osegs]
        for ii, iv in enumerate(PARITY_INTERVALS):
            spec = PARITY_SPECS[(fi + ii) % len(PARITY_SPECS)]
            seen = {}
            for strategy in ("useIndexes", "cursorOnly"):
                q = Q.SearchQuery(intervals=[iv], searchDimensions=PARITY_DIMS, query=spec, filter=flt,
                                  context={"searchStrategy": strategy})
                ids = [[R._accepted_ids(s, d, q) for s in segs] for d in PARITY_DIMS]
                stats = R.RunStats()
                counts, plans = R.search_counts(segs, q, PARITY_DIMS, ids, stats)
                calls += 1
                cursor = strategy == "cursorOnly" or fi == 3  # a numeric bound is a row post-filter
                selected = 0
                for i, o in enumerate(osegs):
                    mask = fmasks[i] & _time_mask(o.time(), iv)
                    selected += int(mask.sum())
                    for d, dim in enumerate(PARITY_DIMS):
                        if dim == "dimMissing":
                            assert len(ids[d][i]) == 0 and plans[i][d] == N.SEARCH_PLAN_NONE
                            continue
                        want_plan = N.SEARCH_PLAN_NONE if len(ids[d][i]) == 0 else \
                            (N.SEARCH_PLAN_CURSOR if cursor else N.SEARCH_PLAN_INDEX)
                        assert plans[i][d] == want_plan, (dim, strategy, fi)
                        # the accepted ids are the oracle dictionary's too
                        assert [o.dictionary(dim)[k] for k in ids[d][i][:5]] == \
                            [segs[i].dictionary(dim)[k] for k in ids[d][i][:5]]
                        want = _expected(o.ids(dim), o.cardinality(dim), mask, ids[d][i])
                        assert np.array_equal(counts[d][i], want), (dim, strategy, fi, ii, i)
                        key = (i, dim)
                        if key in seen:  # single-value dimensions: index and cursor counts are equal
                            assert np.array_equal(seen[key], counts[d][i])
                        seen[key] = counts[d][i].copy()
                m = stats.calls[0]
                assert m["segment_rows"] == sum(o.num_rows for o in osegs)
                assert m["selected_rows"] == selected, (strategy, fi, ii)
                if ii == 0:
                    assert m["pre_filtered_rows"] == sum(int(f.sum()) for f in fmasks)
                if not cursor and ii < 2 and spec["type"] == "all":
                    assert m["bitmap_bytes"] > 0 and m["bytes_read"] > 0
    assert calls == 24
    for s in segs:
        s.close()


# ----------------------------------------------------------------------------------------------
# 3. kernel edge shapes
# ----------------------------------------------------------------------------------------------
def _strings(W, values):
    return W.encode_strings(values)


def _check_segment(mods, seg, truth, times, fdim_ids):
    """truth: {dim: (dictionary, ids per row) or (dictionary, flat ids, offsets)}. Searches every value
    of every dimension ("all") under both strategies, filters selecting ~1 % / ~99 % of the rows and an
    interval cutting the segment, against numpy over `truth`."""
    Q, R, N = mods.Q, mods.R, mods.N
    n = len(times)
    dims = list(truth)
    fdict, frow = fdim_ids[1], fdim_ids[0]
    filters = [(None, np.ones(n, bool))]
    if "7" in fdict:
        seven = frow == fdict.index("7")
        filters.append((Q.SelectorDimFilter("f", "7"), seven))
        filters.append((Q.NotDimFilter(Q.SelectorDimFilter("f", "7")), ~seven))
    intervals = [(int(times[0]), int(times[-1]) + 1)] if n else [(0, 1)]
    if n > 2:
        intervals.append((int(times[n // 3]), int(times[-1])))
    for flt, fmask in filters:
        for iv in intervals:
            mask = fmask & _time_mask(times, iv)
            for strategy in ("useIndexes", "cursorOnly"):
                q = Q.SearchQuery(intervals=[iv], searchDimensions=dims, query={"type": "all"}, filter=flt,
                                  context={"searchStrategy": strategy})
                ids = [[np.arange(len(truth[d][0]), dtype=np.int32)] for d in dims]
                counts, plans = R.search_counts([seg], q, dims, ids)
                for k, d in enumerate(dims):
                    t = truth[d]
                    has_bitmaps = seg.path and not str(seg.path).startswith("incremental:")
                    index_plan = strategy == "useIndexes" and has_bitmaps
                    assert plans[0][k] == (N.SEARCH_PLAN_INDEX if index_plan else N.SEARCH_PLAN_CURSOR)
                    want = _expected(t[1], len(t[0]), mask, ids[k][0], t[2] if len(t) > 2 else None, index_plan)
                    assert np.array_equal(counts[k][0], want), (d, strategy, iv, flt, counts[k][0][:8], want[:8])


def _write(mods, path, times, dims, bitmap, comp):
    W, S = mods.W, mods.S
    spec = W.SegmentSpec(timestamps=np.asarray(times, np.int64), dims=dims, metrics={},
                         interval=(0, int(times[-1]) + 1 if len(times) else 1))
    return S.GpuSegment(W.write_segment(path, spec, bitmap=bitmap, compression=comp))


@pytest.mark.parametrize("bitmap", ["concise", "roaring"])
@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 62, 63, 2047, 65541])
def test_edge_row_counts(mods, tmp_path, bitmap, nrows):
    """A value in every row but one (a long one-fill with a flipped bit), a value only in the last row,
    a value in rows 0 and nrows - 1 only (a long zero-fill), at row counts around the 31-row Concise
    block, the 32-row bitset word and the 65536-row Roaring container."""
    W = mods.W
    r = np.arange(nrows)
    truth = {
        "allbut": _strings(W, np.where(r == nrows // 2, "y", "x").tolist()),
        "last": _strings(W, np.where(r == nrows - 1, "z", "a").tolist()),
        "ends": _strings(W, np.where((r == 0) | (r == nrows - 1), "e", "m").tolist()),
    }
    f = _strings(W, [str(x % 100) for x in r])
    dims = dict(truth, f=f)
    seg = _write(mods, str(tmp_path / "seg"), r * 10, dims, bitmap, "lz4")
    _check_segment(mods, seg, {d: (v[0], v[1]) for d, v in truth.items()}, r * 10, (f[1], f[0]))
    seg.close()


@pytest.mark.parametrize("bitmap", ["concise", "roaring"])
def test_many_small_bitmaps_and_histogram_paths(mods, tmp_path, bitmap):
    """3 000 values at ~10 rows each (bitmaps of a few words: one wave each) beside a 10 000-value
    dictionary (the cursor plan's global-atomic counters) and a 100-value one (its LDS counters)."""
    W = mods.W
    n = 30_000
    rng = np.random.default_rng(7)
    r = np.arange(n)
    truth = {"small": _strings(W, ["v%04d" % x for x in rng.integers(0, 3000, n)]),
             "big": _strings(W, ["b%05d" % (x % 10_000) for x in r]),
             "f": _strings(W, [str(x % 100) for x in r])}
    seg = _write(mods, str(tmp_path / "seg"), r, truth, bitmap, "lz4")
    assert len(truth["small"][0]) > 2900 and len(truth["big"][0]) == 10_000 and len(truth["f"][0]) == 100
    _check_segment(mods, seg, {d: (v[0], v[1]) for d, v in truth.items()}, r, (truth["f"][1], truth["f"][0]))
    seg.close()


@pytest.mark.parametrize("bitmap", ["concise", "roaring"])
def test_split_bitmaps(mods, tmp_path, bitmap):
    """330 000 rows alternating two values: each Concise bitmap is over 8 192 words and each Roaring
    bitmap five bitmap containers (about 40 KiB), so both are split into pieces at attach."""
    W = mods.W
    n = 330_000
    r = np.arange(n)
    alt = (["a", "b"], (r % 2).astype(np.int32))
    f = (sorted({str(x) for x in range(100)}), None)
    fd = {v: i for i, v in enumerate(f[0])}
    f = (f[0], np.array([fd[str(x % 100)] for x in range(100)], np.int32)[r % 100])
    seg = _write(mods, str(tmp_path / "seg"), r, {"alt": alt, "f": f}, bitmap, "uncompressed")
    _check_segment(mods, seg, {"alt": alt}, r, (f[1], f[0]))
    seg.close()


@pytest.mark.parametrize("bitmap", ["concise", "roaring"])
def test_long_runs(mods, tmp_path, bitmap):
    """Long runs (Roaring run containers, Concise one-fills) that start 1, 30 and 31 bits into a bitset
    word, and a bitmap of many literal words followed by a long fill (the workgroup path's queue)."""
    W = mods.W
    n = 70_100
    r = np.arange(n)
    in_run = ((r >= 1) & (r < 5000)) | ((r >= 5 * 1024 + 30) & (r < 12_000)) | ((r >= 12 * 1024 + 31) & (r < 70_000))
    mix = ((r < 8000) & (r % 2 == 0)) | ((r >= 10_000) & (r < 60_000))
    truth = {"run": _strings(W, np.where(in_run, "r", "q").tolist()),
             "mix": _strings(W, np.where(mix, "w", "o").tolist())}
    f = _strings(W, [str(x % 100) for x in r])
    seg = _write(mods, str(tmp_path / "seg"), r, dict(truth, f=f), bitmap, "lz4")
    _check_segment(mods, seg, {d: (v[0], v[1]) for d, v in truth.items()}, r, (f[1], f[0]))
    seg.close()


def _multi_rows(n):
    pool = [["a", "a"], ["a", "b"], ["b"], [], ["c", "c", "c"], ["a", "b", "c"]]
    return [pool[(i * 7 + i // 5) % len(pool)] for i in range(n)]


@pytest.mark.parametrize("bitmap,comp", [("concise", "lz4"), ("roaring", "uncompressed")])
def test_multi_value_duplicates(mods, O, tmp_path, bitmap, comp):
    """A row [a, a]: the index plan counts it once for a, the cursor plan twice."""
    W, S = mods.W, mods.S
    n = 500
    rows = _multi_rows(n)
    mv = W.encode_multi_strings(rows)
    f = W.encode_strings([str(x % 100) for x in range(n)])
    r = np.arange(n)
    seg = _write(mods, str(tmp_path / "seg"), r, {"tags": mv, "f": f}, bitmap, comp)
    o = O.OracleSegment(seg.path)
    off, vals = o.multi("tags")
    assert o.dictionary("tags") == [None, "a", "b", "c"]
    a = 1
    assert int(np.bincount(vals, minlength=4)[a]) > len({int(x) for x in np.repeat(r, np.diff(off))[vals == a]})
    _check_segment(mods, seg, {"tags": (o.dictionary("tags"), vals, off)}, r, (f[1], f[0]))
    seg.close()


def test_segment_from_rows(mods):
    """A dg_segment_from_rows segment has no bitmap index: every dimension takes the cursor plan."""
    I, Q = mods.I, mods.Q
    n = 3000
    rows = _multi_rows(n)
    idx = I.IncrementalIndex(["d", "tags", "f"], [("rows", "count", None)], rollup=False, interval=(0, n))
    for i in range(n):
        idx.add(i, {"d": "v%02d" % (i * i % 37), "tags": rows[i], "f": str(i % 100)})
    seg = idx.to_segment()
    spec = idx.to_spec()
    d, tags, f = spec.dims["d"], spec.dims["tags"], spec.dims["f"]
    lens = np.array([len(x) for x in tags[1]])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate([np.asarray(x, np.int32) for x in tags[1]])
    assert np.array_equal(spec.timestamps, np.arange(n))
    assert seg.dictionary("d") == [v or None for v in d[0]] and seg.dictionary("tags") == [v or None for v in tags[0]]
    _check_segment(mods, seg, {"d": (d[0], np.asarray(d[1])), "tags": (tags[0], flat, off)}, np.arange(n),
                   (np.asarray(f[1]), list(f[0])))
    seg.close()


# ----------------------------------------------------------------------------------------------
# 4. limits
# ----------------------------------------------------------------------------------------------
def test_limits(mods, sample_segs, tmp_path):
    Q, R, N, W = mods.Q, mods.R, mods.N, mods.W
    seg = sample_segs[("concise", "lz4")]
    # index plan: once the map holds 3 hits it returns, in (dimension, id) order, with full counts
    q = Q.SearchQuery(intervals=FULL, searchDimensions=["quality", "market"], query="a", limit=3)
    got = R.run_query(q, [seg])
    assert [(h["dimension"], h["value"], h["count"]) for h in got[0].value] == \
        [("quality", "automotive", 93), ("quality", "entertainment", 93), ("quality", "health", 93)]
    q = Q.SearchQuery(intervals=FULL, searchDimensions=["market", "quality"], query="a", limit=3, sort="strlen")
    got = R.run_query(q, [seg])
    assert [(h["dimension"], h["value"], h["count"]) for h in got[0].value] == \
        [("quality", "automotive", 93), ("market", "total_market", 186), ("quality", "entertainment", 93)]
    # cursor plan: the limit reached is refused, one below it is exact
    for lim, ok in ((5, False), (6, True)):
        q = Q.SearchQuery(intervals=FULL, searchDimensions=["quality"], query="a", limit=lim,
                          context={"searchStrategy": "cursorOnly"})
        if ok:
            assert _triples(R.run_query(q, [seg])) == sorted(
                [("quality", "automotive", 93), ("quality", "mezzanine", 279), ("quality", "travel", 93),
                 ("quality", "health", 93), ("quality", "entertainment", 93)])
        else:
            with pytest.raises(N.UnsupportedQuery):
                R.run_query(q, [seg])
    # a limit at or above maxSearchLimit: the runners stop at 1000 hits each
    n = 6000
    vals = ["k%04d" % (i % 3000) for i in range(n)]
    d = W.encode_strings(vals)
    big = [_write(mods, str(tmp_path / f"big{i}"), np.arange(n), {"d": d}, "roaring", "lz4") for i in range(2)]
    q = Q.SearchQuery(intervals=FULL, searchDimensions=["d"], limit=5000)
    got = R.run_query(q, big)
    assert len(got) == 1 and got[0].value == [{"dimension": "d", "value": "k%04d" % i, "count": 4} for i in range(1000)]
    q = Q.SearchQuery(intervals=FULL, searchDimensions=["d"], limit=999)
    assert len(R.run_query(q, big)[0].value) == 999
    for s in big:
        s.close()


# ----------------------------------------------------------------------------------------------
# 5. several segments in one call
# ----------------------------------------------------------------------------------------------
def test_multi_segment_equals_fold(mods, basic_dirs):
    Q, R, S = mods.Q, mods.R, mods.S
    segs = [S.GpuSegment(p) for p in basic_dirs[("roaring", "lz4")]]
    q = Q.SearchQuery(intervals=[(100_000, 900_000)], searchDimensions=["dimSequential", "dimZipf"],
                      query={"type": "regex", "pattern": "^1"}, limit=900,
                      filter=Q.NotDimFilter(Q.SelectorDimFilter("dimZipf", "1")))
    together = R.search_per_segment(segs, q)
    singles = [R.search_per_segment([s], q)[0] for s in segs]
    assert together == singles and all(len(r) == 1 and r[0].value for r in together)
    merged = R.run_query(q, segs)
    assert merged == R.merge_search(q, singles) and len(merged) == 1
    total = {}
    for rs in singles:
        for h in rs[0].value:
            total[(h["dimension"], h["value"])] = total.get((h["dimension"], h["value"]), 0) + h["count"]
    assert {(h["dimension"], h["value"]): h["count"] for h in merged[0].value} == total
    runner = R.SearchQueryRunnerFactory().createRunner(segs[1])
    assert runner.run(q) == singles[1]
    for s in segs:
        s.close()


# ----------------------------------------------------------------------------------------------
# 6. argument errors
# ----------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(mods, sample_segs):
    Q, R, N = mods.Q, mods.R, mods.N
    seg = sample_segs[("roaring", "lz4")]
    q = Q.SearchQuery(intervals=FULL, searchDimensions=["quality"], query="a")
    card = seg.cardinality("quality")
    for ids, code in (([3, 1], 6), ([1, 1], 6), ([0, card], 6), ([-1], 6)):
        with pytest.raises(N.DruidGpuError) as e:
            R.search_counts([seg], q, ["quality"], [[np.array(ids, np.int32)]])
        assert e.value.code == code, ids
    with pytest.raises(N.UnsupportedQuery):
        R.search_counts([seg], q, ["qualityLong"], [[np.array([0], np.int32)]])
    with pytest.raises(N.UnsupportedQuery):
        R.run_query(Q.SearchQuery(intervals=FULL, searchDimensions=["qualityDouble"], query="1"), [seg])
    got = R.run_query(q, [seg])
    assert _triples(got) == sorted([("quality", "automotive", 93), ("quality", "mezzanine", 279),
                                    ("quality", "travel", 93), ("quality", "health", 93),
                                    ("quality", "entertainment", 93)])
