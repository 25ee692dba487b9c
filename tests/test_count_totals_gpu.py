"""The first radix pass's digit totals taken from cached per-value row counts (dg_sort.hip:
k_rs_totals_counts; dg_engine.cpp: Column::vcnt). When every row of every segment is an element and the
first sort digit lies inside the last dimension's key field, the totals k_rs_hist0 would count from the
elements are a function of how often each dictionary id occurs in each segment and of the merged
dictionary's maps. The first eligible groupBy over a segment builds the counts (and still runs
k_rs_hist0); later ones read them. dg_debug_groupby_totals_source tells which ran: 0 the histogram
kernel, 1 the counts.

Every result is compared bit for bit with the same query under DG_NO_COUNT_TOTALS=1 (keys, long sums,
double sums: the totals only place the digits' output ranges, the stable order is the same) and with
the oracle. Segments hold 20,000 rows (id blocks of at least 8,192 rows, so the generated first pass
is reachable) unless the case is about a tile edge."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

from compare import assert_results

pytestmark = pytest.mark.gpu

IV = [(0, 1 << 40)]
ROWS = 20_000


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("incubator-druid_amd.segment")


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


def _metrics(rng, n):
    return {"m": ("long", rng.integers(-1000, 1000, n)), "x": ("double", rng.integers(-40, 40, n) * 0.125)}


def _times(rng, n):
    return np.sort(rng.integers(0, 6 * 3_600_000, n)).astype(np.int64)


def _spec(W, n, seed, a=(0, 300), b=(0, 1000), with_b=True):
    """Dimension a uniform in [a), b uniform in [b): other ranges give other dictionaries, so the merged
    dictionary's maps are not the identity."""
    rng = np.random.default_rng(seed)
    dims = {"a": W.encode_int_strings(rng.integers(a[0], a[1], n))}
    if with_b:
        dims["b"] = W.encode_int_strings(rng.integers(b[0], b[1], n))
    return W.SegmentSpec(timestamps=_times(rng, n), dims=dims, metrics=_metrics(rng, n))


def _open(S, O, paths):
    return [S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]


def _write(W, S, O, base, specs):
    return _open(S, O, [W.write_segment(str(base / f"s{i}"), sp, lz4_mode="fast") for i, sp in enumerate(specs)])


def _gb(Q, dims=("a", "b"), aggs=None, **kw):
    return Q.GroupByQuery(intervals=IV, dimensions=list(dims),
                          aggregations=aggs or [Q.long_sum("m", "m"), Q.double_sum("x", "x")], **kw)


def _source(N, g):
    src = ctypes.c_int32(-1)
    N.check(N.lib().dg_debug_groupby_totals_source(g[0].context.handle, ctypes.byref(src)))
    return src.value


def _run(R, N, monkeypatch, q, g, counts=True):
    """One dg_groupby_run with the counts allowed or switched off: the fetched groups and the source of
    the first pass's totals."""
    monkeypatch.setenv("DG_NO_COUNT_TOTALS", "0" if counts else "1")
    res = R.groupby_run(g, q, R.RunStats())
    try:
        return res.fetch(), _source(N, g)
    finally:
        res.release()


def _same_bits(a, b):
    assert len(a) == len(b)
    assert np.array_equal(a.times, b.times)
    for ca, cb in zip(a.codes, b.codes):
        assert np.array_equal(ca, cb)
    assert a.dicts == b.dicts
    for va, vb in zip(a.aggs, b.aggs):
        va, vb = np.ascontiguousarray(va), np.ascontiguousarray(vb)
        assert va.dtype == vb.dtype and np.array_equal(va.view(np.uint8), vb.view(np.uint8))  # doubles by their bits


def _check(R, N, O, monkeypatch, q, g, o, sources):
    """Runs q len(sources) times with the counts allowed: call k's totals come from sources[k]; every
    result equals, bit for bit, the run with DG_NO_COUNT_TOTALS=1 (source 0), and the oracle's."""
    off, s_off = _run(R, N, monkeypatch, q, g, counts=False)
    assert s_off == 0
    for want in sources:
        got, src = _run(R, N, monkeypatch, q, g)
        assert src == want
        _same_bits(got, off)
    monkeypatch.setenv("DG_NO_COUNT_TOTALS", "0")
    assert_results(q, R.run_query(q, g), O.run(q, o))


def test_remapped_dictionaries_three_calls(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """Cardinalities of about 1,000 (last) and 300; the three segments' dictionaries differ (shifted value
    ranges), so both dimensions are remapped. The merged dictionaries take 9 + 11 key bits: three digits
    of 7 bits, the first inside b's field."""
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 11), _spec(W, ROWS, 12, a=(150, 450), b=(500, 1500)),
                                      _spec(W, ROWS, 13, a=(100, 400), b=(250, 1250))])
    assert g[0].dictionary("b") != g[1].dictionary("b") != g[2].dictionary("b")
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [0, 1, 1])


def test_first_digit_straddles_two_fields(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """The last dimension has 5 values (3 bits) under a 300-value one (9 bits): two digits of 6 bits, the
    first reaching into a's field. The histogram kernel stays, and nothing is built."""
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 21, b=(0, 5)), _spec(W, ROWS, 22, a=(100, 400), b=(0, 5))])
    before = [s.device_bytes() for s in g]
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [0, 0, 0])
    assert [s.device_bytes() for s in g] == before


def test_missing_dimension_and_tile_edges(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """A segment without the last dimension adds its rows to the null value's digit; a one-row segment and
    segments of exactly one sort tile (4,096 rows) and one row more sit between full-size ones."""
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 31), _spec(W, ROWS, 32, a=(150, 450), with_b=False),
                                      _spec(W, 1, 33, b=(700, 1200)), _spec(W, 4096, 34, b=(300, 1300)),
                                      _spec(W, 4097, 35, b=(600, 1600))])
    assert "b" not in g[1].columns() and [s.num_rows for s in g[2:]] == [1, 4096, 4097]
    _check(R, N, O, monkeypatch, _gb(Q), g[:3], o[:3], [0, 1, 1])
    # the small segments' counts are missing: built by the next call, used by the one after
    _check(R, N, O, monkeypatch, _gb(Q), [g[3], g[4], g[0]], [o[3], o[4], o[0]], [0, 1])
    _check(R, N, O, monkeypatch, _gb(Q), [g[1], g[4]], [o[1], o[4]], [1])
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [1])


def test_ineligible_queries_keep_the_histogram(Q, O, W, R, N, S, tmp_path, monkeypatch):
    rng = np.random.default_rng(41)
    specs = [_spec(W, ROWS, 42), _spec(W, ROWS, 43, a=(150, 450), b=(500, 1500))]
    for sp in specs:
        sp.dims["mv"] = W.encode_multi_strings([[str(v) for v in rng.integers(0, 1000, rng.integers(0, 3))]
                                                for _ in range(ROWS)])
    g, o = _write(W, S, O, tmp_path, specs)
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [0, 1])
    # a filter: the elements are the selected rows
    _check(R, N, O, monkeypatch, _gb(Q, filter=Q.SelectorDimFilter("a", "200")), g, o, [0])
    # a multi-value last dimension: a row is one element per value
    _check(R, N, O, monkeypatch, _gb(Q, dims=("a", "mv")), g, o, [0, 0])
    # floatSum: not a rows-are-elements call
    _check(R, N, O, monkeypatch, _gb(Q, aggs=[Q.long_sum("m", "m"), Q.double_sum("x", "x"), Q.float_sum("f", "x")]),
           g, o, [0])
    # the plain query is back on the counts
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [1])


def test_hourly_groupby_over_time_chunks(Q, O, R, N, S, tmp_path, monkeypatch):
    """Hour granularity over two time chunks (the benchmark's groupby_hourly): the keygen writes the sort
    words, and the sort over them takes its first totals from the counts all the same."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench as B
    paths = [B._write_one((str(tmp_path / f"seg{i}"), ROWS, 9999 + i, "concise", "lz4", "fast", i, "longs", B.BASIC))
             for i in range(2)]
    g, o = _open(S, O, paths)
    _check(R, N, O, monkeypatch, B.make_query(Q, "groupby_hourly"), g, o, [0, 1])


def test_last_in_one_query_first_in_another(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """(a, b) builds b's counts; (b, a) neither needs nor builds b's: it builds a's own."""
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 61, a=(0, 700)), _spec(W, ROWS, 62, a=(300, 1000), b=(500, 1500))])
    base = [s.device_bytes() for s in g]
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [0, 1])
    with_b = [s.device_bytes() for s in g]
    assert [w - b for w, b in zip(with_b, base)] == [4 * s.cardinality("b") for s in g]
    _check(R, N, O, monkeypatch, _gb(Q, dims=("b", "a")), g, o, [0, 1])
    assert [x - w for x, w in zip((s.device_bytes() for s in g), with_b)] == [4 * s.cardinality("a") for s in g]


def test_device_bytes_grow_once(Q, O, W, R, N, S, tmp_path, monkeypatch):
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 71), _spec(W, ROWS, 72, b=(500, 1500))])
    base = [s.device_bytes() for s in g]
    _, src = _run(R, N, monkeypatch, _gb(Q), g, counts=False)  # switched off: nothing is built
    assert src == 0 and [s.device_bytes() for s in g] == base
    _, src = _run(R, N, monkeypatch, _gb(Q), g)
    grown = [s.device_bytes() for s in g]
    assert src == 0 and [x - b for x, b in zip(grown, base)] == [4 * s.cardinality("b") for s in g]
    for _ in range(2):
        _, src = _run(R, N, monkeypatch, _gb(Q), g)
        assert src == 1 and [s.device_bytes() for s in g] == grown
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [1])


def test_hash_grouper_unchanged(Q, O, W, R, N, S, tmp_path, monkeypatch):
    g, o = _write(W, S, O, tmp_path, [_spec(W, ROWS, 81), _spec(W, ROWS, 82, a=(150, 450), b=(500, 1500))])
    q = _gb(Q, context={"forceHashAggregation": True})
    res = R.groupby_run(g, q, R.RunStats())
    try:
        assert res.grouper_info()["grouper"] == N.GROUPER_HASH
    finally:
        res.release()
    _check(R, N, O, monkeypatch, q, g, o, [0, 0])
    _check(R, N, O, monkeypatch, _gb(Q), g, o, [0, 1])
    _check(R, N, O, monkeypatch, q, g, o, [0])
