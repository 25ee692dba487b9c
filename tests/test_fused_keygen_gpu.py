"""The groupBy keygen fused into the first radix pass (dg_sort.hip: k_rs_scatter / k_rs_hist0 with the
generated source, launch_gb_sort_generated): when the query has no filter, no multi-value dimension,
no time bucket and every aggregator input is decoded in place, the sort word of an element is a
function of its index, so the first pass forms it in registers from the id columns and k_gb_keygen
does not run. dg_metrics.keygen_ms is then exactly 0.0 (with phase timing on).

Every eligible shape is run three ways: against the oracle, with the generated first pass, and with
DG_NO_FUSED_KEYGEN=1 (k_gb_keygen + the unchanged passes). The two GPU runs must agree bit for bit —
keys, order, long sums and double sums: the sorted order is the same stable order, so the double
sums add up in the same order. Ineligible shapes must take the keygen and still equal the oracle.

Metric columns here hold values LZ4 finds matches in: a literal-only block is viewed in place instead
of decoded into the payload records, which leaves the column to the keygen."""
import importlib
import os
import sys

import numpy as np
import pytest

from compare import assert_results

pytestmark = pytest.mark.gpu

IV = [(0, 1 << 40)]


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


def _open(S, O, paths):
    return [S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]


def _run(R, N, monkeypatch, q, g, fused):
    """One dg_groupby_run with the generated first pass allowed (fused) or switched off: the fetched
    groups, the call's metrics and the grouper that ran."""
    monkeypatch.setenv("DG_NO_FUSED_KEYGEN", "0" if fused else "1")
    N.lib().dg_set_phase_timing(1)
    stats = R.RunStats()
    res = R.groupby_run(g, q, stats)
    try:
        return res.fetch(), stats.calls[-1], res.grouper_info()
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


def _check_fused(R, N, O, monkeypatch, q, g, o):
    """Eligible query: the generated pass runs (keygen_ms == 0.0), the switch brings the keygen back,
    both agree bit for bit and with the oracle."""
    new, m_new, _ = _run(R, N, monkeypatch, q, g, True)
    old, m_old, _ = _run(R, N, monkeypatch, q, g, False)
    assert m_new["keygen_ms"] == 0.0 and m_old["keygen_ms"] > 0
    assert m_new["sort_passes"] == m_old["sort_passes"] and m_new["key_bits"] == m_old["key_bits"]
    assert m_new["selected_rows"] == m_old["selected_rows"] == sum(s.num_rows for s in g)
    _same_bits(new, old)
    monkeypatch.setenv("DG_NO_FUSED_KEYGEN", "0")
    assert_results(q, R.run_query(q, g), O.run(q, o))


def _check_keygen(R, N, O, monkeypatch, q, g, o):
    """Ineligible query: k_gb_keygen runs whatever the switch says, the result equals the oracle."""
    new, m_new, info = _run(R, N, monkeypatch, q, g, True)
    assert m_new["keygen_ms"] > 0
    assert_results(q, R.run_query(q, g), O.run(q, o))
    return new, info


def _two_dim_spec(W, n, seed, card_a=300, card_b=50):
    rng = np.random.default_rng(seed)
    return W.SegmentSpec(timestamps=_times(rng, n),
                         dims={"a": W.encode_int_strings(rng.integers(0, card_a, n)),
                               "b": W.encode_int_strings(rng.zipf(1.3, n) % card_b)},
                         metrics=_metrics(rng, n))


@pytest.fixture(scope="module")
def straddle(tmp_path_factory, W, S, O):
    """Three segments of 5,000, 4,097 and 1 rows: the sort tiles (4,096 elements) straddle both segment
    boundaries, a wave's share of a tile holds rows of two and of three segments, and the last tile
    holds one element."""
    base = tmp_path_factory.mktemp("fused_straddle")
    paths = [W.write_segment(str(base / f"s{i}"), _two_dim_spec(W, n, 21 + i), lz4_mode="fast")
             for i, n in enumerate((5000, 4097, 1))]
    return _open(S, O, paths)


def _gb(Q, dims=("a", "b"), aggs=None, **kw):
    return Q.GroupByQuery(intervals=IV, dimensions=list(dims),
                          aggregations=aggs or [Q.long_sum("m", "m"), Q.double_sum("x", "x")], **kw)


def test_tiles_straddle_segments(Q, O, R, N, straddle, monkeypatch):
    g, o = straddle
    assert [s.num_rows for s in g] == [5000, 4097, 1]
    _check_fused(R, N, O, monkeypatch, _gb(Q), g, o)
    # every pair and the first segment alone: other bases, a last tile of 5,000 - 4,096 = 904 elements
    for sub in ([0, 1], [1, 2], [0, 2], [0]):
        _check_fused(R, N, O, monkeypatch, _gb(Q), [g[i] for i in sub], [o[i] for i in sub])
    # The one-row segment's 8-byte LZ4 blocks are literal-only: viewed, not decoded into the payload
    # records, which the keygen then writes over that segment's tile (the calls above). Alone, it is
    # the whole call, and the keygen runs as ever.
    _check_keygen(R, N, O, monkeypatch, _gb(Q), g[2:], o[2:])


def test_wide_look_back_status(Q, O, R, N, straddle, monkeypatch):
    monkeypatch.setenv("DG_SORT_WIDE_STATUS", "1")
    g, o = straddle
    _check_fused(R, N, O, monkeypatch, _gb(Q), g, o)


def test_every_id_width_in_one_query(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """Dimensions of 1-, 2-, 3- and 4-byte ids in one key (b: 50 values, a: 300 values, both numBytes by
    cardinality as in test_id_widths; c and d written 3 and 4 bytes wide on request). 70,000 rows: the
    3- and 4-byte columns hold 16,384 rows per block, the 1-byte column 65,536, so sort tiles cross
    block boundaries of some columns inside a block of the others; behind a 1,000-row segment the
    tiles (and a wave's share of them) are not aligned to any block, so one share reads two blocks."""
    widths = {"c": 3, "d": 4}
    part = W.string_column_part
    forced = []

    def spec(n, seed):
        rng = np.random.default_rng(seed)
        sp = _two_dim_spec(W, n, seed)
        # distinct dictionary sizes name the column inside string_column_part
        sp.dims["c"] = W.encode_int_strings(rng.permutation(n) % 400)
        sp.dims["d"] = W.encode_int_strings(rng.permutation(n) % 70)
        return sp

    def write(path, sp):
        by_card = {len(sp.dims[k][0]): w for k, w in widths.items()}
        assert len(by_card) == 2 and not set(by_card) & {len(sp.dims["a"][0]), len(sp.dims["b"][0])}

        def part_by_card(dictionary, ids, bitmap, compression, lz4_mode, num_bytes=None):
            if len(dictionary) in by_card:
                forced.append((len(dictionary), by_card[len(dictionary)]))
            return part(dictionary, ids, bitmap, compression, lz4_mode, by_card.get(len(dictionary), num_bytes))
        monkeypatch.setattr(W, "string_column_part", part_by_card)
        try:
            return W.write_segment(path, sp, lz4_mode="fast")
        finally:
            monkeypatch.setattr(W, "string_column_part", part)

    big, lead = spec(70_000, 31), spec(1000, 32)
    g, o = _open(S, O, [write(str(tmp_path / "lead"), lead), write(str(tmp_path / "big"), big)])
    assert sorted(forced) == [(70, 4), (70, 4), (400, 3), (400, 3)]  # (a: 300 values, 2 bytes; b: 50 values, 1 byte)
    q = _gb(Q, dims=("a", "b", "c", "d"))
    _check_fused(R, N, O, monkeypatch, q, g[1:], o[1:])
    _check_fused(R, N, O, monkeypatch, q, g, o)
    _check_fused(R, N, O, monkeypatch, _gb(Q, dims=("d", "c")), g, o)


def test_missing_dimension_and_remap(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """Dimension b is absent from the second segment (its rows group under null: null_gid) and a's
    dictionaries differ between the segments (values 0..299 against 150..449: the merged dictionary
    remaps both)."""
    rng = np.random.default_rng(41)
    n0, n1 = 6000, 5000
    s0 = _two_dim_spec(W, n0, 42)
    s1 = W.SegmentSpec(timestamps=_times(rng, n1), dims={"a": W.encode_int_strings(rng.integers(150, 450, n1))},
                       metrics=_metrics(rng, n1))
    g, o = _open(S, O, [W.write_segment(str(tmp_path / "s0"), s0, lz4_mode="fast"),
                        W.write_segment(str(tmp_path / "s1"), s1, lz4_mode="fast")])
    assert g[0].dictionary("a") != g[1].dictionary("a") and "b" not in g[1].columns()
    _check_fused(R, N, O, monkeypatch, _gb(Q), g, o)
    _check_fused(R, N, O, monkeypatch, _gb(Q, dims=("b", "a")), list(reversed(g)), list(reversed(o)))


def test_ineligible_shapes_take_the_keygen(Q, O, W, R, N, S, straddle, tmp_path, monkeypatch):
    g, o = straddle
    # a filter: the elements are the selected rows, not the rows
    _check_keygen(R, N, O, monkeypatch, _gb(Q, filter=Q.SelectorDimFilter("b", "1")), g, o)
    # floatSum: its row-order pass reads the keygen's per-tile counts
    _check_keygen(R, N, O, monkeypatch,
                  _gb(Q, aggs=[Q.long_sum("m", "m"), Q.double_sum("x", "x"), Q.float_sum("f", "x")]), g, o)
    # a multi-value dimension: a row is one element per value
    rng = np.random.default_rng(51)
    n = 5000
    rows = [[str(v) for v in rng.integers(0, 30, rng.integers(0, 4))] for _ in range(n)]
    sp = _two_dim_spec(W, n, 52)
    sp.dims["mv"] = W.encode_multi_strings(rows)
    gm, om = _open(S, O, [W.write_segment(str(tmp_path / "mv"), sp, lz4_mode="fast")])
    _check_keygen(R, N, O, monkeypatch, _gb(Q, dims=("a", "mv")), gm, om)
    # the same segment grouped by its single-value dimensions is eligible
    _check_fused(R, N, O, monkeypatch, _gb(Q), gm, om)
    # the hash grouper
    q = _gb(Q, context={"forceHashAggregation": True})
    monkeypatch.setenv("DG_NO_FUSED_KEYGEN", "0")
    stats = R.RunStats()
    res = R.groupby_run(g, q, stats)
    try:
        assert res.grouper_info()["grouper"] == N.GROUPER_HASH
    finally:
        res.release()
    assert_results(q, R.run_query(q, g), O.run(q, o))


def test_hourly_groupby_keeps_the_keygen(Q, O, R, N, S, tmp_path, monkeypatch):
    """The time-bucketed groupBy (the hourly query of test_cfg5_gpu over two small time chunks of the
    same generator) is not fused: its bucket comes from __time. It runs k_gb_keygen as before."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench as B
    paths = [B._write_one((str(tmp_path / f"seg{i}"), 30_000, 9999 + i, "concise", "lz4", "fast", i, "longs", B.BASIC))
             for i in range(2)]
    g, o = _open(S, O, paths)
    q = B.make_query(Q, "groupby_hourly")
    new, info = _check_keygen(R, N, O, monkeypatch, q, g, o)
    assert info["grouper"] == N.GROUPER_SORT
    old, m_old, _ = _run(R, N, monkeypatch, q, g, False)
    assert m_old["keygen_ms"] > 0
    _same_bits(new, old)
