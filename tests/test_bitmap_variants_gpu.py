"""The bitmap kernels against every legal encoding of the same rows (tests/bitmap_variants.py).

Filter path: k_concise_or, k_roaring_or and k_roaring_pieces through GpuSegment.filter_bitmap. Search
index plan: k_search_concise_count and k_search_roaring_count through search_counts under useIndexes.
Expected rows and counts are numpy over the shapes' masks (and, for the ImmutableConciseSetTest
compaction pairs, the oracle's decode of the word lists); test_bitmap_variants.py holds the encoders
to the oracle on the CPU, so a mismatch here is the kernel's. All comparisons are exact.
"""
import importlib

import numpy as np
import pytest

import bitmap_variants as BV

pytestmark = pytest.mark.gpu

N = BV.N_ROWS
DIMS = list(BV.shapes())


@pytest.fixture(scope="module")
def mods():
    class M:
        R = importlib.import_module("incubator-druid_amd.runners")
        N = importlib.import_module("incubator-druid_amd._native")
        S = importlib.import_module("incubator-druid_amd.segment")
    return M


@pytest.fixture(scope="module")
def segs(mods, W, tmp_path_factory):
    """One attached segment per (bitmap type, variant), written once for the module."""
    base = tmp_path_factory.mktemp("bitmap_variants_gpu")
    out = {(k, v): mods.S.GpuSegment(BV.write_variant_segment(W, str(base / f"{k}_{v}"), k, v)) for k, v in BV.VARIANTS}
    yield out
    for s in out.values():
        s.close()


def _bits(seg, flt, Q):
    words, cnt = seg.filter_bitmap(flt.optimize(), Q)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:seg.num_rows].astype(bool), cnt


def _compound(Q):
    """OR(AND(half, NOT edges), cards) over three dimensions, and its rows."""
    s = BV.shapes()
    flt = Q.OrDimFilter([Q.AndDimFilter([Q.SelectorDimFilter("half", "in"),
                                         Q.NotDimFilter(Q.SelectorDimFilter("edges", "in"))]),
                         Q.SelectorDimFilter("cards", "in")])
    return flt, (s["half"] & ~s["edges"]) | s["cards"]


@pytest.mark.parametrize("kind,variant", BV.VARIANTS)
def test_filter_path(mods, Q, segs, kind, variant):
    seg = segs[(kind, variant)]
    assert seg.num_rows == N
    for name, mask in BV.shapes().items():
        for side in BV.SIDES:
            want = mask if side == "in" else ~mask
            got, cnt = _bits(seg, Q.SelectorDimFilter(name, side), Q)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (kind, variant, name, side, len(bad), bad[:8].tolist())
            assert cnt == int(want.sum()), (kind, variant, name, side)
        # both bitmaps of the dimension expanded by one launch into one target: every row
        got, cnt = _bits(seg, Q.InDimFilter(name, list(BV.SIDES)), Q)
        assert got.all() and cnt == N, (kind, variant, name, int(got.sum()))
    flt, want = _compound(Q)
    got, cnt = _bits(seg, flt, Q)
    assert np.array_equal(got, want) and cnt == int(want.sum()), (kind, variant)


@pytest.mark.parametrize("kind,variant", BV.VARIANTS)
def test_search_index_plan(mods, Q, segs, kind, variant):
    """Per-value counts of every shape dimension in one call: unfiltered, under a filter bitset (a
    selector on another shape dimension) and under an interval that cuts the segment."""
    R = mods.R
    seg = segs[(kind, variant)]
    s = BV.shapes()
    r = np.arange(N)
    cut = (N // 3, N - 5)
    ways = [("all", (0, N), None, np.ones(N, bool)),
            ("filter", (0, N), Q.SelectorDimFilter("half", "in"), s["half"]),
            ("dense filter", (0, N), Q.SelectorDimFilter("sparse", "out"), ~s["sparse"]),
            ("interval", cut, None, (r >= cut[0]) & (r < cut[1])),
            ("filter + interval", cut, Q.SelectorDimFilter("four", "in"), s["four"] & (r >= cut[0]) & (r < cut[1]))]
    ids = [[np.arange(2, dtype=np.int32)] for _ in DIMS]
    for label, iv, flt, sel in ways:
        q = Q.SearchQuery(intervals=[iv], searchDimensions=DIMS, query={"type": "all"}, filter=flt,
                          context={"searchStrategy": "useIndexes"})
        counts, plans = R.search_counts([seg], q, DIMS, ids)
        for d, name in enumerate(DIMS):
            assert plans[0][d] == mods.N.SEARCH_PLAN_INDEX
            want = [int((s[name] & sel).sum()), int((~s[name] & sel).sum())]
            assert counts[d][0].tolist() == want, (kind, variant, label, name, counts[d][0].tolist(), want)


@pytest.mark.parametrize("kind,variant", BV.VARIANTS)
def test_timeseries_count_under_the_compound_filter(mods, Q, segs, kind, variant):
    flt, want = _compound(Q)
    q = Q.TimeseriesQuery(intervals=[(0, N)], aggregations=[Q.count("rows")], filter=flt)
    res = mods.R.run_query(q, [segs[(kind, variant)]])
    assert len(res) == 1 and res[0].value["rows"] == int(want.sum()), (kind, variant)


def test_compact_pairs(mods, Q, W, O, kats, tmp_path):
    """The 23 ImmutableConciseSetTest compaction pairs as they stand: a pair's uncompacted and compacted
    word lists expand to the same bitset, the oracle's rows, and count the same under a selection."""
    lists = BV.pair_lists(kats)
    seg = mods.S.GpuSegment(BV.write_pairs_segment(W, str(tmp_path / "pairs"), kats))
    names = [n for n, _ in lists]
    assert seg.dictionary("pairs") == names
    rows = [O.concise_rows(BV._be(words)) for _, words in lists]
    sets = []
    for k, name in enumerate(names):
        got, cnt = _bits(seg, Q.SelectorDimFilter("pairs", name), Q)
        assert np.flatnonzero(got).tolist() == rows[k].tolist() and cnt == len(rows[k]), (name, lists[k][1])
        sets.append(got)
        if k % 2:
            assert np.array_equal(got, sets[k - 1]), name
    ids = [[np.arange(len(names), dtype=np.int32)]]
    # the selections: none (the bitmap's own cardinality), the rows of a list made of two one-fills, of
    # one made of zero-fills and a literal, and an interval
    fill_fill, zero_lit = names.index("p05a"), names.index("p11a")
    for flt_k, iv in ((None, (0, BV.PAIR_ROWS)), (fill_fill, (0, BV.PAIR_ROWS)), (zero_lit, (0, BV.PAIR_ROWS)),
                      (None, (33, 300))):
        sel = np.ones(BV.PAIR_ROWS, bool) if flt_k is None else sets[flt_k].copy()
        sel[:iv[0]] = False
        sel[iv[1]:] = False
        flt = None if flt_k is None else Q.SelectorDimFilter("pairs", names[flt_k])
        q = Q.SearchQuery(intervals=[iv], searchDimensions=["pairs"], query={"type": "all"}, filter=flt,
                          context={"searchStrategy": "useIndexes"})
        counts, plans = mods.R.search_counts([seg], q, ["pairs"], ids)
        assert plans[0][0] == mods.N.SEARCH_PLAN_INDEX
        want = [int(sel[r].sum()) for r in rows]
        assert counts[0][0].tolist() == want, (flt_k, iv)
        assert counts[0][0][0::2].tolist() == counts[0][0][1::2].tolist()
    seg.close()
