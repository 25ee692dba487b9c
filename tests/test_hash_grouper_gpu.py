"""The opt-in hash grouper on the GPU (dg_groupby_run_opts with DG_GROUPER_HASH: k_gb_hash_insert /
k_gb_hash_collect / k_gb_hash_emit, BufferHashGrouper.java:38-133 over ByteBufferHashTable.java:286-327).

Every case runs one query three ways: forced hash (context forceHashAggregation), the default sort
path of the same call, and the CPU oracle. Hash and sort must agree exactly on times, dimension ids,
dictionaries, rows and every count / long* / min / max slot (NaN positions and the sign of zero
included); doubleSum within compare.TOL["double"] (atomic adds arrive in any order), its inputs of one
sign per group. The shapes are the smallest at which each mechanism can go wrong: one group (every
element on one LDS entry and one table position), few groups (all in LDS), about one group per row
(every LDS table overflows: flush + direct path), keys that do not share a word with their
reference, a multi-value dimension, a 4,097-row segment (a one-element last tile)."""
import dataclasses
import importlib
import math

import numpy as np
import pytest

from compare import TOL, assert_results

ALL = ["1970-01-01T00:00:00Z/1970-01-01T00:16:40Z"]  # the basic schema's interval [0, 1,000,000) ms


@pytest.fixture(scope="module")
def mods():
    m = {k: importlib.import_module("incubator-druid_amd." + v)
         for k, v in (("R", "runners"), ("S", "segment"), ("N", "_native"), ("I", "incremental"))}
    return type("M", (), m)


@pytest.fixture(scope="module")
def basic(DG, O, mods, tmp_path_factory):
    """2 segments x 20,000 rows of the basic schema (seeds 9999, 10000: their dimUniform dictionaries differ)."""
    paths = DG.write_basic_dataset(str(tmp_path_factory.mktemp("hashgb")), 2, 20_000, lz4_mode="fast")
    return [mods.S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]


def _hash(q, **extra):
    return dataclasses.replace(q, context={**(q.context or {}), "forceHashAggregation": True, **extra})


def _run(mods, segs, q):
    """(partial, rows per group, grouper info) of one engine call."""
    res = mods.R.groupby_run(segs, q)
    try:
        part = res.fetch()
        rows = np.zeros(max(res.groups, 1), np.int64)
        if res.groups:
            mods.N.check(mods.N.lib().dg_result_fetch_rows(res.handle, 0, res.groups, rows.ctypes.data))
        return part, rows[:res.groups], res.grouper_info()
    finally:
        res.release()


def _same(q, a, b):
    """Two engine results of one query: everything exact but doubleSum (TOL["double"])."""
    (pa, ra, _), (pb, rb, _) = a, b
    assert len(pa) == len(pb)
    assert np.array_equal(pa.times, pb.times)
    assert pa.dicts == pb.dicts
    for ca, cb in zip(pa.codes, pb.codes):
        assert np.array_equal(ca, cb)
    assert np.array_equal(ra, rb)
    for agg, xa, xb in zip(q.aggregations, pa.aggs, pb.aggs):
        if agg.type == "doubleSum":
            both_nan = np.isnan(xa) & np.isnan(xb)
            with np.errstate(invalid="ignore"):  # (inf - inf)
                ok = both_nan | (xa == xb) | (np.abs(xa - xb) <= TOL["double"] * np.maximum(np.abs(xa), np.abs(xb)))
            assert ok.all(), (agg.name, xa[~ok][:3], xb[~ok][:3])
        else:  # bit-equal: NaN positions and signed zeros too
            assert xa.tobytes() == xb.tobytes(), agg.name


def _check(mods, O, q, segs, osegs, hash_expected=True):
    """hash == oracle, hash == sort, and the grouper that ran; returns (hash run, sort run)."""
    h, s = _run(mods, segs, _hash(q)), _run(mods, segs, q)
    assert h[2]["grouper"] == (mods.N.GROUPER_HASH if hash_expected else mods.N.GROUPER_SORT)
    assert s[2]["grouper"] == mods.N.GROUPER_SORT and s[2]["table_slots"] == 0
    _same(q, h, s)
    exp = O.run(q, osegs)
    assert_results(q, mods.R.merge_groupby(q, [h[0]]), exp)
    return h, s


def _nine(Q):
    return [Q.count("n"), Q.long_sum("ls", "sumLongSequential"), Q.long_min("lmin", "maxLongUniform"),
            Q.long_max("lmax", "maxLongUniform"), Q.double_sum("ds", "sumFloatNormal"),
            Q.double_min("dmin", "minFloatZipf"), Q.double_max("dmax", "sumFloatNormal"),
            Q.float_min("fmin", "sumFloatNormal"), Q.float_max("fmax", "minFloatZipf")]


@pytest.mark.gpu
def test_one_group(Q, O, mods, basic):
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=[], aggregations=_nine(Q))
    h, _ = _check(mods, O, q, *basic)
    assert len(h[0]) == 1 and h[1].tolist() == [40_000]
    assert h[2]["direct_elements"] == 0
    assert h[2]["flushed_entries"] == math.ceil(40_000 / 4096)  # one LDS entry per insert tile


@pytest.fixture(scope="module")
def few_groups(Q, O, mods, basic):
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=["dimZipf"], aggregations=_nine(Q))
    return q, _check(mods, O, q, *basic)


@pytest.mark.gpu
def test_few_groups_fit_lds(few_groups):
    _, (h, _) = few_groups
    assert 1 < len(h[0]) <= 101
    assert h[2]["direct_elements"] == 0 and h[2]["flushed_entries"] >= len(h[0])


@pytest.mark.gpu
def test_sixteen_aggregators_smallest_lds_table(Q, O, mods, basic):
    aggs = _nine(Q) + [Q.long_sum("ls2", "maxLongUniform"), Q.long_min("lmin2", "sumLongSequential"),
                       Q.long_max("lmax2", "sumLongSequential"), Q.double_sum("ds2", "minFloatZipf"),
                       Q.double_min("dmin2", "sumFloatNormal"), Q.double_max("dmax2", "minFloatZipf"),
                       Q.float_max("fmax2", "sumFloatNormal")]
    assert len(aggs) == 16
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=["dimZipf"], aggregations=aggs)
    h, _ = _check(mods, O, q, *basic)
    # 101 groups against the 128-entry table of 144-byte entries, full at 0.7 x 128 = 89: both paths run
    assert h[2]["direct_elements"] > 0 and h[2]["flushed_entries"] > 0


@pytest.mark.gpu
def test_one_group_per_row_overflows_lds(Q, O, mods, basic):
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=["dimUniform", "dimHyperUnique"],
                       aggregations=[Q.count("n"), Q.long_sum("ls", "sumLongSequential"),
                                     Q.double_sum("ds", "sumFloatNormal"), Q.double_min("dmin", "minFloatZipf")])
    h, _ = _check(mods, O, q, *basic)
    assert len(h[0]) > 39_000
    assert h[2]["direct_elements"] > 0 and h[2]["flushed_entries"] > 0
    assert h[2]["table_slots"] == 65536  # next power of two >= 40,000 / 0.7


@pytest.mark.gpu
def test_buckets_filters_and_missing_dimensions(Q, O, mods, basic):
    flt = Q.SelectorDimFilter("dimZipf", "3")
    q = Q.GroupByQuery(intervals=["1970-01-01T00:00:10Z/1970-01-01T00:15:00Z"],  # cuts the first and last block
                       granularity={"type": "duration", "duration": 140_000},
                       dimensions=["dimSequential", "dimZipf", "dimNull", "dimSequentialHalfNull", "noSuchDim"],
                       filter=Q.BoundDimFilter("dimUniform", "20000", "80000", ordering="numeric"),
                       aggregations=[Q.count("n"), Q.filtered(Q.long_sum("fls", "sumLongSequential"), flt),
                                     Q.long_max("lmax", "maxLongUniform"), Q.double_sum("ds", "sumFloatNormal")])
    h, _ = _check(mods, O, q, *basic)
    assert len(set(h[0].times.tolist())) == 7


@pytest.mark.gpu
def test_key_and_reference_in_separate_words(Q, O, mods, basic):
    q = Q.GroupByQuery(intervals=ALL, granularity="all",
                       dimensions=["dimUniform", "dimHyperUnique", "dimSequential", "dimSequentialHalfNull"],
                       aggregations=[Q.count("n"), Q.long_min("lmin", "maxLongUniform"), Q.double_max("dmax", "sumFloatNormal")])
    res = mods.R.groupby_run(basic[0], q)
    try:
        card = [int(mods.N.lib().dg_result_dim_cardinality(res.handle, d)) for d in range(4)]
    finally:
        res.release()
    key_bits = sum(max(c - 1, 0).bit_length() for c in card)
    assert key_bits + 16 > 64  # neither the 16-bit row reference nor the 16-bit table position fits the key's word
    h, _ = _check(mods, O, q, *basic)
    assert h[2]["table_slots"] == 65536


@pytest.fixture(scope="module")
def tagged(W, O, mods, tmp_path_factory):
    """A 6,000-row in-memory index with a multi-value dimension (0-3 tags per row) and its persisted form."""
    rng = np.random.default_rng(11)
    idx = mods.I.IncrementalIndex(["dimA", "tags"], [("rows", "count", None), ("sumLong", "longSum", "l"),
                                                     ("sumDouble", "doubleSum", "d"), ("maxDouble", "doubleMax", "d")],
                                  query_granularity="none", rollup=False, interval=(0, 3_600_000))
    t = np.sort(rng.integers(0, 3_600_000, 6_000))
    for i in range(6_000):
        k = int(rng.integers(0, 4))
        idx.add(int(t[i]), {"dimA": "a" + str(int(rng.integers(0, 40))), "l": int(rng.integers(-1000, 1000)),
                            "d": float(rng.uniform(1.0, 100.0)),
                            "tags": ["t" + str(int(x)) for x in rng.integers(0, 12, k)]})
    path = W.write_segment(str(tmp_path_factory.mktemp("hashgb_tags") / "seg"), idx.to_spec(), lz4_mode="fast")
    return [idx.to_segment()], [O.OracleSegment(path)]


@pytest.mark.gpu
def test_multi_value_dimension(Q, O, mods, tagged):
    q = Q.GroupByQuery(intervals=["1970-01-01T00:00:00Z/1970-01-01T01:00:00Z"], granularity="all",
                       dimensions=["tags", "dimA"],
                       aggregations=[Q.long_sum("rows", "rows"), Q.long_sum("sumLong", "sumLong"),
                                     Q.double_sum("sumDouble", "sumDouble"), Q.double_max("maxDouble", "maxDouble")])
    h, _ = _check(mods, O, q, *tagged)
    assert int(h[1].sum()) > 6_000  # rows explode into one element per tag


@pytest.fixture(scope="module")
def special(W, O, mods, tmp_path_factory):
    """4,097 rows (three keygen tiles and two insert tiles, the last of one row), 5 groups over NaN, -0.0, +-inf."""
    n = 4_097
    g = (np.arange(n) % 5).astype(np.int32)
    d = np.linspace(1.0, 2.0, n)
    d[g == 1] = np.where(np.arange((g == 1).sum()) % 7 == 0, np.nan, 3.5)       # NaN among finite values
    d[g == 2] = np.where(np.arange((g == 2).sum()) % 9 == 0, np.inf, 1e300)     # +inf
    d[g == 3] = np.where(np.arange((g == 3).sum()) % 2 == 0, -0.0, 0.0)         # only zeros of both signs
    d[g == 4] = np.where(np.arange((g == 4).sum()) % 11 == 0, -np.inf, -2.25)   # -inf among negatives
    d[n - 1] = -0.0  # the one-row last tile (group 1): a signed zero beside NaN
    with np.errstate(over="ignore"):  # (1e300 is +inf as a float)
        f = d.astype(np.float32)
    spec = W.SegmentSpec(timestamps=np.arange(n, dtype=np.int64), dims={"g": (["g0", "g1", "g2", "g3", "g4"], g)},
                         metrics={"d": ("double", d), "f": ("float", f)}, interval=(0, 5_000))
    path = W.write_segment(str(tmp_path_factory.mktemp("hashgb_special") / "seg"), spec, lz4_mode="fast")
    return [mods.S.GpuSegment(path)], [O.OracleSegment(path)]


@pytest.mark.gpu
def test_nan_signed_zero_and_infinities(Q, O, mods, special):
    q = Q.GroupByQuery(intervals=["1970-01-01T00:00:00Z/1970-01-01T00:00:05Z"], granularity="all", dimensions=["g"],
                       aggregations=[Q.count("n"), Q.double_min("dmin", "d"), Q.double_max("dmax", "d"),
                                     Q.float_min("fmin", "f"), Q.float_max("fmax", "f"), Q.double_sum("ds", "d")])
    h, _ = _check(mods, O, q, *special)
    part = h[0]
    assert len(part) == 5
    dmin, dmax, fmin, fmax, ds = (part.aggs[i] for i in range(1, 6))
    assert np.isnan(dmin[1]) and np.isnan(dmax[1]) and np.isnan(fmin[1]) and np.isnan(fmax[1]) and np.isnan(ds[1])
    assert dmax[2] == np.inf and ds[2] == np.inf and dmin[4] == -np.inf and ds[4] == -np.inf
    assert dmin[3] == 0.0 and np.signbit(dmin[3]) and dmax[3] == 0.0 and not np.signbit(dmax[3])
    assert np.signbit(fmin[3]) and not np.signbit(fmax[3])


@pytest.mark.gpu
def test_buffer_grouper_max_size(Q, O, mods, basic, few_groups):
    q, (h, s) = few_groups
    N = mods.N
    G = len(s[0])
    fit = _run(mods, basic[0], _hash(q, bufferGrouperMaxSize=G))
    slots = 1
    while slots * 7 < G * 10:  # the next power of two >= G / 0.7
        slots *= 2
    assert fit[2]["grouper"] == N.GROUPER_HASH and fit[2]["table_slots"] == slots and fit[2]["max_groups"] == G
    _same(q, fit, s)
    with pytest.raises(N.TableFull) as e:
        _run(mods, basic[0], _hash(q, bufferGrouperMaxSize=G - 1))
    assert e.value.code == 5
    # the limit holds under the sort grouper too (no forceHashAggregation: the context's default)
    limited = dataclasses.replace(q, context={"bufferGrouperMaxSize": G})
    assert _run(mods, basic[0], limited)[2] == {"grouper": N.GROUPER_SORT, "table_slots": 0, "max_groups": G,
                                                "flushed_entries": 0, "direct_elements": 0}
    with pytest.raises(N.TableFull):
        _run(mods, basic[0], dataclasses.replace(q, context={"bufferGrouperMaxSize": G - 1}))
    # the failed call left the context usable: the next query, default options, is right
    again = _run(mods, basic[0], q)
    assert again[2]["grouper"] == N.GROUPER_SORT
    assert_results(q, mods.R.merge_groupby(q, [again[0]]), O.run(q, basic[1]))
    _same(q, _run(mods, basic[0], _hash(q)), again)


@pytest.mark.gpu
def test_float_sum_falls_back_to_the_sort(Q, O, mods, basic):
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=["dimZipf"],
                       aggregations=[Q.count("n"), Q.float_sum("fs", "sumFloatNormal"), Q.long_sum("ls", "sumLongSequential")])
    h, s = _check(mods, O, q, *basic, hash_expected=False)
    assert h[0].aggs[1].tobytes() == s[0].aggs[1].tobytes()  # floatSum too: the same path ran
    assert h[2]["table_slots"] == 0


@pytest.mark.gpu
def test_downstream_limit_run_query_and_context_default(Q, O, mods, basic, monkeypatch):
    R, N = mods.R, mods.N
    segs, osegs = basic
    q = Q.GroupByQuery(intervals=ALL, granularity="all", dimensions=["dimZipf", "dimSequential"],
                       aggregations=[Q.count("n"), Q.long_sum("ls", "sumLongSequential")],
                       limitSpec={"type": "default", "columns": [{"dimension": "dimSequential", "direction": "descending"}],
                                  "limit": 25})
    assert q.apply_limit_push_down()
    parts = []
    for qq in (_hash(q), q):
        res = R.groupby_run(segs, qq, limit_push_down=True)
        try:
            assert res.groups == 25
            assert res.grouper_info()["grouper"] == (N.GROUPER_HASH if qq is not q else N.GROUPER_SORT)
            parts.append(res.fetch())
        finally:
            res.release()
    assert [c.tolist() for c in parts[0].codes] == [c.tolist() for c in parts[1].codes]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts[0].aggs, parts[1].aggs))
    exp = O.run(q, osegs)
    got_hash, got = R.run_query(_hash(q), segs), R.run_query(q, segs)
    assert_results(q, got_hash, exp)
    assert [(r.timestamp, r.event) for r in got_hash] == [(r.timestamp, r.event) for r in got]
    # the context's default grouper: set, then reset; DG_GROUPER overrides it, explicit options win
    plain = dataclasses.replace(q, limitSpec=None)
    ctx = segs[0].context.handle
    try:
        N.check(N.lib().dg_context_set_limit(ctx, N.LIMIT_GROUPER, N.GROUPER_HASH))
        assert _run(mods, segs, plain)[2]["grouper"] == N.GROUPER_HASH
        monkeypatch.setenv("DG_GROUPER", "sort")
        assert _run(mods, segs, plain)[2]["grouper"] == N.GROUPER_SORT
        monkeypatch.delenv("DG_GROUPER")
        sort_opts = dataclasses.replace(plain, context={"forceHashAggregation": False})
        assert _run(mods, segs, sort_opts)[2]["grouper"] == N.GROUPER_SORT
        N.check(N.lib().dg_context_set_limit(ctx, N.LIMIT_GROUPER, 0))
        assert _run(mods, segs, plain)[2]["grouper"] == N.GROUPER_SORT
        monkeypatch.setenv("DG_GROUPER", "hash")
        assert _run(mods, segs, plain)[2]["grouper"] == N.GROUPER_HASH
        assert _run(mods, segs, sort_opts)[2]["grouper"] == N.GROUPER_SORT
    finally:
        N.lib().dg_context_set_limit(ctx, N.LIMIT_GROUPER, 0)
