"""The groupBy sort plan with deferred low key bits (dg_engine.cpp: the planner in dg_groupby_run;
dg_sort.hip: k_gb_reduce<.., DEFER>). The global radix passes order key bits [d, key_bits) only and every
reduce tile orders the runs of equal prefix it holds in LDS (at most 64 elements per run). A longer run
raises a flag, the call then sorts classically, reduces again and remembers the query shape.
dg_debug_groupby_sort_plan reports {passes, defer_bits, reran_classic} of the context's last groupBy.

Every case runs its query with the deferral forced (DG_GB_DEFER_BITS=d) and with DG_GB_DEFER_BITS=0: the
fetched groups are equal bit for bit (keys, long sums and double sums: the words end in the same order),
and they are compared with the oracle. The no-overflow cases first compute, on the CPU, the longest run of
equal prefix of their input's keys (merged dictionary id = rank in the sorted union of the segments'
values, the last dimension in the low bits) and assert it is at most 64. Dimension values are six-digit
numbers, so the dictionaries' string order is the numeric one. Segments hold 20,000 rows (id blocks of at
least 8,192 rows, so the generated first pass is reachable) unless the case is about an edge."""
import ctypes
import importlib

import numpy as np
import pytest

from compare import assert_results

pytestmark = pytest.mark.gpu

IV = [(0, 1 << 40)]
ROWS = 20_000
TILE = 4096
MAX_RUN = 64
BASE = 100_000  # values BASE + v: six digits, string order = numeric order


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("incubator-druid_amd.segment")


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


def _bits(card):
    b = 0
    while (1 << b) < card:
        b += 1
    return b


def _spec(W, a, b, seed, doubles="eighths"):
    """A segment whose rows carry the dimension values BASE + a[i], BASE + b[i], in this row order."""
    rng = np.random.default_rng(seed)
    n = len(a)
    x = rng.integers(-40, 40, n) * 0.125 if doubles == "eighths" else rng.random(n) * 1e6 - 5e5
    return W.SegmentSpec(timestamps=np.sort(rng.integers(0, 6 * 3_600_000, n)).astype(np.int64),
                         dims={"a": W.encode_int_strings(np.asarray(a, dtype=np.int64) + BASE),
                               "b": W.encode_int_strings(np.asarray(b, dtype=np.int64) + BASE)},
                         metrics={"m": ("long", rng.integers(-1000, 1000, n)), "x": ("double", x)})


def _layout(segs):
    """(keys of the call's rows, key bits, b's bits): the merged ids are ranks in the sorted unions."""
    ua = np.unique(np.concatenate([a for a, _ in segs]))
    ub = np.unique(np.concatenate([b for _, b in segs]))
    bb = _bits(len(ub))
    keys = np.concatenate([(np.searchsorted(ua, a).astype(np.int64) << bb) | np.searchsorted(ub, b) for a, b in segs])
    return keys, _bits(len(ua)) + bb, bb


def _longest_run(keys, d):
    return int(np.unique(keys >> d, return_counts=True)[1].max())


def _write(W, S, O, base, segs, **kw):
    paths = [W.write_segment(str(base / f"s{i}"), _spec(W, a, b, 1000 + i, **kw), lz4_mode="fast")
             for i, (a, b) in enumerate(segs)]
    return [S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]


def _gb(Q, **kw):
    return Q.GroupByQuery(intervals=IV, dimensions=["a", "b"],
                          aggregations=[Q.long_sum("m", "m"), Q.double_sum("x", "x")], **kw)


def _plan(N, g):
    out = (ctypes.c_int32 * 3)(-1, -1, -1)
    N.check(N.lib().dg_debug_groupby_sort_plan(g[0].context.handle, out))
    return list(out)


def _source(N, g):
    src = ctypes.c_int32(-1)
    N.check(N.lib().dg_debug_groupby_totals_source(g[0].context.handle, ctypes.byref(src)))
    return src.value


def _run(R, N, monkeypatch, q, g, defer):
    """One dg_groupby_run with DG_GB_DEFER_BITS = defer (None: unset, the planner decides): the fetched
    groups, the sort plan and the source of the first pass's totals."""
    if defer is None:
        monkeypatch.delenv("DG_GB_DEFER_BITS", raising=False)
    else:
        monkeypatch.setenv("DG_GB_DEFER_BITS", str(defer))
    res = R.groupby_run(g, q, R.RunStats())
    try:
        return res.fetch(), _plan(N, g), _source(N, g)
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


def _passes(bits):
    return (bits + 7) // 8


def _check(R, N, O, monkeypatch, q, g, o, defer, key_bits, reran=0, calls=1):
    """q with the deferral forced (`calls` times) against q sorted classically, bit for bit, and against
    the oracle; the plan of every forced call. Returns the totals' sources of the forced calls."""
    off, plan, _ = _run(R, N, monkeypatch, q, g, 0)
    assert plan == [_passes(key_bits), 0, 0]
    sources = []
    for _ in range(calls):
        got, plan, src = _run(R, N, monkeypatch, q, g, defer)
        assert plan == [_passes(key_bits - defer), defer, reran]
        _same_bits(got, off)
        sources.append(src)
    monkeypatch.setenv("DG_GB_DEFER_BITS", str(defer))
    assert_results(q, R.run_query(q, g), O.run(q, o))
    return sources


def _rand(seed, n, a, b):
    rng = np.random.default_rng(seed)
    return rng.integers(a[0], a[1], n), rng.integers(b[0], b[1], n)


def test_two_bits_remapped_dictionaries_first_digit_inside(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """9 + 11 key bits, 2 deferred: three passes of 6 bits over bits [2, 20), the first digit [2, 8) inside
    b's field, so the second forced call takes its totals from the value counts. The segments' value
    ranges differ: both dimensions are remapped."""
    segs = [_rand(11, ROWS, (0, 300), (0, 1000)), _rand(12, ROWS, (150, 450), (500, 1500))]
    keys, kb, bb = _layout(segs)
    assert _longest_run(keys, 2) <= MAX_RUN and 2 + 6 <= bb
    g, o = _write(W, S, O, tmp_path, segs)
    assert g[0].dictionary("b") != g[1].dictionary("b")
    assert _check(R, N, O, monkeypatch, _gb(Q), g, o, 2, kb, calls=2)[1] == 1


def test_first_digit_straddles_two_fields(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """b has 5 values (3 bits) under a 3,000-value a (12 bits); 2 bits deferred: two passes of 7 bits, the
    first over bits [2, 9) reaching into a's field: the histogram kernel counts it, every time."""
    segs = [_rand(21, ROWS, (0, 3000), (0, 5)), _rand(22, ROWS, (0, 3000), (0, 5))]
    keys, kb, bb = _layout(segs)
    assert bb == 3 and _longest_run(keys, 2) <= MAX_RUN
    g, o = _write(W, S, O, tmp_path, segs)
    assert _check(R, N, O, monkeypatch, _gb(Q), g, o, 2, kb, calls=2) == [0, 0]


def _edge_runs(lengths, ntiles):
    """Sorted (a, b) rows of ntiles tiles: run k of lengths[k] equal a values lies across the boundary of
    tiles k and k + 1 (half on either side), every other a occurs once. Also which rows go to the first
    of two segments: a run's upper half (by b), every other single row."""
    a, b, first, v = [], [], [], 0

    def single():
        nonlocal v
        a.append(v)
        b.append(v % MAX_RUN)
        first.append(v % 2 == 0)
        v += 1

    for k, ln in enumerate(lengths):
        while len(a) < TILE * (k + 1) - ln // 2:
            single()
        a += [v] * ln
        b += list(range(ln))
        first += [i >= ln // 2 for i in range(ln)]
        v += 1
    while len(a) < TILE * ntiles:
        single()
    return np.asarray(a), np.asarray(b), np.asarray(first)


def test_runs_across_tile_and_segment_edges(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """b's 6 bits deferred: the prefix is a. Runs of 2, 3, 33, 63 and 64 rows lie across the edges of sort
    tiles 0|1 ... 4|5 (elements 4095 | 4096 of a tile pair); a run's upper half is in the first segment, its
    lower half in the second, and both segments' rows descend in key order: over the call's rows every
    run's low bits descend, so every run reaches the reduce reversed."""
    a, b, first = _edge_runs([2, 3, 33, 63, 64], 6)
    segs = [(a[first][::-1], b[first][::-1]), (a[~first][::-1], b[~first][::-1])]
    keys, kb, bb = _layout(segs)
    assert bb == 6 and _longest_run(keys, 6) == MAX_RUN
    order = np.argsort(keys >> 6, kind="stable")  # what the global passes leave: prefix order, ties in row order
    for k, ln in enumerate([2, 3, 33, 63, 64]):
        edge = keys[order][TILE * (k + 1) - 1:TILE * (k + 1) + 1]
        assert edge[0] >> 6 == edge[1] >> 6 and edge[0] > edge[1]  # one run across the edge, low bits descending
    g, o = _write(W, S, O, tmp_path, segs)
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 6, kb)


def _one_long_run(ln, n=5000):
    """n rows of distinct a, but for one run of ln rows with b = ln - 1 ... 0 around element 4096."""
    a = np.arange(n)
    b = np.arange(n) % 4
    a[TILE - 10:TILE - 10 + ln] = a[TILE - 10]
    b[TILE - 10:TILE - 10 + ln] = np.arange(ln)[::-1]
    return a, b


def test_run_of_64_passes_and_65_sorts_again(Q, O, W, R, N, S, tmp_path, monkeypatch):
    a, b = _one_long_run(64)
    keys, kb, bb = _layout([(a, b)])
    assert bb == 6 and _longest_run(keys, 6) == 64
    g, o = _write(W, S, O, tmp_path / "r64", [(a, b)])
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 6, kb, reran=0)
    a, b = _one_long_run(65)
    keys, kb, bb = _layout([(a, b)])
    assert bb == 7 and _longest_run(keys, 7) == 65
    g, o = _write(W, S, O, tmp_path / "r65", [(a, b)])
    q = _gb(Q)
    _check(R, N, O, monkeypatch, q, g, o, 7, kb, reran=1)
    # the shape is remembered: the same query, the switch still set, sorts classically at once
    off, _, _ = _run(R, N, monkeypatch, q, g, 0)
    got, plan, _ = _run(R, N, monkeypatch, q, g, 7)
    assert plan == [_passes(kb), 0, 0]
    _same_bits(got, off)


def test_small_inputs(Q, O, W, R, N, S, tmp_path, monkeypatch):
    # all rows but three one key (the three give the key its bits): one run of 300, which overflows
    a = np.r_[np.zeros(300, dtype=np.int64), [1, 2, 3]]
    b = np.r_[np.zeros(300, dtype=np.int64), [1, 2, 3]]
    keys, kb, _ = _layout([(a, b)])
    assert kb == 4 and _longest_run(keys, 1) == 300
    g, o = _write(W, S, O, tmp_path / "one", [(a, b)])
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 1, kb, reran=1)
    # n = 1: a key of no bits, nothing to defer
    g, o = _write(W, S, O, tmp_path / "n1", [(np.array([7]), np.array([9]))])
    got, plan, _ = _run(R, N, monkeypatch, _gb(Q), g, 3)
    assert plan == [0, 0, 0] and len(got) == 1
    assert_results(_gb(Q), R.run_query(_gb(Q), g), O.run(_gb(Q), o))
    # two one-row segments: two key bits, one deferred
    segs = [(np.array([1]), np.array([1])), (np.array([0]), np.array([0]))]
    g, o = _write(W, S, O, tmp_path / "n2", segs)
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 1, 2)
    # n = 4097: a one-element last tile whose halo is clamped at the array's end
    segs = [_rand(51, TILE + 1, (0, 2000), (0, 16))]
    keys, kb, bb = _layout(segs)
    assert bb == 4 and _longest_run(keys, 4) <= MAX_RUN
    g, o = _write(W, S, O, tmp_path / "n4097", segs)
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 4, kb)


def test_equal_keys_inside_runs_order_dependent_doubles(Q, O, W, R, N, S, tmp_path, monkeypatch):
    """About four rows per group and doubles whose sum depends on the order of the adds: the groups' rows
    must reach the reduce in the classic order for the sums to come out bit-equal."""
    segs = [_rand(61, ROWS, (0, 100), (0, 100)), _rand(62, ROWS, (0, 100), (0, 100))]
    keys, kb, bb = _layout(segs)
    assert bb == 7 and _longest_run(keys, 2) <= MAX_RUN
    counts = np.unique(keys, return_counts=True)[1]
    assert 3 <= counts.mean() <= 5
    g, o = _write(W, S, O, tmp_path, segs, doubles="wide")
    _check(R, N, O, monkeypatch, _gb(Q), g, o, 2, kb)


def test_planner(Q, O, W, R, N, S, tmp_path, monkeypatch):
    # low cardinality: 40,000 rows over 30 x 20 keys: hundreds of rows per prefix at every pass count
    segs = [_rand(71, ROWS, (0, 30), (0, 20)), _rand(72, ROWS, (0, 30), (0, 20))]
    _, kb, _ = _layout(segs)
    g, o = _write(W, S, O, tmp_path / "low", segs)
    got, plan, _ = _run(R, N, monkeypatch, _gb(Q), g, None)
    assert plan == [_passes(kb), 0, 0]
    off, _, _ = _run(R, N, monkeypatch, _gb(Q), g, 0)
    _same_bits(got, off)
    # 4,000 x 8,000 keys (12 + 13 bits, four classic passes): three passes leave 1 bit and 40,000 * 2 / 32 M
    # rows per prefix, and their first digit, bits [1, 9), stays inside b's field
    segs = [_rand(73, ROWS, (0, 4000), (0, 8000)), _rand(74, ROWS, (0, 4000), (0, 8000))]
    keys, kb, _ = _layout(segs)
    assert kb == 25 and _longest_run(keys, 1) <= MAX_RUN
    g, o = _write(W, S, O, tmp_path / "high", segs)
    for q in (_gb(Q), _gb(Q, filter=Q.SelectorDimFilter("a", str(BASE + 100))), _gb(Q, granularity="hour")):
        got, plan, _ = _run(R, N, monkeypatch, q, g, None)
        assert plan[2] == 0
        off, _, _ = _run(R, N, monkeypatch, q, g, 0)
        _same_bits(got, off)
        monkeypatch.delenv("DG_GB_DEFER_BITS", raising=False)
        assert_results(q, R.run_query(q, g), O.run(q, o))
    got, plan, _ = _run(R, N, monkeypatch, _gb(Q), g, None)
    assert plan == [3, 1, 0]
    # 300 x 1,000 keys (9 + 10 bits): two passes would leave 3 bits at about one row per prefix (the reduce
    # would pay more than the pass saves), and their first digit, bits [3, 11), would leave b's field
    segs = [_rand(75, ROWS, (0, 300), (0, 1000)), _rand(76, ROWS, (0, 300), (0, 1000))]
    _, kb, _ = _layout(segs)
    g, o = _write(W, S, O, tmp_path / "keep", segs)
    _, plan, _ = _run(R, N, monkeypatch, _gb(Q), g, None)
    assert kb == 19 and plan == [3, 0, 0]
