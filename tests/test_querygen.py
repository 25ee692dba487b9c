"""The query generator of tests/querygen.py on the CPU: that it is deterministic, that the oracle answers every
query it draws, that every axis and the asked-for combinations are drawn, that no floating sum steers a
result within its own error bound, the twin rule's re-sorting, the oracle's independence of the segment
layout, and the oracle's floating sums against math.fsum.

Wall time of the 160 expectations on the development machine (one core, `gen` below: the generation runs
every query on the oracle, a steered one a second time without its limit spec): 62 - 67 s for the generation,
0.02 - 1.4 s per query, 0.4 s on average; the 140 s buckets over 33,578 rows and the 30,000-row results are
the slow ones. The merge draw (44 more groupBy queries on the four-piece form of the fixture) and the piece
expectations of all 171 merge queries add 43 s and about 90 s; the module takes 200 s in all."""
import copy
import dataclasses
import json
import math
import time

import numpy as np
import pytest

import querygen as G

SHA256 = "2856142fed704a39367d4136f04224a127421c827515025bb8ddd9afa000ddec"


@pytest.fixture(scope="module")
def gen():
    """The generated queries; the time the generation took (it computes every expectation)."""
    t0 = time.perf_counter()
    qs = G.queries()
    return qs, time.perf_counter() - t0


def _json(qs):
    return [(qid, json.dumps(q.to_json(), sort_keys=True)) for qid, q in qs]


def test_deterministic(gen):
    """A second generation (the oracle's runs stay cached, the draws are made again) gives the same JSON, and
    the digest of it all is the recorded one: the draws do not depend on the numpy at hand."""
    first = _json(gen[0])
    G._GEN.clear()
    assert _json(G.queries()) == first
    assert [qid for qid, _ in first] == G.ids()
    assert len(G.ids("ts")) == 48 and len(G.ids("tn")) == 48 and len(G.ids("gb")) == 64
    assert G.queries_sha256() == SHA256


def test_queries_survive_their_json(Q, gen):
    for qid, q in gen[0]:
        js = q.to_json()
        assert Q.query_from_json(json.loads(json.dumps(js))).to_json() == js, qid


def test_oracle_answers_every_query(gen):
    """No oracle.Unsupported (it would have been raised here), at most 10 % empty expectations, and every
    kind of query has an empty one."""
    qs, seconds = gen
    print("generation with every expectation: %.1f s" % seconds)
    empty = [qid for qid, _ in qs if G.is_empty(G.expected(qid))]
    assert len(empty) <= len(qs) // 10, empty
    assert {qid[:2] for qid in empty} == {"ts", "tn", "gb"}, empty


AXES = (["iv:whole", "iv:cut", "iv:empty", "g:all", "g:hour", "g:dur", "g:p1d", "g:pt1h", "f:none", "f:nothing", "f:not",
         "f:and", "f:or", "agg:filtered", "agg:twin", "ts:desc", "ts:asc", "ts:skip", "ts:noskip",
         "tn:metric:numeric", "tn:metric:inverted", "tn:metric:lex", "tn:metric:alnum", "tn:prevstop",
         "tn:thr:1", "tn:thr:7", "tn:thr:big", "gb:limit:none", "gb:limit:only", "gb:limit:order", "gb:limit:order+limit",
         "gb:order:agg", "gb:order:dim", "gb:order:ascending", "gb:order:descending", "gb:order:lexicographic",
         "gb:order:numeric", "gb:ctx:hash", "gb:ctx:maxsize", "gb:ctx:pushdown", "gb:ctx:dimsfirst", "gb:keyref"]
        + ["f:" + k for k in G.LEAF_KINDS] + ["agg:" + t for t in G.AGG_TYPES] + ["tn:dim:" + d for d in G.TOPN_DIMS]
        + ["gb:dim:" + d for d in G.GB_DIMS] + ["gb:ndims:%d" % n for n in range(5)]
        + ["gb:having:" + k for k in ("none", "gt", "lt", "eq", "dimsel", "and", "or", "not")])


def _with(axes, *wanted):
    """The ids whose axis values hold one of every alternative in `wanted`."""
    return [qid for qid, a in axes.items() if all(a & set(w if isinstance(w, tuple) else (w,)) for w in wanted)]


def test_axis_census(gen):
    axes = G.axes()
    counts = {t: len(_with(axes, t)) for t in AXES}
    assert not {t: n for t, n in counts.items() if n < 3}, counts
    numeric = tuple("f:" + k for k in G.NUMERIC_LEAVES)
    limits = ("gb:limit:only", "gb:limit:order", "gb:limit:order+limit")
    having = tuple("gb:having:" + k for k in ("gt", "lt", "eq", "dimsel"))
    pairs = {"calendar x descending x filtered aggregator": (("g:p1d", "g:pt1h"), "ts:desc", "agg:filtered"),
             "numeric leaf x groupBy with tags": (numeric, "gb:dim:tags"),
             "LONG dimension x hash grouper x hourly": ("gb:dim:vL", "gb:ctx:hash", ("g:hour", "g:pt1h")),
             "floatSum x groupBy x limit spec": ("agg:floatSum", limits, tuple("gb:ndims:%d" % n for n in range(5))),
             "having x multi-value dimension": (having, "gb:dim:tags"),
             "alphanumeric topN x previousStop x filter": ("tn:metric:alnum", "tn:prevstop")}
    for what, wanted in pairs.items():
        found = _with(axes, *wanted)
        if what.startswith("alphanumeric"):
            found = [qid for qid in found if G.query(qid).filter is not None]
        assert found, what


def test_key_and_reference_words(gen):
    """At least four groupBy queries need the key + reference form of the sort words (more than 64 bits of key
    and row reference together), within the 64 key bits the engine accepts."""
    bits = {qid: G.sort_word_bits(q) for qid, q in gen[0] if qid.startswith("gb")}
    assert all(k <= 64 for k, _ in bits.values()), bits
    wide = [qid for qid, (k, r) in bits.items() if k + r > 64]
    assert len(wide) >= 4 and set(_with(G.axes(), "gb:keyref")) <= set(wide), bits


def _steered(Q, q):
    """Whether a bounded floating sum decides q's result."""
    aggs = {a.name: a for a in q.aggregations}

    def bounded(name):
        return name in aggs and G.is_bounded(aggs[name])

    if isinstance(q, Q.TopNQuery):
        return q.metric.type in ("numeric", "inverted") and bounded(q.metric.metric)
    if isinstance(q, Q.GroupByQuery):
        def leaves(h):
            return [] if h is None else [h.aggregation] + [n for x in h.specs for n in leaves(x)]
        return any(bounded(c.dimension) for c in (q.limitSpec.columns if q.limitSpec else [])) or \
            any(n is not None and bounded(n) for n in leaves(q.having))
    return False


def test_floating_sums_never_steer_within_their_bound(Q, gen):
    """On the oracle's result of every generated query: adjacent distinct values of a floating-sum topN metric
    or limit-spec column differ by more than four times the bound, and a having threshold on a floating sum
    lies further than that from every cell. The check is not vacuous: such queries are drawn."""
    steered = [qid for qid, q in gen[0] if _steered(Q, q)]
    print("steered by a floating sum:", steered)
    assert len(steered) >= 5
    for qid, q in gen[0]:
        assert G.steering_violations(q) == [], qid


def test_steering_check_sees_a_near_tie(Q):
    a = Q.AggregatorFactory("doubleSum", "s", "d")
    cells = [(1.0, 1e-3), (1.002, 1e-3), (5.0, 1e-3)]
    assert len(G._adjacent_violations(cells, "m")) == 1
    assert G._adjacent_violations([(1.0, 1e-4), (1.002, 1e-4), (5.0, 1e-4)], "m") == []
    assert G._adjacent_violations([(0.0, 0.0), (0.0, 0.0), (3, 0.0), (3, 0.0)], "m") == []  # exact ties are ties on both sides
    assert len(G._adjacent_violations([(2.0, 1e-9), (2.0, 1e-9)], "m")) == 1  # equal, but not exactly known
    assert G.cell_bound(a, {"s": 1.0, "s_n": 0, "s_abs": 0.0}) == 0.0
    assert G.cell_bound(a, {"s": 1.0, "s_n": 100, "s_abs": 50.0}) == 2 * G.gamma(100, 2.0 ** -53) * 50.0


def test_twin_rule_resorts_by_the_integer(Q):
    """Hand-written rows: the string order of v ("-5" < "10" < "9", and Long.MIN_VALUE's text before "-5") turned
    into the integer order, inside each bucket and under the string dimension before it."""
    q = Q.GroupByQuery(intervals=[(0, 10)], granularity="hour", aggregations=[Q.count("n")],
                       dimensions=["lo", {"type": "default", "dimension": "v", "outputType": "LONG"}])
    rows = [Q.Row(0, {"lo": "a", "v": -5, "n": 1}), Q.Row(0, {"lo": "a", "v": G.LONG_MIN, "n": 2}),
            Q.Row(0, {"lo": "a", "v": 10, "n": 3}), Q.Row(0, {"lo": "a", "v": 9, "n": 4}),
            Q.Row(0, {"lo": "b", "v": -7, "n": 5}), Q.Row(0, {"lo": None, "v": 100, "n": 6}),
            Q.Row(3_600_000, {"lo": "a", "v": G.LONG_MAX, "n": 7}), Q.Row(3_600_000, {"lo": "a", "v": 0, "n": 8})]
    assert [r.event["n"] for r in G.natural_resort(q, rows)] == [6, 2, 1, 4, 3, 5, 8, 7]
    qd = dataclasses.replace(q, context={"sortByDimsFirst": True})
    assert [r.event["n"] for r in G.natural_resort(qd, rows)] == [6, 2, 1, 8, 4, 3, 7, 5]
    oq = G.oracle_query(q)
    assert oq.dimensions == ["lo", "v_s"] and oq.dimensionTypes == ["STRING", "STRING"]
    renamed = G._rename_v(Q, [Q.Row(0, {"lo": "a", "v_s": "-5", "n": 1})], True)
    assert renamed[0].event == {"lo": "a", "v": -5, "n": 1} and type(renamed[0].event["v"]) is int


def test_twin_rule_on_generated_queries(Q, gen):
    """Every generated groupBy over v: the expectation holds the v_s rows (as a multiset of cells), LONG values
    are ints, and without a limit spec the rows are in (time, dimensions) order with v as an integer."""
    seen = 0
    for qid, q in gen[0]:
        if not (isinstance(q, Q.GroupByQuery) and "v" in q.dimensions):
            continue
        seen += 1
        exp = G.expected(qid)
        as_int = q.dimension_type("v") == "LONG"
        assert all(type(r.event["v"]) is (int if as_int else str) for r in exp), qid
        if q.limitSpec is None:
            raw = G._oracle_run(G.oracle_query(q))
            def canon(rows, name):
                return sorted((r.timestamp, json.dumps({("v" if k == name else k): (str(x) if k == name else x)
                                                         for k, x in r.event.items()}, sort_keys=True)) for r in rows)
            assert canon(exp, "v") == canon(raw, "v_s"), qid
            if as_int:
                assert [id(r) for r in G.natural_resort(q, exp)] == [id(r) for r in exp], qid
    assert seen >= 8


def test_oracle_is_independent_of_the_layout(gen):
    """Every fifth query on the three layouts: identical results, floating sums included (the oracle adds in
    row order whatever the bitmaps and codecs)."""
    for qid, q in gen[0][::5]:
        base = G.expected_for(q, 0)
        for layout in (1, 2):
            assert G.expected_for(q, layout) == base, (qid, G.LAYOUTS[layout])


def test_oracle_sums_against_fsum(Q, O, gen):
    """groupBy by mid over everything: the exact sums of d and f per group (math.fsum over the columns read
    through OracleSegment) against the oracle's recursive sums, within gamma(n - 1) * sum|x| (u = 2^-53 for the
    doubleSum, 2^-24 for the floatSum, which adds in float32). The one place where the reference is more
    precise than the oracle. The fixture cancels: some group's |sum| is below 1 % of its sum|x|."""
    q = Q.GroupByQuery(intervals=[G.WHOLE], granularity="all", dimensions=["mid"],
                       aggregations=[Q.double_sum("sd", "d"), Q.count("sd_n"), Q.double_sum("sd_abs", "d_abs"),
                                     Q.float_sum("sf", "f"), Q.count("sf_n"), Q.float_sum("sf_abs", "f_abs")])
    rows = G._oracle_run(q)
    segs = G.oracle_segments()
    mids = np.concatenate([np.array(s.dictionary("mid"), dtype=object)[s.ids("mid")] for s in segs])
    d = np.concatenate([s.numeric("d", "double") for s in segs])
    f = np.concatenate([s.numeric("f", "float") for s in segs]).astype(np.float64)
    assert len(rows) == 300
    worst, cancel = 0.0, 1.0
    for r in rows:
        sel = mids == r.event["mid"]
        n = int(sel.sum())
        assert r.event["sd_n"] == r.event["sf_n"] == n and n > 1
        for name, col, u in (("sd", d, 2.0 ** -53), ("sf", f, 2.0 ** -24)):
            exact, total = math.fsum(col[sel]), math.fsum(np.abs(col[sel]))
            err = abs(r.event[name] - exact)
            assert err <= G.gamma(n - 1, u) * total, (r.event["mid"], name, err)
            assert abs(r.event[name + "_abs"] - total) <= G.gamma(n - 1, u) * total
            # the comparison's bound, built from the oracle's own A, covers twice the one-sided error
            agg = next(a for a in q.aggregations if a.name == name)
            assert 2 * G.gamma(n - 1, u) * total <= G.cell_bound(agg, r.event)
            worst = max(worst, err / (G.gamma(n - 1, u) * total))
            cancel = min(cancel, abs(exact) / total)
    print("oracle error / bound, worst group: %.4f; smallest |sum| / sum|x|: %.2e" % (worst, cancel))
    assert cancel < 1e-2


# ---- the merge draw (querygen.merge_queries) and the four-piece form of the fixture ----
MERGE_SHA256 = "4ea4ffcbf041e0a02a33868bdcd373c5211f0204e25b25889a52dadc4df3d193"


@pytest.fixture(scope="module")
def merge_gen(gen):
    return G.merge_queries()


def test_pieces_hold_the_fixture_rows(O):
    """Each fixture segment cut once at row n // 2: the pieces' rows, two and two, are their segment's, and at
    least one cut parts rows of one instant."""
    whole, pieces = G.oracle_segments(), G.piece_oracle_segments()
    assert [p.num_rows for p in pieces] == [n for r in G.ROWS for n in (r // 2, r - r // 2)]
    parted = 0
    for i, s in enumerate(whole):
        a, b = pieces[2 * i], pieces[2 * i + 1]
        assert np.array_equal(np.concatenate([a.time(), b.time()]), s.time())
        for name, kind in (("l", "long"), ("d", "double"), ("f", "float")):
            assert np.array_equal(np.concatenate([a.numeric(name, kind), b.numeric(name, kind)]), s.numeric(name, kind))
        vals = [np.array(p.dictionary("hi"), dtype=object)[p.ids("hi")] for p in (a, b)]
        assert np.array_equal(np.concatenate(vals), np.array(s.dictionary("hi"), dtype=object)[s.ids("hi")])
        assert set(a.dictionary("hi")) != set(b.dictionary("hi"))  # every piece has its own dictionaries
        parted += int(a.time()[-1] == b.time()[0])
    print("cuts between rows of one instant:", parted)


def test_merge_draw_is_deterministic(gen, merge_gen):
    first = _json(merge_gen)
    G._MGEN.clear()
    assert _json(G.merge_queries()) == first
    assert [qid for qid, _ in first] == G.merge_ids()
    assert G.merge_queries_sha256() == MERGE_SHA256
    # every ts-* and tn-*, the gb-* that do not group by v (GB_NO_V is the draw's outcome), every gm-*
    no_v = tuple(int(qid[3:]) for qid, a in G.axes().items() if qid.startswith("gb") and not a & {"gb:dim:vL", "gb:dim:vS"})
    assert G.GB_NO_V == no_v
    assert len(G.MERGE_LEFT_OUT) <= 4, G.MERGE_LEFT_OUT
    assert set(G.merge_ids()) | set(G.MERGE_LEFT_OUT) == \
        set(G.ids("ts") + G.ids("tn")) | {"gb-%03d" % i for i in no_v} | {"gm-%03d" % i for i in range(G.MERGE_GB)}
    old = dict(gen[0])
    assert all(q.to_json() == old[qid].to_json() for qid, q in merge_gen if not qid.startswith("gm"))
    assert not [qid for qid, q in merge_gen if qid[0] == "g" and "v" in q.dimensions]
    assert not [qid for qid, q in merge_gen if any(a.is_pair for a in q.aggregations)]


def test_merge_census(merge_gen):
    """What the merge planes need to meet, counted over the groupBy merge queries of a fixed-period granularity
    (the ones dg_groupby_merge_devices takes; a calendar one may be split per segment and merged on the host)."""
    axes = G.axes(merge=True)
    assert list(axes) == G.merge_ids()
    gb = {qid: a for qid, a in axes.items() if qid[:2] in ("gb", "gm")}
    fixed = {qid: a for qid, a in gb.items() if a & {"g:all", "g:hour", "g:dur"}}
    assert len(gb) >= 60 and len(fixed) >= 40, (len(gb), len(fixed))
    having = tuple("gb:having:" + k for k in ("gt", "lt", "eq", "dimsel", "and", "or", "not"))
    wanted = {"zero dimensions under all": ("gb:ndims:0", "g:all"),
              "zero dimensions under hour or dur": ("gb:ndims:0", ("g:hour", "g:dur")),
              "tags": ("gb:dim:tags",), "nope": ("gb:dim:nope",), "forceHashAggregation": ("gb:ctx:hash",),
              "having with a limit": (having, ("gb:limit:only", "gb:limit:order+limit")),
              "forceLimitPushDown": ("gb:ctx:pushdown",), "sortByDimsFirst": ("gb:ctx:dimsfirst",),
              "empty interval or nothing-filter": (("iv:empty", "f:nothing"),)}
    counts = {what: len(_with(fixed, *w)) for what, w in wanted.items()}
    print(len(gb), len(fixed), counts)
    assert not {what: n for what, n in counts.items() if n < 4}, counts


def test_pieces_answer_as_the_two_segments(Q, merge_gen):
    """The oracle over the four pieces against the oracle over the two segments, for every timeseries and
    groupBy merge query: floating sums over d / f within cell_bound (the pieces add in another order), every
    other cell, the rows and their order exactly. (A topN's answer depends on the split: its per-segment cut
    and fold order are the reference's.)"""
    n = 0
    for qid, q in merge_gen:
        if not isinstance(q, Q.TopNQuery):
            G.assert_parity(qid, q, G.expected_for(q, G.PIECES), G.expected_for(q), "pieces", "oracle")
            n += 1
    assert n == len(G.merge_ids()) - len(G.merge_ids("tn"))


def test_no_steering_on_the_pieces(merge_gen):
    """Every merge query keeps its steering floating sums apart on the piece expectation too."""
    for qid, q in merge_gen:
        assert G.steering_violations(q, G.PIECES) == [], qid


def test_comparison_finds_what_it_should(Q, gen):
    """first_difference on the oracle's own results: equal to themselves; a floating sum moved by half its bound
    passes, by twice its bound fails; an exact cell moved by one ulp, a sign of zero, two rows swapped, a
    dimension value and a timestamp each fail."""
    qid = next(qid for qid, q in gen[0] if isinstance(q, Q.GroupByQuery) and "agg:twin" in G.axes()[qid]
               and len(G.expected(qid)) > 3 and any(a.type.endswith(("Min", "Max")) and a.output_type != "long"
                                                    for a in q.aggregations))
    q, exp = G.query(qid), G.expected(qid)
    assert G.first_difference(q, copy.deepcopy(exp), exp) is None
    s = next(a for a in q.aggregations if G.is_bounded(a) and not a.name.endswith("_abs"))
    i = next(i for i, r in enumerate(exp) if G.cell_bound(s, r.event) > 0)
    b = G.cell_bound(s, exp[i].event)
    for factor, same in ((0.5, True), (2.0, False)):
        got = copy.deepcopy(exp)
        got[i].event[s.name] += factor * b
        assert (G.first_difference(q, got, exp) is None) == same, factor
    m = next(a for a in q.aggregations if a.type.endswith(("Min", "Max")) and a.output_type != "long")
    got = copy.deepcopy(exp)
    got[i].event[m.name] = float(np.nextafter(np.float64(got[i].event[m.name]), np.inf))
    assert m.name in G.first_difference(q, got, exp)
    got = copy.deepcopy(exp)
    got[0], got[1] = got[1], got[0]
    assert G.first_difference(q, got, exp) is not None
    got = copy.deepcopy(exp)
    got[2].timestamp += 1
    assert "timestamp" in G.first_difference(q, got, exp)
    assert G.first_difference(q, exp[:-1], exp).startswith("%d results" % (len(exp) - 1))
    with pytest.raises(AssertionError) as e:
        G.assert_parity(qid, q, exp[:-1], exp, G.LAYOUTS[0], "DG_NO_SIDE=1")
    assert qid in str(e.value) and "DG_NO_SIDE=1" in str(e.value) and '"queryType": "groupBy"' in str(e.value)
    ts = Q.TimeseriesQuery(intervals=[G.WHOLE], aggregations=[Q.double_min("m", "x")])
    assert G.first_difference(ts, [Q.Result(0, {"m": -0.0})], [Q.Result(0, {"m": 0.0})]) is not None
    assert G.first_difference(ts, [Q.Result(0, {"m": 0})], [Q.Result(0, {"m": 0.0})]) is not None
