"""Post-aggregators on the host: the query classes' compute, the compiler to the postfix program of
include/druidgpu.h, the order keys, JSON, validation, and the evaluator header itself built as plain C++ under
-fsanitize=undefined.

The known answers (tests/golden/post_agg_kats.json, written by make_post_agg_kats.py) are transcribed from the
reference's post-aggregator tests. The programs are run by the tests' own interpreter (post_agg_restate.py), which
imports nothing of the product, and by the stand-alone C++ driver of the product's evaluator header."""
import importlib
import itertools
import json
import math
import os
import shutil
import struct
import subprocess

import pytest

import post_agg_restate as PR
import querygen as G

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "post_agg_kats.json")))
ORDER_VALUES = [-math.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, math.inf, math.nan]
AGG_OF = {"count": "count", "longSum": "longSum", "doubleSum": "doubleSum"}


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


def _word(s):
    return int(s[2:], 16) if s.startswith("d:") else int(s[2:]) & PR.M64


def _py_value(s):
    return PR.dbl(int(s[2:], 16)) if s.startswith("d:") else int(s[2:])


def _case_query(Q, case):
    aggs = [Q.AggregatorFactory(t, name, None if t == "count" else "x") for name, t in sorted(case["aggs"].items())]
    return Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=[case["post"]])


def _slots(q, row):
    words, classes = [], []
    for a in q.aggregations:
        words.append(_word(row[a.name]))
        classes.append(PR.slot_class(a.output_type))
    return words, classes


def _same_value(got, want):
    if want.startswith("l:"):
        assert isinstance(got, int) and not isinstance(got, bool) and got == int(want[2:])
    else:
        assert isinstance(got, float) and PR.bits(got) == int(want[2:], 16)


# ---------------------------------------------------------------------------------------------
# the reference's known answers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS["compute"], ids=[c["name"] for c in KATS["compute"]])
def test_kat_compute(Q, case):
    q = _case_query(Q, case)
    post = q.postAggregations[0]
    _same_value(post.compute({k: _py_value(v) for k, v in case["row"].items()}), case["value"])


@pytest.mark.parametrize("case", KATS["compute"], ids=[c["name"] for c in KATS["compute"]])
def test_kat_compiled_program(Q, case):
    q = _case_query(Q, case)
    post = q.postAggregations[0]
    # (a constant and a fieldAccess have no ordering comparator: compiled as a having leaf compiles them)
    prog = Q.compile_post_aggregator(q.aggregations, q.postAggregations, post.name,
                                     for_order=post.to_json()["type"] not in ("fieldAccess",))
    words, classes = _slots(q, case["row"])
    assert PR.interpret(prog.ops, words, classes) == _word(case["value"])
    assert prog.out_type == ("long" if case["value"].startswith("l:") else "double")
    assert len(prog.ops) <= 64
    want_order = {"constant": PR.ORDER_NONE, "longGreatest": PR.ORDER_LONG, "longLeast": PR.ORDER_LONG}.get(
        post.to_json()["type"], PR.ORDER_NUMERIC_FIRST if post.to_json().get("ordering") else PR.ORDER_DOUBLE)
    assert prog.order == want_order


def test_kat_numeric_first_and_constant_comparators(Q):
    for a, b, sign in KATS["numeric_first"]:
        c = PR.numeric_first_compare(PR.dbl(_word(a)), PR.dbl(_word(b)))
        assert (c > 0) - (c < 0) == sign
        ka, kb = (Q.post_program_order_key(Q.POST_ORDER_NUMERIC_FIRST, _word(x)) for x in (a, b))
        assert (ka > kb) - (ka < kb) == sign
    for a, b, sign in KATS["constant_compare"]:
        assert Q.post_program_order_key(Q.POST_ORDER_NONE, _word(a)) == Q.post_program_order_key(Q.POST_ORDER_NONE, _word(b))
        assert sign == 0


@pytest.mark.parametrize("order", [PR.ORDER_DOUBLE, PR.ORDER_NUMERIC_FIRST])
def test_key_order_is_comparator_order(Q, order):
    """On all pairs of the special values the product's key, the restatement's key and the comparator agree."""
    for a, b in itertools.product(ORDER_VALUES, repeat=2):
        wa, wb = PR.bits(a), PR.bits(b)
        c = PR.compare_words(order, wa, wb)
        for key in (Q.post_program_order_key, PR.order_key):
            ka, kb = key(order, wa), key(order, wb)
            assert (ka > kb) - (ka < kb) == (c > 0) - (c < 0), (order, a, b)
    # a NaN of any payload is the one NaN
    assert Q.post_program_order_key(order, 0xFFF8000000000001) == Q.post_program_order_key(order, PR.NAN_BITS)


def test_long_key_order(Q):
    vals = [PR.LONG_MIN, -1, 0, 1, PR.LONG_MAX]
    keys = [Q.post_program_order_key(Q.POST_ORDER_LONG, v & PR.M64) for v in vals]
    assert keys == sorted(keys) and keys == [PR.order_key(PR.ORDER_LONG, v & PR.M64) for v in vals]


# ---------------------------------------------------------------------------------------------
# compute against the interpreter over compiled programs, special values included
# ---------------------------------------------------------------------------------------------
def _fa(n):
    return {"type": "fieldAccess", "fieldName": n}


POSTS = [
    {"type": "arithmetic", "name": "avg", "fn": "/", "fields": [_fa("ds"), _fa("rows")]},
    {"type": "arithmetic", "name": "lin", "fn": "-", "fields": [_fa("ls"), {"type": "arithmetic", "fn": "*", "fields": [
        _fa("lmin"), {"type": "constant", "value": 3}]}]},
    {"type": "arithmetic", "name": "quot", "fn": "quotient", "fields": [_fa("dmax"), _fa("fs")], "ordering": "numericFirst"},
    {"type": "doubleGreatest", "name": "dg", "fields": [_fa("ds"), _fa("dmax"), {"type": "constant", "value": 1.5}]},
    {"type": "longLeast", "name": "ll", "fields": [_fa("ls"), _fa("rows"), _fa("ds")]},
    {"type": "doubleLeast", "name": "dl", "fields": [_fa("avg"), _fa("fs"), _fa("ls")]},  # (an earlier post-aggregator)
    {"type": "longGreatest", "name": "lg", "fields": [_fa("quot"), {"type": "finalizingFieldAccess", "fieldName": "lf"}]},
    {"type": "arithmetic", "name": "chain", "fn": "+", "fields": [_fa("ds"), _fa("dmax"), _fa("fs"), _fa("rows")]},
]
SPECIAL_D = [0.0, -0.0, 1.5, -2.25, 5e-324, 1e300, -1e300, math.inf, -math.inf, math.nan, 2.0 ** 63, -(2.0 ** 63) - 2048.0]
SPECIAL_L = [0, 1, -1, 3, PR.LONG_MAX, PR.LONG_MIN, (1 << 53) + 1]


def _aggs(Q):
    return [Q.count("rows"), Q.long_sum("ls", "l"), Q.double_sum("ds", "d"), Q.double_max("dmax", "d"),
            Q.long_min("lmin", "l"), Q.float_sum("fs", "f"), Q.long_first("lf", "l")]


def _rows(Q):
    rows = []
    for i, (d, l) in enumerate(itertools.product(SPECIAL_D, SPECIAL_L)):
        d2 = SPECIAL_D[(i * 7 + 3) % len(SPECIAL_D)]
        f = struct.unpack("<f", struct.pack("<f", max(min(SPECIAL_D[(i * 5 + 1) % len(SPECIAL_D)], 3e38), -3e38)))[0]
        rows.append({"rows": SPECIAL_L[(i * 3) % len(SPECIAL_L)], "ls": l, "ds": d, "dmax": d2, "lmin": SPECIAL_L[(i + 2) % 7],
                     "fs": f, "lf": Q.SerializablePair(i, SPECIAL_L[(i + 4) % 7])})
    return rows


def test_compute_equals_interpreted_program(Q):
    q = Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=_aggs(Q), postAggregations=POSTS)
    native = Q.native_aggregations(q.aggregations)
    classes = [PR.slot_class(a.output_type) for a in native]
    progs = {p.name: Q.compile_post_aggregator(q.aggregations, q.postAggregations, p.name) for p in q.postAggregations}
    seen_nan = seen_inf = 0
    for row in _rows(Q):
        words = []
        for a in q.aggregations:
            v = row[a.name]
            if a.is_pair:
                words += [PR.value_word(v.rhs, a.output_type), PR.value_word(v.lhs, "long")]
            else:
                words.append(PR.value_word(v, a.output_type))
        ev = Q.compute_post_aggregations(q, dict(row))
        for name, prog in progs.items():
            want = PR.interpret(prog.ops, words, classes)
            got = ev[name]
            assert Q.post_value_word(got, prog.out_type) == want, (name, row, got)
            assert isinstance(got, int if prog.out_type == "long" else float)
            seen_nan += prog.out_type == "double" and got != got
            seen_inf += prog.out_type == "double" and math.isinf(got)
    assert seen_nan > 20 and seen_inf > 20


def test_d2l_and_division_rules(Q):
    assert [Q.java_d2l(x) for x in (math.nan, math.inf, -math.inf, 1e300, -1e300, 2.0 ** 63, -(2.0 ** 63) - 2048.0, -1.9, 1.9)] == \
        [0, PR.LONG_MAX, PR.LONG_MIN, PR.LONG_MAX, PR.LONG_MIN, PR.LONG_MAX, PR.LONG_MIN, -1, 1]
    div = Q.ArithmeticPostAggregator("x", "/", [_fa("a"), _fa("b")])
    quo = Q.ArithmeticPostAggregator("x", "quotient", [_fa("a"), _fa("b")])
    assert PR.bits(div.compute({"a": 1.0, "b": -0.0})) == PR.bits(0.0)  # -0.0 counts as zero
    assert div.compute({"a": 1.0, "b": math.nan}) != div.compute({"a": 1.0, "b": math.nan})  # a NaN divisor does not
    assert quo.compute({"a": 1.0, "b": -0.0}) == -math.inf and quo.compute({"a": -1, "b": 0}) == -math.inf
    assert quo.compute({"a": 0, "b": 0.0}) != quo.compute({"a": 0, "b": 0.0})
    assert Q.java_double_compare(-0.0, 0.0) < 0 and Q.java_double_compare(math.nan, math.inf) > 0
    assert Q.java_double_compare(math.nan, math.nan) == 0
    g = Q.DoubleGreatestPostAggregator("g", [_fa("a"), _fa("b")])
    assert PR.bits(g.compute({"a": -0.0, "b": 0.0})) == PR.bits(0.0) and PR.bits(g.compute({"a": 0.0, "b": -0.0})) == PR.bits(0.0)
    assert g.compute({"a": math.nan, "b": math.inf}) != g.compute({"a": math.nan, "b": math.inf})  # NaN is greatest


# ---------------------------------------------------------------------------------------------
# JSON, validation
# ---------------------------------------------------------------------------------------------
def _queries(Q, post, **kw):
    aggs = _aggs(Q)
    return [Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=post),
            Q.TopNQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=post, dimension="dim",
                        metric=kw.get("metric", "rows"), threshold=3),
            Q.GroupByQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=post, dimensions=["dim"],
                           limitSpec=kw.get("limitSpec"), having=kw.get("having"))]


def test_json_round_trip(Q):
    for q in _queries(Q, POSTS, metric="avg",
                      limitSpec={"type": "default", "columns": [{"dimension": "quot", "direction": "descending"}], "limit": 5},
                      having={"type": "greaterThan", "aggregation": "avg", "value": 1.5}):
        js = q.to_json()
        assert [p["name"] for p in js["postAggregations"]] == [p["name"] for p in POSTS]
        back = Q.query_from_json(json.loads(json.dumps(js)))
        assert back.to_json() == js and back == q
        assert js["postAggregations"][2]["ordering"] == "numericFirst" and "ordering" not in js["postAggregations"][0]
    for q in _queries(Q, []):  # emitted only when there are some
        assert "postAggregations" not in q.to_json()
        assert Q.query_from_json(q.to_json()) == q


def test_querygen_digests_unchanged():
    """The generated queries serialize as before (tests/test_querygen.py pins the digests themselves)."""
    t = importlib.import_module("test_querygen")
    assert G.queries_sha256() == t.SHA256 and G.merge_queries_sha256() == t.MERGE_SHA256
    assert not any("postAggregations" in G.query(qid).to_json() for qid in G.ids())


def test_validation_errors(Q, N):
    aggs = _aggs(Q)

    def ts(post):
        return Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=post)

    with pytest.raises(ValueError):  # a name used twice
        ts([POSTS[0], dict(POSTS[1], name="avg")])
    with pytest.raises(ValueError):  # an aggregator's name
        ts([dict(POSTS[0], name="rows")])
    with pytest.raises(ValueError):  # a LATER post-aggregator
        ts([POSTS[5], POSTS[0]])
    with pytest.raises(ValueError):  # an unknown field
        ts([{"type": "arithmetic", "name": "x", "fn": "+", "fields": [_fa("rows"), _fa("nope")]}])
    with pytest.raises(ValueError):
        ts([{"type": "arithmetic", "name": "x", "fn": "+", "fields": [_fa("rows")]}])  # fewer than two fields
    with pytest.raises(ValueError):
        ts([{"type": "arithmetic", "name": "x", "fn": "%", "fields": [_fa("rows"), _fa("ls")]}])
    with pytest.raises(ValueError):
        ts([{"type": "arithmetic", "name": "x", "fn": "+", "fields": [_fa("rows"), _fa("ls")], "ordering": "other"}])
    for t in ("javascript", "expression", "hyperUniqueCardinality"):
        with pytest.raises(N.UnsupportedQuery):
            ts([{"type": t, "name": "x", "fieldName": "rows", "fieldNames": ["rows"], "function": "f", "expression": "rows"}])
    # a plain fieldAccess of a first/last aggregator inside arithmetic or greatest / least: the pair is no Number
    for post in ({"type": "arithmetic", "name": "x", "fn": "+", "fields": [_fa("lf"), _fa("rows")]},
                 {"type": "longGreatest", "name": "x", "fields": [_fa("lf")]}):
        q = ts([post])
        with pytest.raises(ValueError):
            Q.compile_post_aggregator(q.aggregations, q.postAggregations, "x")
        with pytest.raises(ValueError):
            q.postAggregations[0].compute({"lf": Q.SerializablePair(1, 2), "rows": 1})
    # a finalizingFieldAccess of a post-aggregator
    q = ts([POSTS[0], {"type": "arithmetic", "name": "x", "fn": "+", "fields": [
        {"type": "finalizingFieldAccess", "fieldName": "avg"}, _fa("rows")]}])
    with pytest.raises(N.UnsupportedQuery):
        Q.compile_post_aggregator(q.aggregations, q.postAggregations, "x")
    # ordering by or ranking on a top-level fieldAccess: it has no comparator
    access = {"type": "fieldAccess", "name": "acc", "fieldName": "ds"}
    with pytest.raises(ValueError):
        Q.TopNQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=[access], dimension="dim", metric="acc",
                    threshold=3)
    with pytest.raises(ValueError):
        q = ts([access])
        Q.compile_post_aggregator(q.aggregations, q.postAggregations, "acc", for_order=True)
    with pytest.raises(ValueError):  # still: a metric that names nothing
        Q.TopNQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=POSTS, dimension="dim", metric="zzz", threshold=3)
    assert Q.TopNQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=POSTS, dimension="dim",
                       metric={"type": "inverted", "metric": "quot"}, threshold=3).metric_program().order == PR.ORDER_NUMERIC_FIRST


def test_program_limits(Q, N):
    aggs = _aggs(Q)
    deep = _fa("rows")
    for _ in range(20):  # right-nested: every level keeps one more operand alive
        deep = {"type": "arithmetic", "fn": "+", "fields": [_fa("rows"), deep]}
    q = Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=[dict(deep, name="deep")])
    with pytest.raises(N.UnsupportedQuery):
        Q.compile_post_aggregator(q.aggregations, q.postAggregations, "deep")
    long = {"type": "arithmetic", "name": "long", "fn": "+", "fields": [_fa("ds")] * 40}
    q = Q.TimeseriesQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=[long])
    with pytest.raises(N.UnsupportedQuery):
        Q.compile_post_aggregator(q.aggregations, q.postAggregations, "long")
    assert q.postAggregations[0].compute({"ds": 0.5}) == 20.0  # the host restatement has no such limit


def test_groupby_host_post_process(Q):
    """postprocess_groupby adds the columns and understands them in having and ORDER BY (numericFirst: non-finite
    values first ascending; comparator-equal rows keep their order)."""
    R = importlib.import_module("incubator-druid_amd.runners")
    aggs = [Q.count("rows"), Q.double_sum("ds", "d")]
    post = [{"type": "arithmetic", "name": "q", "fn": "quotient", "fields": [_fa("ds"), _fa("rows")], "ordering": "numericFirst"}]
    q = Q.GroupByQuery(intervals=["2000/2001"], aggregations=aggs, postAggregations=post, dimensions=["dim"],
                       limitSpec={"type": "default", "columns": [{"dimension": "q", "direction": "ascending"}], "limit": 6},
                       having={"type": "not", "havingSpec": {"type": "equalTo", "aggregation": "q", "value": 2.0}})
    assert not q.apply_limit_push_down()
    data = [("a", 4, 8.0), ("b", 0, 0.0), ("c", 0, 1.0), ("d", 2, 1.0), ("e", 0, -1.0), ("f", 2, 1.0), ("g", 1, -3.0), ("h", 1, 2.0)]
    rows = [Q.Row(0, {"dim": k, "rows": n, "ds": s}) for k, n, s in data]
    out = R.postprocess_groupby(q, rows)
    assert [r.event["dim"] for r in out] == ["e", "c", "b", "g", "d", "f"]
    assert out[0].event["q"] == -math.inf and out[2].event["q"] != out[2].event["q"] and out[4].event["q"] == 0.5
    assert all("q" not in r.event for r in rows)  # the input rows are not touched


# ---------------------------------------------------------------------------------------------
# the evaluator header as plain C++ under the undefined-behaviour sanitizer
# ---------------------------------------------------------------------------------------------
def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return c
    return None


def _line(order, classes, words, ops):
    out = [str(order), str(len(words)), str(len(ops))]
    for c, w in zip(classes, words):
        out += [str(c), "%x" % w]
    for op, arg, imm in ops:
        out += [str(op), str(arg), "%x" % imm]
    return " ".join(out)


def test_evaluator_header_under_ubsan(Q, tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "post_agg_eval")
    src = os.path.join(HERE, "post_agg_eval_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "incubator-druid_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", inc,
                    src, "-o", exe], check=True)
    lines, want = [], []

    def add(order, classes, words, ops, rc=0):
        lines.append(_line(order, classes, words, ops))
        if rc:
            want.append((rc, 0, 0))
        else:
            v = PR.interpret(ops, words, classes)
            want.append((0, v, PR.order_key(order, v)))

    for case in KATS["compute"]:
        q = _case_query(Q, case)
        post = q.postAggregations[0]
        prog = Q.compile_post_aggregator(q.aggregations, q.postAggregations, post.name, for_order=False)
        words, classes = _slots(q, case["row"])
        add(prog.order, classes, words, prog.ops)
        assert want[-1][1] == _word(case["value"])
    # D2L of the values a plain cast is undefined for, and of the edges around them
    for d in (math.nan, math.inf, -math.inf, 1e300, -1e300, 2.0 ** 63, -(2.0 ** 63) - 2048.0, -(2.0 ** 63), 2.0 ** 63 - 1024.0,
              0.5, -0.5, -1.9):
        add(PR.ORDER_LONG, [PR.SLOT_DOUBLE], [struct.unpack("<Q", struct.pack("<d", d))[0]], [(PR.AGG, 0, 0), (PR.D2L, 0, 0)])
    assert [w[1] for w in want[-12:-5]] == [0, PR.LONG_MAX, PR.LONG_MIN & PR.M64, PR.LONG_MAX, PR.LONG_MIN & PR.M64, PR.LONG_MAX,
                                            PR.LONG_MIN & PR.M64]
    # L2D of the extremes, every op over the special doubles, under both double orders
    for l in SPECIAL_L:
        add(PR.ORDER_DOUBLE, [PR.SLOT_LONG], [l & PR.M64], [(PR.AGG, 0, 0), (PR.L2D, 0, 0)])
    for op in (PR.ADD, PR.SUB, PR.MUL, PR.DIV, PR.QUOT, PR.DMAX, PR.DMIN):
        for a, b in itertools.product(SPECIAL_D, repeat=2):
            wa, wb = (struct.unpack("<Q", struct.pack("<d", x))[0] for x in (a, b))
            add(PR.ORDER_NUMERIC_FIRST if op == PR.QUOT else PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE, PR.SLOT_DOUBLE], [wa, wb],
                [(PR.AGG, 0, 0), (PR.AGG, 1, 0), (op, 0, 0)])
    for op in (PR.LMAX, PR.LMIN):
        for a, b in itertools.product(SPECIAL_L, repeat=2):
            add(PR.ORDER_LONG, [PR.SLOT_LONG, PR.SLOT_LONG], [a & PR.M64, b & PR.M64], [(PR.AGG, 0, 0), (PR.AGG, 1, 0), (op, 0, 0)])
    # a float slot widens exactly; a NaN of any payload becomes the canonical one
    add(PR.ORDER_DOUBLE, [PR.SLOT_FLOAT], [0xDEADBEEF3FC00000], [(PR.AGG, 0, 0)])
    add(PR.ORDER_DOUBLE, [PR.SLOT_FLOAT], [0xFFC00001], [(PR.AGG, 0, 0)])
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0xFFF8000000000001], [(PR.AGG, 0, 0)])
    assert want[-3][1] == PR.bits(1.5) and want[-2][1] == want[-1][1] == PR.NAN_BITS
    # no fused multiply-add: a * b + c rounds after the product (2^-60 would survive a fused one)
    x = 1.0 + 2.0 ** -30
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE] * 3, [PR.bits(x), PR.bits(x), PR.bits(-(1.0 + 2.0 ** -29))],
        [(PR.AGG, 0, 0), (PR.AGG, 1, 0), (PR.MUL, 0, 0), (PR.AGG, 2, 0), (PR.ADD, 0, 0)])
    assert want[-1][1] == PR.bits(0.0)
    # what the checker refuses (the driver does not run those)
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(PR.ADD, 0, 0)], rc=-4)                                  # underflow
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(PR.AGG, 0, 0)] * 17 + [(PR.ADD, 0, 0)] * 16, rc=-5)     # overflow
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(PR.AGG, 0, 0), (PR.AGG, 0, 0)], rc=-7)                  # two values
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(PR.AGG, 1, 0)], rc=-3)                                  # slot index
    add(PR.ORDER_DOUBLE, [-1], [0], [(PR.AGG, 0, 0)], rc=-3)                                              # a pair's time
    add(PR.ORDER_DOUBLE, [PR.SLOT_LONG], [0], [(PR.AGG, 0, 0), (PR.AGG, 0, 0), (PR.ADD, 0, 0)], rc=-6)    # longs into ADD
    add(PR.ORDER_LONG, [PR.SLOT_DOUBLE], [0], [(PR.AGG, 0, 0)], rc=-8)                                    # order / type
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(14, 0, 0)], rc=-2)                                      # unknown op
    add(PR.ORDER_DOUBLE, [PR.SLOT_DOUBLE], [0], [(PR.AGG, 0, 0)] + [(PR.AGG, 0, 0), (PR.ADD, 0, 0)] * 32, rc=-1)  # 65 ops
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = [tuple(int(x, 16) if i else int(x) for i, x in enumerate(ln.split())) for ln in run.stdout.splitlines()]
    assert len(got) == len(want) > 600
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lines[i], g, w)
