"""Post-aggregators the device decides on: k_post_eval (dg_result_post_aggregate), groupBy having / ORDER BY over
post columns (dg_result_post_process), topN ranked by a post-aggregator (dg_topn_run_post / dg_topn_merge_post).

The oracle knows no post-aggregators, so the expectations come from this module's own restatement
(post_agg_restate.py: the ops, the comparators, the order keys; below: having, the limit spec's stable sort,
TopNNumericResultBuilder's queue and TopNBinaryFn's fold), and never rest on summation order: the grouping or the
topN runs WITHOUT the post-aggregator and is fetched whole, the restatement is applied to those rows (the device's
own bits), and the run WITH the post-aggregator must equal that, in order, bit for bit."""
import ctypes
import heapq
import importlib
import math
import struct

import numpy as np
import pytest

import post_agg_restate as PR
import querygen as G
import test_special_values as SV

pytestmark = pytest.mark.gpu

PT1M = {"type": "period", "period": "PT1M"}
GROUPS_ALL = 13_757
DIMS2 = ("dimZipf", "dimSequential")


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("incubator-druid_amd.segment")


@pytest.fixture(scope="module")
def segs(basic_dirs, S):
    return [S.GpuSegment(p) for p in basic_dirs[("concise", "lz4")]]


@pytest.fixture(scope="module")
def specials(W, S, tmp_path_factory):
    path = W.write_segment(str(tmp_path_factory.mktemp("post_agg_specials") / "specials"), SV.specials_spec(W), lz4_mode="fast")
    return [S.GpuSegment(path)]


def _fa(n):
    return {"type": "fieldAccess", "fieldName": n}


def _const(v):
    return {"type": "constant", "value": v}


def _arith(name, fn, fields, ordering=None):
    js = {"type": "arithmetic", "name": name, "fn": fn, "fields": fields}
    if ordering:
        js["ordering"] = ordering
    return js


def _dw(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


# ---------------------------------------------------------------------------------------------
# 1. k_post_eval, bit for bit, through the raw ABI (the programs written out by hand)
# ---------------------------------------------------------------------------------------------
def _a_aggs(Q):
    return [Q.count("rows"), Q.long_sum("ls", "sumLongSequential"), Q.double_sum("ds", "sumFloatNormal"),
            Q.AggregatorFactory("doubleMax", "dmax", "sumFloatNormal"), Q.long_min("lmin", "sumLongSequential"),
            Q.float_sum("fs", "sumFloatNormal")]


def _a_query(Q, gran="all", dims_first=False, spec=None, having=None, post=(), aggs=None):
    ctx = {"applyLimitPushDown": False}
    if dims_first:
        ctx["sortByDimsFirst"] = True
    return Q.GroupByQuery(intervals=[(0, 1 << 42)], granularity=gran, dimensions=list(DIMS2), aggregations=aggs or _a_aggs(Q),
                          limitSpec=spec, having=having, context=ctx, postAggregations=list(post),
                          filter=Q.BoundDimFilter("dimSequential", "0", "300", upperStrict=True, ordering="numeric"))


def _b_query(Q, spec=None, having=None, post=(), dims_first=False):
    ctx = {"applyLimitPushDown": False}
    if dims_first:
        ctx["sortByDimsFirst"] = True
    return Q.GroupByQuery(intervals=SV.IV, granularity={"type": "duration", "duration": 4096}, dimensions=["g"],
                          aggregations=SV.specials_aggs(Q), limitSpec=spec, having=having, context=ctx,
                          postAggregations=list(post))


A, CD, CL, L2D, D2L = PR.AGG, PR.CONST_D, PR.CONST_L, PR.L2D, PR.D2L
# shape A slots: 0 rows, 1 ls, 2 ds, 3 dmax, 4 lmin, 5 fs
PROGRAMS_A = [
    ([(A, 2, 0), (A, 0, 0), (L2D, 0, 0), (PR.DIV, 0, 0)], PR.ORDER_DOUBLE),                                          # ds / rows
    ([(A, 1, 0), (L2D, 0, 0), (A, 4, 0), (L2D, 0, 0), (CL, 0, 3), (L2D, 0, 0), (PR.MUL, 0, 0), (PR.SUB, 0, 0)],
     PR.ORDER_DOUBLE),                                                                                               # ls - lmin * 3
    ([(A, 3, 0), (A, 5, 0), (PR.QUOT, 0, 0)], PR.ORDER_NUMERIC_FIRST),                                               # quotient(dmax, fs)
    ([(CD, 0, _dw(-math.inf)), (A, 2, 0), (PR.DMAX, 0, 0), (A, 3, 0), (PR.DMAX, 0, 0), (CD, 0, _dw(1.5)), (PR.DMAX, 0, 0)],
     PR.ORDER_DOUBLE),                                                                                               # doubleGreatest
    ([(CL, 0, PR.LONG_MAX), (A, 1, 0), (PR.LMIN, 0, 0), (A, 0, 0), (PR.LMIN, 0, 0), (A, 2, 0), (D2L, 0, 0), (PR.LMIN, 0, 0)],
     PR.ORDER_LONG),                                                                                                 # longLeast
]
# the specials' slots: 0 n, 1 dmin, 2 dmax, 3 ds, 4 fmin, 5 fmax, 6 fs, 7 ls, 8 lmin, 9 lmax, 10 ls_d, 11 lmax_d, 12 ds_l
PROGRAMS_B = [
    ([(A, 3, 0), (A, 0, 0), (L2D, 0, 0), (PR.DIV, 0, 0)], PR.ORDER_DOUBLE),                                          # ds / n
    ([(A, 7, 0), (L2D, 0, 0), (A, 8, 0), (L2D, 0, 0), (CL, 0, 3), (L2D, 0, 0), (PR.MUL, 0, 0), (PR.SUB, 0, 0)],
     PR.ORDER_DOUBLE),                                                                        # Long.MIN / MAX through L2D
    ([(A, 2, 0), (A, 6, 0), (PR.QUOT, 0, 0)], PR.ORDER_NUMERIC_FIRST),                                               # quotient(dmax, fs)
    ([(CD, 0, _dw(-math.inf)), (A, 3, 0), (PR.DMAX, 0, 0), (A, 2, 0), (PR.DMAX, 0, 0), (CD, 0, _dw(1.5)), (PR.DMAX, 0, 0)],
     PR.ORDER_DOUBLE),
    ([(CL, 0, PR.LONG_MAX), (A, 7, 0), (PR.LMIN, 0, 0), (A, 0, 0), (PR.LMIN, 0, 0), (A, 3, 0), (D2L, 0, 0), (PR.LMIN, 0, 0)],
     PR.ORDER_LONG),
    ([(A, 2, 0), (A, 1, 0), (PR.DIV, 0, 0)], PR.ORDER_DOUBLE),               # "/" by -0.0 (g3), by NaN (g1), by -inf (g4)
    ([(A, 1, 0), (A, 2, 0), (PR.QUOT, 0, 0)], PR.ORDER_NUMERIC_FIRST),       # -0.0 / 0.0 = NaN, 1e300 / inf = 0
    ([(CD, 0, _dw(5e-324)), (A, 2, 0), (PR.MUL, 0, 0)], PR.ORDER_DOUBLE),    # subnormal results
    ([(A, 5, 0), (A, 4, 0), (PR.DMIN, 0, 0), (A, 9, 0), (L2D, 0, 0), (PR.ADD, 0, 0)], PR.ORDER_DOUBLE),  # floats widened
    ([(A, 3, 0), (D2L, 0, 0), (A, 11, 0), (PR.LMAX, 0, 0)], PR.ORDER_LONG),  # D2L of NaN, +-inf, 1e300-sized sums
    ([(A, 1, 0), (CD, 0, _dw(1.0)), (PR.MUL, 0, 0)], PR.ORDER_DOUBLE),       # -0.0 stays -0.0
    # x * x - (1 + 2^-29) with x = 1 + 2^-30: 0.0 when the product is rounded first, 2^-60 from a fused multiply-add
    ([(CD, 0, _dw(1.0 + 2.0 ** -30)), (CD, 0, _dw(1.0 + 2.0 ** -30)), (PR.MUL, 0, 0), (CD, 0, _dw(-(1.0 + 2.0 ** -29))),
      (PR.ADD, 0, 0)], PR.ORDER_DOUBLE),
]


def _post_aggregate(N, res, programs):
    arr, keep = N.make_post_aggs(programs)
    ms = ctypes.c_double(-1.0)
    rc = N.lib().dg_result_post_aggregate(res.handle, arr, len(programs), ctypes.byref(ms))
    return rc, ms.value


def _raw_slots(N, res, na):
    n = int(N.lib().dg_result_groups(res.handle))
    vals = np.zeros(max(n * na, 1), dtype=np.uint64)
    N.check(N.lib().dg_result_fetch_groups(res.handle, 0, n, None, None, vals.ctypes.data))
    return vals[:n * na].reshape(n, na)


def _post_values(N, res, col, n, start=0):
    out = np.zeros(max(n, 1), dtype=np.uint64)
    N.check(N.lib().dg_result_post_values(res.handle, col, start, n, out.ctypes.data))
    return out[:n]


def _eval_check(Q, R, N, segs, q, programs, groups):
    classes = [PR.slot_class(a.output_type) for a in Q.native_aggregations(q.aggregations)]
    res = R.groupby_run(segs, q)
    try:
        assert res.groups == groups
        rc, ms = _post_aggregate(N, res, programs)
        assert rc == 0 and ms >= 0.0
        slots = _raw_slots(N, res, len(classes))
        seen = set()
        for c, (ops, order) in enumerate(programs):
            got = _post_values(N, res, c, groups).tolist()
            for g in range(groups):
                want = PR.interpret(ops, slots[g].tolist(), classes)
                assert got[g] == want, (c, g, hex(got[g]), hex(want), [hex(x) for x in slots[g].tolist()])
                if order != PR.ORDER_LONG:
                    d = PR.dbl(want)
                    seen.add("nan" if d != d else "+inf" if d == math.inf else "-inf" if d == -math.inf else
                             "sub" if d != 0.0 and abs(d) < 2.2250738585072014e-308 else
                             "-0" if want == PR.SIGN else "fin")
            # a page in the middle, across a workgroup's edge
            if groups > 600:
                assert _post_values(N, res, c, 300, 250).tolist() == got[250:550]
        # the slots themselves are untouched
        assert np.array_equal(_raw_slots(N, res, len(classes)), slots)
        return seen
    finally:
        res.release()


def test_post_eval_shape_a(Q, R, N, segs):
    """13,757 groups: 53 full 256-lane workgroups and a ragged last one of 189 lanes (two full waves and 61
    lanes of a third)."""
    seen = _eval_check(Q, R, N, segs, _a_query(Q), PROGRAMS_A, GROUPS_ALL)
    assert "fin" in seen


def test_post_eval_special_values(Q, R, N, specials):
    seen = _eval_check(Q, R, N, specials, _b_query(Q), PROGRAMS_B, 37)
    assert seen >= {"nan", "+inf", "-inf", "sub", "fin", "-0"}, seen


# ---------------------------------------------------------------------------------------------
# 2. groupBy decisions: having and limit specs over post-aggregators
# ---------------------------------------------------------------------------------------------
# name -> (JSON, the restatement over a row's aggregator values -> word, order kind, value type)
def _restate_avg(e, rows="rows", ds="ds"):
    rhs = float(e[rows])
    return PR.bits(0.0 if rhs == 0.0 else e[ds] / rhs)


POSTS_A = {
    "avg": (_arith("avg", "/", [_fa("ds"), _fa("rows")]), _restate_avg, PR.ORDER_DOUBLE, "double"),
    "lin": (_arith("lin", "-", [_fa("ls"), _arith(None, "*", [_fa("lmin"), _const(3)])]),
            lambda e: PR.bits(float(e["ls"]) - float(e["lmin"]) * 3.0), PR.ORDER_DOUBLE, "double"),
    "quot": (_arith("quot", "quotient", [_fa("dmax"), _fa("fs")], "numericFirst"),
             lambda e: PR.bits(PR.ieee_div(e["dmax"], e["fs"])), PR.ORDER_NUMERIC_FIRST, "double"),
    "least": ({"type": "longLeast", "name": "least", "fields": [_fa("ls"), _fa("rows"), _fa("ds")]},
              lambda e: min(e["ls"], e["rows"], PR.d2l(e["ds"])) & PR.M64, PR.ORDER_LONG, "long"),
    "one": ({"type": "constant", "name": "one", "value": 1}, lambda e: 1, PR.ORDER_NONE, "long"),
}
POSTS_B = {
    "avg": (_arith("avg", "/", [_fa("ds"), _fa("n")]), lambda e: _restate_avg(e, "n"), PR.ORDER_DOUBLE, "double"),
    "quot": (_arith("quot", "quotient", [_fa("dmax"), _arith(None, "+", [_fa("lmax_d"), _const(2)])], "numericFirst"),
             lambda e: PR.bits(PR.ieee_div(e["dmax"], float(e["lmax_d"]) + 2.0)), PR.ORDER_NUMERIC_FIRST, "double"),
    "dz": (_arith("dz", "/", [_fa("dmax"), _fa("dmin")]),
           lambda e: PR.bits(0.0 if e["dmin"] == 0.0 else e["dmax"] / e["dmin"]), PR.ORDER_DOUBLE, "double"),
    "great": ({"type": "longGreatest", "name": "great", "fields": [_fa("ds"), _fa("lmax_d")]},
              lambda e: max(PR.d2l(e["ds"]), e["lmax_d"]) & PR.M64, PR.ORDER_LONG, "long"),
}


class _Rev:
    def __init__(self, v):
        self.v = v

    def __lt__(self, o):
        return o.v < self.v

    def __eq__(self, o):
        return self.v == o.v


def _having_restated(h, row, posts):
    """The having tree over a row; a leaf on a post-aggregator compares its value with the leaf's (a double
    against a float value: Double.compare; a long against an int)."""
    t = h["type"]
    if t == "and":
        return all(_having_restated(x, row, posts) for x in h["havingSpecs"])
    if t == "or":
        return any(_having_restated(x, row, posts) for x in h["havingSpecs"])
    if t == "not":
        return not _having_restated(h["havingSpec"], row, posts)
    name, value = h["aggregation"], h["value"]
    if name in posts:
        w, vt = posts[name][1](row.event), posts[name][3]
        if vt == "double":
            assert isinstance(value, float)
            c = PR.double_compare(PR.dbl(w), value)
        else:
            assert isinstance(value, int)
            c = (PR.to_signed(w) > value) - (PR.to_signed(w) < value)
    else:
        v = row.event[name]
        assert isinstance(v, int) and isinstance(value, int)
        c = (v > value) - (v < value)
    return c > 0 if t == "greaterThan" else (c < 0 if t == "lessThan" else c == 0)


def _expected(q, rows, posts):
    """GroupByQuery.postProcess restated: having, then a stable sort by the limit spec's comparator chain (time
    first, or last with sortByDimsFirst; absent for ALL), then the limit. `rows` arrive in the order the merge
    hands them over (comparator-equal groups keep it)."""
    js = q.to_json()
    if js.get("having"):
        rows = [r for r in rows if _having_restated(js["having"], r, posts)]
    ls = js.get("limitSpec")
    if ls is None:
        return rows
    parts = []
    for c in ls["columns"]:
        name, desc = c["dimension"], c["direction"] == "descending"
        if name in posts:
            fn, order = posts[name][1], posts[name][2]
            kf = (lambda f, o: lambda r: PR.order_key(o, f(r.event)))(fn, order)
        elif name in q.dimensions:
            kf = (lambda n: lambda r: r.event[n])(name)  # (ASCII values: LEXICOGRAPHIC is the plain string order)
        else:
            kf = (lambda n: lambda r: r.event[n])(name)
            assert all(isinstance(r.event[name], int) for r in rows[:1])
        parts.append((kf, desc))
    timed = js["granularity"] != "all"
    dims_first = bool(q.context.get("sortByDimsFirst"))

    def key(r):
        ks = tuple(_Rev(f(r)) if d else f(r) for f, d in parts)
        if not timed:
            return ks
        return ks + (r.timestamp,) if dims_first else (r.timestamp,) + ks

    rows = sorted(rows, key=key)
    return rows[:ls["limit"]] if ls.get("limit") else rows


def _bits(v):
    return v if isinstance(v, (int, str)) or v is None else struct.pack("<d", v)


def _event_rows(Q, R, q, part):
    dims = part.dims
    return [Q.Row(int(part.times[r]), {**{d: dims[i][r] for i, d in enumerate(q.dimensions)},
                                       **{a.name: R._py(col[r], a.output_type) for a, col in zip(q.aggregations, part.aggs)}})
            for r in range(len(part))]


def _same_rows(q, got, exp, posts=None):
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        assert a.timestamp == b.timestamp, i
        for n in list(q.dimensions) + [g.name for g in q.aggregations]:
            assert _bits(a.event[n]) == _bits(b.event[n]), (i, n, a.event, b.event)
        for p in q.postAggregations if posts else []:  # the values the host adds: the restatement's bits
            fn, vt = posts[p.name][1], posts[p.name][3]
            got_w = (a.event[p.name] & PR.M64) if vt == "long" else PR.bits(a.event[p.name])
            assert got_w == fn(b.event), (i, p.name, a.event)


_PLAIN = {}


def _plain_rows(R, segs, plain):
    key = (id(segs), repr(plain.to_json()))
    if key not in _PLAIN:
        res = R.groupby_run(segs, plain)
        try:
            _PLAIN[key] = R.merge_groupby(plain, [res.fetch()])
        finally:
            res.release()
    return _PLAIN[key]


def _check(Q, R, segs, q, plain, posts):
    rows = _plain_rows(R, segs, plain)
    exp = _expected(q, list(rows), posts)
    res = R.groupby_run(segs, q)
    try:
        assert res.groups == len(rows)
        assert res.apply_post_process()
        assert res.post_programs and res.post_aggregate_ms >= 0.0  # dg_result_post_aggregate ran in front of it
        info = res.post_info
        assert info["groups_in"] == len(rows) and info["groups_kept"] == len(exp) == res.groups  # only those are fetched
        part = res.fetch()
        assert len(part) == len(exp)
        got = _event_rows(Q, R, q, part)
        # the columns are dropped by the step: they existed to decide
        assert N_lib(R).dg_result_post_values(res.handle, 0, 0, 1, np.zeros(1, dtype=np.uint64).ctypes.data) == R.N.ERR_ARG
    finally:
        res.release()
    _same_rows(q, got, exp)
    # the host pass over what was fetched is idempotent and adds every post-aggregator's value
    _same_rows(q, R.postprocess_groupby(q, list(got)), exp, posts)
    return info, exp


def N_lib(R):
    return R.N.lib()


def _col(name, desc=False):
    return {"dimension": name, "direction": "descending" if desc else "ascending", "dimensionOrder": "lexicographic"}


def _median_value(rows, fn, vt):
    vals = sorted((PR.dbl(fn(r.event)) if vt == "double" else PR.to_signed(fn(r.event))) for r in rows)
    vals = [v for v in vals if v == v]
    return vals[len(vals) // 2]


def _havings(rows, posts, name):
    """greaterThan / equalTo / lessThan on the post-aggregator, alone and under and / or / not."""
    fn, vt = posts[name][1], posts[name][3]
    mid = _median_value(rows, fn, vt)
    gt = {"type": "greaterThan", "aggregation": name, "value": mid}
    eq = {"type": "equalTo", "aggregation": name, "value": mid}
    lt = {"type": "lessThan", "aggregation": name, "value": mid}
    count = "rows" if "rows" in rows[0].event else "n"
    return {"gt": gt, "eq": eq, "lt": lt,
            "and-or-not": {"type": "and", "havingSpecs": [
                {"type": "or", "havingSpecs": [lt, eq]},
                {"type": "not", "havingSpec": {"type": "equalTo", "aggregation": count, "value": rows[0].event[count]}}]}}


SPECS_A = {
    "avg-desc-100": [_col("avg", True)],
    "avg-asc": [_col("avg")],
    "zipf-then-lin-desc": [_col("dimZipf"), _col("lin", True)],
    "rows-desc-then-quot": [_col("rows", True), _col("quot")],
    "quot-numeric-first-desc": [_col("quot", True)],
    "least-asc-then-avg-desc": [_col("least"), _col("avg", True)],
    "constant-then-avg": [_col("one", True), _col("avg")],  # an always-equal comparator decides nothing
}


@pytest.mark.parametrize("spec", sorted(SPECS_A))
def test_groupby_order_by_post_aggregator(Q, R, segs, spec):
    used = [c["dimension"] for c in SPECS_A[spec] if c["dimension"] in POSTS_A]
    post = [POSTS_A[n][0] for n in used]
    ls = {"type": "default", "columns": SPECS_A[spec], "limit": 100}
    q = _a_query(Q, spec=ls, post=post)
    assert not q.apply_limit_push_down()  # never pushed down (testGroupByLimitPushDownPostAggNotSupported)
    info, exp = _check(Q, R, segs, q, _a_query(Q), POSTS_A)
    assert info["groups_in"] == GROUPS_ALL and len(exp) == 100 and info["groups_after_having"] == GROUPS_ALL


@pytest.mark.parametrize("leaf", ["gt", "eq", "lt", "and-or-not"])
@pytest.mark.parametrize("name", ["avg", "least"])
def test_groupby_having_on_post_aggregator(Q, R, segs, name, leaf):
    plain = _a_query(Q)
    rows = _plain_rows(R, segs, plain)
    having = _havings(rows, POSTS_A, name)[leaf]
    for ls in (None, {"type": "default", "columns": [_col("avg", True), _col("dimSequential")], "limit": 50}):
        post = [POSTS_A[n][0] for n in sorted({name} | ({"avg"} if ls else set()))]
        info, exp = _check(Q, R, segs, _a_query(Q, spec=ls, having=having, post=post), plain, POSTS_A)
        kept = info["groups_after_having"]
        assert kept == sum(1 for r in rows if _having_restated(having, r, POSTS_A))
        assert (0 < kept < GROUPS_ALL) if leaf != "eq" else kept >= 1
        assert len(exp) == (min(kept, 50) if ls else kept)


def test_groupby_time_granularity_and_dims_first(Q, R, segs):
    post = [POSTS_A["avg"][0], POSTS_A["quot"][0]]
    ls = {"type": "default", "columns": [_col("quot", True), _col("avg")], "limit": 40}
    for dims_first in (False, True):
        plain = _a_query(Q, PT1M, dims_first)
        rows = _plain_rows(R, segs, plain)
        having = _havings(rows, POSTS_A, "avg")["gt"]
        info, exp = _check(Q, R, segs, _a_query(Q, PT1M, dims_first, ls, having, post), plain, POSTS_A)
        assert info["groups_in"] > GROUPS_ALL and 40 < info["groups_after_having"] < info["groups_in"] and len(exp) == 40
        if dims_first:  # the metric decides before the time: the buckets interleave
            assert len({r.timestamp for r in exp}) > 1 and [r.timestamp for r in exp] != sorted(r.timestamp for r in exp)


@pytest.mark.parametrize("spec", ["quot-desc", "quot-asc", "g-then-dz", "great-desc-avg", "avg-asc-dims-first"])
def test_groupby_special_values(Q, R, specials, spec):
    """37 groups whose post-aggregators are NaN, +-inf, +-0.0 and Long.MAX_VALUE: numericFirst against
    Double.compare, "/" by -0.0, and a having in front."""
    cols = {"quot-desc": [_col("quot", True)], "quot-asc": [_col("quot")], "g-then-dz": [_col("g", True), _col("dz")],
            "great-desc-avg": [_col("great", True), _col("avg")], "avg-asc-dims-first": [_col("avg")]}[spec]
    dims_first = spec.endswith("dims-first")
    plain = _b_query(Q, dims_first=dims_first)
    rows = _plain_rows(R, specials, plain)
    assert len(rows) == 37
    used = [c["dimension"] for c in cols if c["dimension"] in POSTS_B]
    words = {n: [POSTS_B[n][1](r.event) for r in rows] for n in used}
    if "quot" in used:
        ds = [PR.dbl(w) for w in words["quot"]]
        assert any(d != d for d in ds) and math.inf in ds and -math.inf in ds and any(math.isfinite(d) for d in ds)
    for limit, having in ((None, None), (5, None), (30, {"type": "not", "havingSpec": {"type": "equalTo", "aggregation": used[0],
                                                                                       "value": 0.0 if POSTS_B[used[0]][3] == "double" else 0}})):
        ls = {"type": "default", "columns": cols}
        if limit:
            ls["limit"] = limit
        post = [POSTS_B[n][0] for n in used]
        _check(Q, R, specials, _b_query(Q, ls, having, post, dims_first), plain, POSTS_B)


@pytest.fixture(scope="module")
def two_contexts(basic_dirs, S):
    ca, cb = S.GpuContext(0), S.GpuContext(0)
    return [S.GpuSegment(p, context=ca if i % 2 == 0 else cb) for i, p in enumerate(basic_dirs[("concise", "lz4")])]


def test_run_query_two_contexts(Q, R, two_contexts):
    """dg_groupby_merge_devices results take the step too (one per key range); integer aggregators, so the rows
    do not depend on the merge's order."""
    aggs = [Q.count("rows"), Q.long_sum("ls", "sumLongSequential"), Q.long_min("lmin", "sumLongSequential")]
    posts = {"ratio": (_arith("ratio", "/", [_fa("ls"), _fa("rows")]),
                       lambda e: PR.bits(0.0 if e["rows"] == 0 else float(e["ls"]) / float(e["rows"])), PR.ORDER_DOUBLE, "double"),
             "lin": POSTS_A["lin"]}
    ls = {"type": "default", "columns": [_col("ratio", True), _col("lin")], "limit": 60}
    plain = _a_query(Q, aggs=aggs)
    rows = R.run_query(plain, two_contexts)
    assert len(rows) == GROUPS_ALL
    having = {"type": "greaterThan", "aggregation": "ratio", "value": _median_value(rows, posts["ratio"][1], "double")}
    q = _a_query(Q, spec=ls, having=having, post=[posts["ratio"][0], posts["lin"][0]], aggs=aggs)
    exp = _expected(q, list(rows), posts)
    stats = R.RunStats()
    got = R.run_query(q, two_contexts, stats)
    assert len(exp) == 60
    _same_rows(q, got, exp, posts)
    assert len(stats.post) == 2 and sum(p["groups_in"] for p in stats.post) == GROUPS_ALL
    assert all(p["groups_kept"] <= 60 for p in stats.post)


# ---------------------------------------------------------------------------------------------
# 3. topN ranked by a post-aggregator
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_segs(S):
    segs = [S.GpuSegment(p) for p in G.layout_paths(0)]
    yield segs
    for s in segs:
        s.close()


TN_AGGS = (("lsum", "longSum", "l"), ("rows", "count", None), ("dsum", "doubleSum", "d"))
TN_POST = _arith("avg", "/", [_fa("lsum"), _fa("rows")])


def _tn_word(e):
    return PR.bits(0.0 if e["rows"] == 0 else float(e["lsum"]) / float(e["rows"]))


def _tn_query(Q, dim, metric, threshold, gran="all", post=(), dim_type="STRING", interval=G.WHOLE, aggs=TN_AGGS, ctx=None):
    return Q.TopNQuery(intervals=[interval], granularity=gran, dimension=dim, dimension_type=dim_type, metric=metric,
                       threshold=threshold, aggregations=[Q.AggregatorFactory(t, n, f) for n, t, f in aggs],
                       postAggregations=list(post), context=dict(ctx or {}))


def _dim_key(v):
    return (0, "") if v is None else (1, v)


class _Builder:
    """TopNNumericResultBuilder (TopNNumericResultBuilder.java:94-235): a priority queue on (metric, then the
    dimension value); an entry is added while the queue is short or when its metric beats the queue's least."""

    def __init__(self, threshold, dim, key_of):
        self.k, self.dim, self.key_of, self.heap, self.n = threshold, dim, key_of, [], 0

    def add(self, e):
        mk = self.key_of(e)
        if len(self.heap) < self.k or self.heap[0][0] < mk:
            heapq.heappush(self.heap, (mk, _dim_key(e[self.dim]), self.n, e))
            self.n += 1
        if len(self.heap) > self.k:
            heapq.heappop(self.heap)

    def build(self):
        return [h[3] for h in sorted(self.heap, key=lambda h: (-h[0], h[1]))]


def _java_max(a, b):
    """Math.max of two doubles: NaN wins, 0.0 above -0.0."""
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a >= b else b


def _combine(a, b, dim, aggs):
    """AggregatorFactory.combine of the aggregator types these tests use."""
    out = {dim: a[dim]}
    for n, t, _ in aggs:
        if t == "doubleSum":
            out[n] = a[n] + b[n]
        elif t == "doubleMax":
            out[n] = _java_max(a[n], b[n])
        elif t == "longMax":
            out[n] = max(a[n], b[n])
        else:
            assert t in ("longSum", "count")
            out[n] = PR.to_signed((a[n] + b[n]) & PR.M64)
    return out


def _fold(lists, threshold, dim, key_of, aggs):
    """TopNBinaryFn (TopNBinaryFn.java:75-135) over lists in merge order: r1's entries, then r2's new values,
    shared values combined; the metric recomputed; the builder with the query's threshold."""
    acc = None
    for entries in lists:
        if acc is None:
            acc = list(entries)
            continue
        ret = {e[dim]: e for e in acc}
        for e in entries:
            ret[e[dim]] = _combine(ret[e[dim]], e, dim, aggs) if e[dim] in ret else e
        b = _Builder(threshold, dim, key_of)
        for e in ret.values():
            b.add(e)
        acc = b.build()
    return (acc or [])[:threshold]


def _strip(entries, dim, aggs):
    return [{k: e[k] for k in [dim] + [n for n, _, _ in aggs]} for e in entries]


def _same_entries(got, exp, dim, word_of, post_name, aggs=TN_AGGS):
    assert [e[dim] for e in got] == [e[dim] for e in exp]
    for a, b in zip(got, exp):
        for n, _, _ in aggs:
            assert _bits(a[n]) == _bits(b[n]), (n, a, b)
        assert PR.bits(a[post_name]) == word_of(b), (a, b)  # every post-aggregator's value rides along


def _topn_case(Q, R, segs, dim, gran, metrics, thresholds, word_of=_tn_word, post=TN_POST, order=PR.ORDER_DOUBLE,
               aggs=TN_AGGS, interval=G.WHOLE):
    """Per-segment lists and the merged result of every (metric spec, threshold) against the restatement over a
    full-threshold run of the same aggregators."""
    full_q = _tn_query(Q, dim, aggs[1][0], 100_000, gran, aggs=aggs, interval=interval)
    full = R.topn_per_segment(segs, full_q)  # per segment: one Result per bucket, every value of the dimension
    name = post["name"]
    for inverted in metrics:
        def key_of(e, inv=inverted):
            k = PR.order_key(order, word_of(e))
            return (PR.M64 - k) if inv else k

        spec = {"type": "inverted", "metric": {"type": "numeric", "metric": name}} if inverted else name
        for T in thresholds:
            q = _tn_query(Q, dim, spec, T, gran, [post], aggs=aggs, interval=interval)
            K = q.segment_threshold
            per = R.topn_per_segment(segs, q)
            want_lists = {}
            for si, results in enumerate(full):
                assert len(per[si]) == len(results)
                for got_r, full_r in zip(per[si], results):
                    b = _Builder(K, dim, key_of)
                    for e in sorted(_strip(full_r.value, dim, aggs), key=lambda e: _dim_key(e[dim])):  # offered in value order
                        b.add(e)
                    want = b.build()
                    assert got_r.timestamp == full_r.timestamp
                    _same_entries(got_r.value, want, dim, word_of, name, aggs)
                    bucket = 0 if q.granularity.is_all else q.granularity.bucket_start(got_r.timestamp)
                    want_lists.setdefault(bucket, []).append((got_r.timestamp, si, want))
            merged = R.run_query(q, segs)
            assert len(merged) == len(want_lists)
            for r, bucket in zip(merged, sorted(want_lists)):  # the lists in merge order: (timestamp, segment)
                lists = [w for _, _, w in sorted(want_lists[bucket], key=lambda x: (x[0], x[1]))]
                assert q.granularity.is_all or r.timestamp == bucket
                _same_entries(r.value, _fold(lists, T, dim, key_of, aggs), dim, word_of, name, aggs)
    return full


@pytest.mark.parametrize("gran", ["all", "hour"])
@pytest.mark.parametrize("dim", ["lo", "mid", "hi"])
def test_topn_ranked_by_post_aggregator(Q, R, gen_segs, dim, gran):
    """Cardinalities 5, 300 and about 12,000 (below one k_topn_keys workgroup, and many); two segments, so the
    merge re-ranks; under `hour` one list per bucket."""
    full = _topn_case(Q, R, gen_segs, dim, gran, (False, True), (1, 7, 1000))
    card = max(len(r.value) for rs in full for r in rs)
    if gran == "all":  # (hi: the per-segment threshold of 1000 cuts)
        assert {"lo": card == 5, "mid": card == 300, "hi": card > 9_000}[dim]


@pytest.mark.parametrize("dim", ["lo", "mid", "hi"])
def test_topn_plan_switches(Q, R, gen_segs, dim, monkeypatch):
    """The pooled path (no dimension index) feeds the new keys too."""
    monkeypatch.setenv("DG_NO_TOPN_INDEX", "1")
    _topn_case(Q, R, gen_segs, dim, "all", (False, True), (7,))


def test_topn_numeric_first_special_values(Q, R, W, S, tmp_path_factory):
    """quotient(dmax, lmax_d + 2) under numericFirst over the specials in two segments: finite values rank above
    NaN, NaN above +inf, +inf above -inf; inverted, the other way round."""
    base = tmp_path_factory.mktemp("post_agg_topn_specials")
    half = 10_000  # (inside a 4,096 ms bucket: the merge combines that bucket's values too)
    segs = [S.GpuSegment(W.write_segment(str(base / ("s%d" % i)), SV.specials_spec(W, lo, hi), lz4_mode="fast"))
            for i, (lo, hi) in enumerate(((0, half), (half, SV.N_ROWS)))]
    aggs = (("dmax", "doubleMax", "d"), ("n", "count", None), ("lmax_d", "longMax", "d"))
    post = _arith("quot", "quotient", [_fa("dmax"), _arith(None, "+", [_fa("lmax_d"), _const(2)])], "numericFirst")
    word = lambda e: PR.bits(PR.ieee_div(e["dmax"], float(e["lmax_d"]) + 2.0))

    def combine_check(full):
        ds = [PR.dbl(word(e)) for rs in full for r in rs for e in r.value]
        assert any(d != d for d in ds) and math.inf in ds and -math.inf in ds and any(math.isfinite(d) for d in ds)

    try:
        for gran in ("all", {"type": "duration", "duration": 4096}):
            combine_check(_topn_case(Q, R, segs, "g", gran, (False, True), (1, 4, 7), word, post, PR.ORDER_NUMERIC_FIRST, aggs,
                                     interval=SV.IV[0]))
    finally:
        for s in segs:
            s.close()


def test_topn_long_dimension(Q, R, gen_segs):
    """The LONG column v ranked by lsum / rows: which of the values tied with the last entry a list keeps is
    arbitrary in the reference, and the engine reports how many it left out (cut_ties): everything above the
    last key must match exactly, the ties must be values that do tie."""
    for T in (1, 7, 1000):
        full_q = _tn_query(Q, "v", "rows", 100_000, dim_type="LONG")
        q = _tn_query(Q, "v", "avg", T, post=[TN_POST], dim_type="LONG", ctx={"minTopNThreshold": 50})
        key_of = lambda e: PR.order_key(PR.ORDER_DOUBLE, _tn_word(e))
        full = R.topn_per_segment(gen_segs, full_q)
        stats = R.RunStats()
        per = R.topn_per_segment(gen_segs, q, stats)
        ties = sum(c.get("topn_cut_ties", 0) for c in stats.calls)
        K = q.segment_threshold
        for si in range(len(gen_segs)):
            (got_r,), (full_r,) = per[si], full[si]
            b = _Builder(K, "v", key_of)
            for e in sorted(_strip(full_r.value, "v", TN_AGGS), key=lambda e: e["v"]):
                b.add(e)
            want = b.build()
            assert len(got_r.value) == len(want) == min(K, len(full_r.value))
            last = key_of(want[-1])
            above = [e for e in want if key_of(e) > last]
            _same_entries(got_r.value[:len(above)], above, "v", _tn_word, "avg")
            by_value = {e["v"]: e for e in _strip(full_r.value, "v", TN_AGGS)}
            for e in got_r.value[len(above):]:
                assert key_of(by_value[e["v"]]) == last and _bits(e["lsum"]) == _bits(by_value[e["v"]]["lsum"])
            if ties == 0:
                _same_entries(got_r.value, want, "v", _tn_word, "avg")
        merged = R.run_query(q, gen_segs)
        assert len(merged) == 1 and len(merged[0].value) == T
        keys = [key_of(e) for e in merged[0].value]
        assert keys == sorted(keys, reverse=True)


def test_topn_end_to_end_against_oracle(Q, O, R, gen_segs):
    """longSum / count ranked on `mid` (300 values: no per-segment cut) against the oracle's aggregates, which
    are exact in any order."""
    aggs = TN_AGGS[:2]
    full = O.run(_tn_query(Q, "mid", "rows", 100_000, aggs=aggs), G.oracle_segments(0))
    (full_r,) = full
    assert len(full_r.value) == 300
    for inverted in (False, True):
        spec = {"type": "inverted", "metric": {"type": "numeric", "metric": "avg"}} if inverted else "avg"
        key_of = lambda e: (PR.M64 - PR.order_key(PR.ORDER_DOUBLE, _tn_word(e))) if inverted else PR.order_key(PR.ORDER_DOUBLE, _tn_word(e))
        ranked = sorted(_strip(full_r.value, "mid", aggs), key=lambda e: (-key_of(e), e["mid"]))
        assert key_of(ranked[6]) != key_of(ranked[7])  # no tie at the cut: the queue's order does not matter
        (got,) = R.run_query(_tn_query(Q, "mid", spec, 7, post=[TN_POST], aggs=aggs), gen_segs)
        _same_entries(got.value, ranked[:7], "mid", _tn_word, "avg", aggs)


# ---------------------------------------------------------------------------------------------
# 4. refusals: DG_ERR_ARG before any launch, the result usable afterwards
# ---------------------------------------------------------------------------------------------
def test_post_aggregate_refusals(Q, R, N, segs):
    aggs = _a_aggs(Q) + [Q.long_first("lf", "sumLongSequential")]  # native slots 6 (value) and 7 (DG_AGG_PAIR_TIME)
    q = _a_query(Q, aggs=aggs)
    na = len(Q.native_aggregations(aggs))
    assert na == 8
    res = R.groupby_run(segs, q)
    try:
        before = _raw_slots(N, res, na)
        push = (A, 0, 0)
        bad = {
            "underflow": [([(PR.ADD, 0, 0)], PR.ORDER_DOUBLE)],
            "underflow-unary": [([(L2D, 0, 0)], PR.ORDER_DOUBLE)],
            "overflow": [([push] * 17 + [(PR.LMAX, 0, 0)] * 16, PR.ORDER_LONG)],
            "two-values": [([push, push], PR.ORDER_LONG)],
            "no-ops": [([], PR.ORDER_LONG)],
            "too-long": [([push] + [push, (PR.LMAX, 0, 0)] * 32, PR.ORDER_LONG)],
            "slot-index": [([(A, na, 0)], PR.ORDER_LONG)],
            "slot-negative": [([(A, -1, 0)], PR.ORDER_LONG)],
            "pair-time": [([(A, 7, 0)], PR.ORDER_LONG)],
            "unknown-op": [([(14, 0, 0)], PR.ORDER_LONG)],
            "operand-type": [([push, push, (PR.ADD, 0, 0)], PR.ORDER_DOUBLE)],
            "order-kind": [([push], PR.ORDER_DOUBLE)],
            "second-of-two-bad": [([push], PR.ORDER_LONG), ([(PR.ADD, 0, 0)], PR.ORDER_DOUBLE)],
        }
        for name, programs in bad.items():
            rc, _ = _post_aggregate(N, res, programs)
            assert rc == N.ERR_ARG, name
            assert N.lib().dg_last_error().decode() != ""
            assert N.lib().dg_result_post_values(res.handle, 0, 0, 1, np.zeros(1, dtype=np.uint64).ctypes.data) == N.ERR_ARG
        assert N.lib().dg_result_post_aggregate(res.handle, None, 1, None) == N.ERR_ARG
        arr, keep = N.make_post_aggs([([push], PR.ORDER_LONG)] * 17)
        assert N.lib().dg_result_post_aggregate(res.handle, arr, 17, None) == N.ERR_ARG  # more than DG_POST_MAX_COLS
        assert np.array_equal(_raw_slots(N, res, na), before)
        # without post columns an index at the aggregator count is refused as before
        col = N.dg_post_column(N.ORDER_AGG, na, 0, 0, None)
        pp = N.dg_post_process(None, 0, 1, ctypes.cast(ctypes.pointer(col), ctypes.c_void_p), 1, 0, 5, 0)
        assert N.lib().dg_result_post_process(res.handle, ctypes.byref(pp), None) == N.ERR_ARG
        # a valid call: the pair's value slot may be read; then a second call is refused and the columns stay
        good = [([(A, 6, 0), (A, 0, 0), (PR.LMAX, 0, 0)], PR.ORDER_LONG), ([(CL, 0, 7)], PR.ORDER_NONE)]
        rc, _ = _post_aggregate(N, res, good)
        assert rc == 0
        vals = _post_values(N, res, 0, res.groups)
        assert vals.tolist() == [max(PR.to_signed(int(a)), PR.to_signed(int(b))) & PR.M64 for a, b in zip(before[:, 6], before[:, 0])]
        assert set(_post_values(N, res, 1, res.groups).tolist()) == {7}
        assert _post_aggregate(N, res, good)[0] == N.ERR_ARG
        for args in ((2, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, res.groups + 1), (0, res.groups, 1)):
            assert N.lib().dg_result_post_values(res.handle, *args, np.zeros(1, dtype=np.uint64).ctypes.data) == N.ERR_ARG
        assert np.array_equal(_post_values(N, res, 0, res.groups), vals)
        # the push-down's limit is not for a result with post columns; an index past the post columns is refused
        lim = N.dg_limit(None, 0, 3, 0)
        assert N.lib().dg_result_limit(res.handle, ctypes.byref(lim)) == N.ERR_ARG
        col = N.dg_post_column(N.ORDER_AGG, na + 2, 0, 0, None)
        pp = N.dg_post_process(None, 0, 1, ctypes.cast(ctypes.pointer(col), ctypes.c_void_p), 1, 0, 5, 0)
        assert N.lib().dg_result_post_process(res.handle, ctypes.byref(pp), None) == N.ERR_ARG
        assert int(N.lib().dg_result_groups(res.handle)) == res.groups and np.array_equal(_raw_slots(N, res, na), before)
        # ordered by the constant column alone: accepted, nothing to sort by, the first five in key order
        col = N.dg_post_column(N.ORDER_AGG, na + 1, 1, 0, None)
        pp = N.dg_post_process(None, 0, 1, ctypes.cast(ctypes.pointer(col), ctypes.c_void_p), 1, 0, 5, 0)
        assert N.lib().dg_result_post_process(res.handle, ctypes.byref(pp), None) == 0
        assert int(N.lib().dg_result_groups(res.handle)) == 5
        assert np.array_equal(_raw_slots(N, res, na), before[:5])
        # a post-processed result takes no post-aggregators
        assert _post_aggregate(N, res, good)[0] == N.ERR_ARG
        assert np.array_equal(_raw_slots(N, res, na), before[:5])
    finally:
        res.release()
    res = R.groupby_run(segs, q)
    try:  # a result limited by the push-down
        lim = N.dg_limit(None, 0, 3, 0)
        assert N.lib().dg_result_limit(res.handle, ctypes.byref(lim)) == 0
        assert _post_aggregate(N, res, [([(A, 0, 0)], PR.ORDER_LONG)])[0] == N.ERR_ARG
        assert np.array_equal(_raw_slots(N, res, na), before[:3])
    finally:
        res.release()


def test_topn_post_refusals(Q, R, N, gen_segs):
    """DG_POST_ORDER_NONE, a dimension-ordered spec with a program and a bad program are DG_ERR_ARG; the same call
    without the program (metric == NULL) is dg_topn_run_opts itself."""
    q = _tn_query(Q, "mid", "rows", 7)
    K, na, n = q.segment_threshold, 3, len(gen_segs)

    def run(query, programs):
        scan, keep = N.make_scan(query, Q, segments=gen_segs)
        t, keep_t = R._topn_struct(query, K, gen_segs)
        cnt = np.zeros(n, dtype=np.int32)
        ids = np.zeros(n * K, dtype=np.int32)
        vals = np.zeros(n * K * na, dtype=np.uint64)
        bt = np.zeros(n, dtype=np.int64)
        t.bucket_cap, t.out_bucket_time = 1, bt.ctypes.data
        arr = N.make_post_aggs(programs) if programs else (None, None)
        rc = N.lib().dg_topn_run_post(R._handles(gen_segs), n, ctypes.byref(scan), ctypes.byref(t), None, arr[0],
                                      cnt.ctypes.data, ids.ctypes.data, vals.ctypes.data, None)
        return rc, cnt, ids, vals

    ratio = ([(A, 0, 0), (L2D, 0, 0), (A, 1, 0), (L2D, 0, 0), (PR.DIV, 0, 0)], PR.ORDER_DOUBLE)
    assert run(q, [([(CL, 0, 1)], PR.ORDER_NONE)])[0] == N.ERR_ARG
    assert run(q, [([(PR.ADD, 0, 0)], PR.ORDER_DOUBLE)])[0] == N.ERR_ARG
    assert run(q, [([(A, 3, 0)], PR.ORDER_LONG)])[0] == N.ERR_ARG
    lex = _tn_query(Q, "mid", {"type": "dimension", "ordering": "lexicographic"}, 7)
    assert run(lex, [ratio])[0] == N.ERR_ARG
    assert "dimension-ordered" in N.lib().dg_last_error().decode()
    plain = run(q, None)
    assert plain[0] == 0 and plain[1].tolist() == [300, 300]
    ranked = run(q, [ratio])
    assert ranked[0] == 0 and ranked[1].tolist() == [300, 300]
    assert sorted(ranked[2][:300].tolist()) == sorted(plain[2][:300].tolist()) and ranked[2].tolist() != plain[2].tolist()
