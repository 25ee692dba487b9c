"""The host side of dg_result_post_process (CPU): the order key of an aggregator's comparator, the closed
key interval of every greaterThan / lessThan / equalTo leaf, and the postfix program of a having tree.

The interval builder is held to the comparator itself: for every leaf kind, aggregator output type and
value kind, membership of post_order_key(metric) in having_interval(...) must equal what _having_eval
(runners.py) and having_eval (the oracle's restatement of HavingSpecMetricComparator.java:36-80) say of
the metric, on the edge metrics where a bisection could be off by one. The program is held to
_having_eval by a small stack machine over rows."""
import importlib
import itertools
import math
import struct

import numpy as np
import pytest

MAX, MIN = (1 << 63) - 1, -(1 << 63)
NAN, INF = math.nan, math.inf


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


def _next(d, up):
    return float(np.nextafter(d, INF if up else -INF))


def _f32(x):
    return float(np.float32(x))


def _metrics(out_type, value, special):
    """Edge metrics of an output type around `value`."""
    if out_type == "long":
        base = [0, 1, -1, MIN, MAX, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53) - 1, 10 ** 18]
        if value == value and not math.isinf(value):
            v = int(math.floor(value))
            base += [x for x in (v - 1, v, v + 1, v + 2) if MIN <= x <= MAX]
        return base
    base = [0.0, -0.0, 1.0, -1.0, float(MIN), float(MAX), 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, 1e300, -1e300,
            5e-324, -5e-324]
    if value == value and not math.isinf(value):
        v = float(value)
        base += [v, _next(v, True), _next(v, False)]
    if special:
        base += [INF, -INF, NAN]
    if out_type == "float":
        base = [_f32(x) for x in base if abs(x) < 3e38 or x != x or (special and math.isinf(x))]
        if special:
            base += [_f32(INF), _f32(-INF)]
    return base


VALUES = {"int": [0, 1, -1, 2, MAX, MIN, 2 ** 53, 2 ** 53 + 1, 10 ** 18],
          "float": [0.0, -0.0, 2.5, -2.5, 1.0, 2.0 ** 53, 9007199254740993.0, 1e300, -1e300, 0.1, _f32(0.1)],
          "special": [INF, -INF, NAN]}


# (a NaN or infinite value against a long metric is BigDecimal.valueOf's NumberFormatException: no such pair)
PAIRS = [(vk, ot) for vk in ("int", "float", "special") for ot in ("long", "double", "float")
         if (vk, ot) != ("special", "long")]


@pytest.mark.parametrize("value_kind,out_type", PAIRS)
@pytest.mark.parametrize("leaf", ["greaterThan", "lessThan", "equalTo"])
def test_interval_matches_the_comparator(Q, O, R, leaf, value_kind, out_type):
    for value in VALUES[value_kind]:
        lo, hi = R.having_interval(leaf, out_type, value)
        assert (lo, hi) == (1, 0) or 0 <= lo <= hi < 1 << 64
        h = Q.HavingSpec(leaf, aggregation="m", value=value)
        # +-inf and NaN metrics only against double values: against an integer the reference throws
        for m in _metrics(out_type, value, special=value_kind != "int"):
            row = Q.Row(0, {"m": m})
            want = R._having_eval(h, row)
            assert want == O.having_eval(h, row), (leaf, value, m)
            key = R.post_order_key(m, out_type)
            assert (lo <= key <= hi) == want, (leaf, out_type, value, m, hex(lo), hex(hi), hex(key))


def test_nan_and_infinite_metrics_against_an_integer_value(R):
    """The corner the ABI decides: -inf below every integer, +inf and NaN above."""
    for leaf, below, above in (("greaterThan", False, True), ("lessThan", True, False), ("equalTo", False, False)):
        lo, hi = R.having_interval(leaf, "double", 7)
        assert (lo <= R.post_order_key(-INF, "double") <= hi) == below
        for m in (INF, NAN):
            assert (lo <= R.post_order_key(m, "double") <= hi) == above


def test_order_key_is_the_aggregator_comparator(Q, O, R):
    longs = [0, 1, -1, MIN, MAX, 2 ** 53 + 1, -(2 ** 53) - 1]
    doubles = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300, INF, -INF, NAN, 2.0 ** 53 + 2,
               struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]]  # a NaN with its sign bit set
    for agg, vals in ((Q.long_sum("m"), longs), (Q.double_sum("m"), doubles), (Q.float_sum("m"), [_f32(x) for x in doubles if abs(x) < 3e38 or x != x or math.isinf(x)])):
        ot = agg.output_type
        for a, b in itertools.product(vals, vals):
            ka, kb = R.post_order_key(a, ot), R.post_order_key(b, ot)
            assert 0 <= ka < 1 << 64
            assert (ka > kb) - (ka < kb) == O._metric_compare(agg, a, b), (ot, a, b)
            ca, cb = agg.compare_key(a), agg.compare_key(b)
            assert (ka > kb) - (ka < kb) == (ca > cb) - (ca < cb), (ot, a, b)
        for v in vals:  # the inverse used by the bisection
            back = R.post_key_metric(R.post_order_key(v, ot), ot)
            assert back == v or (back != back and v != v)
    k = R.post_order_key
    assert k(NAN, "double") == (1 << 64) - 1 > k(INF, "double") > k(1e300, "double")
    assert k(-0.0, "double") + 1 == k(0.0, "double")
    for f in (0.1, -3.5, 1e-40, 3e38):
        assert k(_f32(f), "float") == k(float(np.float32(f)), "double")  # a float32 widens exactly


def _machine(N, ops, row_ids, row_keys):
    """dg_result_post_process's having program over one group: ids per dimension, order key per aggregator."""
    st = []
    for op, arg, lo, hi in ops:
        if op in (N.HAVING_ALWAYS, N.HAVING_NEVER):
            st.append(op == N.HAVING_ALWAYS)
        elif op in (N.HAVING_AND, N.HAVING_OR):
            assert 0 <= arg <= len(st)
            xs = [st.pop() for _ in range(arg)]
            st.append(all(xs) if op == N.HAVING_AND else any(xs))
        elif op == N.HAVING_NOT:
            st.append(not st.pop())
        elif op == N.HAVING_AGG_RANGE:
            st.append(lo <= row_keys[arg] <= hi)
        else:
            assert op == N.HAVING_DIM_EQ
            st.append(row_ids[arg] == lo)
    assert len(st) == 1
    return st[0]


def _query(Q, having):
    return Q.GroupByQuery(intervals=[(0, 1)], dimensions=["a", "b"],
                          aggregations=[Q.count("rows"), Q.double_sum("ds"), Q.float_sum("fs")], having=having)


DICTS = [[None, "x", "y"], ["p", "q"]]


def _check_program(Q, R, N, having):
    q = _query(Q, having)
    ops = R.having_program(q, lambda d: DICTS[d])
    assert ops is not None and len(ops) <= N.HAVING_MAX_OPS
    for ia, ib, rows, ds in itertools.product(range(3), range(2), (0, 1, 2, 3), (-0.0, 0.0, 2.5, NAN)):
        fs = _f32(ds)
        row = Q.Row(0, {"a": DICTS[0][ia], "b": DICTS[1][ib], "rows": rows, "ds": ds, "fs": fs})
        keys = [R.post_order_key(rows, "long"), R.post_order_key(ds, "double"), R.post_order_key(fs, "float")]
        assert _machine(N, ops, [ia, ib], keys) == R._having_eval(q.having, row), (having, row)
    return ops


def test_program_shapes(Q, R, N):
    gt = {"type": "greaterThan", "aggregation": "rows", "value": 1}
    lt = {"type": "lessThan", "aggregation": "ds", "value": 2.5}
    eq = {"type": "equalTo", "aggregation": "fs", "value": 0.0}
    sel = {"type": "dimSelector", "dimension": "a", "value": "x"}
    for h in (gt, lt, eq, sel, {"type": "always"}, {"type": "never"},
              {"type": "and", "havingSpecs": [gt, {"type": "not", "havingSpec": sel}]},
              {"type": "or", "havingSpecs": [sel, eq, {"type": "and", "havingSpecs": [gt, lt, {"type": "not", "havingSpec": eq}]}]},
              {"type": "not", "havingSpec": {"type": "or", "havingSpecs": [gt, {"type": "not", "havingSpec": lt}]}},
              {"type": "and", "havingSpecs": []}, {"type": "or", "havingSpecs": []}):
        _check_program(Q, R, N, h)
    # postfix: operands first, then the operator with its operand count
    ops = _check_program(Q, R, N, {"type": "and", "havingSpecs": [gt, {"type": "not", "havingSpec": sel}]})
    assert [o[0] for o in ops] == [N.HAVING_AGG_RANGE, N.HAVING_DIM_EQ, N.HAVING_NOT, N.HAVING_AND]
    assert ops[-1][1] == 2 and ops[0][1] == 0 and ops[1][1:3] == (0, 1)


def test_unknown_aggregator_folds_to_a_constant(Q, R, N):
    # metric None compares as 0.0 (HavingSpecMetricComparator :40-43)
    for h, want in (({"type": "greaterThan", "aggregation": "nope", "value": -1}, N.HAVING_ALWAYS),
                    ({"type": "greaterThan", "aggregation": "nope", "value": 1}, N.HAVING_NEVER),
                    ({"type": "lessThan", "aggregation": "nope", "value": 0.5}, N.HAVING_ALWAYS),
                    ({"type": "equalTo", "aggregation": "nope", "value": 0.0}, N.HAVING_ALWAYS),
                    ({"type": "equalTo", "aggregation": "nope", "value": -0.0}, N.HAVING_NEVER),
                    ({"type": "equalTo", "aggregation": "nope", "value": None}, N.HAVING_ALWAYS),
                    ({"type": "equalTo", "aggregation": "rows", "value": None}, N.HAVING_NEVER),
                    ({"type": "greaterThan", "aggregation": "rows", "value": None}, N.HAVING_NEVER)):
        ops = _check_program(Q, R, N, h)
        assert [o[0] for o in ops] == [want], h


def test_dim_selector_lookup(Q, R, N):
    for value in (None, ""):  # emptyToNull on both sides: the null id
        ops = _check_program(Q, R, N, {"type": "dimSelector", "dimension": "a", "value": value})
        assert ops == [(N.HAVING_DIM_EQ, 0, 0, 0)]
    ops = _check_program(Q, R, N, {"type": "dimSelector", "dimension": "b", "value": "q"})
    assert ops == [(N.HAVING_DIM_EQ, 1, 1, 0)]
    for dim, value in (("a", "absent"), ("b", None), ("b", "")):  # no such value in the dictionary: never
        ops = _check_program(Q, R, N, {"type": "dimSelector", "dimension": dim, "value": value})
        assert ops == [(N.HAVING_OR, 0, 0, 0)]
    # a selector on a name that is no dimension sees null
    assert [o[0] for o in _check_program(Q, R, N, {"type": "dimSelector", "dimension": "zz", "value": ""})] == [N.HAVING_ALWAYS]
    assert [o[0] for o in _check_program(Q, R, N, {"type": "dimSelector", "dimension": "zz", "value": "v"})] == [N.HAVING_NEVER]


def test_inexpressible_specs(Q, R, N):
    dictionary = lambda d: DICTS[d]
    ql = Q.GroupByQuery(intervals=[(0, 1)], dimensions=["a", {"type": "default", "dimension": "b", "outputType": "LONG"}],
                        aggregations=[Q.count("rows")], having={"type": "dimSelector", "dimension": "b", "value": "1"})
    assert R.having_program(ql, dictionary) is None  # a LONG-output dimension: refused by the host path
    assert R.having_program(_query(Q, {"type": "greaterThan", "aggregation": "a", "value": 1}), dictionary) is None
    assert R.having_program(_query(Q, {"type": "greaterThan", "aggregation": "rows", "value": "1"}), dictionary) is None
    deep = {"type": "greaterThan", "aggregation": "rows", "value": 1}
    too_long = {"type": "and", "havingSpecs": [deep] * N.HAVING_MAX_OPS}
    assert R.having_program(_query(Q, too_long), dictionary) is None
    too_deep = {"type": "or", "havingSpecs": [{"type": "and", "havingSpecs": [deep] * 20}, {"type": "and", "havingSpecs": [deep] * 20}]}
    assert len(R.having_program(_query(Q, too_deep), dictionary)) == 43  # 20 + 1 + 20 + 1 + 1: inside both bounds
    assert R.having_program(_query(Q, {"type": "and", "havingSpecs": [deep] * 33}), dictionary) is None  # 33 operands alive


def test_struct_layouts(N):
    import ctypes
    assert ctypes.sizeof(N.dg_having_op) == 24
    assert ctypes.sizeof(N.dg_post_column) == 24
    assert ctypes.sizeof(N.dg_post_process) == 40
    assert ctypes.sizeof(N.dg_post_info) == 40
