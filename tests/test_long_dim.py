"""CPU suite of the long-dimension groupBy: dimension-spec parsing, the host orders of a long dimension
(numeric for output type LONG, Java String order of the decimal text for STRING), the host merge of
partials, what the host layer refuses, and the new kernels in the gfx950 code object."""
import ctypes
import importlib

import numpy as np
import pytest

IV = [(0, 1 << 40)]


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


@pytest.fixture(scope="module")
def ORD():
    return importlib.import_module("incubator-druid_amd.ordering")


def test_dimension_specs_and_json_round_trip(Q):
    q = Q.GroupByQuery(intervals=IV, aggregations=[Q.count("rows")],
                       dimensions=["a", {"type": "default", "dimension": "v", "outputType": "LONG"},
                                   {"type": "default", "dimension": "w", "outputName": "w"},
                                   {"dimension": "z", "outputType": "string"}])
    assert q.dimensions == ["a", "v", "w", "z"]  # the names, as ever
    assert q.dimensionTypes == ["STRING", "LONG", "STRING", "STRING"]
    assert q.dimension_type("v") == "LONG" and q.dimension_type("a") == "STRING" and q.dimension_type("rows") == "STRING"
    js = q.to_json()
    assert js["dimensions"][1] == {"type": "default", "dimension": "v", "outputName": "v", "outputType": "LONG"}
    back = Q.query_from_json(js)
    assert back.dimensions == q.dimensions and back.dimensionTypes == q.dimensionTypes and back == q
    assert Q.query_from_json(back.to_json()) == q
    # every output type STRING: the JSON keeps the plain names
    plain = Q.GroupByQuery(intervals=IV, dimensions=["a", "b"], aggregations=[Q.count("rows")])
    assert plain.dimensionTypes == ["STRING", "STRING"] and plain.to_json()["dimensions"] == ["a", "b"]
    assert Q.query_from_json(plain.to_json()).dimensionTypes == ["STRING", "STRING"]
    # a parallel list is accepted too
    q2 = Q.GroupByQuery(intervals=IV, dimensions=["a", "v"], dimensionTypes=["string", "long"], aggregations=[])
    assert q2.dimensionTypes == ["STRING", "LONG"]
    js2 = dict(plain.to_json(), dimensionTypes=["LONG", "STRING"])
    assert Q.query_from_json(js2).dimensionTypes == ["LONG", "STRING"]
    with pytest.raises(ValueError):
        Q.GroupByQuery(intervals=IV, dimensions=[{"dimension": "v", "outputType": "COMPLEX"}], aggregations=[])
    with pytest.raises(ValueError):
        Q.GroupByQuery(intervals=IV, dimensions=["a", "v"], dimensionTypes=["LONG"], aggregations=[])
    with pytest.raises(ValueError):
        Q.GroupByQuery(intervals=IV, dimensions=[{"type": "extraction", "dimension": "v"}], aggregations=[])


VALUES = [0, 9, 10, -5, 100, -50, 99, -1, 1, -100, 5, 1000, -(1 << 63), (1 << 63) - 1, -9, 19, 2]


def test_decimal_text_order_against_numeric_order(ORD):
    as_long = sorted(VALUES, key=ORD.long_dimension_key("LONG"))
    as_text = sorted(VALUES, key=ORD.long_dimension_key("STRING"))
    assert as_long == sorted(VALUES)
    # String.compareTo over the decimal text: '-' before the digits, then digit by digit, a prefix first
    assert [str(v) for v in as_text] == [
        "-1", "-100", "-5", "-50", "-9", "-9223372036854775808", "0", "1", "10", "100", "1000", "19", "2", "5", "9",
        "9223372036854775807", "99"]
    assert as_text != as_long
    i = {v: k for k, v in enumerate(as_text)}
    assert i[-5] < i[10] < i[9]  # "-5" < "10" < "9"
    # compareDimsForLimitPushDown: NUMERIC compares the longs, another comparator String.valueOf of them
    assert sorted(VALUES, key=ORD.long_order_key("numeric")) == as_long
    assert sorted(VALUES, key=ORD.long_order_key("lexicographic")) == as_text
    by_len = sorted(VALUES, key=ORD.long_order_key("strlen"))
    assert [len(str(v)) for v in by_len] == sorted(len(str(v)) for v in VALUES)


def _partial(R, times, codes, dictionary, rows):
    return R.GroupByPartial(np.asarray(times, np.int64), None, [np.asarray(rows, np.int64)],
                            [np.asarray(codes, np.int32)], [dictionary])


def test_host_merge_orders_a_long_dimension_numerically(Q, R):
    aggs = [Q.count("rows")]
    q_long = Q.GroupByQuery(intervals=IV, dimensions=[{"dimension": "v", "outputType": "LONG"}], aggregations=aggs)
    a = _partial(R, [0, 0, 0], [0, 1, 2], [-5, 9, 10], [1, 2, 3])
    b = _partial(R, [0, 0, 0], [0, 1, 2], [-50, 10, 100], [10, 20, 30])
    t, dims, out = R.merge_groupby_columnar(q_long, [a, b])
    assert dims[0].tolist() == [-50, -5, 9, 10, 100] and out[0].tolist() == [10, 1, 2, 23, 30]
    rows = R.merge_groupby(q_long, [a, b])
    assert [r.event["v"] for r in rows] == [-50, -5, 9, 10, 100] and all(isinstance(r.event["v"], int) for r in rows)
    # the same column with output type STRING: the partials carry the decimal text, in its own order
    q_text = Q.GroupByQuery(intervals=IV, dimensions=["v"], aggregations=aggs)
    a = _partial(R, [0, 0, 0], [0, 1, 2], ["-5", "10", "9"], [1, 3, 2])
    b = _partial(R, [0, 0, 0], [0, 1, 2], ["-50", "10", "100"], [10, 20, 30])
    t, dims, out = R.merge_groupby_columnar(q_text, [a, b])
    assert dims[0].tolist() == ["-5", "-50", "10", "100", "9"] and out[0].tolist() == [1, 10, 23, 30, 2]
    # the push-down cut across partials (several devices) follows compareDimsForLimitPushDown
    for ordering, want in (("numeric", [100, 10]), ("lexicographic", [9, 100])):
        q = Q.GroupByQuery(intervals=IV, dimensions=[{"dimension": "v", "outputType": "LONG"}], aggregations=aggs,
                           limitSpec={"type": "default", "limit": 2,
                                      "columns": [{"dimension": "v", "direction": "descending", "dimensionOrder": ordering}]})
        a = _partial(R, [0, 0, 0], [0, 1, 2], [-5, 9, 10], [1, 2, 3])
        b = _partial(R, [0, 0, 0], [0, 1, 2], [-50, 10, 100], [10, 20, 30])
        t, dims, out = R.merge_groupby_columnar(q, [a, b])
        rows = [Q.Row(0, {"v": v, "rows": int(c)}) for v, c in zip(dims[0].tolist(), out[0].tolist())]
        assert [r.event["v"] for r in sorted(rows, key=R._push_down_key(q))[:2]] == want


def test_host_post_processing_over_a_long_dimension_is_refused(Q, R, N):
    aggs = [Q.count("rows")]
    dims = [{"dimension": "v", "outputType": "LONG"}, "a"]
    rows = [Q.Row(0, {"v": 1, "a": "x", "rows": 1}), Q.Row(0, {"v": 2, "a": "y", "rows": 2})]
    desc = {"type": "default", "limit": 1, "columns": [{"dimension": "v", "direction": "descending",
                                                         "dimensionOrder": "numeric"}]}
    with pytest.raises(N.UnsupportedQuery, match="v"):
        R.postprocess_groupby(Q.GroupByQuery(intervals=IV, dimensions=dims, aggregations=aggs, limitSpec=desc), rows)
    lex = {"type": "default", "columns": [{"dimension": "v", "direction": "ascending"}]}
    with pytest.raises(N.UnsupportedQuery, match="v"):  # LEXICOGRAPHIC is not a numeric dimension's natural order
        R.postprocess_groupby(Q.GroupByQuery(intervals=IV, dimensions=dims, aggregations=aggs, limitSpec=lex), rows)
    with pytest.raises(N.UnsupportedQuery, match="v"):
        R.postprocess_groupby(Q.GroupByQuery(intervals=IV, dimensions=dims, aggregations=aggs,
                                             having={"type": "dimSelector", "dimension": "v", "value": "1"}), rows)
    # nothing to sort or evaluate on the long dimension: the natural order, a plain limit, string columns
    nat = {"type": "default", "limit": 1, "columns": [{"dimension": "v", "direction": "ascending",
                                                        "dimensionOrder": "numeric"}]}
    q = Q.GroupByQuery(intervals=IV, dimensions=dims, aggregations=aggs, limitSpec=nat,
                       having={"type": "greaterThan", "aggregation": "rows", "value": 0})
    assert R.postprocess_groupby(q, rows) == rows[:1]
    by_agg = {"type": "default", "columns": [{"dimension": "rows", "direction": "descending"}]}
    q = Q.GroupByQuery(intervals=IV, dimensions=dims, aggregations=aggs, limitSpec=by_agg)
    assert R.postprocess_groupby(q, rows) == rows[::-1]


def test_abi_of_the_new_entry_points(N):
    assert ctypes.sizeof(N.dg_dimension) == 16 and N.dg_dimension.output_type.offset == 8
    for name in ("dg_groupby_run_dims", "dg_result_dim_type", "dg_result_dim_longs", "dg_debug_long_dim_info"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    assert N.lib().dg_abi_version() == 16
    # argument checks that need no device
    assert N.lib().dg_result_dim_longs(None, 0, None) == N.ERR_ARG
    assert N.lib().dg_debug_long_dim_info(None, b"v", None, None, None, None) == N.ERR_ARG


def test_long_dimension_kernels_are_in_the_gfx950_code_object(N):
    data = open(N.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    for k in (b"k_nd_minmax", b"k_nd_words", b"k_nd_unique_count", b"k_nd_scan", b"k_nd_unique_emit", b"k_nd_encode"):
        assert k in data, k
