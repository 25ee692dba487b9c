"""Numeric expressions through the device code: derived columns built by k_expr_eval, and the queries that read
them, against tests/expr_restate.py and the CPU oracle.

The fixture: the rows of querygen.columns(0) and columns(1) (24,577 and 9,001 rows: three full 8-byte blocks
plus a one-value block, one and a half float blocks; the last wave of either segment holds one live lane; v
holds both long extremes) in the three querygen.LAYOUTS (LZ4; LZ4 with `auto` longs, so DELTA / TABLE inputs;
NONE). The twin: the same rows written once more with, for every expression a query uses, an extra stored
metric holding the restatement's values, and for the dimension cases a string dimension String.valueOf(value).

Values: every expression of test_expr.VALUE_EXPRS is derived per layout and read back with dg_rows_run; the
words must equal the restatement's bit for bit.
Queries: the expectation is the oracle over the twin's stored column under tests/compare.py's rules; the
doubleSum over `x * l + 0.5` (multiples of 2^-3 below 2^20: test_expr.test_exact_sum_expression_is_exact) is
compared exactly; first / last, which the oracle does not know, against the engine over the twin's stored
column (exact)."""
import ctypes
import dataclasses
import importlib
import os

import numpy as np
import pytest

import compare
import expr_restate as ER
import querygen
import test_expr as TE

pytestmark = pytest.mark.gpu

IV = [querygen.CUT]
E_SUM = "x * l + 0.5"                        # DOUBLE, exact sums
E_LONG = "if(l % 7 != 0, l / (l % 7), 0)"    # LONG, guarded zero divisors
E_ROUND = "d * f / 3.0 - x"                  # DOUBLE, real rounding: min / max / first / last only
E_FILTER = "(l % 3 == 0) * (x - 0.5)"        # matches when (long) value > 0: x - 0.5 = 0.5 does not
E_VD = "d / 2.0"                             # a DOUBLE-typed virtual column under a numeric bound
E_VF = "d / 3.0"                             # a FLOAT-typed one: the bound sees (float) of the value
E_DIM = "l / 100"                            # a LONG dimension of 101 values
TWINS = {"t_sum": (E_SUM, "DOUBLE"), "t_long": (E_LONG, "LONG"), "t_round": (E_ROUND, "DOUBLE"),
         "t_filter": (E_FILTER, "LONG"), "t_vd": (E_VD, "DOUBLE"), "t_vf": (E_VF, "FLOAT"), "t_dim": (E_DIM, "LONG")}
_KIND = {"LONG": ("long", np.int64), "DOUBLE": ("double", np.float64), "FLOAT": ("float", np.float32)}
_WORD = {"LONG": np.int64, "DOUBLE": np.float64}


def _typed(words, out_type):
    if out_type == "FLOAT":
        return words.astype(np.uint32).view(np.float32)
    return words.view(_WORD[out_type])


@pytest.fixture(scope="module")
def mods():
    m = {k: importlib.import_module("incubator-druid_amd." + v)
         for k, v in (("R", "runners"), ("S", "segment"), ("N", "_native"), ("V", "virtual"))}
    return type("M", (), m)


@pytest.fixture(scope="module")
def restated(Q):
    """(expression, output type, segment) -> the restatement's words, computed once."""
    memo = {}

    def get(text, out_type, i):
        key = (text, out_type, i)
        if key not in memo:
            memo[key] = TE.fixture_values(Q, text, out_type, querygen.columns(i))
            memo[key].setflags(write=False)
        return memo[key]
    return get


@pytest.fixture(scope="module")
def data(Q, W, O, mods, restated, tmp_path_factory):
    """gpu[k]: the fixture's two segments in layout k; twin_gpu / twin_oracle: the twin (LZ4)."""
    base = tmp_path_factory.mktemp("expr_gpu")
    out = {"gpu": {k: [mods.S.GpuSegment(p) for p in querygen.layout_paths(k)] for k in range(len(querygen.LAYOUTS))}}
    paths = []
    for i in range(len(querygen.ROWS)):
        c = querygen.columns(i)
        spec = querygen._spec(W, c)
        for name, (text, out_type) in TWINS.items():
            kind, dtype = _KIND[out_type]
            spec.metrics[name] = (kind, np.ascontiguousarray(_typed(restated(text, out_type, i), out_type), dtype=dtype))
        dim = _typed(restated(E_DIM, "LONG", i), "LONG")
        spec.dims["t_dim_s"] = W.encode_strings([str(int(v)) for v in dim])
        paths.append(W.write_segment(str(base / ("twin%d" % i)), spec, lz4_mode="fast"))
    out["twin_gpu"] = [mods.S.GpuSegment(p) for p in paths]
    out["twin_oracle"] = [O.OracleSegment(p) for p in paths]
    return out


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
def _derive(mods, Q, seg, text, out_type, **kw):
    prog = mods.V.compile_for_segments(Q.parse_expression(text), out_type, [seg])
    name = prog.digest()
    return name, seg.derive(name, prog.ops, prog.inputs, {"LONG": 1, "FLOAT": 2, "DOUBLE": 3}[out_type], **kw)


def _read_column(mods, Q, seg, name):
    q = Q.ScanQuery(intervals=[querygen.WHOLE], columns=[name])
    rs = mods.R.scan_rows([seg], [name], q, None)
    try:
        vals, _ = rs.fetch(0, 0)
        return vals
    finally:
        rs.close()


@pytest.mark.parametrize("layout", range(len(querygen.LAYOUTS)))
def test_derived_values_match_restatement(Q, mods, data, restated, layout):
    for i, seg in enumerate(data["gpu"][layout]):
        before = seg.device_bytes()
        for text, out_type in TE.VALUE_EXPRS:
            name, info = _derive(mods, Q, seg, text, out_type)
            assert info["built"] == 1 and info["poisoned_rows"] == 0 and info["rows"] == seg.num_rows, text
            width = 4 if out_type == "FLOAT" else 8
            assert info["device_bytes"] >= seg.num_rows * width and seg.device_bytes() == before + info["device_bytes"]
            assert seg.column_type(name) == {"LONG": 1, "FLOAT": 2, "DOUBLE": 3}[out_type]
            got = _read_column(mods, Q, seg, name)
            exp = restated(text, out_type, i)
            bits = got.view(np.uint32).astype(np.uint64) if out_type == "FLOAT" else got.view(np.uint64)
            bad = np.nonzero(bits != exp)[0]
            assert len(bad) == 0, (text, layout, i, int(bad[0]), hex(int(bits[bad[0]])), hex(int(exp[bad[0]])))
            assert name not in seg.columns()  # a derived column is found by name, not listed among the stored ones
            seg.drop_derived(name)
            assert seg.device_bytes() == before


# ---------------------------------------------------------------------------------------------
# queries
# ---------------------------------------------------------------------------------------------
def _aggs(form):
    """The aggregators over expressions (form "expr"), over virtual columns (form "vc") or over the twin's
    stored columns (form "twin"): same names, same types."""
    src = {"sum": ("t_sum", E_SUM), "long": ("t_long", E_LONG), "round": ("t_round", E_ROUND)}

    def agg(typ, name, what):
        twin, text = src[what]
        if form == "expr":
            return {"type": typ, "name": name, "expression": text}
        return {"type": typ, "name": name, "fieldName": twin if form == "twin" else "vc_" + what}

    aggs = [{"type": "count", "name": "n"}, agg("longSum", "ls", "long"), agg("doubleSum", "ds", "sum"),
            agg("floatSum", "fs", "sum"), agg("longMin", "lmin", "long"), agg("longMax", "lmax", "long"),
            agg("doubleMin", "dmin", "round"), agg("doubleMax", "dmax", "round"), agg("floatMin", "fmin", "round"),
            agg("floatMax", "fmax", "round"), agg("longSum", "l2d", "sum"), agg("doubleSum", "d2l", "long")]
    flt = {"type": "bound", "dimension": "t_filter", "lower": "0", "lowerStrict": True, "ordering": "numeric"} \
        if form == "twin" else {"type": "expression", "expression": E_FILTER}
    aggs.append({"type": "filtered", "filter": flt, "aggregator": agg("longSum", "fls", "long")})
    return aggs


def _virtual(form, extra=()):
    vcs = list(extra)
    if form == "vc":
        vcs += [{"type": "expression", "name": "vc_sum", "expression": E_SUM, "outputType": "DOUBLE"},
                {"type": "expression", "name": "vc_long", "expression": E_LONG, "outputType": "LONG"},
                # (an aggregator reads the expression's own type, whatever the virtual column's outputType says)
                {"type": "expression", "name": "vc_round", "expression": E_ROUND, "outputType": "LONG"}]
    return vcs


def _query_filter(form):
    """A query-level expression filter AND numeric bounds on a DOUBLE- and on a FLOAT-typed virtual column."""
    if form == "twin":
        names = ("t_filter", "t_vd", "t_vf")
        first = {"type": "bound", "dimension": "t_filter", "lower": "0", "lowerStrict": True, "ordering": "numeric"}
    else:
        names = (None, "vd", "vf")
        first = {"type": "expression", "expression": "(" + E_FILTER + ") + 0"}  # (a second derived column)
    return {"type": "or", "fields": [
        first,
        {"type": "and", "fields": [
            {"type": "bound", "dimension": names[1], "lower": "-200.5", "upper": "450.25", "ordering": "numeric"},
            {"type": "not", "field": {"type": "bound", "dimension": names[2], "lower": "-50.25", "upper": "100",
                                      "upperStrict": True, "ordering": "numeric"}}]}]}


FILTER_VCS = ({"type": "expression", "name": "vd", "expression": E_VD, "outputType": "DOUBLE"},
              {"type": "expression", "name": "vf", "expression": E_VF, "outputType": "FLOAT"})


def _query(Q, kind, form, filtered=False, dim_type=None):
    js = {"dataSource": "ds", "intervals": ["%s/%s" % tuple(Q.format_time(t) for t in querygen.CUT)],
          "aggregations": _aggs(form)}
    vcs = _virtual(form, FILTER_VCS if filtered and form != "twin" else ())
    if filtered:
        js["filter"] = _query_filter(form)
    if kind == "ts":
        js.update(queryType="timeseries", granularity="hour")
    elif kind == "tn":
        js.update(queryType="topN", granularity="all", dimension="lo", metric="ds", threshold=4)
    else:
        js.update(queryType="groupBy", granularity="all", dimensions=["lo", "hn"])
    if dim_type is not None:  # the dimension over the LONG virtual column `bucket` (the twin: its string twin)
        name = "t_dim_s" if form == "twin" else "bucket"
        if form != "twin":
            vcs.append({"type": "expression", "name": "bucket", "expression": E_DIM, "outputType": "LONG"})
        spec = {"type": "default", "dimension": name, "outputName": name,
                "outputType": "STRING" if form == "twin" else dim_type}
        if kind == "tn":
            js.update(dimension=spec, threshold=200)
        else:
            js.update(dimensions=["lo", spec])
    if vcs:
        js["virtualColumns"] = vcs
    return Q.query_from_json(js)


_EXPECTED = {}


def _expected(Q, O, data, kind, filtered, dim=False):
    key = (kind, filtered, dim)
    if key not in _EXPECTED:
        _EXPECTED[key] = O.run(_query(Q, kind, "twin", filtered, "STRING" if dim else None), data["twin_oracle"])
    return _EXPECTED[key]


def _assert_same(q, got, exp):
    compare.assert_results(q, got, exp)
    # the sums over x * l + 0.5 do not depend on the order: exact (and the long sum of its D2L)
    for g, e in zip(got, exp):
        gv, ev = (g.event, e.event) if hasattr(g, "event") else (g.value, e.value)
        for a, b in zip(gv if isinstance(gv, list) else [gv], ev if isinstance(ev, list) else [ev]):
            assert a["ds"] == b["ds"] and a["l2d"] == b["l2d"] and a["d2l"] == b["d2l"], (a, b)


@pytest.mark.parametrize("filtered", (False, True), ids=("plain", "filtered"))
@pytest.mark.parametrize("form", ("expr", "vc"))
@pytest.mark.parametrize("kind", ("ts", "tn", "gb"))
@pytest.mark.parametrize("layout", range(len(querygen.LAYOUTS)))
def test_queries_match_oracle_over_twin(Q, O, mods, data, layout, kind, form, filtered):
    q = _query(Q, kind, form, filtered)
    exp = _expected(Q, O, data, kind, filtered)
    assert len(exp) > 0
    stats = mods.R.RunStats()
    got = mods.R.run_query(q, data["gpu"][layout], stats)
    _assert_same(q, got, exp)
    assert stats.derived_built + stats.derived_reused >= 2 * 3  # (sum, long, round at the least, on two segments)


@pytest.mark.parametrize("layout", range(len(querygen.LAYOUTS)))
def test_first_last_over_virtual_column(Q, mods, data, layout):
    """The oracle does not know first / last: the engine over the derived column against the engine over the
    twin's stored column, pairs and all."""
    def q(field, vcs):
        return Q.TimeseriesQuery(intervals=IV, granularity="hour", virtualColumns=vcs, aggregations=[
            Q.double_first("df", field), Q.double_last("dl", field), Q.long_first("lf", field), Q.float_last("fl", field)])
    vcs = [{"type": "expression", "name": "r", "expression": E_ROUND, "outputType": "DOUBLE"}]
    got = mods.R.run_query(q("r", vcs), data["gpu"][layout])
    exp = mods.R.run_query(q("t_round", []), data["twin_gpu"])
    assert len(got) == len(exp) > 24 and got == exp


@pytest.mark.parametrize("kind", ("tn", "gb"))
@pytest.mark.parametrize("layout", range(len(querygen.LAYOUTS)))
def test_first_last_pairs_in_topn_and_groupby(Q, mods, data, layout, kind):
    """The topN pair path and the groupBy's k_fl_keys / k_fl_resolve gather (two segments, row_base) over a derived
    column: exact against the same query over the twin's stored t_round. The pairs sit beside a sum, and in the
    topN a first/last value ranks the result."""
    def q(field, vcs):
        aggs = [Q.double_first("df", field), Q.long_last("ll", field), Q.double_last("dl", field),
                Q.float_first("ff", field), Q.count("n"), Q.double_max("dm", field)]
        if kind == "tn":
            return Q.TopNQuery(intervals=IV, granularity="all", dimension="mid", metric="dl", threshold=25,
                               aggregations=aggs, virtualColumns=vcs)
        return Q.GroupByQuery(intervals=IV, granularity="hour", dimensions=["lo", "hn"], aggregations=aggs, virtualColumns=vcs)
    vcs = [{"type": "expression", "name": "r", "expression": E_ROUND, "outputType": "DOUBLE"}]
    got = mods.R.run_query(q("r", vcs), data["gpu"][layout])
    exp = mods.R.run_query(q("t_round", []), data["twin_gpu"])
    if kind == "tn":
        assert len(exp) == 1 and len(exp[0].value) == 25
    else:
        assert len(exp) > 2000
    assert got == exp


def _as_int_rows(Q, rows, name):
    out = [Q.Row(r.timestamp, {("bucket" if k == name else k): (int(v) if k == name else v) for k, v in r.event.items()})
           for r in rows]
    return sorted(out, key=lambda r: (r.timestamp, querygen._jkey(r.event["lo"]), r.event["bucket"]))


@pytest.mark.parametrize("dim_type", ("STRING", "LONG"))
@pytest.mark.parametrize("layout", (0, 2))
def test_groupby_dimension_over_virtual_column(Q, O, mods, data, layout, dim_type):
    q = _query(Q, "gb", "expr", False, dim_type)
    exp = _expected(Q, O, data, "gb", False, True)
    got = mods.R.run_query(q, data["gpu"][layout])
    if dim_type == "LONG":  # re-sorted as integers, the twin rule for v
        exp = _as_int_rows(Q, exp, "t_dim_s")
    else:
        exp = [Q.Row(r.timestamp, {("bucket" if k == "t_dim_s" else k): v for k, v in r.event.items()}) for r in exp]
    assert len(exp) > 400
    _assert_same(q, got, exp)


@pytest.mark.parametrize("dim_type", ("STRING", "LONG"))
@pytest.mark.parametrize("layout", (1,))
def test_topn_dimension_over_virtual_column(Q, O, mods, data, layout, dim_type):
    q = _query(Q, "tn", "vc", False, dim_type)
    exp = _expected(Q, O, data, "tn", False, True)
    got = mods.R.run_query(q, data["gpu"][layout])
    conv = int if dim_type == "LONG" else str
    exp = [Q.Result(r.timestamp, [{("bucket" if k == "t_dim_s" else k): (conv(v) if k == "t_dim_s" else v)
                                   for k, v in e.items()} for e in r.value]) for r in exp]
    assert len(exp) == 1 and len(exp[0].value) == 101  # every value of l / 100: the threshold cuts nothing
    _assert_same(q, got, exp)


# ---------------------------------------------------------------------------------------------
# refusals and lifecycle
# ---------------------------------------------------------------------------------------------
def test_division_by_zero_is_refused_and_leaves_nothing(Q, mods, data):
    seg = data["gpu"][0][0]
    seg.drop_derived()
    before = seg.device_bytes()
    q = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "longSum", "name": "s", "expression": "l / (l % 7)"}])
    zero = int(np.count_nonzero(querygen.columns(0)["l"] % 7 == 0))
    with pytest.raises(mods.N.UnsupportedQuery, match="division by zero in %d rows" % zero):
        mods.R.run_query(q, [seg])
    assert seg.derived_columns() == [] and seg.device_bytes() == before
    # the guarded form of the same division is answered
    ok = dataclasses.replace(q, aggregations=[{"type": "longSum", "name": "s", "expression": E_LONG}])
    assert len(mods.R.run_query(ok, [seg])) == 1
    seg.drop_derived()
    assert seg.device_bytes() == before


def test_string_missing_and_colliding_inputs_are_refused(Q, mods, data):
    seg = data["gpu"][0][0]
    for text, msg in (("lo + 1", "column lo is not numeric"), ("nope * 2", "no column nope"), ("tags + 1", "not numeric")):
        q = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "doubleSum", "name": "s", "expression": text}])
        with pytest.raises(mods.N.UnsupportedQuery, match=msg):
            mods.R.run_query(q, [seg])
    # the C-ABI's own refusals, before any launch
    L = mods.N.lib()
    ops = [(Q.EX_INPUT, 0, 0)]

    def rc(name, ops, inputs, out_type):
        e, keep = mods.N.make_expr(ops, inputs, out_type)
        return L.dg_segment_derive_column(seg.handle, name.encode(), ctypes.byref(e), None, 0, None)

    before = seg.device_bytes()
    assert rc("zz", ops, ["lo"], 1) == 2 and rc("zz", ops, ["nope"], 1) == 2 and rc("zz", ops, ["tags"], 1) == 2
    assert rc("l", ops, ["l"], 1) == mods.N.ERR_ARG                       # a stored column's name
    assert rc("__time", ops, ["l"], 1) == mods.N.ERR_ARG
    assert rc("zz", ops, ["l"], 3) == mods.N.ERR_ARG                      # a long is no DOUBLE output
    assert rc("zz", ops + [(Q.EX_ADD, 0, 0)], ["l"], 1) == mods.N.ERR_ARG  # stack underflow
    assert rc("zz", ops * 65, ["l"], 1) == mods.N.ERR_ARG
    assert rc("zz", ops, ["l"] * 9, 1) == mods.N.ERR_ARG
    assert rc("zz", ops, ["l"], 1) == 0 and rc("zz", ops, ["l"], 1) == 0  # built, then found
    assert rc("zz", [(Q.EX_INPUT, 0, 0), (Q.EX_NEG, 0, 0)], ["l"], 1) == mods.N.ERR_ARG  # another program, same name
    assert rc("yy", ops, ["zz"], 1) == mods.N.ERR_ARG                     # a derived column is no input
    assert L.dg_segment_drop_derived(seg.handle, b"zz") == 0
    assert L.dg_segment_drop_derived(seg.handle, b"zz") == 8              # DG_ERR_NOT_FOUND
    assert L.dg_segment_drop_derived(seg.handle, b"l") == mods.N.ERR_ARG
    assert seg.device_bytes() == before


def test_dimension_and_filter_uses_the_engine_refuses(Q, mods, data):
    segs = data["gpu"][0]
    aggs = [Q.count("n")]
    for out_type in ("DOUBLE", "FLOAT", "STRING"):
        vcs = [{"type": "expression", "name": "b", "expression": E_DIM, "outputType": out_type}]
        for q in (Q.GroupByQuery(intervals=IV, dimensions=["b"], aggregations=aggs, virtualColumns=vcs),
                  Q.TopNQuery(intervals=IV, dimension="b", metric="n", threshold=3, aggregations=aggs, virtualColumns=vcs)):
            with pytest.raises(mods.N.UnsupportedQuery, match="dimension over virtual column b of output type " + out_type):
                mods.R.run_query(q, segs)
    vcs = [{"type": "expression", "name": "b", "expression": E_DIM, "outputType": "STRING"}]
    q = Q.TimeseriesQuery(intervals=IV, aggregations=aggs, virtualColumns=vcs, filter=Q.SelectorDimFilter("b", "3"))
    with pytest.raises(mods.N.UnsupportedQuery, match="virtual column b of output type STRING"):
        mods.R.run_query(q, segs)
    q = dataclasses.replace(q, filter=Q.RegexDimFilter("b", "3.*"),
                            virtualColumns=[dict(vcs[0], outputType="LONG")])
    with pytest.raises(mods.N.UnsupportedQuery, match="filter RegexDimFilter on virtual column b"):
        mods.R.run_query(q, segs)
    # a selector on a LONG virtual column is answered: the rows whose bucket is 3
    q = dataclasses.replace(q, filter=Q.SelectorDimFilter("b", "3"))
    n = sum(int(np.count_nonzero((querygen.columns(i)["l"] >= 300) & (querygen.columns(i)["l"] < 400) &
                                 (querygen.columns(i)["t"] >= querygen.CUT[0]) & (querygen.columns(i)["t"] < querygen.CUT[1])))
            for i in range(2))
    assert mods.R.run_query(q, segs)[0].value["n"] == n > 100
    for s in segs:
        s.drop_derived()


def test_reuse_eviction_and_drop(Q, mods, data):
    seg = data["gpu"][2][1]
    seg.drop_derived()
    attached = seg.device_bytes()

    def run(k):
        stats = mods.R.RunStats()
        q = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "longSum", "name": "s", "expression": "l + %d" % k}])
        res = mods.R.run_query(q, [seg], stats)
        return res[0].value["s"], stats

    first, s1 = run(0)
    again, s2 = run(0)
    assert first == again and (s1.derived_built, s1.derived_reused) == (1, 0)
    assert (s2.derived_built, s2.derived_reused) == (0, 1) and s1.derived_build_ms > 0 and s2.derived_build_ms == 0
    oldest = seg.derived_columns()[0]
    for k in range(1, 8):
        run(k)
    assert len(seg.derived_columns()) == 8 and seg.derived_columns()[0] == oldest
    run(0)  # used again: the first expression is now the most recent
    assert seg.derived_columns()[-1] == oldest
    victim = seg.derived_columns()[0]
    full = seg.device_bytes()
    _, s9 = run(8)  # a ninth distinct expression evicts the least recently used
    assert s9.derived_built == 1 and len(seg.derived_columns()) == 8
    assert victim not in seg.derived_columns() and oldest in seg.derived_columns() and seg.device_bytes() == full
    # a query that needs more than the segment keeps is refused, not answered with some of its columns dropped
    q = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "longSum", "name": "s%d" % k, "expression": "l * %d" % (k + 2)}
                                                      for k in range(9)])
    with pytest.raises(mods.N.UnsupportedQuery, match="more than 8 derived columns"):
        mods.R.run_query(q, [seg])
    seg.drop_derived()
    assert seg.derived_columns() == [] and seg.device_bytes() == attached


def test_cancelled_build_leaves_nothing_and_the_next_query_is_exact(Q, O, mods, data):
    seg = data["gpu"][0][1]
    seg.drop_derived()
    before = seg.device_bytes()
    flag = ctypes.c_int32(1)  # set before the call
    q = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "longSum", "name": "s", "expression": E_LONG}])
    with pytest.raises(mods.N.QueryInterrupted):
        mods.R.timeseries_per_segment([seg], q, cancel=flag)
    assert seg.derived_columns() == [] and seg.device_bytes() == before
    got = mods.R.run_query(q, [seg])
    exp = O.run(Q.TimeseriesQuery(intervals=IV, aggregations=[Q.long_sum("s", "t_long")]), [data["twin_oracle"][1]])
    compare.assert_results(q, got, exp)
    seg.drop_derived()
