"""A seeded generator of timeseries / topN / groupBy queries over one small fixture, the CPU oracle's
expectation of each, and a comparison whose floating-sum tolerance is derived, not measured.

The fixture (fixture_specs): two segments over the same three days from 2018-03-10T00:00Z, 24,577 and 9,001
rows, on a one-second grid with duplicate instants; string dimensions lo / mid / hi / hn / tags / v_s, the
LONG columns v and l, the DOUBLE columns d / d_abs / x and the FLOAT columns f / f_abs (see the function).
Every column is built from integer draws only, so it is the same bit for bit wherever it is built: d and f
are a sum of twelve uniform draws scaled to a standard deviation of 1e3 (normal to the eye, mixed sign; no
transcendental function whose last bit could differ between two machines).

The queries (queries()): 48 timeseries, 48 topN, 64 groupBy, each drawn from its own
numpy.random.default_rng([SEED, kind, index, attempt]) with integer draws only. A draw whose floating sums
could steer the result differently within their error bound (topN metric, limit-spec column, having
operand; steering_violations), or whose result is empty without the empty interval or the filter that selects
nothing having been drawn, is drawn again with the next attempt number; thresholds of a having spec are
taken from the oracle's cells at generation time. A few indices are pinned to combinations the census of
tests/test_querygen.py asks for (PINS). axes() gives the axis values every query was drawn with.

The twin rule for the LONG column v: the oracle groups by string dimensions only, so a query over v is
answered by the oracle over v_s = String.valueOf(v) (oracle_query) and turned back (expected):
* groupBy, outputType STRING: the v_s rows with the dimension renamed;
* groupBy, outputType LONG: a limit that is pushed down orders every dimension as a string
  (GroupByQuery.compareDimsForLimitPushDown with a non-numeric comparator), so the rows are the v_s rows
  with ints; otherwise the v_s rows before the limit spec, re-sorted by (time, dimensions) with v compared
  as an integer (natural_resort), then the limit spec applied over that order;
* topN (numeric metrics only, outputType STRING): the v_s entries; where the engine reports values cut
  among metric ties (TopNRaw.cut_ties) and the oracle's full ranking has a tie across the cut, only the
  entries strictly better than the last one are compared and the others must come from the tied values.

The sum bound (cell_bound): a doubleSum over d (floatSum over f) comes with a count n and the same sum A
over d_abs (f_abs) under the same filter. Recursive summation in any order is within gamma(n-1) * sum|x| of
the exact sum, gamma(n) = n u / (1 - n u), u = 2^-53 (2^-24); A over-estimates sum|x| by at most the same
factor, so two correct sides differ by at most 2 gamma(n) A. Every other cell is exact: counts, long
aggregates, min / max (with the sign of zero), every sum over x (multiples of 0.125, |x| <= 8: exact in
float32 too) and over l, timestamps, dimension values and the row order.

The merge draw (merge_queries()): the queries the cross-segment, cross-device and cross-rank merges are held
to — every ts-* and tn-*, the gb-* that do not group by v, and MERGE_GB further groupBy draws gm-* from
default_rng([SEED, 3, index, attempt]) with v taken out of the dimension pool (no device-side merge takes a
LONG dimension), a few pinned (MERGE_PINS). They run over the same rows as four segments (piece_paths: each
fixture segment cut once at row n // 2, in layout 0), and their expectation is the oracle over those four
(expected_for(q, PIECES)): the steering and empty-result redraws of a gm-* draw are evaluated there.

Deviations from the plan this generator was written to, each forced by the engine's arithmetic:
* the key+reference sort words need key bits + row-reference bits > 64; with 33,578 rows (16 bits) and the
  fixture's cardinalities (hi 15 bits, mid 9, v 10, hn 6) an hourly bucket (7 bits) gives 63. The four
  pinned queries therefore bucket by the 140,000 ms duration (11 bits: 67);
* a topN with the 140,000 ms duration runs over a one-hour interval (FINE), not the three days: 1,852
  cursors of 1,000 entries each are hundreds of megabytes of result lists;
* floatSum is drawn over f and x, doubleSum over d, x and l: a floatSum over l or a doubleSum over f is
  neither exact nor has a twin to bound it;
* a floating sum over d or f is a topN metric only over dimensions of fewer than 1,000 values, where the
  per-segment threshold of 1,000 cuts nothing; alphanumeric topN is not drawn over hi (12,000 values
  through the restated Java comparator take seconds on the CPU).
"""
import atexit
import copy
import dataclasses
import importlib
import json
import math
import os
import shutil
import sys
import tempfile

import numpy as np

from compare import _close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEED = 20180311
T0 = 1_520_640_000_000  # 2018-03-10T00:00:00Z
DAY = 86_400_000
ROWS = (24_577, 9_001)
LAYOUTS = (("concise", "lz4", {}), ("roaring", "lz4", {"long_encoding": "auto"}), ("roaring", "none", {}))
N_TS, N_TN, N_GB = 48, 48, 64
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1

WHOLE = (T0 - DAY, T0 + 4 * DAY)
CUT = (T0 + 40_643_000, T0 + 2 * DAY + 78_011_000)  # inside the first and the last (full) block of both segments
EMPTY = (T0 + 5 * DAY, T0 + 6 * DAY)
FINE = (T0 + DAY + 1_234_000, T0 + DAY + 4_834_000)  # one hour: a topN under the 140 s duration
INTERVALS = {"whole": WHOLE, "cut": CUT, "empty": EMPTY}
GRANS = {"all": "all", "hour": "hour", "dur": {"type": "duration", "duration": 140_000},
         "p1d": {"type": "period", "period": "P1D", "timeZone": "America/Los_Angeles"},
         "pt1h": {"type": "period", "period": "PT1H", "timeZone": "America/Los_Angeles"}}
HI_POOL = ((0, 16_000), (15_000, 21_000))  # value ranges of hi per segment: about rows / 2 distinct each


def _mods():
    return (importlib.import_module("incubator-druid_amd.query"), importlib.import_module("incubator-druid_amd.writer"),
            importlib.import_module("oracle"))


# ---------------------------------------------------------------------------------------------
# fixture
# ---------------------------------------------------------------------------------------------
_COLUMNS = {}


def columns(i):
    """The rows of segment i as plain arrays / lists (the source of fixture_specs and of the generator's values)."""
    if i in _COLUMNS:
        return _COLUMNS[i]
    n = ROWS[i]
    rng = np.random.default_rng([SEED, 100 + i])
    t = T0 + np.sort(rng.integers(0, 3 * 86_400, n)).astype(np.int64) * 1000
    lo = rng.integers(0, 5, n)
    mid = rng.integers(0, 300, n)
    hi = rng.integers(HI_POOL[i][0], HI_POOL[i][1], n)
    hn = rng.integers(0, 100, n)  # >= 50: null
    ntags = rng.integers(0, 4, n)
    tagv = rng.integers(0, 12, (n, 3))
    v = rng.integers(-500, 501, n).astype(np.int64)
    edge = rng.integers(0, n, 10)
    v[edge[:5]] = LONG_MIN
    v[edge[5:]] = LONG_MAX
    l = rng.integers(-5000, 5001, n).astype(np.int64)
    # twelve uniform draws of 20 bits: mean 6, variance 1 in units of 2^20; every step below is exact or one
    # correctly rounded IEEE operation
    d = (rng.integers(0, 1 << 20, (n, 12)).sum(axis=1).astype(np.float64) / float(1 << 20) - 6.0) * 1e3
    f = ((rng.integers(0, 1 << 20, (n, 12)).sum(axis=1).astype(np.float64) / float(1 << 20) - 6.0) * 1e3).astype(np.float32)
    x = rng.integers(-64, 65, n).astype(np.float64) * 0.125
    c = {"t": t, "lo": ["lo%d" % k for k in lo], "mid": ["m%03d" % k for k in mid], "hi": ["h%05d" % k for k in hi],
         "hn": [None if k >= 50 else "n%02d" % k for k in hn],
         "tags": [["t%02d" % tagv[r, j] for j in range(ntags[r])] for r in range(n)],
         "v": v, "v_s": [str(int(k)) for k in v], "l": l, "d": d, "d_abs": np.abs(d), "f": f, "f_abs": np.abs(f), "x": x}
    _COLUMNS[i] = c
    return c


def _spec(W, c):
    """Rows given as columns()-style arrays / lists as a writer.SegmentSpec (nope is in none)."""
    dims = {k: W.encode_strings(c[k]) for k in ("lo", "mid", "hi", "hn", "v_s")}
    dims["tags"] = W.encode_multi_strings(c["tags"])
    metrics = {"v": ("long", c["v"]), "l": ("long", c["l"]), "d": ("double", c["d"]), "d_abs": ("double", c["d_abs"]),
               "f": ("float", c["f"]), "f_abs": ("float", c["f_abs"]), "x": ("double", c["x"])}
    return W.SegmentSpec(timestamps=c["t"], dims=dims, metrics=metrics)


def fixture_specs(W):
    """The two segments as writer.SegmentSpec (nope is in neither)."""
    return [_spec(W, columns(i)) for i in range(len(ROWS))]


PIECES = "pieces"  # the `layout` of the four-segment form of the fixture


def piece_specs(W):
    """The same rows as four segments: each fixture segment cut once at row n // 2 (the rows are time-sorted
    with duplicate instants, so a cut may part equal timestamps). Every piece has its own dictionaries."""
    out = []
    for i, n in enumerate(ROWS):
        c = columns(i)
        for a, b in ((0, n // 2), (n // 2, n)):
            out.append(_spec(W, {k: x[a:b] for k, x in c.items()}))
    return out


_STATE = {"base": None, "paths": {}, "oracle": {}}


def _write(name, specs, layout):
    _, W, _ = _mods()
    if _STATE["base"] is None:
        _STATE["base"] = tempfile.mkdtemp(prefix="querygen_")
        atexit.register(shutil.rmtree, _STATE["base"], ignore_errors=True)
    bitmap, comp, kw = LAYOUTS[layout]
    return [W.write_segment(os.path.join(_STATE["base"], "%s_s%d" % (name, i)), s, bitmap=bitmap, compression=comp,
                            lz4_mode="fast", **kw) for i, s in enumerate(specs(W))]


def layout_paths(k):
    """The segment directories of layout k (LAYOUTS), written at first use into a directory removed at exit."""
    if k not in _STATE["paths"]:
        _STATE["paths"][k] = _write("l%d" % k, fixture_specs, k)
    return _STATE["paths"][k]


def piece_paths():
    """The four pieces' directories, in layout 0 (the merges do not depend on the layout)."""
    if PIECES not in _STATE["paths"]:
        _STATE["paths"][PIECES] = _write("p", piece_specs, 0)
    return _STATE["paths"][PIECES]


def oracle_segments(k=0):
    if k not in _STATE["oracle"]:
        _, _, O = _mods()
        _STATE["oracle"][k] = [O.OracleSegment(p) for p in (piece_paths() if k == PIECES else layout_paths(k))]
    return _STATE["oracle"][k]


def piece_oracle_segments():
    return oracle_segments(PIECES)


# ---------------------------------------------------------------------------------------------
# the oracle side of a query, cached
# ---------------------------------------------------------------------------------------------
_RUNS = {}


def oracle_query(q):
    """q as the oracle can answer it: the LONG column v replaced by its string twin v_s."""
    Q, _, _ = _mods()
    if isinstance(q, Q.GroupByQuery) and "v" in q.dimensions:
        ls = q.limitSpec
        if ls is not None:
            ls = Q.DefaultLimitSpec([dataclasses.replace(c, dimension="v_s" if c.dimension == "v" else c.dimension)
                                     for c in ls.columns], ls.limit)
        return dataclasses.replace(q, dimensions=["v_s" if d == "v" else d for d in q.dimensions],
                                   dimensionTypes=["STRING"] * len(q.dimensions), limitSpec=ls)
    if isinstance(q, Q.TopNQuery) and q.dimension == "v":
        return dataclasses.replace(q, dimension="v_s", dimension_type="STRING")
    return q


def _oracle_run(q, layout=0):
    """oracle.run of q over layout `layout`, computed once; the caller must not change what it gets.
    While it runs, oracle.filter_mask remembers the mask of every (segment, filter): the oracle evaluates a
    filtered aggregator's filter once per cursor, which over 1,852 buckets of 140 s takes minutes."""
    _, _, O = _mods()
    key = (layout, json.dumps(q.to_json(), sort_keys=True))
    if key in _RUNS:
        return _RUNS[key]
    plain, memo = O.filter_mask, {}

    def remembered(seg, f):
        if f is None:
            return plain(seg, f)
        k = (id(seg), repr(f))
        if k not in memo:
            memo[k] = plain(seg, f)
            memo[k].setflags(write=False)
        return memo[k]

    O.filter_mask = remembered
    try:
        _RUNS[key] = O.run(q, oracle_segments(layout))
    finally:
        O.filter_mask = plain
    return _RUNS[key]


def _jkey(s):
    return (0, b"") if s is None else (1, s.encode("utf-16-be", "surrogatepass"))


def natural_resort(q, rows):
    """Rows of a groupBy over the LONG-output dimension v in the natural order of GroupByQuery.getRowOrdering:
    the time, then every dimension, strings in Java String order and v as an integer (with sortByDimsFirst
    and a granularity: the dimensions, then the time). Stable."""
    def dims(r):
        return tuple((1, int(r.event[d])) if d == "v" else _jkey(r.event[d]) for d in q.dimensions)

    if q._ctx_bool("sortByDimsFirst", False) and not q.granularity.is_all:
        return sorted(rows, key=lambda r: (dims(r), r.timestamp))
    return sorted(rows, key=lambda r: (r.timestamp, dims(r)))


def _rename_v(Q, rows, as_int):
    out = []
    for r in rows:
        ev = {("v" if k == "v_s" else k): (int(x) if as_int and k == "v_s" else x) for k, x in r.event.items()}
        out.append(Q.Row(r.timestamp, ev))
    return out


def expected_for(q, layout=0):
    """The expectation of q: the oracle's result, through the twin rule where q is over v. A fresh copy."""
    Q, _, O = _mods()
    oq = oracle_query(q)
    if isinstance(q, Q.GroupByQuery) and "v" in q.dimensions:
        as_int = q.dimension_type("v") == "LONG"
        if not as_int or O.o_limit_push_down(oq):
            return _rename_v(Q, _oracle_run(oq, layout), as_int)
        ctx = {k: x for k, x in oq.context.items() if k != "forceLimitPushDown"}
        rows = _rename_v(Q, _oracle_run(dataclasses.replace(oq, limitSpec=None, context=ctx), layout), True)
        return O.groupby_post_process(q, natural_resort(q, rows))
    res = copy.deepcopy(_oracle_run(oq, layout))
    if isinstance(q, Q.TopNQuery) and q.dimension == "v":
        for r in res:
            r.value = [{("v" if k == "v_s" else k): x for k, x in e.items()} for e in r.value]
    return res


# ---------------------------------------------------------------------------------------------
# the derived bound
# ---------------------------------------------------------------------------------------------
U = {"doubleSum": 2.0 ** -53, "floatSum": 2.0 ** -24}


def gamma(n, u):
    return n * u / (1.0 - n * u)


def is_bounded(agg):
    """A floating sum that is not exact: doubleSum over d / d_abs, floatSum over f / f_abs."""
    return (agg.type == "doubleSum" and agg.fieldName in ("d", "d_abs")) or \
           (agg.type == "floatSum" and agg.fieldName in ("f", "f_abs"))


def cell_bound(agg, cells):
    """2 gamma(n) A for a bounded aggregator's cell among the oracle's `cells` of its row (its count twin
    <name>_n and its absolute-value twin <name>_abs; the latter bounds itself), 0.0 for every other cell."""
    if not is_bounded(agg):
        return 0.0
    base = agg.name[:-4] if agg.name.endswith("_abs") else agg.name
    n, a = cells[base + "_n"], cells[base + "_abs"]
    return 2.0 * gamma(n, U[agg.type]) * abs(a) if n else 0.0


# ---------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _dim_value(rng, dim):
    seg = int(rng.integers(0, 2))
    c = columns(seg)
    r = int(rng.integers(0, ROWS[seg]))
    if dim == "tags":
        return "t%02d" % int(rng.integers(0, 12))
    v = c[dim][r]
    return v if v is not None else "n07"


LEAF_KINDS = ("selector", "selector-null", "selector-missing", "in", "bound-lex", "bound-num", "bound-alnum",
              "bound-strlen", "regex", "like", "search", "num-l-bound", "num-l-selector", "num-d-bound", "num-d-selector")
NUMERIC_LEAVES = ("num-l-bound", "num-l-selector", "num-d-bound", "num-d-selector")


def _leaf(rng, tags, kinds=LEAF_KINDS):
    k = _pick(rng, kinds)
    tags.add("f:" + k)
    if k == "selector":
        dim = _pick(rng, ("lo", "mid", "hi", "hn", "tags"))
        return {"type": "selector", "dimension": dim, "value": _dim_value(rng, dim)}
    if k == "selector-null":
        return {"type": "selector", "dimension": "hn", "value": None}
    if k == "selector-missing":
        return {"type": "selector", "dimension": "nope", "value": None}
    if k == "in":
        dim = _pick(rng, ("mid", "tags", "hn"))
        vals = [_dim_value(rng, dim) for _ in range(int(rng.integers(2, 9)))]
        if dim == "hn":
            vals.append(None)
        return {"type": "in", "dimension": dim, "values": vals}
    if k == "bound-lex":
        a, b = sorted(int(x) for x in rng.integers(0, 300, 2))
        return {"type": "bound", "dimension": "mid", "lower": "m%03d" % a, "upper": "m%03d" % (b + 20),
                "lowerStrict": bool(rng.integers(0, 2)), "upperStrict": bool(rng.integers(0, 2)), "ordering": "lexicographic"}
    if k == "bound-num":
        a, b = sorted(int(x) for x in rng.integers(-500, 501, 2))
        return {"type": "bound", "dimension": "v_s", "lower": str(a), "upper": str(b + 100),
                "lowerStrict": bool(rng.integers(0, 2)), "upperStrict": False, "ordering": "numeric"}
    if k == "bound-alnum":
        a = int(rng.integers(0, 12_000))
        return {"type": "bound", "dimension": "hi", "lower": "h%05d" % a, "upper": "h%05d" % (a + 6_000),
                "lowerStrict": False, "upperStrict": True, "ordering": "alphanumeric"}
    if k == "bound-strlen":
        return {"type": "bound", "dimension": "v_s", "lower": _pick(rng, ("00", "-9", "5")), "upper": _pick(rng, ("999", "-99")),
                "lowerStrict": False, "upperStrict": False, "ordering": "strlen"}
    if k == "regex":
        return _pick(rng, ({"type": "regex", "dimension": "mid", "pattern": "^m1[0-4]"},
                           {"type": "regex", "dimension": "hi", "pattern": "[37]$"},
                           {"type": "regex", "dimension": "tags", "pattern": "t0[1-5]"}))
    if k == "like":
        return _pick(rng, ({"type": "like", "dimension": "hi", "pattern": "h0%3"},
                           {"type": "like", "dimension": "mid", "pattern": "m_5%"},
                           {"type": "like", "dimension": "hn", "pattern": "n1_"}))
    if k == "search":
        return _pick(rng, ({"type": "search", "dimension": "tags", "query": {"type": "contains", "value": "1", "caseSensitive": True}},
                           {"type": "search", "dimension": "mid", "query": {"type": "insensitive_contains", "value": "M2"}},
                           {"type": "search", "dimension": "lo", "query": {"type": "contains", "value": "O3", "caseSensitive": False}}))
    if k == "num-l-bound":
        a, b = sorted(int(x) for x in rng.integers(-5000, 5001, 2))
        return {"type": "bound", "dimension": "l", "lower": str(a), "upper": str(b + 500), "lowerStrict": bool(rng.integers(0, 2)),
                "upperStrict": bool(rng.integers(0, 2)), "ordering": "numeric"}
    if k == "num-l-selector":
        vals = [str(int(x)) for x in rng.integers(-5000, 5001, int(rng.integers(1, 40)))]
        return {"type": "selector", "dimension": "l", "value": vals[0]} if len(vals) == 1 else \
            {"type": "in", "dimension": "l", "values": vals}
    if k == "num-d-bound":
        a = int(rng.integers(-2000, 1000))
        return {"type": "bound", "dimension": "d", "lower": "%d.5" % a, "upper": str(a + int(rng.integers(300, 3000))),
                "lowerStrict": True, "upperStrict": False, "ordering": "numeric"}
    seg = int(rng.integers(0, 2))  # num-d-selector: the decimal form of a row's own value
    return {"type": "selector", "dimension": "d", "value": repr(float(columns(seg)["d"][int(rng.integers(0, ROWS[seg]))]))}


NOTHING = ({"type": "selector", "dimension": "lo", "value": "zz"},
           {"type": "and", "fields": [{"type": "selector", "dimension": "lo", "value": "lo1"},
                                      {"type": "selector", "dimension": "lo", "value": "lo2"}]},
           {"type": "not", "field": {"type": "selector", "dimension": "nope", "value": None}})


def _tree(rng, tags, depth):
    """A filter of depth <= 3 - `depth` + 1 levels: a leaf, or not / and / or over smaller trees."""
    r = int(rng.integers(0, 10)) if depth < 3 else 0
    if r < 5:
        return _leaf(rng, tags)
    if r < 6:
        tags.add("f:not")
        return {"type": "not", "field": _tree(rng, tags, depth + 1)}
    kind = "and" if r < 8 else "or"
    tags.add("f:" + kind)
    return {"type": kind, "fields": [_tree(rng, tags, depth + 1) for _ in range(int(rng.integers(2, 4)))]}


def _filter(rng, tags, force=None):
    r = int(rng.integers(0, 40))
    if force == "numeric":
        tags.add("f:and")
        return {"type": "and", "fields": [_leaf(rng, tags, NUMERIC_LEAVES), _leaf(rng, tags, ("selector", "in", "bound-lex"))]}
    if force == "some" and r < 10:
        r = 10
    if r < 8:
        tags.add("f:none")
        return None
    if r == 30:
        tags.add("f:nothing")
        return _pick(rng, NOTHING)
    return _tree(rng, tags, 1)


AGG_FIELDS = {"count": (None,), "longSum": ("l",), "longMin": ("l",), "longMax": ("l",),
              "doubleSum": ("d", "d", "x", "l"), "doubleMin": ("d", "f", "x", "l"), "doubleMax": ("d", "f", "x", "l"),
              "floatSum": ("f", "f", "x"), "floatMin": ("d", "f", "x", "l"), "floatMax": ("d", "f", "x", "l")}
AGG_TYPES = tuple(AGG_FIELDS)
MAX_AGGS = 16  # the engine's limit of aggregators per query


def _wrap(agg, flt):
    return agg if flt is None else {"type": "filtered", "filter": flt, "aggregator": agg}


def _aggs(rng, tags, force=(), filtered_first=False):
    """(aggregator JSON list, names of the drawn ones: the twins are not among them). force: the types of
    the first aggregators; filtered_first: the first one is wrapped whatever the draw says."""
    out, names = [], []
    forced = list(force)
    want = max(int(rng.integers(1, 7)), len(forced))
    k = 0
    while len(names) < want:
        t = forced.pop(0) if forced else _pick(rng, AGG_TYPES)
        field = _pick(rng, AGG_FIELDS[t])
        flt = None
        if int(rng.integers(0, 4)) == 0 or (filtered_first and not names):
            flt = _leaf(rng, set())
        name = "a%d" % k
        k += 1
        js = {"type": t, "name": name}
        if field is not None:
            js["fieldName"] = field
        add = [_wrap(js, flt)]
        if (t, field) in (("doubleSum", "d"), ("floatSum", "f")):
            add.append(_wrap({"type": "count", "name": name + "_n"}, flt))
            add.append(_wrap({"type": t, "name": name + "_abs", "fieldName": field + "_abs"}, flt))
        if len(out) + len(add) > MAX_AGGS:
            break
        out += add
        names.append(name)
        tags.add("agg:" + t)
        if flt is not None:
            tags.add("agg:filtered")
        if len(add) > 1:
            tags.add("agg:twin")
    return out, names


def _common(rng, tags, force):
    iv = force.get("iv") or _pick(rng, ("whole",) * 5 + ("empty",) + ("cut",) * 10 + ("whole",) * 5)
    g = force.get("g") or _pick(rng, tuple(GRANS))
    tags.update(("iv:" + iv, "g:" + g))
    flt = _filter(rng, tags, force.get("filter"))
    aggs, names = _aggs(rng, tags, force.get("aggs", ()), bool(force.get("filtered_agg")))
    js = {"dataSource": "querygen", "intervals": [list(INTERVALS[iv])], "granularity": GRANS[g], "aggregations": aggs}
    if flt is not None:
        js["filter"] = flt
    return js, names, iv, g


def _draw_timeseries(rng, force):
    tags = set()
    js, _, _, _ = _common(rng, tags, force)
    desc = force.get("desc", bool(rng.integers(0, 2)))
    skip = bool(rng.integers(0, 2))
    tags.update(("ts:desc" if desc else "ts:asc", "ts:skip" if skip else "ts:noskip"))
    js.update({"queryType": "timeseries", "descending": desc, "context": {"skipEmptyBuckets": skip}})
    return js, tags


TOPN_DIMS = ("lo", "mid", "hi", "hn", "tags", "nope", "v")
SMALL_DIMS = ("lo", "mid", "hn", "tags", "nope")  # fewer than 1,000 values: the per-segment threshold cuts nothing


def _draw_topn(rng, force):
    tags = set()
    js, names, iv, g = _common(rng, tags, force)
    if g == "dur":
        js["intervals"] = [list(FINE)]
    dim = force.get("dim") or _pick(rng, TOPN_DIMS)
    mk = force.get("metric") or _pick(rng, ("numeric", "numeric", "inverted", "lex", "alnum"))
    if dim == "v" and mk in ("lex", "alnum"):
        mk = "numeric" if mk == "lex" else "inverted"
    if dim == "hi" and mk == "alnum":
        dim = "mid"
    tags.update(("tn:dim:" + dim, "tn:metric:" + mk))
    if mk in ("numeric", "inverted"):
        name = _pick(rng, names)
        agg = next(a for a in js["aggregations"] if (a.get("aggregator") or a)["name"] == name)
        inner = agg.get("aggregator") or agg
        if (inner["type"], inner.get("fieldName")) in (("doubleSum", "d"), ("floatSum", "f")) and dim not in SMALL_DIMS:
            dim = _pick(rng, SMALL_DIMS)
            tags.add("tn:dim:" + dim)
        metric = {"type": "numeric", "metric": name}
        if mk == "inverted":
            metric = {"type": "inverted", "metric": metric}
    else:
        stop = None
        if force.get("stop") or int(rng.integers(0, 3)) == 0:
            stop = _dim_value(rng, dim) if dim != "nope" else "a"
            tags.add("tn:prevstop")
        metric = {"type": "dimension", "ordering": "lexicographic" if mk == "lex" else "alphanumeric", "previousStop": stop}
    thr = _pick(rng, (1, 7, 100_000))
    tags.add("tn:thr:%s" % ("big" if thr > 7 else thr))
    js.update({"queryType": "topN", "dimension": dim, "metric": metric, "threshold": thr})
    return js, tags


GB_DIMS = ("lo", "mid", "hi", "hn", "tags", "nope", "vL", "vS")


def _having_leaf(rng, tags, js, names, pre, aggs_by_name):
    """One having leaf over the cells of `pre` (the oracle's rows without having and limit spec), or None."""
    kind = _pick(rng, ("gt", "lt", "eq", "dimsel"))
    dims = [d for d in js["dimensions"] if isinstance(d, str) and d in ("lo", "mid", "hn", "tags", "nope")]
    if kind == "dimsel":
        if not dims:
            kind = "gt"
        else:
            d = _pick(rng, dims)
            vals = sorted({r.event[d] for r in pre}, key=_jkey) or [None]
            tags.add("gb:having:dimsel")
            return {"type": "dimSelector", "dimension": d, "value": _pick(rng, vals)}
    name = _pick(rng, names)
    agg = aggs_by_name[name]
    cells = sorted({r.event[name] for r in pre if not (isinstance(r.event[name], float) and math.isinf(r.event[name]))})
    if not cells:
        return None
    if is_bounded(agg):
        if kind == "eq" or len(cells) < 2:
            kind = "gt"
        i = int(rng.integers(0, len(cells) - 1)) if len(cells) > 1 else 0
        value = (cells[i] + cells[min(i + 1, len(cells) - 1)]) / 2.0 + (1.0 if len(cells) < 2 else 0.0)
    else:  # (greaterThan the largest cell, or lessThan the smallest, would select nothing)
        value = _pick(rng, cells[:-1] if kind == "gt" and len(cells) > 1 else cells[1:] if kind == "lt" and len(cells) > 1 else cells)
    tags.add("gb:having:" + kind)
    return {"type": {"gt": "greaterThan", "lt": "lessThan", "eq": "equalTo"}[kind], "aggregation": name, "value": value}


def _draw_groupby(rng, force):
    Q, _, _ = _mods()
    tags = set()
    js, names, iv, g = _common(rng, tags, force)
    if "dims" in force:
        dims = list(force["dims"])
    else:
        nd = int(rng.integers(0, 5))
        pool = list(force.get("pool", GB_DIMS))
        dims = []
        while len(dims) < nd:
            d = pool.pop(int(rng.integers(0, len(pool))))
            if d in ("vL", "vS"):
                pool = [p for p in pool if p not in ("vL", "vS")]
            dims.append(d)
    tags.add("gb:ndims:%d" % len(dims))
    for d in dims:
        tags.add("gb:dim:" + d)
    long_v = "vL" in dims
    js["dimensions"] = [{"type": "default", "dimension": "v", "outputName": "v", "outputType": "LONG" if d == "vL" else "STRING"}
                        if d in ("vL", "vS") else d for d in dims]
    if not long_v:
        js["dimensions"] = [d if isinstance(d, str) else "v" for d in js["dimensions"]]
    js["queryType"] = "groupBy"
    aggs_by_name = {a.name: a for a in Q.query_from_json(js).aggregations}
    # ---- having: thresholds from the oracle's cells of the query without having and limit spec ----
    hk = force.get("having") or _pick(rng, ("none", "none", "none", "leaf", "leaf", "and", "or", "not"))
    having = None
    if hk != "none":
        pre = _oracle_run(oracle_query(Q.query_from_json(js)), force.get("layout", 0))
        n_leaf = 1 if hk in ("leaf", "not") else 2
        leaves = [_having_leaf(rng, tags, js, names, pre, aggs_by_name) for _ in range(n_leaf)]
        if all(x is not None for x in leaves):
            having = leaves[0] if hk == "leaf" else {"type": "not", "havingSpec": leaves[0]} if hk == "not" else \
                {"type": hk, "havingSpecs": leaves}
            if hk != "leaf":
                tags.add("gb:having:" + hk)
    if having is None:
        tags.add("gb:having:none")
    else:
        js["having"] = having
    # ---- limit spec ----
    lk = force.get("limit") or _pick(rng, ("none", "none", "only", "order", "order", "order+limit", "order+limit"))
    tags.add("gb:limit:" + lk)
    if lk != "none":
        cols = []
        if lk != "only":
            order_dims = [d for d in dims if d != "vL"]
            for _ in range(int(rng.integers(1, 3))):
                if order_dims and int(rng.integers(0, 2)):
                    d = _pick(rng, order_dims)
                    order = _pick(rng, ("lexicographic", "numeric"))
                    col = {"dimension": "v" if d == "vS" else d, "dimensionOrder": order}
                    tags.update(("gb:order:dim", "gb:order:" + order))
                else:
                    col = {"dimension": _pick(rng, names), "dimensionOrder": "lexicographic"}
                    tags.add("gb:order:agg")
                col["direction"] = _pick(rng, ("ascending", "descending"))
                tags.add("gb:order:" + col["direction"])
                if col["dimension"] not in [c["dimension"] for c in cols]:
                    cols.append(col)
        spec = {"type": "default", "columns": cols}
        if lk != "order":
            spec["limit"] = _pick(rng, (5, 100))
        js["limitSpec"] = spec
    # ---- context ----
    ctx = {}
    if force.get("hash") or int(rng.integers(0, 4)) == 0:
        ctx["forceHashAggregation"] = True
        tags.add("gb:ctx:hash")
    if int(rng.integers(0, 5)) == 0:
        ctx["bufferGrouperMaxSize"] = 1_000_000
        tags.add("gb:ctx:maxsize")
    if "limit" in js.get("limitSpec", {}) and having is None and (int(rng.integers(0, 3)) == 0 or force.get("pushdown")):
        ctx["forceLimitPushDown"] = True
        tags.add("gb:ctx:pushdown")
    if int(rng.integers(0, 5)) == 0 or force.get("dimsfirst"):
        ctx["sortByDimsFirst"] = True
        tags.add("gb:ctx:dimsfirst")
    if ctx:
        js["context"] = ctx
    return js, tags


# index -> forced axis values: the combinations the census asks for, and the key+reference word form
PINS = {
    ("ts", 0): {"g": "p1d", "desc": True, "filtered_agg": True}, ("ts", 1): {"g": "pt1h", "desc": True, "filtered_agg": True},
    ("tn", 0): {"dim": "mid", "metric": "alnum", "stop": True, "filter": "some"},
    ("tn", 1): {"dim": "hn", "metric": "alnum", "stop": True, "filter": "some"},
    ("gb", 0): {"dims": ("hi", "mid", "vL", "hn"), "g": "dur", "iv": "whole"},
    ("gb", 1): {"dims": ("mid", "hi", "hn", "vS"), "g": "dur", "iv": "whole"},
    ("gb", 2): {"dims": ("vL", "hn", "hi", "mid"), "g": "dur", "iv": "whole", "limit": "none"},
    ("gb", 3): {"dims": ("hn", "vS", "mid", "hi"), "g": "dur", "iv": "whole", "having": "none"},
    ("gb", 4): {"dims": ("vL", "lo"), "g": "hour", "hash": True}, ("gb", 5): {"dims": ("mid", "vL"), "g": "pt1h", "hash": True},
    ("gb", 6): {"dims": ("tags", "lo"), "filter": "numeric"}, ("gb", 7): {"dims": ("tags",), "filter": "numeric", "g": "hour"},
    ("gb", 8): {"dims": ("lo", "hn"), "aggs": ("floatSum",), "limit": "order+limit"},
    ("gb", 9): {"dims": ("mid",), "aggs": ("floatSum", "doubleSum"), "limit": "order"},
    ("gb", 10): {"dims": ("tags", "mid"), "having": "leaf"}, ("gb", 11): {"dims": ("lo", "tags"), "having": "and", "g": "p1d"},
}
KINDS = (("ts", N_TS, _draw_timeseries), ("tn", N_TN, _draw_topn), ("gb", N_GB, _draw_groupby))
MAX_ATTEMPTS = 40
_GEN = {}


def _generate():
    Q, _, _ = _mods()
    out, axes = [], {}
    for ki, (kind, count, draw) in enumerate(KINDS):
        for i in range(count):
            qid = "%s-%03d" % (kind, i)
            for attempt in range(MAX_ATTEMPTS):
                js, tags = draw(np.random.default_rng([SEED, ki, i, attempt]), PINS.get((kind, i), {}))
                q = Q.query_from_json(js)
                if steering_violations(q):
                    continue
                # an empty result comes from the axes meant to give one, not from an unlucky conjunction
                if not is_empty(expected_for(q)) or tags & {"iv:empty", "f:nothing"}:
                    break
            else:
                raise AssertionError(f"{qid}: no draw in {MAX_ATTEMPTS} attempts keeps its floating sums apart")
            if kind == "gb" and i < 4:
                tags.add("gb:keyref")
            out.append((qid, q))
            axes[qid] = tags
    _GEN["queries"], _GEN["axes"] = out, axes


def queries():
    """[(id, query)]: the same list at every call."""
    if "queries" not in _GEN:
        _generate()
    return list(_GEN["queries"])


def axes(merge=False):
    """id -> the axis values the query was drawn with (merge: of the merge queries, the gm-* draws included)."""
    queries()
    if not merge:
        return _GEN["axes"]
    both = dict(_GEN["axes"], **_merge_gen()["axes"])
    return {qid: both[qid] for qid, _ in merge_queries()}


def query(qid):
    return dict(merge_queries() if qid.startswith("gm") else queries())[qid]


def ids(kind=None):
    """The ids, without generating anything (for parametrize)."""
    return ["%s-%03d" % (k, i) for k, n, _ in KINDS for i in range(n) if kind in (None, k)]


def expected(qid):
    return expected_for(query(qid))


def queries_sha256():
    import hashlib
    return hashlib.sha256("".join(json.dumps(q.to_json(), sort_keys=True) for _, q in queries()).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------
# the merge draw: the queries the cross-segment, cross-device and cross-rank merges are held to, over the
# four pieces (expected_for(q, PIECES): a topN's per-segment cut and fold order depend on the split)
# ---------------------------------------------------------------------------------------------
MERGE_GB = 44  # gm-*: further groupBy draws that no device-side merge refuses (no dimension over v)
MERGE_POOL = tuple(d for d in GB_DIMS if d not in ("vL", "vS"))
# the gb-* indices that do not group by v (a draw's outcome, kept here so that ids need no generation;
# tests/test_querygen.py holds it to the draw)
GB_NO_V = (6, 7, 8, 9, 10, 11, 15, 19, 21, 23, 26, 27, 28, 29, 30, 32, 38, 40, 41, 43, 45, 49, 50, 51, 52, 56, 58, 59, 60, 61, 62)
# index -> forced axis values: what the merge census of tests/test_querygen.py asks for among the queries of a
# fixed-period granularity, the ones dg_groupby_merge_devices takes
MERGE_PINS = {
    0: {"dims": (), "g": "all"}, 1: {"dims": (), "g": "all", "hash": True}, 2: {"dims": (), "g": "all", "iv": "cut"},
    3: {"dims": (), "g": "all", "iv": "empty"},
    4: {"dims": ("mid", "lo"), "g": "hour", "having": "none", "limit": "order+limit", "pushdown": True},
    5: {"dims": ("hi",), "g": "all", "having": "none", "limit": "only", "pushdown": True},
    6: {"dims": ("tags", "hn"), "g": "dur", "having": "none", "limit": "order+limit", "pushdown": True},
    7: {"dims": ("lo", "nope"), "g": "all", "having": "none", "limit": "only", "pushdown": True},
    8: {"g": "hour", "iv": "empty"},
}
# id -> reason: a ts / tn / gb query whose floating sums steer its result within their bound on the pieces only
# (at most 4; gm-* draws are drawn again instead)
MERGE_LEFT_OUT = {}
_MGEN = {}


def _merge_gen():
    if "queries" in _MGEN:
        return _MGEN
    Q, _, _ = _mods()
    out, axes = [], {}
    for i in range(MERGE_GB):
        qid = "gm-%03d" % i
        force = dict(MERGE_PINS.get(i, {}), pool=MERGE_POOL, layout=PIECES)
        for attempt in range(MAX_ATTEMPTS):
            js, tags = _draw_groupby(np.random.default_rng([SEED, 3, i, attempt]), force)
            q = Q.query_from_json(js)
            if steering_violations(q, PIECES):
                continue
            if not is_empty(expected_for(q, PIECES)) or tags & {"iv:empty", "f:nothing"}:
                break
        else:
            raise AssertionError(f"{qid}: no draw in {MAX_ATTEMPTS} attempts keeps its floating sums apart")
        out.append((qid, q))
        axes[qid] = tags
    _MGEN["queries"], _MGEN["axes"] = out, axes
    return _MGEN


def merge_ids(kind=None):
    """The merge queries' ids, without generating anything: every ts-* and tn-*, the gb-* that do not group by
    v, every gm-*, less MERGE_LEFT_OUT."""
    out = ids("ts") + ids("tn") + ["gb-%03d" % i for i in GB_NO_V] + ["gm-%03d" % i for i in range(MERGE_GB)]
    return [qid for qid in out if qid not in MERGE_LEFT_OUT and kind in (None, qid[:2])]


def merge_queries():
    """[(id, query)] of merge_ids()."""
    old = dict(queries())
    new = dict(_merge_gen()["queries"])
    return [(qid, new[qid] if qid in new else old[qid]) for qid in merge_ids()]


def merge_queries_sha256():
    import hashlib
    return hashlib.sha256("".join(qid + json.dumps(q.to_json(), sort_keys=True) for qid, q in merge_queries()).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------
# floating sums that steer a result
# ---------------------------------------------------------------------------------------------
def _adjacent_violations(cells, what):
    """cells: (value, bound) of one ordering context. Adjacent distinct values must differ by more than 4x the
    larger bound; equal values are only allowed where both are exact."""
    out = []
    cells = sorted(cells)
    for (a, ba), (b, bb) in zip(cells, cells[1:]):
        m = max(ba, bb)
        if m > 0.0 and abs(b - a) <= 4.0 * m:
            out.append(f"{what}: {a!r} and {b!r} lie within 4 x {m!r}")
    return out


def steering_violations(q, layout=0):
    """Where a bounded floating sum decides q's result — a topN metric, a limit-spec column, a having operand —
    the oracle's cells (over `layout`) must be further apart than four times the bound. Returns the violations found."""
    Q, _, _ = _mods()
    aggs = {a.name: a for a in q.aggregations}
    out = []
    if isinstance(q, Q.TopNQuery):
        name = q.metric.metric if q.metric.type in ("numeric", "inverted") else None
        if name is None or not is_bounded(aggs[name]):
            return out
        full = _oracle_run(dataclasses.replace(oracle_query(q), threshold=100_000), layout)
        for r in full:
            out += _adjacent_violations([(e[name], cell_bound(aggs[name], e)) for e in r.value], f"metric {name} at {r.timestamp}")
        return out
    if not isinstance(q, Q.GroupByQuery):
        return out
    oq = oracle_query(q)
    cols = [c.dimension for c in (q.limitSpec.columns if q.limitSpec else []) if c.dimension in aggs and is_bounded(aggs[c.dimension])]
    leaves = []

    def walk(h):
        if h is None:
            return
        if h.type in ("greaterThan", "lessThan", "equalTo") and h.aggregation in aggs and is_bounded(aggs[h.aggregation]):
            leaves.append(h)
        for x in h.specs:
            walk(x)
    walk(q.having)
    if not cols and not leaves:
        return out
    ctx = {k: x for k, x in oq.context.items() if k != "forceLimitPushDown"}
    if leaves:
        pre = _oracle_run(dataclasses.replace(oq, limitSpec=None, having=None, context=ctx), layout)
        for h in leaves:
            a = aggs[h.aggregation]
            for r in pre:
                b = cell_bound(a, r.event)
                if abs(r.event[a.name] - float(h.value)) <= 4.0 * b or (b > 0.0 and h.type == "equalTo"):
                    out.append(f"having {h.aggregation} {h.type} {h.value!r}: cell {r.event[a.name]!r} within 4 x {b!r}")
                    break
    if cols:
        rows = _oracle_run(dataclasses.replace(oq, limitSpec=None, context=ctx), layout)  # (after the having spec)
        one = q.granularity.is_all or q._ctx_bool("sortByDimsFirst", False)
        for name in cols:
            groups = {}
            for r in rows:
                groups.setdefault(0 if one else r.timestamp, []).append((r.event[name], cell_bound(aggs[name], r.event)))
            for t, cells in groups.items():
                out += _adjacent_violations(cells, f"order column {name} at {t}")
    return out


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def _cell_plan(q):
    """name -> the bounded aggregator behind it, or None for a cell compared exactly."""
    return {a.name: a for a in q.aggregations if is_bounded(a)}


def _cells_difference(plan, got, exp, where):
    """where: a callable giving the cells' place for the message (only built on a difference)."""
    if got.keys() != exp.keys():
        return f"{where()}: keys {sorted(got)} != {sorted(exp)}"
    for k, e in exp.items():
        g = got[k]
        if k in plan:
            b = cell_bound(plan[k], exp)
            if not (abs(g - e) <= b):
                return f"{where()}: {k}: got {g!r} expected {e!r}, |difference| {abs(g - e)!r} > bound {b!r}"
        elif type(g) is not type(e) or not _close(g, e, 0.0):
            return f"{where()}: {k}: got {g!r} expected {e!r}"
    return None


def first_difference(q, got, exp, cut_ties=0):
    """The first cell in which `got` differs from the expectation `exp` of q, as text; None when there is none."""
    Q, _, _ = _mods()
    if len(got) != len(exp):
        return f"{len(got)} results, expected {len(exp)}: got {got[:2]!r} expected {exp[:2]!r}"
    plan = _cell_plan(q)
    relaxed = isinstance(q, Q.TopNQuery) and q.dimension == "v" and cut_ties > 0
    full = _oracle_run(dataclasses.replace(oracle_query(q), threshold=100_000)) if relaxed else None
    for i, (g, e) in enumerate(zip(got, exp)):
        if g.timestamp != e.timestamp:
            return f"result {i}: timestamp {g.timestamp} expected {e.timestamp}"
        if isinstance(g, Q.Row):
            d = _cells_difference(plan, g.event, e.event, lambda: f"row {i} at {g.timestamp}")
        elif isinstance(e.value, list):
            d = None
            if len(g.value) != len(e.value):
                return f"result {i} at {g.timestamp}: {len(g.value)} entries, expected {len(e.value)}"
            n = len(e.value)
            tied = None
            if relaxed and n:
                m = q.metric.metric
                ranking = next(r.value for r in full if r.timestamp == e.timestamp)
                if len(ranking) > n and _close(ranking[n][m], ranking[n - 1][m], 0.0):  # a tie across the cut
                    last = e.value[-1][m]
                    n = next(j for j, x in enumerate(e.value) if _close(x[m], last, 0.0))
                    tied = {x["v_s"] for x in ranking if _close(x[m], last, 0.0)}
            for j in range(n):
                d = _cells_difference(plan, g.value[j], e.value[j], lambda: f"result {i} at {g.timestamp} entry {j}")
                if d:
                    break
            if not d and tied is not None:
                for j in range(n, len(g.value)):
                    if g.value[j]["v"] not in tied:
                        d = f"result {i} at {g.timestamp} entry {j}: {g.value[j]['v']!r} is not among the values tied at the cut"
                        break
        else:
            d = _cells_difference(plan, g.value, e.value, lambda: f"result {i} at {g.timestamp}")
        if d:
            return d
    return None


def assert_parity(qid, q, got, exp, layout="", route="", cut_ties=0):
    d = first_difference(q, got, exp, cut_ties)
    assert d is None, (f"{qid} (replay with -k {qid}) layout {layout} route {route or 'default'}: {d}\n"
                       f"query: {json.dumps(q.to_json(), sort_keys=True)}")


def is_empty(res):
    """No row, and no topN entry in any result."""
    return all(isinstance(getattr(r, "value", None), list) and not r.value for r in res)


def bits_for(card):
    b = 0
    while (1 << b) < card:
        b += 1
    return b


def sort_word_bits(q):
    """(key bits, reference bits) of the engine's groupBy sort word for q over the fixture, from the oracle's
    dictionaries: every dimension's merged cardinality (a multi-value dimension's empty rows and a missing
    dimension count as the null value), the buckets of a fixed-period granularity over the data's part of the
    interval, and one reference per row of the call."""
    segs = oracle_segments()
    bits = 0
    for d in oracle_query(q).dimensions:
        vals = set()
        for s in segs:
            vals |= set(s.dictionary(d)) if s.is_dim(d) else {None}
            if s.is_dim(d) and s.is_multi(d):
                vals.add(None)
        bits += bits_for(max(len({x or None for x in vals}), 1))
    g = q.granularity
    if g.period_ms:
        lo = max(q.interval[0], min(int(s.time()[0]) for s in segs))
        hi = min(q.interval[1], max(g.bucket_end(int(s.time()[-1])) for s in segs))
        if hi > lo:
            bits += bits_for((hi - g.bucket_start(lo)) // g.period_ms)
    return bits, bits_for(sum(s.num_rows for s in segs))
