"""Java numeric edge semantics, pinned on the CPU oracle independently of the kernels: the fixtures
tests/test_special_values_gpu.py runs through the device code (built here as plain functions), the
values the oracle gives for them as literals, and the topN orders it gives over NaN and -0.0.

The rules and where the reference states them:
* doubleMin / doubleMax / floatMin / floatMax fold with Math.min / Math.max (DoubleMinAggregator.java:46,
  DoubleMaxAggregator.java:46, FloatMinAggregator.java:46, FloatMaxAggregator.java:46; combine :30): NaN
  if either input is NaN, -0.0 below +0.0;
* a long aggregator over a double column reads (long) getDouble() (DoubleColumnSelector.java:54): NaN
  -> 0, saturating at Long.MIN_VALUE / Long.MAX_VALUE; longSum wraps (LongSumAggregator.java:45);
* a topN orders by the aggregator's comparator, Doubles.compare = Double.compare for the double and
  float aggregators (DoubleSumAggregator.java:37, SimpleDoubleAggregatorFactory.java:101): NaN greatest,
  -0.0 below +0.0; TopNNumericResultBuilder keeps the largest `threshold` by (metric, dimension value)
  (TopNNumericResultBuilder.java:94-106, add :186-190) and lists them metric descending, dimension
  value ascending (:225-232); InvertedTopNMetricSpec inverts the metric comparator
  (InvertedTopNMetricSpec.java:65-84).

Every segment has 24,577 rows: three full 8,192-value LZ4 blocks and a last block of one value."""
import math

import numpy as np
import pytest

from compare import TOL, _close

N_ROWS = 24_577
IV = ["1970-01-01T00:00:00Z/1970-01-01T00:00:30Z"]  # [0, 30,000) ms: every row
MAX, MIN = (1 << 63) - 1, -(1 << 63)
NAN, INF = math.nan, math.inf
KS = (0, 1, 8191, 8192, 24575, 24576)  # poisoned rows: first / second value of a 16-byte pair, last value of a
#                                        block, first of the next, last of the last full block, the lone last value


# ---------------------------------------------------------------------------------------------
# fixtures (plain functions: the GPU module builds the same segments)
# ---------------------------------------------------------------------------------------------
def specials_columns(n=N_ROWS):
    """g = row % 6; d per group: g0 linspace(1, 2), g1 3.5 with NaN (its sign bit set) at every 7th of its rows, g2 1e300 with
    +inf at every 9th, g3 -0.0 / +0.0 alternating, g4 -2.25 with -inf at every 11th, g5 +1e19 / -1e19
    alternating; f = (float) d; l = the row number, Long.MAX_VALUE in g1, Long.MIN_VALUE in g2."""
    g = (np.arange(n) % 6).astype(np.int32)
    d = np.linspace(1.0, 2.0, n)

    def put(k, every, special, plain):
        idx = np.arange(int((g == k).sum()))
        d[g == k] = np.where(idx % every == 0, special, plain)

    put(1, 7, -np.nan, 3.5)  # (sign bit set: Double.compare and Math.min / max know one NaN, the greatest)
    put(2, 9, np.inf, 1e300)
    put(3, 2, -0.0, 0.0)
    put(4, 11, -np.inf, -2.25)
    put(5, 2, 1e19, -1e19)
    with np.errstate(over="ignore"):  # (1e300 is +inf as a float)
        f = d.astype(np.float32)
    l = np.arange(n, dtype=np.int64)
    l[g == 1] = MAX
    l[g == 2] = MIN
    return g, d, f, l


def specials_spec(W, lo=0, hi=N_ROWS, n=N_ROWS):
    """Rows [lo, hi) of the specials fixture as a segment of the interval [lo, hi) ms (the last: to 30,000)."""
    g, d, f, l = specials_columns(n)
    s = slice(lo, hi)
    return W.SegmentSpec(timestamps=np.arange(lo, hi, dtype=np.int64),
                         dims={"g": (["g%d" % k for k in range(6)], g[s])},
                         metrics={"d": ("double", d[s]), "f": ("float", f[s]), "l": ("long", l[s])},
                         interval=(lo, 30_000 if hi == n else hi))


def specials_aggs(Q):
    return [Q.count("n"), Q.double_min("dmin", "d"), Q.double_max("dmax", "d"), Q.double_sum("ds", "d"),
            Q.float_min("fmin", "f"), Q.float_max("fmax", "f"), Q.float_sum("fs", "f"),
            Q.long_sum("ls", "l"), Q.long_min("lmin", "l"), Q.long_max("lmax", "l"),
            Q.long_sum("ls_d", "d"), Q.long_max("lmax_d", "d"), Q.double_sum("ds_l", "l")]


F19 = 9.999999980506448e18  # (float) 1e19
# granularity ALL timeseries filtered to g = gK, as the CPU oracle computes them (the test below holds it to
# them); fs is compared with the oracle only, and g5's ds is exempt (EXEMPT below)
SPECIALS_EXPECTED = {
    "g0": dict(n=4097, dmin=1.0, dmax=2.0, ds=6145.5, fmin=1.0, fmax=2.0, ls=50343936, lmin=0, lmax=24576,
               ls_d=4098, lmax_d=2, ds_l=50343936.0),
    "g1": dict(n=4096, dmin=NAN, dmax=NAN, ds=NAN, fmin=NAN, fmax=NAN, ls=-4096, lmin=MAX, lmax=MAX,
               ls_d=10530, lmax_d=3, ds_l=3.777893186295716e22),
    "g2": dict(n=4096, dmin=1e300, dmax=INF, ds=INF, fmin=INF, fmax=INF, ls=0, lmin=MIN, lmax=MIN,
               ls_d=-4096, lmax_d=MAX, ds_l=-3.777893186295716e22),
    "g3": dict(n=4096, dmin=-0.0, dmax=0.0, ds=0.0, fmin=-0.0, fmax=0.0, ls=50331648, lmin=3, lmax=24573,
               ls_d=0, lmax_d=0, ds_l=50331648.0),
    "g4": dict(n=4096, dmin=-INF, dmax=-2.25, ds=-INF, fmin=-INF, fmax=-2.25, ls=50335744, lmin=4, lmax=24574,
               ls_d=9223372036854768362, lmax_d=-2, ds_l=50335744.0),
    "g5": dict(n=4096, dmin=-1e19, dmax=1e19, fmin=-F19, fmax=F19, ls=50339840, lmin=5, lmax=24575,
               ls_d=-2048, lmax_d=MAX, ds_l=50339840.0),
}
SUMS = {"ds": TOL["double"], "ds_l": TOL["double"], "fs": TOL["float"]}  # every other cell is exact
# Cells left out of every comparison: sums that cancel, whose value depends on the addition order. g5's ds
# and fs (+1e19 and -1e19 alternating), and ds_l over every row at once ("all"): 4,096 times 2^63 and 4,096
# times -2^63 among row numbers; while a partial sum stands near 3.8e22 one ulp is 2^23 = 8.4e6, so the
# 2.0e8 left at the end is known to a few ulps of that only, not to 1e-9 of itself.
EXEMPT = {("g5", "ds"), ("g5", "fs"), ("all", "ds_l")}


def drop_exempt(results, dim="g", group=None):
    """The results without the EXEMPT cells: in the topN entries / groupBy rows whose `dim` is the group, or
    (`group`: a timeseries filtered to it, "all" for the unfiltered one) everywhere."""
    for r in results:
        value = getattr(r, "value", None)
        for e in [r.event] if value is None else value if isinstance(value, list) else [value]:
            g = group or e.get(dim)
            for name in [name for gg, name in EXEMPT if gg == g]:
                e.pop(name, None)
    return results


def poisoned_spec(W, n=N_ROWS):
    """Per poisoned row k: nan_k with one NaN at row k, negz_k with one -0.0 at row k among +0.0 and
    positive values, posz_k its mirror image (one +0.0 among -0.0 and negative values), lo_k / hi_k the row
    number with Long.MIN_VALUE / Long.MAX_VALUE at row k; g6 = row % 6.
    Filler: two rows of three hold the constant (1.5, +0.0, -0.0), every third a value of a ramp. Columns of
    the constant alone (1.5 everywhere, +0.0 everywhere) compress to blocks the light decoder takes, which
    never folds; with the ramp every full block folds on both decoder routes. A doubleMax over a column
    that is +0.0 but for one -0.0 cannot tell a dropped row, so the maximum is checked on the mirror image."""
    ramp, third = np.linspace(0.5, 1.5, n), np.arange(n) % 3 == 1  # (the lone last row: the constant)
    metrics = {}
    for k in KS:
        a = np.where(third, ramp + 0.75, 1.5)  # within [1.25, 2.25]
        a[k] = np.nan
        z = np.where(third, ramp, 0.0)
        z[k] = -0.0
        p = np.where(third, -ramp, -0.0)
        p[k] = 0.0
        lo, hi = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
        lo[k], hi[k] = MIN, MAX
        metrics.update({f"nan_{k}": ("double", a), f"negz_{k}": ("double", z), f"posz_{k}": ("double", p),
                        f"lo_{k}": ("long", lo), f"hi_{k}": ("long", hi)})
    g6 = (np.arange(n) % 6).astype(np.int32)
    return W.SegmentSpec(timestamps=np.arange(n, dtype=np.int64), dims={"g6": (["v%d" % k for k in range(6)], g6)},
                         metrics=metrics, interval=(0, 30_000))


def poisoned_aggs(Q, k):
    """The seven aggregators over row k's columns (a query holds at most 16: two rows' worth)."""
    return [Q.double_min(f"nmin_{k}", f"nan_{k}"), Q.double_max(f"nmax_{k}", f"nan_{k}"),
            Q.double_sum(f"nsum_{k}", f"nan_{k}"), Q.double_min(f"zmin_{k}", f"negz_{k}"),
            Q.double_max(f"zmax_{k}", f"posz_{k}"), Q.long_min(f"lmin_{k}", f"lo_{k}"), Q.long_max(f"lmax_{k}", f"hi_{k}")]


def check_poisoned(value, k, holds):
    """One result's cells of row k. Its rows hold row k: NaN, -0.0 as the minimum and +0.0 as the maximum of
    the zero columns (sign bits included), the long extremes. They do not: none of these."""
    nmin, nmax, nsum, zmin, zmax = (value[f"{s}_{k}"] for s in ("nmin", "nmax", "nsum", "zmin", "zmax"))
    assert zmin == 0.0 and zmax == 0.0, (k, zmin, zmax)
    if holds:
        assert math.isnan(nmin) and math.isnan(nmax) and math.isnan(nsum), (k, value)
        assert math.copysign(1.0, zmin) < 0 and math.copysign(1.0, zmax) > 0, (k, zmin, zmax)
        assert value[f"lmin_{k}"] == MIN and value[f"lmax_{k}"] == MAX
    else:
        assert 1.25 <= nmin <= nmax <= 2.25 and nsum >= nmax, (k, value)
        assert math.copysign(1.0, zmin) > 0 and math.copysign(1.0, zmax) < 0, (k, zmin, zmax)
        assert value[f"lmin_{k}"] > MIN and value[f"lmax_{k}"] < MAX


RANKED_CARD = 600
RANKED_TIES = range(4, 304)  # the 300 values sharing t's maximum


def ranked_spec(W, n=N_ROWS):
    """h = row % 600. m: 0.5, and on value j's second row 1.0 advanced j ulps (nextafter applied j times):
    the doubleMax keys differ in their last ten bits only. t: 0.25, and on the second row of value 0 NaN,
    1 +inf, 2 -inf, 3 -0.0, 4..303 exactly 7.0 (300 ties), the others 1 + j / 1024 (distinct, below 7)."""
    j = np.arange(n) % RANKED_CARD
    second = (np.arange(n) // RANKED_CARD) == 1
    m = np.full(n, 0.5)
    m[second] = 1.0 + j[second] * np.finfo(np.float64).eps
    assert m[RANKED_CARD + 3] == np.nextafter(np.nextafter(np.nextafter(1.0, 2.0), 2.0), 2.0)
    t = np.full(n, 0.25)
    peak = 1.0 + np.arange(RANKED_CARD) / 1024.0
    peak[RANKED_TIES.start:RANKED_TIES.stop] = 7.0
    peak[:4] = [np.nan, np.inf, -np.inf, -0.0]
    t[second] = peak[j[second]]
    t[j == 2] = -np.inf  # (a maximum of -inf / -0.0 needs every row of the value at or below it)
    t[(j == 3) & ~second] = -1.0
    names = ["h%d" % k for k in range(RANKED_CARD)]
    dictionary, ids = W.encode_strings([names[x] for x in j])
    return W.SegmentSpec(timestamps=np.arange(n, dtype=np.int64), dims={"h": (dictionary, ids)},
                         metrics={"m": ("double", m), "t": ("double", t)}, interval=(0, 30_000))


def ranked_aggs(Q):
    return [Q.count("n"), Q.double_max("mmax", "m"), Q.double_max("tmax", "t")]


def topn(Q, dim, metric, threshold, aggs, inverted=False, **kw):
    """A topN whose per-segment threshold is the query's own (minTopNThreshold defaults to 1,000, above
    every cardinality here: no selection would run)."""
    spec = {"type": "inverted", "metric": {"type": "numeric", "metric": metric}} if inverted else metric
    return Q.TopNQuery(intervals=IV, dimension=dim, metric=spec, threshold=threshold, aggregations=aggs,
                       context={"minTopNThreshold": threshold}, **kw)


def ranking_query(Q, metric, inverted, threshold, dim="g"):
    """A topN over `specials` ranked by one aggregator. g5's cancelling sum is no ranking key: the query
    ranked by ds leaves g5 out (filter g != g5)."""
    flt = Q.NotDimFilter(Q.SelectorDimFilter(dim, "g5")) if metric in ("ds", "fs") else None
    return topn(Q, dim, metric, threshold, specials_aggs(Q), inverted, filter=flt)


# ---------------------------------------------------------------------------------------------
# the oracle on them
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segs(W, O, tmp_path_factory):
    base = tmp_path_factory.mktemp("special_values")
    out = {}
    for name, spec in (("specials", specials_spec(W)), ("poisoned", poisoned_spec(W)), ("ranked", ranked_spec(W))):
        out[name] = O.OracleSegment(W.write_segment(str(base / name), spec, lz4_mode="fast"))
    return out


@pytest.mark.parametrize("group", sorted(SPECIALS_EXPECTED))
def test_specials_table_is_what_the_oracle_computes(Q, O, segs, group):
    q = Q.TimeseriesQuery(intervals=IV, granularity="all", aggregations=specials_aggs(Q),
                          filter=Q.SelectorDimFilter("g", group))
    (res,) = O.run(q, [segs["specials"]])
    exp = SPECIALS_EXPECTED[group]
    assert set(exp) | {"fs"} | ({"ds"} if group == "g5" else set()) == set(res.value)
    for name, v in exp.items():
        assert _close(res.value[name], v, SUMS.get(name, 0.0)), (group, name, res.value[name], v)


def test_poisoned_rows_reach_the_oracle_result(Q, O, segs):
    for k in KS:
        aggs = poisoned_aggs(Q, k)
        (res,) = O.run(Q.TimeseriesQuery(intervals=IV, granularity="all", aggregations=aggs), [segs["poisoned"]])
        check_poisoned(res.value, k, True)
        per_block = O.run(Q.TimeseriesQuery(intervals=IV, granularity={"type": "duration", "duration": 8192},
                                            aggregations=aggs), [segs["poisoned"]])
        assert [r.timestamp for r in per_block] == [0, 8192, 16384, 24576]
        for b, r in enumerate(per_block):
            check_poisoned(r.value, k, k // 8192 == b)
        # row k kept / dropped by the filter g6 != v
        for v, holds in (((k + 1) % 6, True), (k % 6, False)):
            flt = Q.NotDimFilter(Q.SelectorDimFilter("g6", "v%d" % v))
            (res,) = O.run(Q.TimeseriesQuery(intervals=IV, granularity="all", aggregations=aggs, filter=flt),
                           [segs["poisoned"]])
            check_poisoned(res.value, k, holds)


# the oracle's topN orders over `specials`, threshold 6 (every group), as observed; the rules they follow:
# Double.compare puts NaN (g1) greatest, so first, and last under an inverted spec; -0.0 (g3's dmin) sorts
# below every positive value, so ahead of g0's 1.0 under an inverted spec; ls and lmax_d are Long.compare
SPECIALS_ORDER = {
    ("dmax", False): ["g1", "g2", "g5", "g0", "g3", "g4"],
    ("dmin", False): ["g1", "g2", "g0", "g3", "g5", "g4"],
    ("ds", False): ["g1", "g2", "g0", "g3", "g4"],
    ("fmin", False): ["g1", "g2", "g0", "g3", "g5", "g4"],
    ("lmax_d", False): ["g2", "g5", "g1", "g0", "g3", "g4"],
    ("ls", False): ["g0", "g5", "g4", "g3", "g2", "g1"],
    ("dmax", True): ["g4", "g3", "g0", "g5", "g2", "g1"],
    ("dmin", True): ["g4", "g5", "g3", "g0", "g2", "g1"],
    ("ds", True): ["g4", "g3", "g0", "g2", "g1"],
    ("fmin", True): ["g4", "g5", "g3", "g0", "g2", "g1"],
    ("lmax_d", True): ["g4", "g3", "g0", "g1", "g2", "g5"],
    ("ls", True): ["g1", "g2", "g3", "g4", "g5", "g0"],
}


@pytest.mark.parametrize("metric,inverted", sorted(SPECIALS_ORDER))
def test_oracle_topn_order_over_nan_and_signed_zero(Q, O, segs, metric, inverted):
    (res,) = O.run(ranking_query(Q, metric, inverted, 6), [segs["specials"]])
    order = [e["g"] for e in res.value]
    assert order == SPECIALS_ORDER[(metric, inverted)]
    if metric in ("dmax", "dmin", "ds", "fmin"):
        assert order[-1 if inverted else 0] == "g1"  # NaN
    if metric == "dmin" and inverted:
        assert order.index("g3") < order.index("g0")  # -0.0 ahead of 1.0


def test_oracle_ranks_last_bit_maxima_and_threshold_ties(Q, O, segs):
    aggs = ranked_aggs(Q)
    (res,) = O.run(topn(Q, "h", "mmax", 10, aggs), [segs["ranked"]])
    assert [e["h"] for e in res.value] == ["h%d" % j for j in range(599, 589, -1)]
    (res,) = O.run(topn(Q, "h", "mmax", 10, aggs, inverted=True), [segs["ranked"]])
    assert [e["h"] for e in res.value] == ["h%d" % j for j in range(10)]
    # ties at the threshold: a value enters the full queue only when the queue's least metric is below its
    # own (TopNNumericResultBuilder.java:186-190), and the values are offered in dictionary order, so of the
    # 300 values at 7.0 the first in that order stay; the list runs metric descending, value ascending
    # (:225-232)
    tied = sorted("h%d" % j for j in RANKED_TIES)
    for threshold in (10, 300):
        (res,) = O.run(topn(Q, "h", "tmax", threshold, aggs), [segs["ranked"]])
        assert [e["h"] for e in res.value] == ["h0", "h1"] + tied[:threshold - 2]
        assert math.isnan(res.value[0]["tmax"]) and res.value[1]["tmax"] == INF and res.value[2]["tmax"] == 7.0
    (res,) = O.run(topn(Q, "h", "tmax", 10, aggs, inverted=True), [segs["ranked"]])
    assert [e["h"] for e in res.value] == ["h2", "h3"] + ["h%d" % j for j in range(304, 312)]
    assert res.value[1]["tmax"] == 0.0 and math.copysign(1.0, res.value[1]["tmax"]) < 0
