"""Writes tests/golden/post_agg_kats.json: the post-aggregators' known-answer tests.

Transcribed by hand from the reference's post-aggregator tests (paths relative to the reference root,
processing/src/test/java/org/apache/druid/query/aggregation/post/):

* "compute": the post-aggregator as this project's JSON, the row's values and the expected value. A double is
  written as its bit pattern ("d:<16 hex digits>", so NaN, the infinities and -0.0 survive JSON), a long as
  "l:<decimal>".
    ArithmeticPostAggregatorTest.java:40-86 testCompute (roku = 6.0, rows = a count of 3: 9, 3, 18, 2),
      :122-140 testQuotient (value / 0 under quotient: NaN, NaN, +inf, -inf),
      :142-158 testDiv (value / 0 under "/": always 0.0)
    DoubleGreatestPostAggregatorTest.java:37-61 (6.0), DoubleLeastPostAggregatorTest.java:37-61 (3.0),
    LongGreatestPostAggregatorTest.java:37-61 (6), LongLeastPostAggregatorTest.java:37-61 (3)
    ConstantPostAggregatorTest.java:33-43 (7, 0.0, 1.0)
* "numeric_first": ArithmeticPostAggregatorTest.java:160-186 testNumericFirstOrdering: the sign of
  numericFirst.compare(a, b), values in the same notation.
* "constant_compare": ConstantPostAggregatorTest.java:46-54: the constant's comparator calls everything equal.

    python tests/golden/make_post_agg_kats.py
"""
import json
import math
import os
import struct


def d(x):
    return "d:%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def l(x):
    return "l:%d" % x


NAN = "d:7ff8000000000000"


def fa(name):
    return {"type": "fieldAccess", "name": name, "fieldName": name}


def const(name, v):
    return {"type": "constant", "name": name, "value": v}


def arith(name, fn, fields, ordering=None):
    js = {"type": "arithmetic", "name": name, "fn": fn, "fields": fields}
    if ordering:
        js["ordering"] = ordering
    return js


ROKU_ROWS = [const("roku", 6.0), fa("rows")]
ROWS3 = {"rows": l(3)}

compute = [
    {"name": "testCompute +", "post": arith("add", "+", ROKU_ROWS), "aggs": {"rows": "count"}, "row": ROWS3, "value": d(9.0)},
    {"name": "testCompute -", "post": arith("subtract", "-", ROKU_ROWS), "aggs": {"rows": "count"}, "row": ROWS3,
     "value": d(3.0)},
    {"name": "testCompute *", "post": arith("multiply", "*", ROKU_ROWS), "aggs": {"rows": "count"}, "row": ROWS3,
     "value": d(18.0)},
    {"name": "testCompute /", "post": arith("divide", "/", ROKU_ROWS), "aggs": {"rows": "count"}, "row": ROWS3,
     "value": d(2.0)},
]
QUOT = arith("q", "quotient", [fa("value"), const("zero", 0)], "numericFirst")
for tag, row, want in (("0 long", l(0), NAN), ("NaN", NAN, NAN), ("1 long", l(1), d(math.inf)), ("-1 long", l(-1), d(-math.inf))):
    compute.append({"name": "testQuotient " + tag, "post": QUOT,
                    "aggs": {"value": "longSum" if row.startswith("l:") else "doubleSum"}, "row": {"value": row}, "value": want})
DIV = arith("q", "/", [fa("value"), const("denomiator", 0)])
for tag, row in (("0 long", l(0)), ("NaN", NAN), ("1 long", l(1)), ("-1 long", l(-1))):
    compute.append({"name": "testDiv " + tag, "post": DIV,
                    "aggs": {"value": "longSum" if row.startswith("l:") else "doubleSum"}, "row": {"value": row},
                    "value": d(0.0)})
for t, want in (("doubleGreatest", d(6.0)), ("doubleLeast", d(3.0)), ("longGreatest", l(6)), ("longLeast", l(3))):
    compute.append({"name": t, "post": {"type": t, "name": "x", "fields": ROKU_ROWS}, "aggs": {"rows": "count"},
                    "row": ROWS3, "value": want})
compute += [
    {"name": "constant shichi", "post": const("shichi", 7), "aggs": {}, "row": {}, "value": l(7)},
    {"name": "constant rei", "post": const("rei", 0.0), "aggs": {}, "row": {}, "value": d(0.0)},
    {"name": "constant ichi", "post": const("ichi", 1.0), "aggs": {}, "row": {}, "value": d(1.0)},
]

INF, NINF, ZERO = d(math.inf), d(-math.inf), d(0.0)
numeric_first = [
    [NAN, ZERO, -1], [INF, ZERO, -1], [NINF, ZERO, -1], [ZERO, NAN, 1], [ZERO, INF, 1], [ZERO, NINF, 1],
    [NINF, INF, -1], [INF, NINF, 1], [NAN, INF, 1], [NAN, NINF, 1], [INF, NAN, -1], [NINF, NAN, -1],
]
constant_compare = [[l(0), l(1), 0], [l(0), l(1), 0], [l(1), l(0), 0]]

if __name__ == "__main__":
    out = {"compute": compute, "numeric_first": numeric_first, "constant_compare": constant_compare}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "post_agg_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(compute), "compute cases")
