"""Writes tests/golden/first_last_kats.json: known-answer tests of the first / last aggregators.

Transcribed by hand from the reference's runner tests over the TestIndex sample data
(druid.sample.numeric.tsv; paths relative to processing/src/test/java/org/apache/druid/query/), in the
style of engine_kats.json: the query as this project's JSON and the expected results. They run on the
`sample_dirs` segment, whose rows are in (time, market, quality) order, the order of the reference's
persisted segment, so the ascending / descending tie behaviour is the reference's.

* timeseries/TimeseriesQueryRunnerTest.java:1801-1903 testTimeseriesWithFirstLastAggregator: doubleFirst /
  doubleLast over `index` by month, ascending and descending ("There's a difference between ascending and
  descending results since granularity of druid.sample.tsv is days, with multiple first and last times").
  The literals there are `new Float(x).doubleValue()`: float-rounded.
* groupby/GroupByQueryRunnerTest.java:1977-2006 testGroupByWithFirstLast: longFirst / longLast over `index`
  by market and month.
* topn/TopNQueryRunnerTest.java:827-925 testTopNOverFirstLastAggregator: longFirst / longLast over `index`,
  ordered by `last`, by month (:839-840 the factories).
* topn/TopNQueryRunnerTest.java:1052-1160 testTopNOverFirstLastFloatAggregatorUsingDoubleColumn (floatFirst /
  floatLast over the double column `index`, :1064-1065) and :1163-1270 ...UsingFloatColumn (over `indexFloat`,
  :1175-1176): the same expectations.

Left out: testTopNOverFirstLastAggregatorChunkPeriod (:938-1040, the factories at :950-951) runs the same
query under the context key chunkPeriod, which this project's runners do not read: it would repeat the
first topN case. No case here needs the multi-value dimension `placementish`, which the fixture lacks.

Doubles compare at the reference's own relative 1e-6 (tests/compare.py assert_kat, TestHelper.java:319-329).

    python tests/golden/make_first_last_kats.py
"""
import json
import os

FULL = "1970-01-01T00:00:00.000Z/2020-01-01T00:00:00.000Z"
MONTHS = ["2011-01-01T00:00:00.000Z", "2011-02-01T00:00:00.000Z", "2011-03-01T00:00:00.000Z", "2011-04-01T00:00:00.000Z"]


def agg(t, name, field):
    return {"type": t, "name": name, "fieldName": field}


def timeseries(descending):
    return {"queryType": "timeseries", "dataSource": "testing", "granularity": "month", "intervals": [FULL],
            "descending": descending, "aggregations": [agg("doubleFirst", "first", "index"), agg("doubleLast", "last", "index")]}


TS_ASC = [(100.000000, 943.497198), (132.123776, 1101.918270), (153.059937, 1063.201156), (135.885094, 780.271977)]
TS_DESC = [(1234.247546, 106.793700), (1004.940887, 151.752485), (913.561076, 122.258195), (800.000000, 133.740047)]

# (market, first, last) per month, in the groupBy's row order (market ascending)
LONGS = [
    [("spot", 100, 155), ("total_market", 1000, 1127), ("upfront", 800, 943)],
    [("spot", 132, 114), ("total_market", 1203, 1292), ("upfront", 1667, 1101)],
    [("spot", 153, 125), ("total_market", 1124, 1366), ("upfront", 1166, 1063)],
    [("spot", 135, 120), ("total_market", 1314, 1029), ("upfront", 1447, 780)],
]
FLOATS = [
    [("total_market", 1000.0, 1127.23095703125), ("upfront", 800.0, 943.4971923828125), ("spot", 100.0, 155.7449493408203)],
    [("total_market", 1203.4656, 1292.5428466796875), ("upfront", 1667.497802734375, 1101.918212890625),
     ("spot", 132.123779296875, 114.2845687866211)],
    [("total_market", 1124.2014, 1366.4476), ("upfront", 1166.1411, 1063.2012), ("spot", 153.05994, 125.83968)],
    [("total_market", 1314.8397, 1029.057), ("upfront", 1447.3412, 780.272), ("spot", 135.8851, 120.290344)],
]


def topn(kind, field):
    return {"queryType": "topN", "dataSource": "testing", "granularity": "month", "intervals": [FULL],
            "dimension": "market", "metric": "last", "threshold": 3,
            "aggregations": [agg(kind + "First", "first", field), agg(kind + "Last", "last", field)]}


def topn_expected(table, order):
    out = []
    for month, rows in zip(MONTHS, table):
        by = {m: (f, l) for m, f, l in rows}
        out.append({"timestamp": month,
                    "result": [{"market": m, "first": by[m][0], "last": by[m][1]} for m in order(rows)]})
    return out


def by_last(rows):  # the topN's own order: `last` descending
    return [m for m, _, _ in sorted(rows, key=lambda r: -r[2])]


def main():
    cases = []
    src = "timeseries/TimeseriesQueryRunnerTest.java:1801-1903"
    for name, desc, exp in (("testTimeseriesWithFirstLastAggregator[ascending]", False, list(zip(MONTHS, TS_ASC))),
                            ("testTimeseriesWithFirstLastAggregator[descending]", True, list(zip(MONTHS[::-1], TS_DESC)))):
        cases.append({"name": name, "source": src, "query": timeseries(desc),
                      "expected": [{"timestamp": t, "result": {"first": f, "last": l}} for t, (f, l) in exp]})
    cases.append({
        "name": "testGroupByWithFirstLast", "source": "groupby/GroupByQueryRunnerTest.java:1977-2006",
        "query": {"queryType": "groupBy", "dataSource": "testing", "granularity": "month", "intervals": [FULL],
                  "dimensions": ["market"],
                  "aggregations": [agg("longFirst", "first", "index"), agg("longLast", "last", "index")]},
        "expected_events": [{"timestamp": month, "event": {"market": m, "first": f, "last": l}}
                            for month, rows in zip(MONTHS, LONGS) for m, f, l in rows]})
    cases.append({"name": "testTopNOverFirstLastAggregator", "source": "topn/TopNQueryRunnerTest.java:827-925",
                  "query": topn("long", "index"), "expected": topn_expected(LONGS, by_last)})
    cases.append({"name": "testTopNOverFirstLastFloatAggregatorUsingDoubleColumn",
                  "source": "topn/TopNQueryRunnerTest.java:1052-1160", "query": topn("float", "index"),
                  "expected": topn_expected(FLOATS, lambda rows: [m for m, _, _ in rows])})
    cases.append({"name": "testTopNOverFirstLastFloatAggregatorUsingFloatColumn",
                  "source": "topn/TopNQueryRunnerTest.java:1163-1270", "query": topn("float", "indexFloat"),
                  "expected": topn_expected(FLOATS, lambda rows: [m for m, _, _ in rows])})
    out = {"_source": __doc__.split("\n\n")[1].replace("\n", " "), "cases": cases}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "first_last_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
