"""Writes tests/golden/scan_kats.json: the scan query's known-answer tests.

Transcribed by hand from the reference's processing/src/test/java/org/apache/druid/query/scan/
ScanQueryRunnerTest.java (paths relative to the reference root) over the TestIndex sample data
(druid.sample.numeric.tsv, the rows of 2011-01-12 and 2011-01-13: V_0112 / V_0113, :76-105):

* testSelectWithDimsAndMets (:281-312) and ...AsCompactedList (:315-347): columns market, index; the
  builder's limit 3 (newTestQuery, :140-148).
* testFullOnSelectWithFilterAndLimit (:350-406): market = spot, columns quality, index, limits 3, 1, 5, 7, 0.
* testFullSelectNoResults (:466-485): a filter no row passes -> no batch at all.
* testFullSelectNoDimensionAndMetric (:488-510): columns foo, foo2 the segment lacks -> null in every row.
* testSelectWithUnderscoreUnderscoreTime (:234-278): columns __time, market, index.

Each with legacy false and true (the test's second parameter, :117-129): in legacy mode the column
list gets "timestamp" in front (ScanQueryEngine.java:88-90) and its value is the row's time as a
DateTime, written here as its ISO instant. The reference runs every query over one segment, so a case
expects one batch (or none); "events" are restricted to the result's columns, in row order (toExpected
takes the first `limit` of the interval's rows, :635-659; limit 0 = all). A compacted case lists the
same events; the test turns them into lists in "columns" order.

    python tests/golden/make_scan_kats.py
"""
import json
import os

I_0112_0114 = "2011-01-12T00:00:00.000Z/2011-01-14T00:00:00.000Z"
MARKETS = ["spot"] * 9 + ["total_market"] * 2 + ["upfront"] * 2
QUALITIES = ["automotive", "business", "entertainment", "health", "mezzanine", "news", "premium", "technology",
             "travel", "mezzanine", "premium", "mezzanine", "premium"]
INDEX_0112 = [100.0] * 9 + [1000.0, 1000.0, 800.0, 800.0]
INDEX_0113 = [94.874713, 103.629399, 110.087299, 114.947403, 104.465767, 102.851683, 108.863011, 111.356672,
              106.236928, 1040.945505, 1689.012875, 826.060182, 1564.617729]
T_0112, T_0113 = "2011-01-12T00:00:00.000Z", "2011-01-13T00:00:00.000Z"
MS = {T_0112: 1294790400000, T_0113: 1294876800000}

ROWS = [{"t": t, "market": m, "quality": q, "index": x}
        for t, xs in ((T_0112, INDEX_0112), (T_0113, INDEX_0113))
        for m, q, x in zip(MARKETS, QUALITIES, xs)]


def event(row, columns, legacy):
    ev = {}
    for c in columns:
        if c == "timestamp" and legacy:
            ev[c] = row["t"]
        elif c == "__time":
            ev[c] = MS[row["t"]]
        else:
            ev[c] = row.get(c)  # (foo / foo2: null)
    return ev


def case(name, legacy, columns, limit, rows, flt=None, compacted=False):
    out_cols = (["timestamp"] if legacy and "timestamp" not in columns else []) + list(columns)
    q = {"queryType": "scan", "dataSource": "testing", "intervals": [I_0112_0114], "columns": list(columns),
         "limit": limit, "legacy": legacy}
    if flt is not None:
        q["filter"] = flt
    if compacted:
        q["resultFormat"] = "compactedList"
    kept = rows if limit == 0 else rows[:limit]
    return {"name": name, "legacy": legacy, "query": q, "columns": out_cols,
            "events": [event(r, out_cols, legacy) for r in kept]}


def sel(d, v):
    return {"type": "selector", "dimension": d, "value": v}


def build():
    cases = []
    spot = [r for r in ROWS if r["market"] == "spot"]
    for legacy in (False, True):
        cases.append(case("testSelectWithDimsAndMets", legacy, ["market", "index"], 3, ROWS))
        cases.append(case("testSelectWithDimsAndMetsAsCompactedList", legacy, ["market", "index"], 3, ROWS,
                          compacted=True))
        for limit in (3, 1, 5, 7, 0):
            cases.append(case(f"testFullOnSelectWithFilterAndLimit[{limit}]", legacy, ["quality", "index"], limit, spot,
                              flt=sel("market", "spot")))
        no = case("testFullSelectNoResults", legacy, [], 3, [],
                  flt={"type": "and", "fields": [sel("market", "spot"), sel("market", "foo")]})
        no["columns"] = None  # (the default column list; no batch is returned to carry one)
        cases.append(no)
        cases.append(case("testFullSelectNoDimensionAndMetric", legacy, ["foo", "foo2"], 3, ROWS))
        cases.append(case("testSelectWithUnderscoreUnderscoreTime", legacy, ["__time", "market", "index"], 3, ROWS))
    return {"segmentId_note": "the reference's QueryRunnerTestHelper.segmentId; here GpuSegment.identifier",
            "cases": cases}


def main():
    out = build()
    cases = out["cases"]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(cases), "cases")


if __name__ == "__main__":
    main()
