"""Writes tests/golden/search_kats.json: the search query's known-answer tests.

Transcribed by hand from the reference's search tests (paths relative to the reference root,
processing/src/test/java/org/apache/druid/query/search/):

* "runner": SearchQueryRunnerTest.java:129-590 over the TestIndex sample data (druid.sample.numeric.tsv):
  the query as this project's JSON and the expected hits [dimension, value, count]
  (checkSearchQuery compares them as a multiset and the result timestamp, :782-811). "segment" tells
  which fixture the case needs: "sample" (the string dimensions of make_sample_segment.py) or
  "placementish" (the same rows with the multi-value dimension placementish, TSV column 8).
  Cases with an extraction function or a numeric / __time search dimension are left out.
* "with_case": SearchQueryRunnerWithCaseTest.java:78-234: its four rows and, per query, the expected
  set of values per dimension.
* "binary_fn": SearchBinaryFnTest.java:56-404: merge inputs and outputs (a hit without a count is
  [dimension, value]); toHits sorts its arguments by the comparator, so "sorted": true inputs are
  listed unsorted here as there. Timestamps: 0 stands for the test's currTime.
* "sort_spec": SearchSortSpecTest.java:34-95: the sign of compare(a, b).

    python tests/golden/make_search_kats.py
"""
import json
import os

FULL = "1970-01-01T00:00:00.000Z/2020-01-01T00:00:00.000Z"
Q, M, PL, PLISH, PN = "quality", "market", "placement", "placementish", "partial_null_column"


def sel(d, v):
    return {"type": "selector", "dimension": d, "value": v}


def AND(*fs):
    return {"type": "and", "fields": list(fs)}


def OR(*fs):
    return {"type": "or", "fields": list(fs)}


def ic(v):
    return {"type": "insensitive_contains", "value": v}


QUALITY_A = [[Q, "automotive", 93], [Q, "mezzanine", 279], [Q, "travel", 93], [Q, "health", 93],
             [Q, "entertainment", 93]]
MARKET_A = [[M, "total_market", 186]]

RUNNER = [
    {"name": "testSearch", "segment": "placementish", "query": ic("a"),
     "hits": QUALITY_A + MARKET_A + [[PLISH, "a", 93], [PN, "value", 186]]},
    {"name": "testSearchSameValueInMultiDims", "segment": "placementish", "searchDimensions": [PL, PLISH],
     "query": ic("e"), "hits": [[PL, "preferred", 1209], [PLISH, "e", 93], [PLISH, "preferred", 1209]]},
    {"name": "testSearchSameValueInMultiDims2", "segment": "placementish", "searchDimensions": [PL, PLISH],
     "query": ic("e"), "sort": "strlen",
     "hits": [[PLISH, "e", 93], [PL, "preferred", 1209], [PLISH, "preferred", 1209]], "ordered": True},
    {"name": "testFragmentSearch", "segment": "sample", "query": {"type": "fragment", "values": ["auto", "ve"]},
     "hits": [[Q, "automotive", 93]]},
    {"name": "testSearchWithDimensionQuality", "segment": "sample", "searchDimensions": [Q], "query": ic("a"),
     "hits": QUALITY_A},
    {"name": "testSearchWithDimensionProvider", "segment": "sample", "searchDimensions": [M], "query": ic("a"),
     "hits": MARKET_A},
    {"name": "testSearchWithDimensionsQualityAndProvider", "segment": "sample", "searchDimensions": [Q, M],
     "query": ic("a"), "hits": QUALITY_A + MARKET_A},
    {"name": "testSearchWithDimensionsPlacementAndProvider", "segment": "sample", "searchDimensions": [PLISH, M],
     "query": ic("mark"), "hits": MARKET_A},
    {"name": "testSearchWithSingleFilter1", "segment": "sample", "searchDimensions": [Q], "query": ic("a"),
     "filter": AND(sel(M, "total_market"), sel(Q, "mezzanine")), "hits": [[Q, "mezzanine", 93]]},
    {"name": "testSearchWithSingleFilter2", "segment": "sample", "searchDimensions": [M], "query": ic("a"),
     "filter": sel(M, "total_market"), "hits": MARKET_A},
    {"name": "testSearchMultiAndFilter", "segment": "sample", "searchDimensions": [Q], "query": ic("a"),
     "filter": AND(sel(M, "spot"), sel(Q, "automotive")), "hits": [[Q, "automotive", 93]]},
    {"name": "testSearchWithMultiOrFilter", "segment": "sample", "searchDimensions": [Q], "query": ic("a"),
     "filter": OR(sel(Q, "total_market"), sel(Q, "automotive")), "hits": [[Q, "automotive", 93]]},
    {"name": "testSearchWithEmptyResults", "segment": "sample", "query": ic("abcd123"), "hits": []},
    {"name": "testSearchWithFilterEmptyResults", "segment": "sample", "query": ic("a"),
     "filter": AND(sel(M, "total_market"), sel(Q, "automotive")), "hits": []},
    {"name": "testSearchNonExistingDimension", "segment": "sample", "searchDimensions": ["does_not_exist"],
     "query": ic("a"), "hits": []},
    {"name": "testSearchAll", "segment": "sample", "searchDimensions": [M], "query": ic(""),
     "hits": [[M, "spot", 837], [M, "total_market", 186], [M, "upfront", 186]]},
    {"name": "testSearchAll_noSpec", "segment": "sample", "searchDimensions": [M], "query": None,
     "hits": [[M, "spot", 837], [M, "total_market", 186], [M, "upfront", 186]]},
    {"name": "testSearchWithNumericSort", "segment": "placementish", "query": ic("a"), "sort": "numeric",
     "hits": [[PLISH, "a", 93], [Q, "automotive", 93], [Q, "entertainment", 93], [Q, "health", 93],
              [Q, "mezzanine", 279], [M, "total_market", 186], [Q, "travel", 93], [PN, "value", 186]],
     "ordered": True},
]

# timestamp, market, quality, placement, placementish (multi-value)
CASE_ROWS = [
    ["2011-01-12T00:00:00.000Z", "spot", "AutoMotive", "PREFERRED", ["a", "preferred"]],
    ["2011-01-12T00:00:00.000Z", "SPot", "business", "preferred", ["b", "Preferred"]],
    ["2011-01-12T00:00:00.000Z", "spot", "entertainment", "PREFERRed", ["e", "preferred"]],
    ["2011-01-13T00:00:00.000Z", "spot", "automotive", "preferred", ["a", "preferred"]],
]


def cs(v):
    return {"type": "contains", "value": v, "caseSensitive": True}


WITH_CASE = {
    "rows": CASE_ROWS,
    "cases": [
        {"name": "testSearch_SPOT", "query": ic("SPOT"), "expected": {M: ["spot", "SPot"]}},
        {"name": "testSearch_spot_cs", "query": cs("spot"), "expected": {M: ["spot"]}},
        {"name": "testSearch_SPot_cs", "query": cs("SPot"), "expected": {M: ["SPot"]}},
        {"name": "testSearchSameValueInMultiDims", "searchDimensions": [PL, PLISH], "query": ic("PREFERRED"),
         "expected": {PL: ["PREFERRED", "preferred", "PREFERRed"], PLISH: ["preferred", "Preferred"]}},
        {"name": "testSearchSameValueInMultiDims_cs", "searchDimensions": [PL, PLISH], "query": cs("preferred"),
         "expected": {PL: ["preferred"], PLISH: ["preferred"]}},
        {"name": "testSearchIntervals", "searchDimensions": [Q], "query": ic("otive"),
         "intervals": "2011-01-12T00:00:00.000Z/2011-01-13T00:00:00.000Z", "expected": {Q: ["AutoMotive"]}},
        {"name": "testSearchNoOverrappingIntervals", "searchDimensions": [Q], "query": ic("business"),
         "intervals": "2011-01-10T00:00:00.000Z/2011-01-11T00:00:00.000Z", "expected": {Q: []}},
        {"name": "testFragmentSearch", "query": {"type": "fragment", "values": ["auto", "ve"]},
         "expected": {Q: ["automotive", "AutoMotive"]}},
        {"name": "testFragmentSearch_cs", "query": {"type": "fragment", "values": ["auto", "ve"], "caseSensitive": True},
         "expected": {Q: ["automotive"]}},
    ],
}

HOUR = 3600 * 1000
DAY_TS = 1500000000000 + 12345  # a stand-in for currTime that is not on a day boundary
BINARY_FN = [
    {"name": "testMerge", "sort": "lexicographic", "granularity": "all", "limit": 2147483647,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": {"ts": 0, "hits": [["blah2", "foo2"]]},
     "expected": {"ts": 0, "hits": [["blah", "foo"], ["blah2", "foo2"]]}},
    {"name": "testMergeDay", "sort": "lexicographic", "granularity": "day", "limit": 2147483647,
     "r1": {"ts": DAY_TS, "hits": [["blah", "foo"]]}, "r2": {"ts": DAY_TS, "hits": [["blah2", "foo2"]]},
     "expected": {"ts": DAY_TS - DAY_TS % (24 * HOUR), "hits": [["blah", "foo"], ["blah2", "foo2"]]}},
    {"name": "testMergeOneResultNull", "sort": "lexicographic", "granularity": "all", "limit": 2147483647,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": None, "expected": {"ts": 0, "hits": [["blah", "foo"]]}},
    {"name": "testMergeShiftedTimestamp", "sort": "lexicographic", "granularity": "all", "limit": 2147483647,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": {"ts": 2 * HOUR, "hits": [["blah2", "foo2"]]},
     "expected": {"ts": 0, "hits": [["blah", "foo"], ["blah2", "foo2"]]}},
    {"name": "testStrlenMerge", "sort": "strlen", "granularity": "all", "limit": 2147483647, "sorted": True,
     "r1": {"ts": 0, "hits": [["blah", "thisislong"]]}, "r2": {"ts": 0, "hits": [["blah", "short"]]},
     "expected": {"ts": 0, "hits": [["blah", "short"], ["blah", "thisislong"]]}},
    {"name": "testStrlenMerge2", "sort": "strlen", "granularity": "all", "limit": 2147483647, "sorted": True,
     "r1": {"ts": 0, "hits": [["blah", "short"], ["blah", "thisislong"], ["blah2", "thisislong"]]},
     "r2": {"ts": 0, "hits": [["blah", "short"], ["blah2", "thisislong"]]},
     "expected": {"ts": 0, "hits": [["blah", "short"], ["blah", "thisislong"], ["blah2", "thisislong"]]}},
    {"name": "testAlphanumericMerge", "sort": "alphanumeric", "granularity": "all", "limit": 2147483647, "sorted": True,
     "r1": {"ts": 0, "hits": [["blah", "a100"], ["blah", "a9"], ["alah", "a100"]]},
     "r2": {"ts": 0, "hits": [["blah", "b0"], ["alah", "c3"]]},
     "expected": {"ts": 0, "hits": [["blah", "a9"], ["alah", "a100"], ["blah", "a100"], ["blah", "b0"], ["alah", "c3"]]}},
    {"name": "testMergeUniqueResults", "sort": "lexicographic", "granularity": "all", "limit": 2147483647,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": {"ts": 0, "hits": [["blah", "foo"]]},
     "expected": {"ts": 0, "hits": [["blah", "foo"]]}},
    {"name": "testMergeLimit", "sort": "lexicographic", "granularity": "all", "limit": 1,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": {"ts": 0, "hits": [["blah2", "foo2"]]},
     "expected": {"ts": 0, "hits": [["blah", "foo"]]}},
    {"name": "testMergeCountWithNull", "sort": "lexicographic", "granularity": "all", "limit": 2147483647,
     "r1": {"ts": 0, "hits": [["blah", "foo"]]}, "r2": {"ts": 0, "hits": [["blah", "foo", 3]]},
     "expected": {"ts": 0, "hits": [["blah", "foo"]]}},
]

SORT_SPEC = [
    {"sort": "lexicographic", "a": ["test", "banana"], "b": ["test", "banana"], "sign": 0},
    {"sort": "lexicographic", "a": ["test", "banana"], "b": ["test", "apple"], "sign": 1},
    {"sort": "lexicographic", "a": ["test", "apple"], "b": ["test", "banana"], "sign": -1},
    {"sort": "alphanumeric", "a": ["test", "a100"], "b": ["test", "a9"], "sign": 1},
    {"sort": "alphanumeric", "a": ["test", "b0"], "b": ["test", "a100"], "sign": 1},
    {"sort": "alphanumeric", "a": ["test", "b0"], "b": ["test", "a9"], "sign": 1},
    {"sort": "numeric", "a": ["test", "1001001.12412"], "b": ["test", "-1421"], "sign": 1},
    {"sort": "numeric", "a": ["test", "not-numeric-at-all"], "b": ["test", "1001001.12412"], "sign": -1},
    {"sort": "numeric", "a": ["test", "not-numeric-at-all"], "b": ["test", "-1421"], "sign": -1},
    {"sort": "numeric", "a": ["test", "1001001.12412"], "b": ["best", "1001001.12412"], "sign": 1},
    {"sort": "lexicographic", "a": ["test", "apple"], "b": ["test", "banana"], "sign": -1},
    {"sort": "lexicographic", "a": ["test", "orange"], "b": ["test", "apple"], "sign": 1},
    {"sort": "lexicographic", "a": ["test", "orange"], "b": ["test", "banana"], "sign": 1},
    {"sort": "lexicographic", "a": ["test", "apple"], "b": ["test", "apple"], "sign": 0},
]


def main():
    out = {"intervals": FULL, "timestamp": "2011-01-12T00:00:00.000Z", "runner": RUNNER, "with_case": WITH_CASE,
           "binary_fn": BINARY_FN, "sort_spec": SORT_SPEC}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
