"""Every query of tests/querygen.py on the GPU against the CPU oracle: on the default plan over the three
segment layouts, and on layout 0 once more per alternate plan, one switch at a time. One test case is one
query (`-k gb-017` replays it); a mismatch names the query, its JSON, the layout, the switch and the first
differing cell. Floating sums over d / f are compared within the derived bound of querygen.cell_bound, every
other cell exactly; that bound replaces the 1e-9 / 1e-5 relative rule of tests/compare.py in these tests only.

Switches, each confirmed to be read where the comment says:
* timeseries: DG_NO_FUSE (dg_engine.cpp, per call), DG_NO_TIME_SKIP (per call);
* topN: DG_NO_TOPN_INDEX (per call);
* groupBy: DG_NO_FUSED_KEYGEN, DG_NO_COUNT_TOTALS, DG_NO_SIDE, DG_GB_DEFER_BITS=0, DG_GB_DEFER_PASSES=1,
  DG_GROUPER=hash / sort (all in dg_groupby_run, per call), DG_SORT_WIDE_STATUS (dg_sort.hip, per sort);
* DG_NO_RUN_DECODE, DG_NO_FLOW_DECODE: read when a segment is attached (dg_segment.cpp decode_routes), so a
  second and third copy of layout 0 are attached under them and run the timeseries and groupBy queries.
None of the listed switches had to be dropped.

The plan census (the last test) asserts what the whole run has passed through: the hash grouper, the sort
grouper with and without deferred key bits (dg_debug_groupby_sort_plan), calls with and without decoder-fused
blocks (dg_metrics.lz4_fused_blocks), the key + reference sort words and the device-side having / limit step
(dg_result_post_process, RunStats.post). The word form is not exposed by the engine: it is told from
dg_metrics.key_bits and the call's rows as the engine's own rule does (key bits + reference bits > 64)."""
import ctypes
import importlib
import os

import pytest

import querygen as G

pytestmark = pytest.mark.gpu

ROUTES = {"ts": [{"DG_NO_FUSE": "1"}, {"DG_NO_TIME_SKIP": "1"}],
          "tn": [{"DG_NO_TOPN_INDEX": "1"}],
          "gb": [{"DG_NO_FUSED_KEYGEN": "1"}, {"DG_NO_COUNT_TOTALS": "1"}, {"DG_NO_SIDE": "1"}, {"DG_SORT_WIDE_STATUS": "1"},
                 {"DG_GB_DEFER_BITS": "0"}, {"DG_GB_DEFER_PASSES": "1"}, {"DG_GROUPER": "hash"}, {"DG_GROUPER": "sort"}]}
ATTACH_ROUTES = ({"DG_NO_RUN_DECODE": "1"}, {"DG_NO_FLOW_DECODE": "1"})  # for ts and gb
SWITCHES = sorted({k for rs in ROUTES.values() for r in rs for k in r} | {k for r in ATTACH_ROUTES for k in r})

# query id -> reason: a diagnosed engine defect kept as a strict expected failure (at most 8)
XFAIL = {}

RAN = set()
CENSUS = {"hash": 0, "sort_deferred": 0, "sort_classic": 0, "fused": 0, "unfused": 0, "key_ref": 0, "post": 0, "runs": 0}


def _route_name(route):
    return ",".join(f"{k}={v}" for k, v in route.items())


@pytest.fixture(scope="module")
def env():
    """The generated queries with their expectations, the three layouts attached, two more copies of layout
    0 attached under the decoder switches, and R.groupby_run watched for the census."""
    R = importlib.import_module("incubator-druid_amd.runners")
    S = importlib.import_module("incubator-druid_amd.segment")
    N = importlib.import_module("incubator-druid_amd._native")
    for k in SWITCHES:
        os.environ.pop(k, None)
    G.queries()
    layouts = [[S.GpuSegment(p) for p in G.layout_paths(k)] for k in range(len(G.LAYOUTS))]
    attached = {}
    for route in ATTACH_ROUTES:
        os.environ.update(route)
        try:
            attached[_route_name(route)] = [S.GpuSegment(p) for p in G.layout_paths(0)]
        finally:
            for k in route:
                del os.environ[k]
    plain = R.groupby_run

    def watched(segments, query, *args, **kw):
        res = plain(segments, query, *args, **kw)
        plan = (ctypes.c_int32 * 3)(-1, -1, -1)
        N.check(N.lib().dg_debug_groupby_sort_plan(segments[0].context.handle, plan))
        if res.grouper_info()["grouper"] == N.GROUPER_HASH:
            CENSUS["hash"] += 1
        elif plan[0] > 0:
            CENSUS["sort_deferred" if plan[1] > 0 else "sort_classic"] += 1
        return res

    R.groupby_run = watched
    try:
        yield type("Env", (), {"R": R, "layouts": layouts, "attached": attached})
    finally:
        R.groupby_run = plain
        for segs in layouts + list(attached.values()):
            for s in segs:
                s.close()


def _run(env, monkeypatch, q, segs, route):
    """q over segs with the route's switches set: (results, values a numeric topN cut among ties)."""
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    try:
        stats = env.R.RunStats()
        got = env.R.run_query(q, segs, stats)
    finally:
        for k in route:
            monkeypatch.delenv(k)
    rows = sum(s.num_rows for s in segs)
    CENSUS["runs"] += 1
    for c in stats.calls:
        CENSUS["fused" if c["lz4_fused_blocks"] > 0 else "unfused"] += 1
        if c["sort_passes"] > 0 and c["key_bits"] + G.bits_for(rows) > 64:
            CENSUS["key_ref"] += 1
    CENSUS["post"] += len(stats.post)
    return got, sum(c.get("topn_cut_ties", 0) for c in stats.calls)


@pytest.mark.parametrize("qid", [pytest.param(qid, marks=pytest.mark.xfail(strict=True, reason=XFAIL[qid])) if qid in XFAIL
                                 else qid for qid in G.ids()])
def test_parity(qid, env, monkeypatch):
    q, exp, kind = G.query(qid), G.expected(qid), qid[:2]
    RAN.add(qid)
    for k, segs in enumerate(env.layouts):
        got, ties = _run(env, monkeypatch, q, segs, {})
        G.assert_parity(qid, q, got, exp, G.LAYOUTS[k], "", ties)
    for route in ROUTES[kind]:
        got, ties = _run(env, monkeypatch, q, env.layouts[0], route)
        G.assert_parity(qid, q, got, exp, G.LAYOUTS[0], _route_name(route), ties)
    if kind != "tn":
        for name, segs in env.attached.items():
            got, ties = _run(env, monkeypatch, q, segs, {})
            G.assert_parity(qid, q, got, exp, G.LAYOUTS[0], name + " at attach", ties)


def test_plan_census(env):
    """Over the whole run (it follows the parametrized cases) every plan was taken at least once."""
    print(CENSUS)
    if RAN != set(G.ids()):
        pytest.skip("the census is of the whole module's run: %d of %d cases ran" % (len(RAN), len(G.ids())))
    assert CENSUS["runs"] >= len(G.ids()) * 4
    assert not [k for k, n in CENSUS.items() if n == 0], CENSUS
