"""The merge queries of tests/querygen.py (merge_queries: every ts-* and tn-*, the gb-* that do not group by v,
the gm-* draws) over the fixture cut into four segments (querygen.piece_paths), on every plane that merges
partial results, against the CPU oracle over the same four pieces (expected_for(q, PIECES): a topN's
per-segment cut and fold order depend on the split). One test case is one query (`-k gm-017` replays it); a
mismatch names the query, its JSON, the plane, the rank split and the first differing cell. Floating sums over
d / f are compared within querygen.cell_bound, which holds for any summation order and so for any split into
pieces, parts and ranks (float32 all_reduce adds included); every other cell, the rows and their order exactly.

Plane 1, per-segment runners: what createRunner(piece).run hands to the toolchest for every piece on its own
  (factory.per_segment: the partial results before SegmentQueryRunner.run merges its single segment, since a
  per-piece merge_topn would cut to the query threshold and a per-piece merge_groupby would apply the having and
  limit specs), merged by factory.toolchest.merge and finalized: merge_timeseries, merge_topn, merge_groupby
  over four partials, each already cut by its own limit push-down.
Plane 2, two contexts on one GPU, pieces 0 and 2 on one and 1 and 3 on the other: run_query over the four
  (run_timeseries + dg_timeseries_merge, topn_per_segment + merge_topn, dg_groupby_merge_devices with every
  context a target), and groupBy once more through groupby_merge_devices with one target and with both, finished
  as GroupByQueryRunnerFactory.run_merged finishes its ranges.
Plane 3, two ranks as two threads joined by the loopback stand-in of test_merge_gpu.py, split [[p0, p1],
  [p2, p3]] and [[p0], [p1, p2, p3]]: groupBy through GroupByExchange.exchange and merge_groupby over the
  ranges in rank order, timeseries through allreduce_timeseries of every rank's run, topN through gather_topn.

Refusals are predicted from the query alone (_refusal) and asserted, never swallowed: a first/last pair and a
groupBy dimension over v in the device-side merges (the draw holds neither), a cluster key over 63 bits (it is
at most 49 here, asserted), and a topN over v in gather_topn (plane 3 only). No calendar query of this fixture
has to be split per segment (segment_queries), asserted as well, so the engine calls of plane 3 are exact.

The plan census (the last test) asserts what the whole run has passed through.

Wall time of the module on its own on an MI355X host: 93 s, of which 52 s are the generation and the oracle's
piece expectations (23 s when tests/test_querygen_gpu.py has generated the queries in the same run); the
slowest case takes 3.4 s, most take 0.1 - 0.5 s."""
import importlib
import threading

import pytest

import querygen as G
import test_merge_gpu as TM

pytestmark = pytest.mark.gpu

SPLITS = {"p0p1|p2p3": ((0, 1), (2, 3)), "p0|p1p2p3": ((0,), (1, 2, 3))}
MAX_KEY_BITS = 49  # hi 15, mid 9, hn 6, tags 4, lo 3, nope 1, and 11 bucket bits

# query id -> reason: a diagnosed engine defect kept as a strict expected failure (at most 8)
XFAIL = {}

RAN = set()
REFUSED = set()  # (query id, plane) of every refusal seen
MERGED = set()  # query ids dg_groupby_merge_devices was called for
WHERE = {"qid": None, "plane": 0}
LOCK = threading.Lock()
CENSUS = {"runs": {1: 0, 2: 0, 3: 0}, "empty_range": 0, "empty_part": 0, "range_cut": 0, "post": 0, "hash_part": 0,
          "splits": {k: 0 for k in SPLITS}}


def _refusal(Q, q, plane):
    """Why the documented rules refuse q on `plane`, or None: told from the query alone."""
    if plane == 1:
        return None
    if any(a.is_pair for a in q.aggregations) and (plane == 3 or isinstance(q, Q.GroupByQuery)):
        return "a first/last pair"
    if isinstance(q, Q.GroupByQuery):
        if "v" in q.dimensions:
            return "a groupBy dimension over the LONG column v"
        if G.sort_word_bits(q)[0] > 63:
            return "a cluster key over 63 bits"
    if isinstance(q, Q.TopNQuery) and plane == 3 and q.dimension == "v":
        return "a topN over the LONG column v across processes"
    return None


@pytest.fixture(scope="module")
def env():
    """The merge queries, the pieces attached on the default context and on two more contexts of the same GPU,
    and the engine's entry points watched for the census."""
    R = importlib.import_module("incubator-druid_amd.runners")
    S = importlib.import_module("incubator-druid_amd.segment")
    D = importlib.import_module("incubator-druid_amd.distributed")
    N = importlib.import_module("incubator-druid_amd._native")
    Q = importlib.import_module("incubator-druid_amd.query")
    G.merge_queries()
    pieces = [S.GpuSegment(p) for p in G.piece_paths()]
    ca, cb = S.GpuContext(0), S.GpuContext(0)
    two = [S.GpuSegment(p, context=ca if i % 2 == 0 else cb) for i, p in enumerate(G.piece_paths())]
    plain_run, plain_merge, plain_cut = R.groupby_run, R.groupby_merge_devices, R.GroupByResult.apply_limit_push_down

    def watched_run(segments, query, *args, **kw):
        res = plain_run(segments, query, *args, **kw)
        if WHERE["plane"] in (2, 3):  # a part of a device-side merge
            with LOCK:
                CENSUS["empty_part"] += int(res.groups == 0)
                CENSUS["hash_part"] += int(res.groups > 0 and res.grouper_info()["grouper"] == N.GROUPER_HASH)
        return res

    def watched_merge(segments, query, *args, **kw):
        res = plain_merge(segments, query, *args, **kw)
        MERGED.add(WHERE["qid"])
        CENSUS["empty_range"] += sum(int(r.groups == 0) for r in res)
        return res

    def watched_cut(self):
        before = self.groups
        done = plain_cut(self)
        if done and self.groups < before and WHERE["plane"] in (2, 3):  # a merged key range
            with LOCK:
                CENSUS["range_cut"] += 1
        return done

    R.groupby_run, R.groupby_merge_devices, R.GroupByResult.apply_limit_push_down = watched_run, watched_merge, watched_cut
    try:
        yield type("Env", (), {"R": R, "D": D, "N": N, "Q": Q, "pieces": pieces, "two": two, "targets": (ca, cb)})
    finally:
        R.groupby_run, R.groupby_merge_devices, R.GroupByResult.apply_limit_push_down = plain_run, plain_merge, plain_cut
        for s in pieces + two:
            s.close()


def _ties(stats):
    return sum(c.get("topn_cut_ties", 0) for c in stats.calls)


def _per_segment_runners(env, q):
    """Plane 1: (merged and finalized results, values a numeric topN cut among ties)."""
    R = env.R
    f, stats, partials = R.FACTORIES[type(q)], R.RunStats(), []
    for s in env.pieces:
        partials += f.per_segment([s], q, stats)
    return R.finalize_results(q, f.toolchest.merge(q, partials)), _ties(stats)


def _merge_devices(env, q, targets):
    """groupBy over the two contexts' pieces with the given range owners, finished as run_merged finishes it."""
    R = env.R
    stats = R.RunStats()
    res = R.groupby_merge_devices(env.two, q, stats, targets=targets)
    try:
        assert len(res) == len(targets)
        for r in res:
            r.apply_limit_push_down()
            if r.apply_post_process():
                stats.post.append(r.post_info)
        CENSUS["post"] += len(stats.post)
        return R.finalize_results(q, R.merge_groupby(q, [r.fetch() for r in res]))
    finally:
        for r in res:
            r.release()


def _ranks(env, split, work):
    """work(dist, the rank's pieces) on every rank of `split` at once; the ranks' return values in rank order.
    The first error that is not another rank's broken barrier is raised here."""
    hub = TM._Hub(len(split))
    out, err = [None] * len(split), [None] * len(split)

    def run(rank):
        try:
            out[rank] = work(TM.LoopbackDist(hub, rank), [env.pieces[i] for i in split[rank]])
        except BaseException as e:  # noqa: BLE001 (raised in the main thread below)
            err[rank] = e
            hub.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(len(split))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    errs = [e for e in err if e is not None]
    if errs:
        raise next((e for e in errs if not isinstance(e, threading.BrokenBarrierError)), errs[0])
    return out


def _two_ranks(env, q, split):
    """Plane 3: the cluster's result as rank 0 (topN), every rank (timeseries) or the ranges in rank order give it."""
    R, D, Q = env.R, env.D, env.Q
    if isinstance(q, Q.GroupByQuery):
        def work(dist, segs):
            ex = D.GroupByExchange(dist, q, segs)
            res = R.groupby_run(segs, q)
            try:
                merged = ex.exchange(res)
            finally:
                res.release()
            try:
                with LOCK:
                    CENSUS["empty_range"] += int(merged.groups == 0)
                return merged.fetch()
            finally:
                merged.release()
        return R.finalize_results(q, R.merge_groupby(q, _ranks(env, split, work)))
    if isinstance(q, Q.TimeseriesQuery):
        def work(dist, segs):
            return D.allreduce_timeseries(dist, q, R.run_timeseries(segs, q))
        got = _ranks(env, split, work)
        assert all(G.first_difference(q, g, got[0]) is None and len(g) == len(got[0]) for g in got[1:])  # every rank gets it
        return got[0]

    def work(dist, segs):
        gdict = D.GlobalDictionary.build(dist, [s.dictionary(q.dimension) for s in segs])
        trans = [gdict.translate(s.dictionary(q.dimension)) for s in segs]
        return D.gather_topn(dist, q, R.topn_raw(segs, q), gdict, trans, segs)
    got = _ranks(env, split, work)
    assert all(g is None for g in got[1:])
    return got[0]


def _held(env, qid, q, exp, plane, route, fn):
    """fn()'s results against exp; for a query the rules refuse on this plane, the refusal instead."""
    WHERE.update(qid=qid, plane=plane)
    try:
        why = _refusal(env.Q, q, plane)
        if why is not None:
            with pytest.raises(env.N.UnsupportedQuery):
                fn()
            REFUSED.add((qid, plane))
            return
        got = fn()
        ties = 0
        if isinstance(got, tuple):
            got, ties = got
        CENSUS["runs"][plane] += 1
        G.assert_parity(qid, q, got, exp, G.PIECES, "plane %d %s" % (plane, route), ties)
    finally:
        WHERE.update(qid=None, plane=0)


@pytest.mark.parametrize("qid", [pytest.param(qid, marks=pytest.mark.xfail(strict=True, reason=XFAIL[qid])) if qid in XFAIL
                                 else qid for qid in G.merge_ids()])
def test_merge_parity(qid, env):
    R, Q = env.R, env.Q
    q, exp = G.query(qid), G.expected_for(G.query(qid), G.PIECES)
    RAN.add(qid)
    # the fixture's calendar queries stay on the query's own bucket list: none is split per segment
    assert R.exact_granularity(q, env.pieces) is q and R.segment_queries(q, env.pieces) is None
    if isinstance(q, Q.GroupByQuery):
        assert G.sort_word_bits(q)[0] <= MAX_KEY_BITS
    _held(env, qid, q, exp, 1, "per-segment runners", lambda: _per_segment_runners(env, q))

    def merged_runner():
        stats = R.RunStats()
        got = R.run_query(q, env.two, stats)
        CENSUS["post"] += len(stats.post)
        return got, _ties(stats)
    _held(env, qid, q, exp, 2, "run_query over two contexts", merged_runner)
    if isinstance(q, Q.GroupByQuery):
        ca, cb = env.targets
        _held(env, qid, q, exp, 2, "groupby_merge_devices, one target", lambda: _merge_devices(env, q, [ca]))
        _held(env, qid, q, exp, 2, "groupby_merge_devices, two targets", lambda: _merge_devices(env, q, [ca, cb]))
    for name, split in SPLITS.items():
        _held(env, qid, q, exp, 3, "rank split " + name, lambda: _two_ranks(env, q, split))
        CENSUS["splits"][name] += 1


def test_refusal_rules(env):
    """The rules on hand-made queries (the draw holds no pair and no merge query groups by v), and the draw's
    share of them: the topN queries over v, on plane 3 only."""
    Q = env.Q
    iv = [G.WHOLE]
    pair = Q.query_from_json({"queryType": "groupBy", "dataSource": "x", "intervals": [list(G.WHOLE)], "granularity": "all",
                              "dimensions": ["lo"], "aggregations": [{"type": "longFirst", "name": "a", "fieldName": "l"}]})
    assert [_refusal(Q, pair, p) for p in (1, 2, 3)] == [None, "a first/last pair", "a first/last pair"]
    over_v = Q.GroupByQuery(intervals=iv, dimensions=["v"], aggregations=[Q.count("n")])
    assert _refusal(Q, over_v, 1) is None and _refusal(Q, over_v, 2) and _refusal(Q, over_v, 3)
    tn = Q.TopNQuery(intervals=iv, dimension="v", metric="n", threshold=3, aggregations=[Q.count("n")])
    assert [_refusal(Q, tn, p) for p in (1, 2, 3)] == [None, None, "a topN over the LONG column v across processes"]
    predicted = {(qid, p) for qid, q in G.merge_queries() for p in (1, 2, 3) if _refusal(Q, q, p)}
    assert predicted == {(qid, 3) for qid, q in G.merge_queries() if qid.startswith("tn") and q.dimension == "v"}
    # (8 draws chose v; one of them moved to a small dimension for its floating-sum metric, as _draw_topn does)
    assert len(predicted) == 7 and len([a for a in G.axes(merge=True).values() if "tn:dim:v" in a]) == 8


def test_plan_census(env):
    """Over the whole run (it follows the parametrized cases): what the planes have passed through."""
    print(CENSUS, "merged on the devices: %d queries" % len(MERGED), "refused: %d" % len(REFUSED))
    ids = G.merge_ids()
    if RAN != set(ids):
        pytest.skip("the census is of the whole module's run: %d of %d cases ran" % (len(RAN), len(ids)))
    Q = env.Q
    predicted = {(qid, p) for qid, q in G.merge_queries() for p in (1, 2, 3) if _refusal(Q, q, p)}
    assert REFUSED == predicted
    gb = len(G.merge_ids("gb")) + len(G.merge_ids("gm"))
    assert CENSUS["runs"][1] == len(ids)
    assert CENSUS["runs"][2] == len(ids) + 2 * gb
    assert CENSUS["runs"][3] == 2 * len(ids) - len(predicted) * len(SPLITS)
    assert all(n == len(ids) for n in CENSUS["splits"].values()), CENSUS["splits"]
    assert len(MERGED) >= 40, len(MERGED)
    for what in ("empty_range", "empty_part", "range_cut", "post", "hash_part"):
        assert CENSUS[what] > 0, (what, CENSUS)
