"""Cross-device groupBy merge through the C-ABI (dg_result_export / dg_keys_partition / dg_merge),
QueryRunnerFactory.mergeRunners over devices with GroupByMergingQueryRunnerV2 semantics.

The product exchange (distributed.GroupByExchange: cluster dictionaries, key space, sampled
splitters, all_to_all of counts and records, device merge) runs here with two "ranks" as two threads
of one process on one GPU, joined by a loopback stand-in for torch.distributed (tests only; the
driver's multi-GPU bench runs the same code over RCCL). The concatenated key ranges must equal the
oracle's merged result over all segments: ~1.2M groups with 3-byte ids and per-rank dictionaries,
NaN / -0.0 Math.min/max, floatSum float adds, granularity buckets spanning both ranks."""
import importlib
import threading

import numpy as np
import pytest

from compare import TOL, assert_results

pytestmark = pytest.mark.gpu

IV = ["1970-01-01/2020-01-01"]


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("incubator-druid_amd.segment")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("incubator-druid_amd.distributed")


class _Hub:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world


class LoopbackDist:
    """torch.distributed's collectives as the exchange uses them, between threads (test harness)."""

    def __init__(self, hub, rank):
        self.hub, self.rank = hub, rank

    def get_world_size(self):
        return self.hub.world

    def get_rank(self):
        return self.rank

    def get_backend(self):
        return "nccl"  # tensors live on the GPU

    def _exchange(self, obj):
        self.hub.barrier.wait()
        self.hub.slots[self.rank] = obj
        self.hub.barrier.wait()
        got = list(self.hub.slots)
        self.hub.barrier.wait()
        return got

    def all_gather_object(self, out, obj):
        out[:] = self._exchange(obj)

    def all_gather(self, bufs, t):
        for b, x in zip(bufs, self._exchange(t.clone())):
            b.copy_(x)

    class ReduceOp:
        SUM, MIN, MAX = "sum", "min", "max"

    def all_reduce(self, t, op=ReduceOp.SUM):
        """In place, folded in rank order in the tensor's own type (a float32 sum adds in float32)."""
        import torch
        got = self._exchange(t.clone())
        acc = got[0].clone()
        for x in got[1:]:
            acc = acc + x if op == self.ReduceOp.SUM else (torch.minimum if op == self.ReduceOp.MIN else torch.maximum)(acc, x)
        t.copy_(acc)

    def all_to_all_single(self, out, inp, out_splits=None, in_splits=None):
        import torch
        w = self.hub.world
        if in_splits is None:
            in_splits = [inp.numel() // w] * w
        offs = np.concatenate([[0], np.cumsum(in_splits)]).astype(np.int64)
        pieces = [inp[int(offs[r]):int(offs[r + 1])].clone() for r in range(w)]
        got = self._exchange(pieces)
        mine = [got[src][self.rank] for src in range(w)]
        if mine and sum(p.numel() for p in mine):
            out.copy_(torch.cat(mine))


def _run_ranks(R, D, Q, rank_segs, query):
    """Each rank: dg_groupby_run over its segments, then the exchange; returns the ranges in rank order."""
    hub = _Hub(len(rank_segs))
    out, err = [None] * len(rank_segs), []

    def work(rank):
        try:
            dist = LoopbackDist(hub, rank)
            ex = D.GroupByExchange(dist, query, rank_segs[rank])
            res = R.groupby_run(rank_segs[rank], query)
            merged = ex.exchange(res)
            res.release()
            out[rank] = merged.fetch()
            merged.release()
        except Exception as e:  # surface in the main thread
            err.append(e)
            hub.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(len(rank_segs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if err:
        raise err[0]
    return out


def _rows(Q, query, parts):
    rows = []
    for p in parts:
        for r in range(len(p)):
            ev = {d: p.dims[i][r] for i, d in enumerate(query.dimensions)}
            for a, col in zip(query.aggregations, p.aggs):
                ev[a.name] = importlib.import_module("incubator-druid_amd.runners")._py(col[r], a.output_type)
            rows.append(Q.Row(int(p.times[r]), ev))
    return rows


@pytest.fixture(scope="module")
def special_dirs(tmp_path_factory, DG, W):
    import test_distributed as TD
    return TD._write_dataset(DG, W, str(tmp_path_factory.mktemp("merge_special")), 4, 30_000)


def _special_aggs(Q):
    return [Q.count("rows"), Q.long_sum("sumLongSequential"), Q.double_sum("sumFloatNormal"),
            Q.float_sum("fsum", "sumFloatNormal"),
            Q.AggregatorFactory("doubleMin", "sdmin", "specialDouble"),
            Q.AggregatorFactory("doubleMax", "sdmax", "specialDouble"),
            Q.AggregatorFactory("floatMin", "sfmin", "specialFloat"),
            Q.AggregatorFactory("floatMax", "sfmax", "specialFloat"),
            Q.AggregatorFactory("longMin", "lmin", "maxLongUniform")]


@pytest.mark.parametrize("name", ["all_zipf", "uniform_seq", "minute", "uneven_ranks"])
def test_two_rank_exchange_matches_oracle(R, S, D, Q, O, special_dirs, name):
    g = [S.GpuSegment(p) for p in special_dirs]
    o = [O.OracleSegment(p) for p in special_dirs]
    aggs = _special_aggs(Q)
    if name == "all_zipf":
        q = Q.GroupByQuery(intervals=IV, dimensions=["dimZipf"], aggregations=aggs)
    elif name == "uniform_seq":
        q = Q.GroupByQuery(intervals=IV, dimensions=["dimUniform", "dimSequential"], aggregations=aggs)
    elif name == "minute":
        q = Q.GroupByQuery(intervals=IV, granularity="minute", dimensions=["dimZipf", "dimNull"], aggregations=aggs,
                           filter=Q.BoundDimFilter("dimSequential", "100", "400"))
    else:  # 1 segment on rank 0, 3 on rank 1
        q = Q.GroupByQuery(intervals=IV, dimensions=["dimSequential"], aggregations=aggs,
                           filter=Q.SelectorDimFilter("dimSequential", "5"))
    rank_segs = [g[:2], g[2:]] if name != "uneven_ranks" else [g[:1], g[1:]]
    parts = _run_ranks(R, D, Q, rank_segs, q)
    assert_results(q, _rows(Q, q, parts), O.run(q, o))


@pytest.fixture(scope="module")
def cfg3_ranks(tmp_path_factory, DG, S, O):
    """Config 3's shape: dimUniform (~100k values) x dimHyperUnique, 3-byte ids, 2 ranks x 2 x 300k
    rows, different dictionaries per segment -> ~1.2M groups across the cluster."""
    base = tmp_path_factory.mktemp("merge_cfg3")
    paths = DG.write_basic_dataset(str(base), 4, 300_000, lz4_mode="fast",
                                   dims=["dimUniform", "dimHyperUnique"],
                                   metrics=["sumLongSequential", "sumFloatNormal", "minFloatZipf"])
    return [S.GpuSegment(p) for p in paths], [O.OracleSegment(p) for p in paths]


def test_two_rank_exchange_million_groups(R, D, Q, O, cfg3_ranks):
    g, o = cfg3_ranks
    aggs = [Q.count("rows"), Q.long_sum("sumLongSequential"), Q.double_sum("sumFloatNormal"),
            Q.AggregatorFactory("doubleMin", "dmin", "minFloatZipf")]
    q = Q.GroupByQuery(intervals=IV, dimensions=["dimUniform", "dimHyperUnique"], aggregations=aggs)
    parts = _run_ranks(R, D, Q, [g[:2], g[2:]], q)
    assert all(len(p) > 200_000 for p in parts)  # the splitters balance the ranges
    exp = O.run(q, o)
    assert sum(len(p) for p in parts) == len(exp) > 1_000_000
    keys = [tuple(r.event[d] for d in q.dimensions) for r in exp]
    got_keys = [k for p in parts for k in zip(*[list(c) for c in p.dims])]
    assert got_keys == keys
    for i, a in enumerate(aggs):
        col = np.concatenate([p.aggs[i] for p in parts])
        e = np.array([r.event[a.name] for r in exp])
        if a.type == "doubleSum":
            assert np.allclose(col, e, rtol=TOL["double"], atol=0)
        else:
            assert np.array_equal(col, e.astype(col.dtype)), a.name
