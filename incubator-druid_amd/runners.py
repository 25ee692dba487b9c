"""Query runners: the QueryRunnerFactory / QueryToolChest surface over the GPU engine.

Mirrors the reference's per-segment runner + merge structure:

* ``TimeseriesQueryRunnerFactory`` (query/timeseries/TimeseriesQueryRunnerFactory.java:66-105):
  ``createRunner(segment)`` -> per-segment results (one Result per granularity bucket,
  TimeseriesQueryEngine.java:57-111); ``mergeRunners`` -> results combined per bucket with
  ``AggregatorFactory.combine`` (TimeseriesBinaryFn.java:55-81).
* ``TopNQueryRunnerFactory`` (query/topn/TopNQueryRunnerFactory.java:61-90): per-segment top
  ``max(threshold, minTopNThreshold)`` (TopNQueryQueryToolChest.java:553-561) from the GPU, merged
  pairwise by TopNBinaryFn (TopNBinaryFn.java:75-135) with the query threshold, then truncated.
* ``GroupByQueryRunnerFactory`` (GroupByStrategyV2.process/mergeRunners, GroupByStrategyV2.java:453-477):
  per-segment grouping on the GPU, merged by dimension values (GroupByMergingQueryRunnerV2.java:170-290)
  and ordered by timestamp then dimension values.

* ``SearchQueryRunnerFactory`` (query/search/SearchQueryRunnerFactory.java): per-segment hit counts from the
  GPU (dg_search_run), the limit logic of SearchQueryRunner.run (SearchQueryRunner.java:207-260) over them,
  merged by SearchBinaryFn (SearchBinaryFn.java:53-117).

* ``ScanQueryRunnerFactory`` (query/scan/ScanQueryRunnerFactory.java:64-96): the selected rows' column
  values gathered on the GPU (dg_rows_run) into a resident rowset, cut on the host into ScanResultValue
  batches (ScanQueryEngine.java:162-236); the merged runner concatenates the segments' batches under one
  running count.

Segments that share a device are executed as ONE batched native call (all their rows in one
launch sequence); results are still kept per segment and merged exactly like the reference merges
per-segment runners. Cross-device / cross-rank merging is in distributed.py.
"""
from __future__ import annotations

import ctypes
import time
import dataclasses
import heapq
import math
from collections import OrderedDict, defaultdict
from decimal import Decimal
from fractions import Fraction
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from . import ordering as O
from . import query as Q
from . import virtual as V
from .segment import GpuSegment


# ----------------------------------------------------------------------------------------------
# slot decoding
# ----------------------------------------------------------------------------------------------
def _native_width(query) -> int:
    """Slots per record of a native call: one per aggregator, two per first/last aggregator (the pair's
    value, then its time: make_scan's DG_AGG_PAIR_TIME entry)."""
    return sum(2 if a.is_pair else 1 for a in query.aggregations)


def _decode_slots(aggs: Sequence[Q.AggregatorFactory], slots: np.ndarray) -> List[np.ndarray]:
    """[n, native width] uint64 ABI slots -> one typed column per aggregator; a first/last aggregator's
    column holds SerializablePair(time, value) objects (its value slot and the pair-time slot after it),
    built one by one in Python: for a groupBy result of millions of groups that loop dominates the fetch
    (the other aggregators' columns are views of the slot rows)."""
    def typed(col, out_type):  # (strided views of the slot rows; floats are narrowed)
        if out_type == "long":
            return col.view(np.int64)
        if out_type == "double":
            return col.view(np.float64)
        return (col & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)

    out = []
    cols = slots.T
    for a, at in zip(aggs, Q.native_index(aggs)):
        v = typed(cols[at], a.output_type)
        if a.is_pair:
            pairs = np.empty(len(v), dtype=object)
            for i, (t, x) in enumerate(zip(cols[at + 1].view(np.int64).tolist(), v.tolist())):
                pairs[i] = Q.SerializablePair(t, x)
            v = pairs
        out.append(v)
    return out


def _py(v, out_type):
    if isinstance(v, Q.SerializablePair):
        return v
    return int(v) if out_type == "long" else float(v)


def finalize_results(query, results):
    """FinalizeResultsQueryRunner (query/FinalizeResultsQueryRunner.java:84-120) at the top of the runner
    chain: every aggregator's value through AggregatorFactory.finalizeComputation — a first/last pair
    becomes its rhs. Results of a query without such aggregators are returned as they are."""
    aggs = [a for a in getattr(query, "aggregations", []) if a.is_pair]
    if not aggs:
        return results
    out = []
    for r in results:
        if isinstance(r, Q.Row):
            ev = dict(r.event)
            for a in aggs:
                if a.name in ev:
                    ev[a.name] = a.finalize_computation(ev[a.name])
            out.append(Q.Row(r.timestamp, ev))
            continue
        if isinstance(r.value, list):
            vals = []
            for e in r.value:
                e = dict(e)
                for a in aggs:
                    if a.name in e:
                        e[a.name] = a.finalize_computation(e[a.name])
                vals.append(e)
            out.append(Q.Result(r.timestamp, vals))
        else:
            v = dict(r.value)
            for a in aggs:
                if a.name in v:
                    v[a.name] = a.finalize_computation(v[a.name])
            out.append(Q.Result(r.timestamp, v))
    return out


def _group_by_device(segments: Sequence[GpuSegment]) -> "OrderedDict[int, List[int]]":
    g: "OrderedDict[int, List[int]]" = OrderedDict()
    for i, s in enumerate(segments):
        g.setdefault(id(s.context), []).append(i)
    return g


def _handles(segs: Sequence[GpuSegment]):
    arr = (ctypes.c_void_p * len(segs))(*[s.handle.value for s in segs])
    return arr


class RunStats:
    """Per-call QueryMetrics counters accumulated over native calls."""

    def __init__(self):
        self.calls: List[Dict] = []
        self.post: List[Dict] = []  # dg_post_info of every groupBy post-processing step on the device
        # derived columns of the query's expressions (virtual.lower_query): built by this query, found already
        # built, and the device time of the builds
        self.derived_built = 0
        self.derived_reused = 0
        self.derived_build_ms = 0.0

    def add(self, m: N.dg_metrics, span=None):
        d = m.as_dict()
        if span is not None:  # host wall clock (time.perf_counter) at the call's start and end
            d["t_start"], d["t_end"] = span
        self.calls.append(d)

    def total(self, key):
        return sum(c[key] for c in self.calls)


# ----------------------------------------------------------------------------------------------
# timeseries
# ----------------------------------------------------------------------------------------------
def timeseries_per_segment(segments: Sequence[GpuSegment], query: Q.TimeseriesQuery,
                           stats: Optional[RunStats] = None,
                           cancel: Optional[ctypes.c_int32] = None) -> List[List[Q.Result]]:
    query = V.lower_query(query, segments, stats, cancel)
    split = segment_queries(query, segments)
    if split is not None:  # every segment on its own calendar chain
        return [timeseries_per_segment([s], q, stats, cancel)[0] if q is not None else []
                for s, q in zip(segments, split)]
    out: List[List[Q.Result]] = [[] for _ in segments]
    na = _native_width(query)
    for _, idx in _group_by_device(segments).items():
        segs = [segments[i] for i in idx]
        cap = _bucket_cap(segs, query)
        scan, keep = N.make_scan(query, Q, segments=segs, cancel=cancel)
        n = len(segs)
        nb = np.zeros(n, dtype=np.int32)
        times = np.zeros(n * cap, dtype=np.int64)
        rows = np.zeros(n * cap, dtype=np.int64)
        vals = np.zeros(n * cap * max(na, 1), dtype=np.uint64)
        m = N.dg_metrics()
        N.check(N.lib().dg_timeseries_run(_handles(segs), n, ctypes.byref(scan), cap, nb.ctypes.data,
                                          times.ctypes.data, rows.ctypes.data, vals.ctypes.data, ctypes.byref(m)))
        if stats is not None:
            stats.add(m)
        for k, i in enumerate(idx):
            res = []
            cols = _decode_slots(query.aggregations, vals.reshape(-1, max(na, 1))[k * cap:k * cap + nb[k], :na])
            for b in range(nb[k]):
                if query.skip_empty_buckets and rows[k * cap + b] == 0:
                    continue
                res.append(Q.Result(int(times[k * cap + b]),
                                    {a.name: _py(c[b], a.output_type) for a, c in zip(query.aggregations, cols)}))
            out[i] = res
    return out


def run_timeseries(segments: Sequence[GpuSegment], query: Q.TimeseriesQuery,
                   stats: Optional[RunStats] = None) -> List[Q.Result]:
    """QueryRunnerFactory.mergeRunners over segments on any devices: one dg_timeseries_run per device,
    then every segment's bucket list (in segment order) folded natively by dg_timeseries_merge
    (TimeseriesBinaryFn, ResultMergeQueryRunner order: time, then runner)."""
    query = V.lower_query(query, segments, stats)
    na = _native_width(query)
    groups = list(_group_by_device(segments).items())
    caps = {dev: _bucket_cap([segments[i] for i in idx], query) for dev, idx in groups}
    cap = max(caps.values()) if caps else 1
    n_all = len(segments)
    nb = np.zeros(max(n_all, 1), dtype=np.int32)
    times = np.zeros(max(n_all, 1) * cap, dtype=np.int64)
    rows = np.zeros(max(n_all, 1) * cap, dtype=np.int64)
    vals = np.zeros(max(n_all, 1) * cap * max(na, 1), dtype=np.uint64)
    scan = keep = None
    for dev, idx in groups:
        segs = [segments[i] for i in idx]
        c = caps[dev]
        scan, keep = N.make_scan(query, Q, segments=segs)
        n = len(segs)
        d_nb = np.zeros(n, dtype=np.int32)
        d_t = np.zeros(n * c, dtype=np.int64)
        d_r = np.zeros(n * c, dtype=np.int64)
        d_v = np.zeros(n * c * max(na, 1), dtype=np.uint64)
        m = N.dg_metrics()
        N.check(N.lib().dg_timeseries_run(_handles(segs), n, ctypes.byref(scan), c, d_nb.ctypes.data, d_t.ctypes.data,
                                          d_r.ctypes.data, d_v.ctypes.data, ctypes.byref(m)))
        if stats is not None:
            stats.add(m)
        for k, i in enumerate(idx):  # into the segment's slot of the call-wide lists
            nb[i] = d_nb[k]
            times[i * cap:i * cap + c] = d_t[k * c:(k + 1) * c]
            rows[i * cap:i * cap + c] = d_r[k * c:(k + 1) * c]
            vals[i * cap * na:(i * cap + c) * na] = d_v[k * c * na:(k + 1) * c * na]
    if scan is None:
        scan, keep = N.make_scan(query, Q, filters=False)
    g = query.granularity
    if g.is_calendar:  # TimeseriesBinaryFn keys a result by gran.bucketStart(its timestamp)
        starts = {}
        for i in range(n_all):
            for k in range(int(nb[i])):
                t = int(times[i * cap + k])
                if t not in starts:
                    starts[t] = g.bucket_start(t)
                times[i * cap + k] = starts[t]
    out_cap = max(n_all, 1) * cap
    on = ctypes.c_int32()
    o_t = np.zeros(out_cap, dtype=np.int64)
    o_v = np.zeros(out_cap * max(na, 1), dtype=np.uint64)
    N.check(N.lib().dg_timeseries_merge(ctypes.byref(scan), n_all, nb.ctypes.data, cap, times.ctypes.data,
                                        rows.ctypes.data, vals.ctypes.data, int(query.skip_empty_buckets), out_cap,
                                        ctypes.byref(on), o_t.ctypes.data, None, o_v.ctypes.data))
    m = on.value
    cols = _decode_slots(query.aggregations, o_v.reshape(-1, max(na, 1))[:m, :na])
    # post-aggregators after the merge, from the merged aggregators (TimeseriesQueryQueryToolChest.java:378-386)
    return [Q.Result(int(o_t[b]), Q.compute_post_aggregations(
        query, {a.name: _py(c[b], a.output_type) for a, c in zip(query.aggregations, cols)})) for b in range(m)]


def _bucket_cap(segs, query) -> int:
    g = query.granularity
    if g.is_all:
        return 1
    cap = 1
    qs, qe = query.interval
    for s in segs:
        lo = max(qs, s.min_time)
        hi = min(qe, g.bucket_end(s.max_time))
        if hi > lo:
            if g.is_calendar:  # buckets of the segment's actual interval on the query's bucket list
                cap = max(cap, len(g.iterable((lo, hi))))
            else:
                cap = max(cap, (hi - g.bucket_start(lo) + g.period_ms - 1) // g.period_ms)
    return int(cap)


def merge_timeseries(query: Q.TimeseriesQuery, per_segment: List[List[Q.Result]]) -> List[Q.Result]:
    """ResultMergeQueryRunner + TimeseriesBinaryFn: combine results of the same bucket."""
    gran = query.granularity
    merged: Dict[int, Q.Result] = {}
    flat = sorted(((r.timestamp, si, k, r) for si, rs in enumerate(per_segment) for k, r in enumerate(rs)),
                  key=lambda x: (x[0], x[1], x[2]))
    for ts, _, _, r in flat:
        key = 0 if gran.is_all else gran.bucket_start(ts)
        if key not in merged:
            merged[key] = Q.Result(r.timestamp if gran.is_all else key, dict(r.value))
        else:
            acc = merged[key].value
            for a in query.aggregations:
                acc[a.name] = a.combine(acc[a.name], r.value[a.name])
    out = [merged[k] for k in sorted(merged)]
    for r in out:  # (TimeseriesQueryQueryToolChest.java:378-386: from the merged aggregators)
        Q.compute_post_aggregations(query, r.value)
    if query.descending:
        out.reverse()
    return out


# ----------------------------------------------------------------------------------------------
# topN
# ----------------------------------------------------------------------------------------------
def _java_key(s: Optional[str]):
    return (0, b"") if s is None else (1, s.encode("utf-16-be", "surrogatepass"))


_NUMERIC_COLS = (N.COL_LONG, N.COL_FLOAT, N.COL_DOUBLE)
_OUT_TYPES = {"STRING": N.COL_STRING, "LONG": N.COL_LONG, "FLOAT": N.COL_FLOAT, "DOUBLE": N.COL_DOUBLE}


def numeric_key(v: float, single: bool = False) -> int:
    """The order-preserving signed key of a float's canonical bits (Float.floatToIntBits /
    Double.doubleToLongBits folded with b ^ ((b >> 31 or 63) & 0x7fff…)): ascending keys are Float.compare /
    Double.compare order (-0.0 < 0.0, NaN greatest). The fold is its own inverse (numeric_key_value)."""
    if single:
        b = 0x7fc00000 if v != v else int(np.array([v], dtype=np.float32).view(np.int32)[0])
        return b ^ ((b >> 31) & 0x7fffffff)
    b = 0x7ff8000000000000 if v != v else int(np.array([v], dtype=np.float64).view(np.int64)[0])
    return b ^ ((b >> 63) & 0x7fffffffffffffff)


def numeric_key_value(key: int, single: bool = False) -> float:
    if single:
        b = key ^ ((key >> 31) & 0x7fffffff)
        return float(np.array([b], dtype=np.int32).view(np.float32)[0])
    b = key ^ ((key >> 63) & 0x7fffffffffffffff)
    return float(np.array([b], dtype=np.int64).view(np.float64)[0])


def _dim_tie_key(v):
    """dimValue.compareTo of the builder's comparator (TopNNumericResultBuilder.java:94-107): String.compareTo
    with nulls first, Long.compareTo, Double / Float.compareTo (a float32 widens exactly)."""
    if v is None or isinstance(v, str):
        return _java_key(v)
    if isinstance(v, float):
        return (1, numeric_key(v))
    return (1, int(v))


def _text_sort_key(query: Q.TopNQuery):
    """The dimension-ordered spec's comparator as a sort key over the entries' dimension values: over the
    strings themselves, or for a numeric output type over Objects.toString of the value."""
    key = O.sort_key(query.metric.ordering, query.metric.inverted)
    if query.dimension_type == "STRING":
        return key
    return lambda v: key(_dim_text(v))


def _dim_text(v):
    """Objects.toString of a dimension value (TopNLexicographicResultBuilder.java:66-125); null stays null."""
    return v if v is None or isinstance(v, str) else str(v)


class _HeapItem:
    __slots__ = ("mk", "dk", "entry")

    def __init__(self, mk, dk, entry):
        self.mk, self.dk, self.entry = mk, dk, entry

    def __lt__(self, o):
        return (self.mk, self.dk) < (o.mk, o.dk)


class TopNResultBuilder:
    """TopNNumericResultBuilder (TopNNumericResultBuilder.java:94-235): bounded priority queue,
    add only when below threshold or strictly better than the current minimum metric."""

    def __init__(self, query: Q.TopNQuery, threshold: int):
        spec = query.metric
        # a metric naming a post-aggregator ranks under its comparator (NumericTopNMetricSpec.getComparator)
        self.prog = query.metric_program()
        agg = None if self.prog is not None else next(a for a in query.aggregations if a.name == spec.metric)
        self.metric = spec.metric
        self.dim = query.dimension
        self.inverted = spec.type == "inverted"
        self.agg = agg
        self.threshold = threshold
        # (a string dimension's values: String.compareTo, nulls first; numeric output types: their compareTo)
        self.dim_key = _java_key if query.dimension_type == "STRING" else _dim_tie_key
        self.heap: List[_HeapItem] = []

    def _mk(self, v):
        if self.prog is not None:
            k = Q.post_program_order_key(self.prog.order, Q.post_value_word(v, self.prog.out_type))
        else:
            k = self.agg.compare_key(v)
        return _Rev(k) if self.inverted else k

    def add(self, entry: Dict):
        mk = self._mk(entry[self.metric])
        if len(self.heap) < self.threshold or self.heap[0].mk < mk:
            heapq.heappush(self.heap, _HeapItem(mk, self.dim_key(entry[self.dim]), entry))
        if len(self.heap) > self.threshold:
            heapq.heappop(self.heap)

    def build(self) -> List[Dict]:
        items = sorted(self.heap, key=lambda h: (_Rev(h.mk), h.dk))
        return [h.entry for h in items]


class JavaPriorityQueue:
    """java.util.PriorityQueue with a comparator (offer = siftUp, poll = siftDown, toArray = the
    heap array): which of several comparator-equal entries a poll removes, and the order a stable
    sort leaves them in, follow from this exact layout."""

    def __init__(self, cmp):
        self.cmp = cmp
        self.q: List = []

    def __len__(self):
        return len(self.q)

    def offer(self, x):
        q, cmp = self.q, self.cmp
        k = len(q)
        q.append(x)
        while k > 0:
            parent = (k - 1) >> 1
            if cmp(x, q[parent]) >= 0:
                break
            q[k] = q[parent]
            k = parent
        q[k] = x

    def poll(self):
        q, cmp = self.q, self.cmp
        top = q[0]
        x = q.pop()
        n = len(q)
        if n:
            k = 0
            while k < (n >> 1):
                child = 2 * k + 1
                if child + 1 < n and cmp(q[child], q[child + 1]) > 0:
                    child += 1
                if cmp(x, q[child]) <= 0:
                    break
                q[k] = q[child]
                k = child
            q[k] = x
        return top


def _memo_key(key):
    """key(v) computed once per value (a comparator calls it on both sides of every comparison)."""
    memo: Dict = {}

    def k(v):
        r = memo.get(v, memo)
        if r is memo:
            r = memo[v] = key(v)
        return r
    return k


def _key_cmp(key):
    def cmp(a, b):
        ka, kb = key(a), key(b)
        return (ka > kb) - (ka < kb)
    return cmp


class LexicographicResultBuilder:
    """TopNLexicographicResultBuilder (query/topn/TopNLexicographicResultBuilder.java:40-176) with
    the topN comparator given as a sort key (ordering.sort_key): shouldAdd takes every non-null
    value once the queue is full (the head's topN metric value it compares against is never set),
    values must come after previousStop; the queue's head is the largest value, polled past the
    threshold; build() sorts the queue's array by the comparator, stably."""

    def __init__(self, query: Q.TopNQuery, threshold: int):
        spec = query.metric
        self.dim = query.dimension
        self.key = _memo_key(_text_sort_key(query))
        self.cmp = _key_cmp(self.key)
        self.threshold = threshold
        self.stop = spec.previous_stop
        self.pq = JavaPriorityQueue(lambda a, b: self.cmp(b[self.dim], a[self.dim]))

    def add(self, entry: Dict):
        v = entry[self.dim]
        if len(self.pq) >= self.threshold and v is None:
            return
        if self.stop is not None and self.cmp(v, self.stop) <= 0:
            return
        self.pq.offer(entry)
        if len(self.pq) > self.threshold:
            self.pq.poll()

    def build(self) -> List[Dict]:
        return sorted(self.pq.q, key=lambda e: self.key(e[self.dim]))


def _result_builder(query: Q.TopNQuery, threshold: int):
    if query.metric.type == "dimension":
        return LexicographicResultBuilder(query, threshold)
    return TopNResultBuilder(query, threshold)


class _Rev:
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def __lt__(self, o):
        return o.v < self.v

    def __eq__(self, o):
        return self.v == o.v


class TopNRaw:
    """dg_topn_run output for segments of one device: list L = i * bcap + b (segment i, cursor b; bcap = 1
    for ALL granularity) has `cnt[L]` entries (-1 = no cursor), entry j at L * K + j of `ids`
    (segment-local dictionary ids, or ids into a numeric column's value list) and `vals` (n_aggs slots);
    `ts[L]` is the list's result timestamp; `cut_ties[L]` counts the values of a numeric dimension whose
    metric equals the list's last entry's and that are not in the list (dg_topn_opts.out_cut_ties: nonzero
    where the reference's pick among them depends on its hash map's iteration order)."""

    def __init__(self, segments, cnt, ids, vals, K, ts, bcap=1, cut_ties=None):
        self.segments, self.cnt, self.ids, self.vals, self.K, self.ts = segments, cnt, ids, vals, K, ts
        self.bcap = bcap
        self.numeric = cut_ties is not None  # the dimension is numeric (then the counts were asked for)
        self._cut_ties = cut_ties

    @property
    def cut_ties(self) -> np.ndarray:
        if self._cut_ties is None:  # a string dimension: nothing is cut arbitrarily
            self._cut_ties = np.zeros(len(self.cnt), dtype=np.int32)
        return self._cut_ties


def _numeric_dimension(segments: Sequence[GpuSegment], query: Q.TopNQuery) -> bool:
    """The topN runs over a numeric dimension: a numeric output type, or a LONG / FLOAT / DOUBLE column."""
    if query.dimension_type != "STRING":
        return True
    dim = query.native_dimension
    for s in segments:
        if s.column_type(dim) in _NUMERIC_COLS:
            return True
    return False


def _topn_opts(query: Q.TopNQuery, cut_ties: Optional[np.ndarray] = None) -> N.dg_topn_opts:
    o = N.dg_topn_opts()
    o.output_type = _OUT_TYPES[query.dimension_type]
    o.out_cut_ties = cut_ties.ctypes.data if cut_ties is not None else None
    return o


def topn_dim_values(seg: GpuSegment, query: Q.TopNQuery, ids) -> List:
    """The dimension values of result ids: dictionary strings, or for a numeric column the values converted
    to the dimension's output type (convertAggregatorStoreKeyToColumnValue): int, float, or the decimal str."""
    dim = query.native_dimension
    if seg.column_type(dim) not in _NUMERIC_COLS:
        return [seg.dim_value(dim, int(x)) for x in ids]
    vals = seg.numeric_dim_values(dim, ids).tolist()
    return [str(v) for v in vals] if query.dimension_type == "STRING" else vals


def _topn_struct(query: Q.TopNQuery, threshold: int, segments: Optional[Sequence[GpuSegment]] = None):
    """dg_topn for a numeric / inverted metric, or a dimension ordering (then the segments'
    dictionary orders are registered and their previousStop cuts computed). Returns the struct and
    the buffers it points into."""
    t = N.dg_topn()
    dim = query.native_dimension.encode()
    t.dimension = dim
    t.threshold = threshold
    spec = query.metric
    keep = [dim]
    if spec.type == "dimension":
        t.metric_agg, t.inverted = 0, 0
        t.dim_order = O.order_slot(spec.ordering, spec.inverted)
        if spec.previous_stop is not None:
            stop = spec.previous_stop.encode()
            t.previous_stop = stop
            keep.append(stop)
        if segments is not None:
            mins = np.zeros(len(segments), dtype=np.int32)
            for i, seg in enumerate(segments):
                order = seg.dim_order(query.dimension, spec.ordering, spec.inverted)
                if order is not None:
                    mins[i] = order.min_rank(spec.previous_stop)
                else:  # missing dimension: its one value is null, never after a previousStop (a numeric
                    #    column: the engine derives the ranks itself and refuses a previousStop)
                    mins[i] = 0 if spec.previous_stop is None else 1
            t.min_rank = mins.ctypes.data
            keep.append(mins)
    else:
        # (the native slot of the metric's value: a first/last aggregator orders by its pair's rhs; a metric
        # naming a post-aggregator travels as a program, _topn_metric, and the slot is ignored)
        names = [a.name for a in query.aggregations]
        t.metric_agg = Q.native_index(query.aggregations)[names.index(spec.metric)] if spec.metric in names else 0
        t.inverted = int(spec.type == "inverted")
        t.dim_order = -1
    return t, keep


def _check_topn(query: Q.TopNQuery):
    pass


def _topn_metric(query: Q.TopNQuery):
    """The trailing program of dg_topn_run_post / dg_topn_merge_post: (pointer or None, keep-alive)."""
    prog = query.metric_program()
    if prog is None:
        return None, None
    arr, keep = N.make_post_aggs([(prog.ops, prog.order)])
    return arr, (arr, keep)


def topn_raw(segments: Sequence[GpuSegment], query: Q.TopNQuery, stats: Optional[RunStats] = None,
             cancel: Optional[ctypes.c_int32] = None, descending: bool = False) -> TopNRaw:
    """One batched dg_topn_run_opts over segments that share a device (PooledTopNAlgorithm, or over a numeric
    dimension DimExtractionTopNAlgorithm, + TopNNumericResultBuilder per segment, threshold
    max(threshold, minTopNThreshold)). cancel: a flag another thread may set (DG_ERR_INTERRUPTED).
    descending: descending cursors (dg_scan.descending; a TopNQuery itself is never descending,
    TopNQuery.java:74): every cursor's rows last to first, a segment's lists latest bucket first."""
    _check_topn(query)
    if len(_group_by_device(segments)) != 1:
        raise ValueError("topn_raw: segments must share one device")
    query = V.lower_query(query, segments, stats, cancel)
    na = _native_width(query)
    K = query.segment_threshold
    scan, keep = N.make_scan(query, Q, segments=segments, cancel=cancel)
    if descending:
        scan.descending = 1
    t, keep_t = _topn_struct(query, K, segments)
    n = len(segments)
    bcap = _bucket_cap(segments, query)
    cnt = np.zeros(n * bcap, dtype=np.int32)
    ids = np.zeros(n * bcap * K, dtype=np.int32)
    vals = np.zeros(n * bcap * K * max(na, 1), dtype=np.uint64)
    bt = np.zeros(n * bcap, dtype=np.int64)
    t.bucket_cap = bcap
    t.out_bucket_time = bt.ctypes.data
    cut = opts = None  # (a string dimension: dg_topn_run_opts without options is dg_topn_run)
    if _numeric_dimension(segments, query):
        cut = np.zeros(n * bcap, dtype=np.int32)
        opts = ctypes.byref(_topn_opts(query, cut))
    m = N.dg_metrics()
    metric, keep_m = _topn_metric(query)
    N.check(N.lib().dg_topn_run_post(_handles(segments), n, ctypes.byref(scan), ctypes.byref(t), opts, metric,
                                     cnt.ctypes.data, ids.ctypes.data, vals.ctypes.data, ctypes.byref(m)))
    if stats is not None:
        stats.add(m)
        if cut is not None:
            stats.calls[-1]["topn_cut_ties"] = int(cut.sum())
    if query.granularity.is_all:  # the cursor's time: start of the segment's part of the interval
        ts = np.array([max(query.interval[0], s.min_time) for s in segments], dtype=np.int64)
    else:
        ts = bt
    return TopNRaw(list(segments), cnt, ids, vals, K, ts, bcap, cut)


def topn_merge_raw(query: Q.TopNQuery, cnt: np.ndarray, keys: np.ndarray, vals: np.ndarray, K: int,
                   ts: np.ndarray, handles=None):
    """dg_topn_merge over lists ordered by (timestamp, index) (TopNQueryQueryToolChest merge order).
    Returns (timestamp, list index, keys, value slots) of the merged entries, or None when no list
    has a cursor. handles: per-list segment handles (segment mode) or None (global ids)."""
    na = _native_width(query)
    live = [i for i in range(len(cnt)) if cnt[i] >= 0]
    if not live:
        return None
    order = np.array(sorted(live, key=lambda i: (int(ts[i]), i)), dtype=np.int64)
    n = len(order)
    if n == len(cnt) and not np.any(order != np.arange(n)):  # every list, already in merge order
        o_cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        o_keys = np.ascontiguousarray(keys, dtype=np.int64)
        o_vals = np.ascontiguousarray(vals)
    else:
        o_cnt = np.ascontiguousarray(cnt[order].astype(np.int32))
        o_keys = np.ascontiguousarray(keys.reshape(-1, K)[order].astype(np.int64))
        o_vals = np.ascontiguousarray(vals.reshape(-1, K, max(na, 1))[order])
    lists = N.dg_topn_lists()
    lists.n_lists = n
    lists.list_n = o_cnt.ctypes.data
    lists.stride = K
    lists.keys = o_keys.ctypes.data
    lists.values = o_vals.ctypes.data
    scan, keep = N.make_scan(query, Q, filters=False)  # the fold needs the aggregators only
    t, dim = _topn_struct(query, query.threshold)
    out_n = ctypes.c_int32()
    T = query.threshold
    out_list = np.zeros(T, dtype=np.int32)
    out_keys = np.zeros(T, dtype=np.int64)
    out_vals = np.zeros(T * max(na, 1), dtype=np.uint64)
    hs = None
    if handles is not None:
        hs = (ctypes.c_void_p * n)(*[handles[i] for i in order])
    opts = None if query.dimension_type == "STRING" else ctypes.byref(_topn_opts(query))  # (None: output STRING)
    metric, keep_m = _topn_metric(query)
    N.check(N.lib().dg_topn_merge_post(hs, ctypes.byref(scan), ctypes.byref(t), ctypes.byref(lists), opts, metric,
                                       ctypes.byref(out_n), out_list.ctypes.data, out_keys.ctypes.data,
                                       out_vals.ctypes.data))
    k = out_n.value
    if k < 0:
        return None
    return int(ts[order[0]]), order[out_list[:k]], out_keys[:k], out_vals[:k * na].reshape(k, na) if na else None


def _topn_entries(query: Q.TopNQuery, values: List[Optional[str]], slots) -> List[Dict]:
    # (tolist: Python ints / floats per column at once, as _py of each element would give)
    cols = [c.tolist() for c in _decode_slots(query.aggregations, slots)] if len(values) and query.aggregations else []
    names = [a.name for a in query.aggregations]
    dim = query.dimension
    out = []
    for j, v in enumerate(values):
        e = {dim: v}
        for name, col in zip(names, cols):
            e[name] = col[j]
        # every post-aggregator's value, from the entry's aggregators (TopNQueryQueryToolChest.java:196-206)
        out.append(Q.compute_post_aggregations(query, e))
    return out


def merge_dimension_lists(query: Q.TopNQuery, lists: Sequence[Tuple[int, int, "callable", np.ndarray]],
                          tie_free: bool) -> List[Q.Result]:
    """TopNBinaryFn fold of dimension-ordered per-segment lists, given in merge order as
    (timestamp, length, value_of(j), [length, n_aggs] slots), with the builder's literal queue
    (LexicographicResultBuilder). Each list is its segment's values in comparator order. When no
    two values compare equal (`tie_free`: no segment order has ties, and the head entries checked
    here have distinct keys), every value the fold keeps or ranks sits in the first `threshold`
    non-null entries of each list holding it, and the queue sizes the fold sees (which decide
    whether a late null is taken) are the same over those heads: the fold runs over the heads only."""
    if not lists:
        return []
    spec = query.metric
    T = query.threshold

    def head(c, value_of):  # the first T non-null entries (a list's null comes first)
        return min(c, T + (1 if c and value_of(0) is None else 0))

    def fold(limit):
        per = []
        for ts, c, value_of, slots in lists:
            k = c if limit is None else head(c, value_of)
            per.append([Q.Result(ts, _topn_entries(query, [value_of(j) for j in range(k)], slots[:k]))])
        return merge_topn(query, per)

    if not tie_free:
        return fold(None)
    key = _text_sort_key(query)
    heads = {value_of(j) for _, c, value_of, _ in lists for j in range(head(c, value_of))}
    keys = sorted(key(v) for v in heads)
    if any(a == b for a, b in zip(keys, keys[1:])):
        return fold(None)
    return fold(T)


def _merge_topn_dimension(query: Q.TopNQuery, segments: Sequence[GpuSegment], raw: TopNRaw) -> List[Q.Result]:
    spec = query.metric
    K, na = raw.K, _native_width(query)
    live = sorted((i for i in range(len(segments)) if raw.cnt[i] >= 0), key=lambda i: (int(raw.ts[i]), i))
    orders = [segments[i].dim_order(query.dimension, spec.ordering, spec.inverted) for i in live]
    tie_free = not any(o is not None and o.has_ties for o in orders)
    slots = raw.vals.reshape(-1, max(na, 1))
    lists = []
    for i in live:
        seg, base = segments[i], i * K
        memo: Dict[int, Optional[str]] = {}  # (each entry's value looked up once)
        if raw.numeric:
            memo.update(enumerate(topn_dim_values(seg, query, raw.ids[base:base + int(raw.cnt[i])])))

        def value_of(j, seg=seg, base=base, memo=memo):
            v = memo.get(j, memo)
            if v is memo:
                v = memo[j] = seg.dim_value(query.dimension, int(raw.ids[base + j]))
            return v
        lists.append((int(raw.ts[i]), int(raw.cnt[i]), value_of, slots[base:base + int(raw.cnt[i])]))
    return merge_dimension_lists(query, lists, tie_free)


def run_topn(segments: Sequence[GpuSegment], query: Q.TopNQuery, stats: Optional[RunStats] = None) -> List[Q.Result]:
    """Per-segment topN on the GPU + TopNBinaryFn merge in the engine (one device); falls back to the
    Python merge when the segments span devices."""
    _check_topn(query)
    query = V.lower_query(query, segments, stats)
    if len(_group_by_device(segments)) != 1 or not query.granularity.is_all:
        return merge_topn(query, topn_per_segment(segments, query, stats))
    if query.metric.type == "dimension":
        return _merge_topn_dimension(query, segments, topn_raw(segments, query, stats))
    raw = topn_raw(segments, query, stats)
    handles = [s.handle for s in segments]
    res = topn_merge_raw(query, raw.cnt, raw.ids, raw.vals, raw.K, raw.ts, handles)
    if res is None:
        return []
    ts, lists, keys, slots = res
    if raw.numeric:
        values = [topn_dim_values(segments[int(l)], query, [int(k)])[0] for l, k in zip(lists, keys)]
    else:
        values = [segments[int(l)].dim_value(query.dimension, int(k)) for l, k in zip(lists, keys)]
    return [Q.Result(ts, _topn_entries(query, values, slots))]


def topn_per_segment(segments: Sequence[GpuSegment], query: Q.TopNQuery,
                     stats: Optional[RunStats] = None, descending: bool = False) -> List[List[Q.Result]]:
    """Per-segment results (what each segment's QueryRunner returns), as Result lists.
    descending: topn_raw's descending cursors."""
    _check_topn(query)
    query = V.lower_query(query, segments, stats)
    split = segment_queries(query, segments)
    if split is not None:  # every segment on its own calendar chain
        return [topn_per_segment([s], q, stats, descending)[0] if q is not None else []
                for s, q in zip(segments, split)]
    out: List[List[Q.Result]] = [[] for _ in segments]
    na = _native_width(query)
    for _, idx in _group_by_device(segments).items():
        segs = [segments[i] for i in idx]
        raw = topn_raw(segs, query, stats, descending=descending)
        K, bcap = raw.K, raw.bcap
        for k, i in enumerate(idx):
            seg = segs[k]
            res = []
            for b in range(bcap):
                L = k * bcap + b
                if raw.cnt[L] < 0:  # no cursor: the segment does not overlap the interval / bucket
                    continue
                c = int(raw.cnt[L])
                values = topn_dim_values(seg, query, raw.ids[L * K:L * K + c])
                slots = raw.vals.reshape(-1, max(na, 1))[L * K:L * K + c, :na]
                res.append(Q.Result(int(raw.ts[L]), _topn_entries(query, values, slots)))
            out[i] = res
    return out


def topn_binary_fn(query: Q.TopNQuery, r1: Optional[Q.Result], r2: Optional[Q.Result]) -> Optional[Q.Result]:
    """TopNBinaryFn.apply (TopNBinaryFn.java:75-135)."""
    if r1 is None:
        return r2
    if r2 is None:
        return r1
    dim = query.dimension
    ret: Dict = {}
    # equals of the value object: a Float / Double by its bits (-0.0 is not 0.0, NaN is NaN)
    by_bits = query.dimension_type in ("FLOAT", "DOUBLE")
    for v in r1.value:
        ret[numeric_key(v[dim]) if by_bits else v[dim]] = v
    for v in r2.value:
        k = numeric_key(v[dim]) if by_bits else v[dim]
        if k in ret:
            a = ret[k]
            c = {dim: v[dim]}
            for agg in query.aggregations:
                c[agg.name] = agg.combine(a[agg.name], v[agg.name])
            # recomputed after the combine, before the builder ranks (TopNBinaryFn.java:97-110)
            ret[k] = Q.compute_post_aggregations(query, c)
        else:
            ret[k] = v
    bob = _result_builder(query, query.threshold)
    for v in ret.values():
        bob.add(v)
    ts = r1.timestamp if query.granularity.is_all else query.granularity.bucket_start(r1.timestamp)
    return Q.Result(ts, bob.build())


def merge_topn(query: Q.TopNQuery, per_segment: List[List[Q.Result]]) -> List[Q.Result]:
    gran = query.granularity
    flat = sorted(((r.timestamp, si, r) for si, rs in enumerate(per_segment) for r in rs), key=lambda x: (x[0], x[1]))
    merged: Dict[int, Q.Result] = {}
    for ts, _, r in flat:
        key = 0 if gran.is_all else gran.bucket_start(ts)
        merged[key] = topn_binary_fn(query, merged.get(key), r)
    out = [Q.Result(merged[k].timestamp, merged[k].value[:query.threshold]) for k in sorted(merged)]
    # result ordering ResultGranularTimestampComparator.create(gran, descending) (TopNQueryQueryToolChest.java:132;
    # a TopNQuery is never descending, TopNQuery.java:74)
    return out[::-1] if getattr(query, "descending", False) else out


# ----------------------------------------------------------------------------------------------
# groupBy
# ----------------------------------------------------------------------------------------------
class GroupByPartial:
    """Columnar per-segment groupBy output: bucket times, dimension values, aggregate columns.
    Engine partials also carry `codes` (segment-local dictionary ids per dimension) and `dicts` (the
    segments' sorted dictionaries): the merge then works on integer codes, and the value columns are
    only materialised when asked for."""

    def __init__(self, times: np.ndarray, dims: Optional[List[np.ndarray]], aggs: List[np.ndarray],
                 codes: Optional[List[np.ndarray]] = None, dicts: Optional[List[List[Optional[str]]]] = None,
                 merged: bool = False):
        self.times, self._dims, self.aggs = times, dims, aggs
        self.codes, self.dicts = codes, dicts
        self.merged = merged  # already one merged, ordered result (a whole device's engine call)

    @property
    def dims(self) -> List[np.ndarray]:
        if self._dims is None:
            self._dims = [np.array(dd, dtype=object)[c] for c, dd in zip(self.codes, self.dicts)]
        return self._dims

    def __len__(self):
        return len(self.times)


class PinnedPool:
    """Pinned host memory for result delivery (dg_host_alloc), allocated once and reused: the shim's
    direct ByteBuffers (the processing pool allocates its buffers once at startup,
    OffheapBufferGenerator.java:53). Fetches into it go by DMA, no staging copy on the host."""

    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        N.check(N.lib().dg_host_alloc(int(nbytes), ctypes.byref(self.ptr)))
        self.nbytes, self.off = int(nbytes), 0
        self._holder = None  # weak reference to the partial whose arrays are views of this memory

    def _check_free(self, what: str):
        if self._holder is not None and self._holder() is not None:
            raise RuntimeError(f"PinnedPool.{what}: the memory is still in use by a fetched partial (drop it first)")
        self._holder = None

    def hold(self, partial) -> None:
        """Mark the pool as backing `partial` (one fetch at a time): reset() and close() refuse while it
        lives, and the partial keeps the pool alive."""
        import weakref
        self._holder = weakref.ref(partial)
        partial._pool = self

    def reset(self):
        self._check_free("reset")
        self.off = 0

    def take(self, dtype, n: int) -> np.ndarray:
        dt = np.dtype(dtype)
        self.off = (self.off + 63) & ~63
        nb = n * dt.itemsize
        if self.off + nb > self.nbytes:
            raise MemoryError(f"pinned pool of {self.nbytes} bytes: {self.off + nb} needed")
        buf = (ctypes.c_char * nb).from_address(self.ptr.value + self.off)
        self.off += nb
        return np.frombuffer(buf, dtype=dt, count=n)

    def close(self):
        if self.ptr:
            self._check_free("close")
            N.lib().dg_host_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


class GroupByResult:
    """A dg_result: the merged groups of one dg_groupby_run (or of a dg_merge across devices, whose
    ids index the caller's cluster dictionaries), resident in HBM until fetched."""

    def __init__(self, handle: ctypes.c_void_p, query: Q.GroupByQuery,
                 dictionaries: Optional[List[List[Optional[str]]]] = None):
        self.handle, self.query = handle, query
        self.groups = int(N.lib().dg_result_groups(handle))
        self._dicts = dictionaries
        self.time_map: Optional[np.ndarray] = None  # bucket index -> time (a dg_merge over a calendar grid)
        self.post_info: Optional[Dict] = None  # dg_post_info of apply_post_process, once it ran
        self.post_programs: List = []          # post_process_spec: the programs of dg_result_post_aggregate
        self.post_aggregate_ms = 0.0           # its device time

    def dim_types(self, d: int) -> Tuple[int, int]:
        """(column type, output type) of dimension d as N.COL_* (dg_result_dim_type); a dg_merge result has
        the caller's dictionaries: strings."""
        if self._dicts is not None:
            return N.COL_STRING, N.COL_STRING
        ct, ot = ctypes.c_int32(), ctypes.c_int32()
        N.check(N.lib().dg_result_dim_type(self.handle, d, ctypes.byref(ct), ctypes.byref(ot)))
        return ct.value, ot.value

    def dictionary(self, d: int) -> List:
        """The merged dictionary of dimension d in merged-id order: strings (None = null); Python ints for
        a long dimension whose output type is LONG (dg_result_dim_longs), its values' decimal strings when
        the output type is STRING."""
        if self._dicts is not None:
            return self._dicts[d]
        L = N.lib()
        card = int(L.dg_result_dim_cardinality(self.handle, d))
        if self.dim_types(d) == (N.COL_LONG, N.COL_LONG):
            vals = np.zeros(max(card, 1), dtype=np.int64)
            N.check(L.dg_result_dim_longs(self.handle, d, vals.ctypes.data))
            return vals[:card].tolist()
        offs = np.zeros(card + 1, dtype=np.int64)
        total = ctypes.c_int64()
        N.check(L.dg_result_dim_dictionary(self.handle, d, None, None, ctypes.byref(total)))
        buf = ctypes.create_string_buffer(max(total.value, 1))
        N.check(L.dg_result_dim_dictionary(self.handle, d, offs.ctypes.data, buf, ctypes.byref(total)))
        raw = buf.raw
        return [raw[int(offs[i]):int(offs[i + 1])].decode("utf-8") if offs[i + 1] > offs[i] else None
                for i in range(card)]

    def fetch(self, start: int = 0, count: Optional[int] = None, pool: "Optional[PinnedPool]" = None) -> "GroupByPartial":
        """Groups [start, start + count) to the host. Under ALL granularity no bucket times cross PCIe
        (every group's is the universal timestamp, the query interval's start). pool: pinned host
        memory (dg_host_alloc) the columns land in by DMA; the partial's arrays are views of it."""
        q = self.query
        nd, na = len(q.dimensions), _native_width(q)
        count = self.groups - start if count is None else count
        all_gran = q.granularity.is_all and self.time_map is None
        if pool is not None:
            pool.reset()
            t = None if all_gran else pool.take(np.int64, max(count, 1))
            ids = pool.take(np.int32, max(count * nd, 1))
            vals = pool.take(np.uint64, max(count * na, 1))
        else:
            # (np.empty: the library's staged copy is the first touch of these pages, spread over threads)
            t = None if all_gran else np.empty(max(count, 1), dtype=np.int64)
            ids = np.empty(max(count * nd, 1), dtype=np.int32)
            vals = np.empty(max(count * na, 1), dtype=np.uint64)
        if count:
            N.check(N.lib().dg_result_fetch_groups(self.handle, start, count, t.ctypes.data if t is not None else None,
                                                   ids.ctypes.data if nd else None, vals.ctypes.data if na else None))
        if all_gran:  # GroupByStrategyV2.getUniversalTimestamp (:125-138), one value for every group
            t = np.broadcast_to(np.int64(q.interval[0]), (count,))
        if self.time_map is not None:
            t[:count] = self.time_map[t[:count]]
        ids = ids[:count * nd].reshape(count, nd) if nd else np.zeros((count, 0), np.int32)
        codes = [ids[:, d] for d in range(nd)]  # strided views of the [count][ndims] id rows
        aggs = _decode_slots(q.aggregations, vals[:count * na].reshape(count, na)) if na else []
        part = GroupByPartial(t[:count], None, aggs, codes, [self.dictionary(d) for d in range(nd)], merged=True)
        if pool is not None:
            pool.hold(part)
        return part

    def grouper_info(self) -> Dict:
        """What grouped this result (dg_result_grouper_info): the grouper that ran (N.GROUPER_*), its HBM
        table's slots, the group limit in force and the hash insert's LDS flush / direct counts."""
        info = N.dg_grouper_info()
        N.check(N.lib().dg_result_grouper_info(self.handle, ctypes.byref(info)))
        return info.as_dict()

    def apply_limit_push_down(self) -> bool:
        """LimitedBufferHashGrouper's outcome on the device (dg_result_limit): when the query pushes
        its limit down (GroupByQuery.isApplyLimitPushDown), keep the first `limit` groups in the
        push-down row order (GroupByQuery.getRowOrderingForPushDown :423-528). Every dimension is
        passed as a column: the ORDER BY ones with their comparator and direction, then the others
        ascending under LEXICOGRAPHIC (UTF-8 byte order, which differs from the dictionary's Java
        String order only for values beyond U+D7FF, so the id order is used when none has one)."""
        q = self.query
        if self.groups == 0 or not q.apply_limit_push_down():
            return False
        order = q.order_by_dims()
        cols, keep, seen = [], [], set()
        spec = [(d, c.direction == "descending", c.dimensionOrder) for d, c in zip(order, q.limitSpec.columns)]
        spec += [(d, False, "lexicographic") for d in range(len(q.dimensions)) if d not in order]
        for d, desc, ordering in spec:
            if d in seen:
                continue
            seen.add(d)
            rank = None
            if q.dimensionTypes[d] == "LONG":
                # compareDimsForLimitPushDown (GroupByQuery.java:600-633) over a numeric-typed dimension: NUMERIC
                # compares the longs (the id order of a LONG-output dimension), any other comparator
                # compares String.valueOf of them
                if ordering != "numeric":
                    texts = [str(v) for v in self.dictionary(d)]
                    rank = np.ascontiguousarray(O.DictionaryOrder(texts, ordering).rank, dtype=np.int32)
                    keep.append(rank)
            elif ordering != "lexicographic" or _beyond_bmp_low(self.dictionary(d)):
                rank = np.ascontiguousarray(O.DictionaryOrder(self.dictionary(d), ordering).rank, dtype=np.int32)
                keep.append(rank)
            cols.append(N.dg_order_column(d, int(desc), rank.ctypes.data if rank is not None else None))
        arr = (N.dg_order_column * len(cols))(*cols)
        lim = N.dg_limit(ctypes.cast(arr, ctypes.c_void_p), len(cols), int(q.limitSpec.limit),
                         int(q._ctx_bool("sortByDimsFirst", False)))
        N.check(N.lib().dg_result_limit(self.handle, ctypes.byref(lim)))
        self.groups = int(N.lib().dg_result_groups(self.handle))
        return True

    def post_process_spec(self):
        """query.having / query.limitSpec as (having ops, order columns, sort, limit) of a
        dg_result_post_process call, or None when there is nothing to apply or the spec cannot be
        expressed: a having or an ORDER BY on a LONG-output dimension (postprocess_groupby refuses
        those), an ORDER BY on an unknown column, a having leaf the program has no op for. Order columns
        are (kind, index, descending, rank or None); dimension ranks are built as apply_limit_push_down
        builds them."""
        q = self.query
        ls = q.limitSpec
        if q.having is None and ls is None:
            return None
        ops: List = []
        post = PostColumns(q)
        self.post_programs = post.programs
        if q.having is not None:
            try:
                ops = having_program(q, self.dictionary, post)
            except (ValueError, ArithmeticError):  # (a value the comparator itself refuses: the host path raises it)
                return None
            if ops is None:
                return None
        cols, sort, limit = [], False, 0
        if ls is not None:
            try:
                sort = _limit_needs_sort(q)
            except ValueError:
                return None
            aggs = {a.name: i for a, i in zip(q.aggregations, Q.native_index(q.aggregations))}  # (native slots)
            for c in ls.columns if sort else []:
                if c.dimension in aggs:
                    cols.append((N.ORDER_AGG, aggs[c.dimension], c.direction == "descending", None))
                elif q.post_aggregator(c.dimension) is not None:
                    # post column j is "aggregator" n_aggs + j, compared under the post-aggregator's comparator
                    cols.append((N.ORDER_AGG, post.index(c.dimension, True), c.direction == "descending", None))
                elif c.dimension in q.dimensions:
                    d = q.dimensions.index(c.dimension)
                    if q.dimensionTypes[d] != "STRING":
                        return None
                    rank = None
                    if c.dimensionOrder != "lexicographic" or _beyond_bmp_low(self.dictionary(d)):
                        rank = np.ascontiguousarray(O.DictionaryOrder(self.dictionary(d), c.dimensionOrder).rank,
                                                    dtype=np.int32)
                    cols.append((N.ORDER_DIM, d, c.direction == "descending", rank))
                else:
                    return None
            if ls.limit is not None and ls.limit < (1 << 31):
                limit = int(ls.limit)
        if len(post.programs) > N.POST_MAX_COLS:
            return None
        return ops, cols, sort, limit

    def apply_post_process(self) -> bool:
        """GroupByQuery.postProcess on the device (dg_result_post_process): the having spec, then the
        limit spec's order and cut, so that only the surviving groups are fetched. Returns whether the
        device step ran (self.post_info then holds its dg_post_info); it does not when the query pushes
        its limit down (apply_limit_push_down's case), has neither spec, or post_process_spec cannot
        express it. The host's postprocess_groupby still runs over what is fetched: it is idempotent."""
        q = self.query
        if q.apply_limit_push_down():
            return False
        spec = self.post_process_spec()
        if spec is None:
            return False
        ops, cols, sort, limit = spec
        if self.post_programs:  # the post-aggregators the having or the limit spec decides on, as columns
            parr, keep = N.make_post_aggs(self.post_programs)
            ms = ctypes.c_double()
            N.check(N.lib().dg_result_post_aggregate(self.handle, parr, len(self.post_programs), ctypes.byref(ms)))
            self.post_aggregate_ms = ms.value
            del keep
        harr = (N.dg_having_op * max(len(ops), 1))(*[N.dg_having_op(*o) for o in ops])
        carr = (N.dg_post_column * max(len(cols), 1))(
            *[N.dg_post_column(k, i, int(desc), 0, rank.ctypes.data if rank is not None else None)
              for k, i, desc, rank in cols])
        pp = N.dg_post_process(ctypes.cast(harr, ctypes.c_void_p), len(ops), len(cols),
                               ctypes.cast(carr, ctypes.c_void_p), int(sort),
                               int(q._ctx_bool("sortByDimsFirst", False)), limit, 0)
        info = N.dg_post_info()
        N.check(N.lib().dg_result_post_process(self.handle, ctypes.byref(pp), ctypes.byref(info)))
        self.post_info = info.as_dict()
        self.groups = int(N.lib().dg_result_groups(self.handle))
        return True

    def release(self):
        if self.handle:
            N.lib().dg_result_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _beyond_bmp_low(values) -> bool:
    """Whether any value holds a character whose UTF-8 order differs from its UTF-16 order."""
    return any(v is not None and any(ord(ch) > 0xD7FF for ch in v) for v in values)


def grouper_options(query: Q.GroupByQuery) -> Optional[Tuple[int, int]]:
    """The query context's grouper keys as dg_groupby_opts fields (grouper, max_groups), or None when
    the query names neither (the call then takes the context's defaults): forceHashAggregation ->
    DG_GROUPER_HASH (false: the sort, explicitly), bufferGrouperMaxSize -> max_groups
    (GroupByQueryConfig.java:35-40,179-200). -1 / 0 leave a field to the context's default."""
    ctx = query.context or {}
    if "forceHashAggregation" not in ctx and "bufferGrouperMaxSize" not in ctx:
        return None
    grouper = -1
    if "forceHashAggregation" in ctx:
        grouper = N.GROUPER_HASH if query.force_hash_aggregation() else N.GROUPER_SORT
    return grouper, query.buffer_grouper_max_size()


def groupby_run(segments: Sequence[GpuSegment], query: Q.GroupByQuery,
                stats: Optional[RunStats] = None, limit_push_down: bool = False,
                cancel: Optional[ctypes.c_int32] = None, post_process: bool = False) -> GroupByResult:
    """One dg_groupby_run over segments of ONE device: GroupByStrategyV2.mergeRunners over their
    per-segment runners (GroupByMergingQueryRunnerV2.java:170-290), the groups left in HBM. With
    `limit_push_down`, a query that pushes its limit down keeps only its first `limit` groups
    (GroupByResult.apply_limit_push_down); a result meant for the cross-device exchange stays whole.
    With `post_process`, the having and limit specs are applied to the resident groups
    (GroupByResult.apply_post_process): only for a result that holds every group of the query whole,
    never for a partial that is merged with others afterwards.
    cancel: a flag another thread may set (Thread.interrupt): the call then fails DG_ERR_INTERRUPTED;
    the query context's "timeout" (ms) fails it with DG_ERR_TIMEOUT."""
    if len(_group_by_device(segments)) != 1:
        raise ValueError("groupby_run: segments must share one device")
    query = V.lower_query(query, segments, stats, cancel)
    nd = len(query.dimensions)
    scan, keep = N.make_scan(query, Q, segments=segments, cancel=cancel)
    dims = (ctypes.c_char_p * max(nd, 1))(*[d.encode() for d in query.native_dimensions])
    g = N.dg_groupby()
    g.dimensions = ctypes.cast(dims, ctypes.POINTER(ctypes.c_char_p))
    g.n_dims = nd
    res = ctypes.c_void_p()
    m = N.dg_metrics()
    t0 = time.perf_counter()
    opts = grouper_options(query)
    if any(t != "STRING" for t in query.dimensionTypes):
        # DimensionSpec.getOutputType of every dimension goes with it (dg_groupby_run_dims)
        types = {"STRING": N.COL_STRING, "LONG": N.COL_LONG, "FLOAT": N.COL_FLOAT, "DOUBLE": N.COL_DOUBLE}
        specs = (N.dg_dimension * max(nd, 1))()
        for i, t in enumerate(query.dimensionTypes):
            specs[i].dimension = dims[i]
            specs[i].output_type = types[t]
        o = N.dg_groupby_opts(opts[0], 0, opts[1]) if opts is not None else None
        N.check(N.lib().dg_groupby_run_dims(_handles(segments), len(segments), ctypes.byref(scan), specs, nd,
                                            ctypes.byref(o) if o is not None else None, ctypes.byref(res), ctypes.byref(m)))
    elif opts is None:
        N.check(N.lib().dg_groupby_run(_handles(segments), len(segments), ctypes.byref(scan), ctypes.byref(g),
                                       ctypes.byref(res), ctypes.byref(m)))
    else:
        o = N.dg_groupby_opts(opts[0], 0, opts[1])
        N.check(N.lib().dg_groupby_run_opts(_handles(segments), len(segments), ctypes.byref(scan), ctypes.byref(g),
                                            ctypes.byref(o), ctypes.byref(res), ctypes.byref(m)))
    if stats is not None:
        stats.add(m, (t0, time.perf_counter()))
    out = GroupByResult(res, query)
    if limit_push_down:
        out.apply_limit_push_down()
    if post_process:
        out.apply_post_process()
    return out


def groupby_per_device(segments: Sequence[GpuSegment], query: Q.GroupByQuery,
                       stats: Optional[RunStats] = None, post_process: bool = False) -> List[GroupByPartial]:
    """The merged, ordered groups of every device's segments (one engine call per device).
    post_process: the caller merges nothing else into these groups (the merged runner over one device's
    segments), so the having and limit specs run on the device before the fetch; per-segment partials
    and several devices' partials are merged first and stay whole."""
    query = V.lower_query(query, segments, stats)
    out = []
    groups = _group_by_device(segments)
    for _, idx in groups.items():
        r = groupby_run([segments[i] for i in idx], query, stats, limit_push_down=True,
                        post_process=post_process and len(groups) == 1)
        try:
            if stats is not None and r.post_info is not None:
                stats.post.append(r.post_info)
            out.append(r.fetch())
        finally:
            r.release()
    return out


def _per_device_concurrently(groups, fn, release=None):
    """fn(segment indices of one device) for every device at once, one host thread each, results in
    device order (ChainedExecutionQueryRunner submits every runner to the processing pool; the native
    calls release the GIL, so the devices' kernels are in flight together). Every future is waited
    for; if one fails, `release` frees the results of the others before the first error is raised
    (ChainedExecutionQueryRunner cancels the pending futures the same way, :158-167)."""
    items = list(groups.values())
    if len(items) == 1:
        return [fn(items[0])]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(items)) as ex:
        futs = [ex.submit(fn, idx) for idx in items]
        results, err = [], None
        for f in futs:
            try:
                results.append(f.result())
            except BaseException as e:  # noqa: BLE001 (re-raised below, after the cleanup)
                results.append(None)
                err = err or e
    if err is not None:
        if release is not None:
            for r in results:
                if r is not None:
                    release(r)
        raise err
    return results


def groupby_merge_devices(segments: Sequence[GpuSegment], query: Q.GroupByQuery, stats: Optional[RunStats] = None,
                          targets: Optional[Sequence] = None) -> "List[GroupByResult]":
    """mergeRunners over segments of several devices in one process: one dg_groupby_run per device, all
    devices at once, then dg_groupby_merge_devices moves key ranges between the devices itself (peer
    copies) and merges them there, every target concurrently. targets: the contexts owning the key
    ranges (default: every participating device's context, so no device funnels the others' groups);
    returns the per-target results in key order."""
    for a in query.aggregations:  # (before any engine call or peer copy)
        if a.is_pair:
            raise N.UnsupportedQuery(2, f"{a.type}({a.name}): the device-side groupBy merge does not combine first/last pairs")
    query = V.lower_query(query, segments, stats)  # (before the devices' threads start)
    groups = _group_by_device(segments)
    parts = []
    try:
        def one(idx):
            return groupby_run([segments[i] for i in idx], query, stats)
        parts = _per_device_concurrently(groups, one, release=lambda r: r.release())
        ctxs = [segments[idx[0]].context for idx in groups.values()] if targets is None else list(targets)
        outs = (ctypes.c_void_p * len(ctxs))()
        hp = (ctypes.c_void_p * len(parts))(*[p.handle.value for p in parts])
        ht = (ctypes.c_void_p * len(ctxs))(*[c.handle.value for c in ctxs])
        m = N.dg_metrics()
        N.check(N.lib().dg_groupby_merge_devices(hp, len(parts), ht, len(ctxs), outs, ctypes.byref(m)))
        if stats is not None:
            stats.add(m)
    finally:
        for p in parts:
            p.release()
    return [GroupByResult(ctypes.c_void_p(o), query) for o in outs]


def groupby_per_segment(segments: Sequence[GpuSegment], query: Q.GroupByQuery,
                        stats: Optional[RunStats] = None) -> List[GroupByPartial]:
    """What each segment's QueryRunner returns (createRunner(segment).run), one engine call each
    (a calendar granularity on the segment's own bucket chain, segment_queries)."""
    query = V.lower_query(query, segments, stats)
    split = segment_queries(query, segments) or [query] * len(segments)
    return [groupby_per_device([s], q, stats)[0] for s, q in zip(segments, split) if q is not None]


def merge_groupby_columnar(query: Q.GroupByQuery, partials: Sequence[GroupByPartial]):
    """Merge per-segment partials by (bucket, dimension values); returns sorted columnar arrays."""
    gran = query.granularity
    parts = [p for p in partials if p is not None and len(p)]
    nd = len(query.dimensions)
    if not parts:
        return np.zeros(0, np.int64), [np.zeros(0, object) for _ in range(nd)], [np.zeros(0) for _ in query.aggregations]
    if len(parts) == 1 and parts[0].merged:  # the engine merged and ordered the call's segments already
        return parts[0].times, parts[0].dims, parts[0].aggs
    times = np.concatenate([p.times for p in parts])
    keys_t = times if not gran.is_all else np.zeros(len(times), np.int64)
    if gran.is_calendar and len(times):
        # segments on their own bucket chains (segment_queries): the toolchest's mergeResults orders
        # and combines rows by gran.bucketStart(timestamp) and emits that start
        # (GroupByQuery.getRowOrdering(true), GroupByQuery.java:575-576; GroupByBinaryFnV2.java:78-81)
        u, inv = np.unique(times, return_inverse=True)
        keys_t = np.array([gran.bucket_start(int(x)) for x in u], np.int64)[inv]
    dim_codes = []
    dim_values = []
    coded = all(p.codes is not None for p in parts)
    for d in range(nd):
        # a LONG-output dimension's values are longs and merge in numeric order (LongRowBasedKeySerdeHelper,
        # RowBasedGrouperHelper.java:1389-1437); every other dimension's are strings in Java String order
        vkey = int if query.dimensionTypes[d] == "LONG" else _java_key
        if coded:
            # segment dictionaries are sorted (GenericIndexed STRING_STRATEGY): merge them into one
            # global dictionary and remap each segment's ids with one vectorised lookup
            dicts = [p.dicts[d] for p in parts]
            if all(dd is dicts[0] or dd == dicts[0] for dd in dicts[1:]):
                uniq, maps = list(dicts[0]), [None] * len(parts)
            else:
                uniq = sorted(set().union(*map(set, dicts)), key=vkey)
                index = {v: i for i, v in enumerate(uniq)}
                maps = [np.array([index[v] for v in dd], dtype=np.int64) for dd in dicts]
            dim_codes.append(np.concatenate([p.codes[d].astype(np.int64) if m is None else m[p.codes[d]]
                                             for p, m in zip(parts, maps)]))
            dim_values.append(np.array(uniq, dtype=object))
            continue
        col = np.concatenate([p.dims[d] for p in parts])
        uniq = sorted(set(col.tolist()), key=vkey)  # global dictionary in Java order, null first
        index = {v: i for i, v in enumerate(uniq)}
        dim_codes.append(np.fromiter((index[v] for v in col), dtype=np.int64, count=len(col)))
        dim_values.append(np.array(uniq, dtype=object))
    order_keys = [keys_t] + dim_codes
    # one composite int64 key (time rank, then each dimension's code) when the ranges fit: a single
    # argsort instead of a multi-key lexsort
    if len(keys_t) and keys_t.min() == keys_t.max():
        t_rank, n_t = np.zeros(len(keys_t), np.int64), 1
    else:
        t_vals, t_rank = np.unique(keys_t, return_inverse=True)
        n_t = len(t_vals)
    radices = [n_t] + [len(v) for v in dim_values]
    if float(np.prod([float(r) for r in radices])) < 2.0 ** 62:
        comp = t_rank.astype(np.int64)
        for c, r in zip(dim_codes, radices[1:]):
            comp = comp * r + c
        order = np.argsort(comp, kind="stable")  # equal keys fold in partial (segment) order
        sc = comp[order]
        change = np.ones(len(order), dtype=bool)
        if len(order) > 1:
            change[1:] = sc[1:] != sc[:-1]
        sk = [k[order] for k in order_keys]
    else:
        order = np.lexsort(tuple(reversed(order_keys)))
        sk = [k[order] for k in order_keys]
        change = np.ones(len(order), dtype=bool)
        if len(order) > 1:
            diff = np.zeros(len(order) - 1, dtype=bool)
            for k in sk:
                diff |= k[1:] != k[:-1]
            change[1:] = diff
    starts = np.nonzero(change)[0]
    out_aggs = []
    for a_i, a in enumerate(query.aggregations):
        col = np.concatenate([p.aggs[a_i] for p in parts])[order]
        out_aggs.append(_reduce(a, col, starts))
    # ALL granularity: every merged row carries the universal timestamp, the query interval's start
    # (GroupByStrategyV2.getUniversalTimestamp, strategy/GroupByStrategyV2.java:125-138)
    out_times = np.full(len(starts), query.interval[0], np.int64) if gran.is_all else sk[0][starts]
    out_dims = [dim_values[d][sk[1 + d][starts]] for d in range(nd)]
    return out_times, out_dims, out_aggs


def _java_minmax_reduce(col: np.ndarray, starts: np.ndarray, is_min: bool) -> np.ndarray:
    """Math.min / Math.max folded over runs (DoubleMinAggregator.combine, java/lang/Math.java): NaN
    wins, and -0.0 < 0.0 — reduced on order-preserving integer keys (the engine's ord_key)."""
    if col.dtype == np.float32:
        bits, sign, udt = col.view(np.uint32).astype(np.uint64), np.uint64(1 << 31), np.uint32
    else:
        bits, sign, udt = col.view(np.uint64), np.uint64(1 << 63), np.uint64
    neg = (bits & sign) != 0
    key = np.where(neg, ~bits & (sign | (sign - np.uint64(1))), bits | sign)
    nan = np.isnan(col)
    red = (np.minimum if is_min else np.maximum).reduceat(key, starts)
    any_nan = np.logical_or.reduceat(nan, starts) if len(col) else np.zeros(0, bool)
    neg_key = (red & sign) == 0
    mask = sign | (sign - np.uint64(1))
    raw = np.where(neg_key, ~red & mask, red & ~sign).astype(udt)
    out = raw.view(col.dtype).copy()
    out[any_nan] = np.nan
    return out


def _reduce(a: Q.AggregatorFactory, col: np.ndarray, starts: np.ndarray) -> np.ndarray:
    k = a.kind
    if a.is_pair:  # a left fold of the factory's combine over each run, in partial (segment) order
        out = np.empty(len(starts), dtype=object)
        ends = list(starts[1:]) + [len(col)]
        for g, (s0, s1) in enumerate(zip(starts.tolist(), ends)):
            acc = col[s0]
            for i in range(s0 + 1, int(s1)):
                acc = a.combine(acc, col[i])
            out[g] = acc
        return out
    if k in (0, 1):
        return np.add.reduceat(col.astype(np.int64), starts)
    if k == 4:
        return np.minimum.reduceat(col, starts)
    if k == 5:
        return np.maximum.reduceat(col, starts)
    if k in (2, 3):
        return np.add.reduceat(col, starts)
    return _java_minmax_reduce(col, starts, k in (6, 8))


def merge_groupby(query: Q.GroupByQuery, partials: Sequence[GroupByPartial]) -> List[Q.Row]:
    t, dims, aggs = merge_groupby_columnar(query, partials)
    rows = []
    for r in range(len(t)):
        ev = {d: dims[i][r] for i, d in enumerate(query.dimensions)}
        for a, col in zip(query.aggregations, aggs):
            ev[a.name] = _py(col[r], a.output_type)
        rows.append(Q.Row(int(t[r]), ev))
    if query.apply_limit_push_down():
        # the partials hold (at least) the first `limit` groups of every device in the push-down
        # order; across devices the cut is taken again in that order
        rows = sorted(rows, key=_push_down_key(query))[:query.limitSpec.limit]
    elif query._ctx_bool("sortByDimsFirst", False) and not query.granularity.is_all:
        # getRowOrdering(false) with sortByDimsFirst: dimensions, then time (GroupByQuery.java:543-553)
        keys = [int if t == "LONG" else _java_key for t in query.dimensionTypes]
        rows.sort(key=lambda r: tuple(k(r.event[d]) for k, d in zip(keys, query.dimensions)))
    return postprocess_groupby(query, rows)


def _push_down_key(query: Q.GroupByQuery):
    """Sort key of GroupByQuery.getRowOrderingForPushDown (:423-528): ORDER BY dimensions under their
    comparator and direction, the other dimensions ascending under LEXICOGRAPHIC, the time first (last
    with sortByDimsFirst; absent for ALL)."""
    def dim_key(name, ordering):  # (a LONG-output dimension: compareDimsForLimitPushDown :600-633)
        return O.long_order_key(ordering) if query.dimension_type(name) == "LONG" else O.sort_key(ordering)

    fields, seen = [], set()
    for c in query.limitSpec.columns:
        fields.append((c.dimension, dim_key(c.dimension, c.dimensionOrder), c.direction == "descending"))
        seen.add(c.dimension)
    fields += [(d, dim_key(d, "lexicographic"), False) for d in query.dimensions if d not in seen]
    gran_all = query.granularity.is_all
    dims_first = query._ctx_bool("sortByDimsFirst", False)

    def key(r):
        ks = tuple(O._Desc(f(r.event.get(n))) if desc else f(r.event.get(n)) for n, f, desc in fields)
        if gran_all:
            return ks
        return ks + (r.timestamp,) if dims_first else (r.timestamp,) + ks
    return key


# ----------------------------------------------------------------------------------------------
# groupBy post-processing (GroupByQuery.postProcess: having, then the limitSpec;
# GroupByStrategyV2.applyPostProcessing). Host-side over the merged rows, which arrive in the
# natural (time, dimensions) order.
# ----------------------------------------------------------------------------------------------
def _double_key(v: float):
    if v != v:
        return (1, 0.0, 0)  # Doubles.compare: NaN greatest, -0.0 < 0.0
    return (0, v, 1 if (v == 0.0 and math.copysign(1.0, v) > 0) else 0)


def _having_compare(metric, value) -> int:
    """HavingSpecMetricComparator.compare (having/HavingSpecMetricComparator.java:36-80)."""
    if metric is None:
        a, b = _double_key(0.0), _double_key(float(value))
        return (a > b) - (a < b)
    if isinstance(metric, int):
        if isinstance(value, int):
            return (metric > value) - (metric < value)
        x, y = Fraction(metric), Fraction(Decimal(repr(float(value))))  # BigDecimal.valueOf
        return (x > y) - (x < y)
    m = float(metric)
    if isinstance(value, int):
        x, y = Fraction(Decimal(repr(m))), Fraction(value)
        return (x > y) - (x < y)
    a, b = _double_key(m), _double_key(float(value))
    return (a > b) - (a < b)


def _having_eval(h: Q.HavingSpec, row: Q.Row) -> bool:
    t = h.type
    if t == "always":
        return True
    if t == "never":
        return False
    if t == "and":
        return all(_having_eval(x, row) for x in h.specs)
    if t == "or":
        return any(_having_eval(x, row) for x in h.specs)
    if t == "not":
        return not _having_eval(h.specs[0], row)
    if t == "dimSelector":  # DimensionSelectorHavingSpec.eval: emptyToNull on both sides
        return (row.event.get(h.dimension) or None) == (h.value or None)
    metric = row.event.get(h.aggregation)
    if isinstance(metric, Q.SerializablePair):  # a first/last aggregator compares by its value
        metric = metric.rhs
    if t == "equalTo" and metric is None and h.value is None:
        return True
    if h.value is None:
        return False
    c = _having_compare(metric, h.value)
    return c > 0 if t == "greaterThan" else (c < 0 if t == "lessThan" else c == 0)


def _limit_needs_sort(query: Q.GroupByQuery) -> bool:
    """DefaultLimitSpec.build (orderby/DefaultLimitSpec.java:122-188): whether the natural order is
    not good enough (then a sort by makeComparator, else just the limit)."""
    ls = query.limitSpec
    if len(query.dimensions) < len(ls.columns):
        return True
    aggs = {a.name for a in query.aggregations} | {p.name for p in query.postAggregations}
    for i, c in enumerate(ls.columns):
        if c.dimension in aggs:
            return True
        if c.dimension not in query.dimensions:
            raise ValueError(f"Unknown column in order clause[{c.dimension}]")
        # string dimensions: the natural comparator is LEXICOGRAPHIC; numeric-typed ones: NUMERIC
        natural = "numeric" if query.dimension_type(c.dimension) == "LONG" else "lexicographic"
        if c.direction != "ascending" or c.dimensionOrder != natural or c.dimension != query.dimensions[i]:
            return True
    return not query.granularity.is_all and query._ctx_bool("sortByDimsFirst", False)


def _having_dimensions(h: Q.HavingSpec) -> List[str]:
    return ([h.dimension] if h.type == "dimSelector" else []) + [d for x in h.specs for d in _having_dimensions(x)]


# ---- the same rules as a dg_result_post_process spec (the device step in front of the fetch) ----
_KEY_MAX = (1 << 64) - 1
_KEY_SIGN = 1 << 63
_KEY_POS_INF = 0xFFF0000000000000  # order key of +inf: every key above it is NaN
_KEY_NEG_INF = 0x000FFFFFFFFFFFFF  # order key of -inf


def post_order_key(v, out_type: str) -> int:
    """An aggregator's comparator as an unsigned 64-bit number (dg_result_post_process): Long.compare for
    long outputs, Doubles.compare for double outputs (every NaN one key, the greatest; -0.0 < 0.0) and
    for float outputs through their exactly widened value."""
    if out_type == "long":
        return (int(v) + _KEY_SIGN) & _KEY_MAX
    d = float(v)
    if d != d:
        return _KEY_MAX
    u = int(np.array([d], dtype=np.float64).view(np.uint64)[0])
    return (~u & _KEY_MAX) if u & _KEY_SIGN else (u | _KEY_SIGN)


def post_key_metric(key: int, out_type: str):
    """The metric an order key stands for. No double has a key above +inf's but the NaN key, or below
    -inf's: those read as NaN and as -inf, which keeps the comparator monotone over the whole key space."""
    if out_type == "long":
        return key - _KEY_SIGN
    if key > _KEY_POS_INF:
        return math.nan
    if key < _KEY_NEG_INF:
        return -math.inf
    u = (key & ~_KEY_SIGN) if key & _KEY_SIGN else (~key & _KEY_MAX)
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


def _key_compare(key: int, out_type: str, value) -> int:
    """_having_compare of the key's metric. One corner is decided here: an infinite or NaN metric against
    an integer value (a NumberFormatException of BigDecimal.valueOf in the reference) counts as below
    every integer for -inf and above for +inf / NaN."""
    metric = post_key_metric(key, out_type)
    if out_type != "long" and isinstance(value, int) and (metric != metric or math.isinf(metric)):
        return -1 if metric == -math.inf else 1
    return _having_compare(metric, value)


def having_interval(kind: str, out_type: str, value) -> Tuple[int, int]:
    """The closed order-key interval [lo, hi] a greaterThan / lessThan / equalTo leaf accepts (lo > hi:
    none): HavingSpecMetricComparator.compare is monotone in the metric for a fixed value, so the ends
    are found by bisection over the key space with _having_compare itself."""
    def first(pred):  # the least key with pred (monotone: false ... false true ... true), 2^64 when none
        lo, hi = 0, _KEY_MAX + 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if pred(mid):
                hi = mid
            else:
                lo = mid + 1
        return lo

    ge = first(lambda k: _key_compare(k, out_type, value) >= 0)
    gt = first(lambda k: _key_compare(k, out_type, value) > 0)
    lo, hi = {"greaterThan": (gt, _KEY_MAX), "lessThan": (0, ge - 1), "equalTo": (ge, gt - 1)}[kind]
    return (lo, hi) if 0 <= lo <= hi <= _KEY_MAX else (1, 0)


class PostColumns:
    """The post-aggregator columns one dg_result_post_aggregate call evaluates for a query's having and limit
    specs: index(name, for_order) gives the "aggregator" index n_aggs + j of the column (dg_result_post_process),
    one column per (post-aggregator, order kind). for_order: the post-aggregator's own comparator (an ORDER BY
    column); otherwise the value type's natural order, which HavingSpecMetricComparator's intervals are cut in."""

    def __init__(self, query: Q.GroupByQuery):
        self.query = query
        self.n_aggs = _native_width(query)
        self.programs: List[Tuple[List[Tuple[int, int, int]], int]] = []
        self.out_types: List[str] = []
        self._at: Dict[Tuple[str, int], int] = {}

    def index(self, name: str, for_order: bool) -> int:
        prog = Q.compile_post_aggregator(self.query.aggregations, self.query.postAggregations, name, for_order)
        k = (name, prog.order)
        if k not in self._at:
            self._at[k] = len(self.programs)
            self.programs.append((prog.ops, prog.order))
            self.out_types.append(prog.out_type)
        return self.n_aggs + self._at[k]

    def out_type(self, index: int) -> str:
        return self.out_types[index - self.n_aggs]


def having_program(query: Q.GroupByQuery, dictionary,
                   post: Optional[PostColumns] = None) -> Optional[List[Tuple[int, int, int, int]]]:
    """query.having as dg_having_op tuples (op, arg, lo, hi) in postfix order, or None when it cannot be
    expressed (a leaf on a LONG-output dimension, a metric leaf naming a dimension, a value that is no
    number, a program beyond the ABI's length or stack). dictionary(d): the result's merged dictionary
    of dimension d. A leaf on a name that is no aggregator folds to a constant, as _having_eval's
    `metric is None` does; a dimSelector looks its value up (null and "" are the null id, an absent value
    never matches)."""
    aggs = {a.name: (i, a) for a, i in zip(query.aggregations, Q.native_index(query.aggregations))}  # (native slots)
    ops: List[Tuple[int, int, int, int]] = []

    def const(b):
        ops.append((N.HAVING_ALWAYS if b else N.HAVING_NEVER, 0, 0, 0))
        return True

    def emit(h: Q.HavingSpec) -> bool:
        t = h.type
        if t in ("always", "never"):
            return const(t == "always")
        if t in ("and", "or"):
            if not all(emit(x) for x in h.specs):
                return False
            ops.append((N.HAVING_AND if t == "and" else N.HAVING_OR, len(h.specs), 0, 0))
            return True
        if t == "not":
            if not emit(h.specs[0]):
                return False
            ops.append((N.HAVING_NOT, 0, 0, 0))
            return True
        if t == "dimSelector":
            if h.dimension in aggs:
                return False
            if h.dimension not in query.dimensions:
                return const((h.value or None) is None)
            d = query.dimensions.index(h.dimension)
            if query.dimensionTypes[d] != "STRING":
                return False
            want = h.value or None
            if want is not None and not isinstance(want, str):
                return False
            ids = [i for i, v in enumerate(dictionary(d)) if (v or None) == want]
            for i in ids:
                ops.append((N.HAVING_DIM_EQ, d, i, 0))
            if len(ids) != 1:
                ops.append((N.HAVING_OR, len(ids), 0, 0))
            return True
        if t not in ("greaterThan", "lessThan", "equalTo"):
            return False
        if h.aggregation in query.dimensions:
            return False
        if h.aggregation not in aggs and query.post_aggregator(h.aggregation) is not None:
            if h.value is None:
                return const(False)
            if post is None or isinstance(h.value, bool) or not isinstance(h.value, (int, float)):
                return False
            i = post.index(h.aggregation, False)
            lo, hi = having_interval(t, post.out_type(i), h.value)
            ops.append((N.HAVING_AGG_RANGE, i, lo, hi))
            return True
        if h.aggregation not in aggs:  # metric is None
            return const(_having_eval(h, Q.Row(0, {})))
        if h.value is None:
            return const(False)
        if isinstance(h.value, bool) or not isinstance(h.value, (int, float)):
            return False
        i, a = aggs[h.aggregation]
        lo, hi = having_interval(t, a.output_type, h.value)
        ops.append((N.HAVING_AGG_RANGE, i, lo, hi))
        return True

    if not emit(query.having) or len(ops) > N.HAVING_MAX_OPS:
        return None
    depth = 0
    for op, arg, _, _ in ops:  # the ABI's stack bound
        depth += 1 - arg if op in (N.HAVING_AND, N.HAVING_OR) else (0 if op == N.HAVING_NOT else 1)
        if depth > 32:
            return None
    return ops


def postprocess_groupby(query: Q.GroupByQuery, rows: List[Q.Row]) -> List[Q.Row]:
    """A having spec that selects on a LONG-output dimension, or a limit spec that has to sort on one, is
    refused (UnsupportedQuery): the host rules here are the string dimensions'. Post-aggregators are computed
    for every row first (GroupByStrategyV2.mergeResults, GroupByStrategyV2.java:286-300, computes them before
    postProcess): having and ORDER BY read them like aggregators, under the post-aggregator's comparator."""
    if query.postAggregations:
        rows = [Q.Row(r.timestamp, Q.compute_post_aggregations(query, dict(r.event))) for r in rows]
    if query.having is not None:
        for d in _having_dimensions(query.having):
            if query.dimension_type(d) == "LONG":
                raise N.UnsupportedQuery(2, f"having spec on the LONG-output dimension {d}")
        rows = [r for r in rows if _having_eval(query.having, r)]
    ls = query.limitSpec
    if ls is None:
        return rows
    if _limit_needs_sort(query):
        for c in ls.columns:
            if query.dimension_type(c.dimension) == "LONG":
                raise N.UnsupportedQuery(2, f"limit spec sorts on the LONG-output dimension {c.dimension}")
        aggs = {a.name: a for a in query.aggregations}
        dims = set(query.dimensions)
        parts = []
        for c in ls.columns:
            if c.dimension in aggs:
                fn = aggs[c.dimension].compare_key
                kf = (lambda f, n: lambda r: f(r.event[n]))(fn, c.dimension)
            elif query.post_aggregator(c.dimension) is not None:
                prog = Q.compile_post_aggregator(query.aggregations, query.postAggregations, c.dimension, True)
                fn = (lambda pr: lambda v: Q.post_program_order_key(pr.order, Q.post_value_word(v, pr.out_type)))(prog)
                kf = (lambda f, n: lambda r: f(r.event[n]))(fn, c.dimension)
            elif c.dimension in dims:
                sk = O.sort_key(c.dimensionOrder)
                kf = (lambda f, n: lambda r: f(r.event.get(n)))(sk, c.dimension)
            else:
                raise ValueError(f"Unknown column in order clause[{c.dimension}]")
            parts.append((kf, c.direction == "descending"))
        by_dims_first = query._ctx_bool("sortByDimsFirst", False)
        gran_all = query.granularity.is_all

        def key(r):
            ks = tuple(O._Desc(f(r)) if desc else f(r) for f, desc in parts)
            if gran_all:
                return ks
            return ks + (r.timestamp,) if by_dims_first else (r.timestamp,) + ks

        rows = sorted(rows, key=key)  # stable: ties keep the natural order
    return rows if ls.limit is None else rows[:ls.limit]


# ----------------------------------------------------------------------------------------------
# search
# ----------------------------------------------------------------------------------------------
def search_hit_key(sort: str):
    """SearchSortSpec.getComparator (query/search/SearchSortSpec.java:50-66) as a sort key of
    (dimension, value): the value under the sort's StringComparator, then the dimension name
    LEXICOGRAPHIC. Hit values are never null (SearchHit: null -> "")."""
    vk = O.sort_key(sort)
    return lambda dim, value: (vk(value), O.lexicographic_key(dim))


class SearchHitMap:
    """Object2IntRBTreeMap<SearchHit> keyed by the sort's comparator: two hits the comparator calls
    equal (NUMERIC: "1" and "1.0" of one dimension) share one entry, under the first key inserted."""

    def __init__(self, sort: str):
        self.key = search_hit_key(sort)
        self.entries: Dict = {}  # comparator key -> [dimension, value, count]

    def __len__(self):
        return len(self.entries)

    def add_to(self, dim: str, value: Optional[str], n: int):
        value = "" if value is None else value
        e = self.entries.setdefault(self.key(dim, value), [dim, value, 0])
        e[2] += n

    def put_all(self, other: "SearchHitMap"):
        for k, (dim, value, n) in other.entries.items():
            e = self.entries.get(k)
            if e is None:
                self.entries[k] = [dim, value, n]
            else:
                e[2] = n  # put: the value is replaced, the key object stays

    def hits(self, limit: int) -> List[Dict]:
        return [{"dimension": d, "value": v, "count": n}
                for _, (d, v, n) in sorted(self.entries.items(), key=lambda kv: kv[0])][:max(limit, 0)]


def _runner_limit(query: Q.SearchQuery) -> int:
    """SearchThresholdAdjustingQueryRunner (SearchQueryQueryToolChest.java:353-437): a query limit at or
    above maxSearchLimit runs its per-segment runners with maxSearchLimit."""
    return Q.MAX_SEARCH_LIMIT if query.limit >= Q.MAX_SEARCH_LIMIT else query.limit


def search_segment_result(query: Q.SearchQuery, timestamp: int, dims, plans, limit: int) -> Q.Result:
    """SearchQueryRunner.run (query/search/SearchQueryRunner.java:207-260) over the engine's counts of
    one segment. dims: per search dimension (output name, [(value, count) in dictionary id order]);
    plans: the plan the engine took for each (N.SEARCH_PLAN_*). The execution plan is the index-only
    executor over the bitmap dimensions, then the cursor executor over the others
    (UseIndexesStrategy.getExecutionPlan :66-109)."""
    def index_only(dd, lim):  # IndexOnlyExecutor.execute (UseIndexesStrategy.java:236-281)
        ret = SearchHitMap(query.sort)
        for name, vals in dd:
            for value, n in vals:
                if n > 0:
                    ret.add_to(name, value, n)
                    if len(ret) >= lim:
                        return ret
        return ret

    def cursor_based(dd, lim):  # CursorBasedExecutor over the full scan's counts
        ret = SearchHitMap(query.sort)
        for name, vals in dd:
            for value, n in vals:
                if n > 0:
                    ret.add_to(name, value, n)
        if len(ret) >= lim:
            # the reference stops at the row where its map reaches the limit; its counts are those of
            # the rows up to there, which a whole-segment count cannot restate
            raise N.UnsupportedQuery(2, f"search cursor plan reached its limit ({len(ret)} hits >= {lim})")
        return ret

    executors = []
    for kind, fn in ((N.SEARCH_PLAN_INDEX, index_only), (N.SEARCH_PLAN_CURSOR, cursor_based)):
        dd = [d for d, p in zip(dims, plans) if p == kind]
        if dd:
            executors.append((fn, dd))
    ret = SearchHitMap(query.sort)
    remain = limit
    for fn, dd in executors:
        ret.put_all(fn(dd, remain))
        remain -= len(ret)
    return Q.Result(timestamp, ret.hits(limit))


def _accepted_ids(seg: GpuSegment, dim: str, query: Q.SearchQuery) -> np.ndarray:
    """Dictionary ids of `dim` the query's SearchQuerySpec accepts (cached per segment and spec)."""
    if seg.column_type(dim) == N.COL_MISSING:
        return np.zeros(0, dtype=np.int32)
    if seg.column_type(dim) != N.COL_STRING:
        return np.zeros(1, dtype=np.int32)  # (the engine refuses the column: DG_ERR_UNSUPPORTED)
    cache = seg.__dict__.setdefault("_search_cache", {})
    key = (dim, repr(sorted(query.query.items(), key=lambda kv: kv[0])))
    if key not in cache:
        cache[key] = np.asarray([i for i, v in enumerate(seg.dictionary(dim)) if query.accept(v)], dtype=np.int32)
    return cache[key]


def search_dimensions(seg: GpuSegment, query: Q.SearchQuery) -> List[Tuple[str, str]]:
    """SearchStrategy.getDimsToSearch: the query's dimension specs, or every (string) dimension of the
    segment in its order."""
    if query.dimension_specs:
        return list(query.dimension_specs)
    return [(c, c) for c in seg.columns() if c != "__time" and seg.column_type(c) == N.COL_STRING]


def search_counts(segments: Sequence[GpuSegment], query: Q.SearchQuery, dims: Sequence[str],
                  ids: Sequence[Sequence[np.ndarray]], stats: Optional[RunStats] = None,
                  cancel: Optional[ctypes.c_int32] = None):
    """One dg_search_run over segments of one device. ids[d][i]: accepted ids of dims[d] in segment i
    (int32, ascending). Returns (counts[d][i] int64 arrays, plans[i][d])."""
    n, nd = len(segments), len(dims)
    scan, keep = N.make_scan(query, Q, segments=segments, cancel=cancel)
    sdims = (N.dg_search_dim * max(nd, 1))()
    total = 0
    for d, name in enumerate(dims):
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in ids[d]]
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        cnt = np.asarray([len(a) for a in arrs], dtype=np.int32)
        nm = name.encode("utf-8")
        keep += [arrs, ptrs, cnt, nm]
        sdims[d].dimension = nm
        sdims[d].ids = ctypes.cast(ptrs, ctypes.c_void_p)
        sdims[d].n_ids = cnt.ctypes.data
        total += int(cnt.sum())
    st = N.dg_search(sdims, nd, N.SEARCH_CURSOR_ONLY if query.strategy == "cursorOnly" else N.SEARCH_USE_INDEXES)
    out = np.zeros(max(total, 1), dtype=np.int64)
    plan = np.zeros(max(n * nd, 1), dtype=np.int32)
    m = N.dg_metrics()
    N.check(N.lib().dg_search_run(_handles(segments), n, ctypes.byref(scan), ctypes.byref(st), out.ctypes.data,
                                  plan.ctypes.data, ctypes.byref(m)))
    if stats is not None:
        stats.add(m)
    counts = [[None] * n for _ in range(nd)]
    pos = 0
    for i in range(n):
        for d in range(nd):
            k = len(ids[d][i])
            counts[d][i] = out[pos:pos + k]
            pos += k
    return counts, plan[:n * nd].reshape(n, nd)


def search_per_segment(segments: Sequence[GpuSegment], query: Q.SearchQuery, stats: Optional[RunStats] = None,
                       cancel: Optional[ctypes.c_int32] = None) -> List[List[Q.Result]]:
    """SearchQueryRunnerFactory.createRunner(segment).run for every segment (each device's segments in
    one dg_search_run), behind the toolchest's threshold adjustment."""
    query.strategy  # (refuses searchStrategy auto before any work)
    limit = _runner_limit(query)
    out: List[List[Q.Result]] = [[] for _ in segments]
    for _, idx in _group_by_device(segments).items():
        segs = [segments[i] for i in idx]
        per_seg = [search_dimensions(s, query) for s in segs]
        names: List[str] = []
        for specs in per_seg:
            for d, _ in specs:
                if d not in names:
                    names.append(d)
        # a dimension a segment does not search (the default list of another segment) gets no ids there
        ids = [[_accepted_ids(s, d, query) if any(d == x for x, _ in specs) else np.zeros(0, np.int32)
                for s, specs in zip(segs, per_seg)] for d in names]
        counts, plans = search_counts(segs, query, names, ids, stats, cancel)
        for k, i in enumerate(idx):
            seg = segs[k]
            dd, pp = [], []
            for d, o in per_seg[k]:
                x = names.index(d)
                if seg.column_type(d) != N.COL_STRING:
                    continue
                dic = seg.dictionary(d)
                dd.append((o, [(dic[j], int(c)) for j, c in zip(ids[x][k], counts[x][k])]))
                pp.append(int(plans[k][x]))
            r = search_segment_result(query, seg.interval[0], dd, pp, limit)
            out[i] = [Q.Result(r.timestamp, r.value[:query.limit])]
    return out


def search_binary_fn(query: Q.SearchQuery, r1: Optional[Q.Result], r2: Optional[Q.Result]) -> Optional[Q.Result]:
    """SearchBinaryFn.apply (query/search/SearchBinaryFn.java:53-117): the two sorted hit lists merged
    under the sort's comparator, equal (dimension, value) hits adding their counts (a hit without a
    count makes the sum countless); the limit applies under ALL granularity only."""
    if r1 is None:
        return r2
    if r2 is None:
        return r1
    gran = query.granularity
    limit = query.limit if gran.is_all else -1
    key = search_hit_key(query.sort)
    merged = heapq.merge(r1.value, r2.value, key=lambda h: key(h["dimension"], h["value"]))
    results: List[Dict] = []
    prev = None
    for hit in merged:
        if prev is None:
            prev = hit
            continue
        if prev["dimension"] == hit["dimension"] and prev["value"] == hit["value"]:
            both = prev.get("count") is not None and hit.get("count") is not None
            prev = {"dimension": prev["dimension"], "value": prev["value"],
                    "count": prev["count"] + hit["count"] if both else None}
        else:
            results.append(prev)
            prev = hit
            if limit > 0 and len(results) >= limit:
                break
    if prev is not None and (limit < 0 or len(results) < limit):
        results.append(prev)
    return Q.Result(r1.timestamp if gran.is_all else gran.bucket_start(r1.timestamp), results)


def merge_search(query: Q.SearchQuery, per_segment: List[List[Q.Result]]) -> List[Q.Result]:
    """SearchQueryQueryToolChest.mergeResults: ResultMergeQueryRunner folds the runners' results of one
    granularity bucket (time, then runner order) with SearchBinaryFn under the query's limit."""
    gran = query.granularity
    flat = sorted(((r.timestamp, si, k, r) for si, rs in enumerate(per_segment) for k, r in enumerate(rs)),
                  key=lambda x: (x[0], x[1], x[2]))
    merged: "OrderedDict[int, Q.Result]" = OrderedDict()
    for ts, _, _, r in flat:
        b = 0 if gran.is_all else gran.bucket_start(ts)
        merged[b] = search_binary_fn(query, merged.get(b), r)
    return [merged[b] for b in sorted(merged)]


def run_search(segments: Sequence[GpuSegment], query: Q.SearchQuery, stats: Optional[RunStats] = None) -> List[Q.Result]:
    return merge_search(query, search_per_segment(segments, query, stats))


# ----------------------------------------------------------------------------------------------
# scan
# ----------------------------------------------------------------------------------------------
def scan_native_column(column: str, legacy: bool) -> str:
    """The segment column a result column reads: legacy ``timestamp`` is __time (ScanQueryEngine.java:152-154)."""
    return Q.SCAN_TIME_COLUMN if legacy and column == Q.SCAN_LEGACY_TIMESTAMP else column


def scan_segment_columns(seg: GpuSegment, query: Q.ScanQuery) -> List[str]:
    """The column list of one segment's batches (ScanQueryEngine.java:85-113): the dimensions are
    getAvailableDimensions, the metrics every other column in the segment's column order."""
    if query.columns:
        return query.column_list([], [])
    dims = [d for d in seg.dimensions() if d != Q.SCAN_TIME_COLUMN]
    mets = [c for c in seg.columns() if c != Q.SCAN_TIME_COLUMN and c not in dims]
    return query.column_list(dims, mets)


def scan_events(columns: Sequence[str], arrays: Dict[str, object], dictionaries: Dict[str, Sequence[Optional[str]]],
                legacy: bool, compacted: bool = False, n: Optional[int] = None) -> List:
    """One batch's events from its columns (getColumnValue, ScanQueryEngine.java:238-250). arrays[column]:
    None for a column the segment lacks (null in every row), an int64 / float32 / float64 array, an int32
    array of dictionary ids (dictionaries[column] resolves them, None for the empty string), or (ids,
    offsets) for a multi-value column (DimensionSelector.defaultGetObject: null for an empty row, the value
    of a one-element row, else the list). In legacy mode ``timestamp`` holds __time and is shown as a UTC
    ISO instant. Returns dicts in column order (list) or lists (compactedList)."""
    cols: List[List] = []
    for c in columns:
        a = arrays.get(c)
        if a is None:
            cols.append(None)
            continue
        if isinstance(a, tuple):
            ids, offs = a
            d = dictionaries[c]
            vals = [d[i] for i in ids.tolist()]
            o = [int(x) for x in offs]
            col = []
            for k in range(len(o) - 1):
                row = vals[o[k]:o[k + 1]]
                col.append(None if not row else row[0] if len(row) == 1 else row)
        elif legacy and c == Q.SCAN_LEGACY_TIMESTAMP:
            col = [Q.format_time(int(t)) for t in a.tolist()]
        elif c in dictionaries and a.dtype == np.int32:
            d = dictionaries[c]
            col = [d[i] for i in a.tolist()]
        else:
            col = a.astype(np.float64).tolist() if a.dtype == np.float32 else a.tolist()  # (float32 widens exactly)
        if n is None:
            n = len(col)
        cols.append(col)
    n = n or 0
    cols = [c if c is not None else [None] * n for c in cols]
    if compacted:
        return [list(r) for r in zip(*cols)] if cols else [[] for _ in range(n)]
    names = list(columns)
    return [dict(zip(names, r)) for r in zip(*cols)] if cols else [{} for _ in range(n)]


def scan_batches(rowset, seg_ids: Sequence[str], seg_columns: Sequence[Sequence[str]],
                 native_index: Sequence[Sequence[int]], dictionaries, query: Q.ScanQuery) -> List[Q.ScanResultValue]:
    """The rowset cut into ScanResultValue batches of at most batchSize rows, segment by segment (a batch
    never spans segments, ScanQueryEngine.java:162-236); a segment without kept rows yields none.
    rowset: rows(seg) and fetch(seg, col, start, count) -> (values, offsets); native_index[s][k]: the rowset
    column of seg_columns[s][k]; dictionaries(s, column) -> the segment's dictionary."""
    out: List[Q.ScanResultValue] = []
    compacted = query.resultFormat == "compactedList"
    for s, sid in enumerate(seg_ids):
        rows = rowset.rows(s)
        cols = list(seg_columns[s])
        for start in range(0, rows, query.batchSize):
            count = min(query.batchSize, rows - start)
            arrays, dicts = {}, {}
            for c, x in zip(cols, native_index[s]):
                vals, offs = rowset.fetch(s, x, start, count)
                if vals is None:
                    arrays[c] = None
                    continue
                arrays[c] = vals if offs is None else (vals, offs)
                if vals.dtype == np.int32:
                    dicts[c] = dictionaries(s, c)
            out.append(Q.ScanResultValue(sid, cols, scan_events(cols, arrays, dicts, query.legacy, compacted, count)))
    return out


def scan_rows(segments: Sequence[GpuSegment], columns: Sequence[str], query: Q.ScanQuery, limit: Optional[int],
              stats: Optional[RunStats] = None, cancel: Optional[ctypes.c_int32] = None) -> "N.RowSet":
    """One dg_rows_run over segments of one context: the first ``limit`` selected rows (None: all) of the
    segments in order, the named segment columns gathered into a resident rowset."""
    scan, keep = N.make_scan(query, Q, segments=segments, cancel=cancel)
    names = (ctypes.c_char_p * max(len(columns), 1))(*[c.encode("utf-8") for c in columns])
    spec = N.dg_rows(names, len(columns), int(limit) if limit is not None else 0)
    h = ctypes.c_void_p()
    m = N.dg_metrics()
    N.check(N.lib().dg_rows_run(_handles(segments), len(segments), ctypes.byref(scan), ctypes.byref(spec),
                                ctypes.byref(h), ctypes.byref(m)))
    if stats is not None:
        stats.add(m)
    del keep
    return N.RowSet(h, len(segments), len(columns))


def _consecutive_by_context(segments: Sequence[GpuSegment]) -> List[List[int]]:
    """Maximal runs of consecutive segments on one context (scan results keep the segment order)."""
    runs: List[List[int]] = []
    for i, s in enumerate(segments):
        if runs and segments[runs[-1][-1]].context is s.context:
            runs[-1].append(i)
        else:
            runs.append([i])
    return runs


def _scan_run(segs: Sequence[GpuSegment], query: Q.ScanQuery, limit: Optional[int], stats, cancel):
    """(rowset, batches-builder arguments) of one native call."""
    seg_columns = [scan_segment_columns(s, query) for s in segs]
    native: List[str] = []
    for cols in seg_columns:
        for c in cols:
            nc = scan_native_column(c, query.legacy)
            if nc not in native:
                native.append(nc)
    index = [[native.index(scan_native_column(c, query.legacy)) for c in cols] for cols in seg_columns]
    rowset = scan_rows(segs, native, query, limit, stats, cancel)
    return rowset, seg_columns, index


def run_scan(segments: Sequence[GpuSegment], query: Q.ScanQuery, stats: Optional[RunStats] = None,
             cancel: Optional[ctypes.c_int32] = None, rows_fn=None) -> List[Q.ScanResultValue]:
    """ScanQueryRunnerFactory.mergeRunners(...).run (ScanQueryRunnerFactory.java:64-96): the segments'
    batches concatenated in runner order under one running count (the response context's, ScanQueryEngine
    .java:68-73,:125): one native call per run of consecutive segments on one context, each with the limit
    that is left; a run reached once the limit is full is not started. rows_fn (tests): stands in for
    _scan_run."""
    rows_fn = rows_fn or _scan_run
    out: List[Q.ScanResultValue] = []
    remaining = query.row_limit
    for idx in _consecutive_by_context(segments):
        if remaining is not None and remaining <= 0:
            break
        segs = [segments[i] for i in idx]
        rowset, seg_columns, index = rows_fn(segs, query, remaining, stats, cancel)
        try:
            out.extend(scan_batches(rowset, [s.identifier for s in segs], seg_columns, index,
                                    lambda s, c: segs[s].dictionary(scan_native_column(c, query.legacy)), query))
            if remaining is not None:
                remaining -= rowset.rows(-1)
        finally:
            rowset.close()
    return out


def merge_scan(query: Q.ScanQuery, per_segment: List[List[Q.ScanResultValue]]) -> List[Q.ScanResultValue]:
    """ScanQueryQueryToolChest.mergeResults over separately run runners: concatenation in runner order,
    cut at the limit by ScanQueryLimitRowIterator (the batch that crosses it keeps its first events)."""
    out: List[Q.ScanResultValue] = []
    remaining = query.row_limit
    for batches in per_segment:
        for b in batches:
            if remaining is not None:
                if remaining <= 0:
                    return out
                if len(b.events) > remaining:
                    b = Q.ScanResultValue(b.segmentId, b.columns, b.events[:remaining])
                remaining -= len(b.events)
            out.append(b)
    return out


# ----------------------------------------------------------------------------------------------
# factories (QueryRunnerFactory surface)
# ----------------------------------------------------------------------------------------------
def exact_granularity(query, segments: Sequence[GpuSegment]):
    """A period granularity on the fixed grid that is exact only from some instant on
    (Granularity.exact_from: the hours branch gives timestamps before its origin the aligned point
    after them, PeriodGranularity.java:313-326; truncateMillisPeriod's Java remainders misalign
    negative timestamps): when the data reaches before that instant, the query with the calendar
    restatement instead, its interval clipped to the data so the bucket list stays finite."""
    g = query.granularity
    ef = getattr(g, "exact_from", None)
    if ef is None:
        return query
    live = [s for s in segments if s.num_rows]
    if not live or min(s.min_time for s in live) >= ef or query.interval[0] >= ef:
        return query
    lo = max(query.interval[0], min(s.min_time for s in live))
    hi = min(query.interval[1], max(s.max_time for s in live) + 1)
    return dataclasses.replace(query, intervals=[(lo, max(hi, lo + 1))], granularity=g.calendar_form())


def segment_queries(query, segments: Sequence[GpuSegment]):
    """Calendar granularities: makeCursors iterates gran.getIterable(actualInterval) per segment
    (QueryableIndexStorageAdapter.java:367-456; actualInterval = [max(query start, minTime),
    min(query end, bucketEnd(maxTime)))), i.e. bucketStart(actual start) and increments from there.
    With an origin whose day clamps (P1M from Jan 31: truncate gives Apr 30, the chain from the query
    start Apr 28) that chain is not a slice of the query interval's, which the engine buckets every
    segment of a call on. Returns None when every segment's chain lies on the query's list (the
    batched path is exact); else one query per segment (None for a segment outside the interval)
    whose interval is the segment's actual interval, so each runs on its own chain."""
    g = query.granularity
    if not g.is_calendar:
        return None
    qs, qe = query.interval
    qlist = g.bucket_starts((qs, qe))
    qpos = {t: i for i, t in enumerate(qlist)}
    out, diverge = [], False
    for s in segments:
        lo, hi = max(qs, s.min_time), min(qe, g.bucket_end(s.max_time))
        if s.num_rows == 0 or hi <= lo:
            out.append(None)
            continue
        sl = g.bucket_starts((lo, hi))
        i = qpos.get(sl[0])
        diverge |= i is None or qlist[i:i + len(sl)] != sl
        out.append(dataclasses.replace(query, intervals=[(lo, hi)]))
    return out if diverge else None


def _run_split(factory, segments, queries, query, stats):
    """Per segment on its own bucket chain (segment_queries), merged by the toolchest (the
    reference's per-segment runners + mergeResults)."""
    per = []
    for s, q in zip(segments, queries):
        if q is not None:
            per.extend(factory.per_segment([s], q, stats))
    return factory.toolchest.merge(query, per)


class SegmentQueryRunner:
    """QueryRunner for one segment (QueryRunnerFactory.createRunner)."""

    def __init__(self, factory, segment: GpuSegment):
        self.factory, self.segment = factory, segment

    def run(self, query):
        query = exact_granularity(V.lower_query(query, [self.segment]), [self.segment])
        split = segment_queries(query, [self.segment])
        if split is not None:
            return _run_split(self.factory, [self.segment], split, query, None)
        return self.factory.toolchest.merge(query, self.factory.per_segment([self.segment], query))


class MergedQueryRunner:
    """QueryRunnerFactory.mergeRunners: all segments of one device run as one batched native call."""

    def __init__(self, factory, runners: Iterable[SegmentQueryRunner]):
        self.factory = factory
        self.segments = [r.segment for r in runners]
        self.stats = RunStats()

    def run(self, query):
        query = exact_granularity(V.lower_query(query, self.segments, self.stats), self.segments)
        split = segment_queries(query, self.segments)
        if split is not None:
            return _run_split(self.factory, self.segments, split, query, self.stats)
        return self.factory.run_merged(self.segments, query, self.stats)


class _ToolChest:
    def __init__(self, merge_fn):
        self.merge = merge_fn


class TimeseriesQueryRunnerFactory:
    toolchest = _ToolChest(merge_timeseries)

    @staticmethod
    def per_segment(segments, query, stats=None):
        return timeseries_per_segment(segments, query, stats)

    def run_merged(self, segments, query, stats=None):
        # every device's segments in one engine call, the buckets folded natively (dg_timeseries_merge)
        return run_timeseries(segments, query, stats)

    def createRunner(self, segment):
        return SegmentQueryRunner(self, segment)

    def mergeRunners(self, runners):
        return MergedQueryRunner(self, runners)


class TopNQueryRunnerFactory(TimeseriesQueryRunnerFactory):
    toolchest = _ToolChest(merge_topn)

    @staticmethod
    def per_segment(segments, query, stats=None):
        return topn_per_segment(segments, query, stats)

    def run_merged(self, segments, query, stats=None):
        # TopNBinaryFn fold inside the engine (dg_topn_merge)
        return run_topn(segments, query, stats)


class GroupByQueryRunnerFactory(TimeseriesQueryRunnerFactory):
    toolchest = _ToolChest(merge_groupby)

    @staticmethod
    def per_segment(segments, query, stats=None):
        return groupby_per_segment(segments, query, stats)

    def run_merged(self, segments, query, stats=None):
        # the engine merges each device's segments (GroupByMergingQueryRunnerV2) and the devices'
        # results by value on the device (dg_groupby_merge_devices: peer copies, no host merge)
        if len(_group_by_device(segments)) == 1:
            return self.toolchest.merge(query, groupby_per_device(segments, query, stats, post_process=True))
        res = groupby_merge_devices(segments, query, stats)
        try:
            for r in res:  # (each key range keeps its first `limit` groups; the toolchest re-limits)
                r.apply_limit_push_down()
                # a key range holds whole groups: having per range is exact, and the first `limit` of every
                # range contain the first `limit` of them all
                if r.apply_post_process() and stats is not None:
                    stats.post.append(r.post_info)
            return self.toolchest.merge(query, [r.fetch() for r in res])
        finally:
            for r in res:
                r.release()


class SearchQueryRunnerFactory(TimeseriesQueryRunnerFactory):
    toolchest = _ToolChest(merge_search)

    @staticmethod
    def per_segment(segments, query, stats=None):
        return search_per_segment(segments, query, stats)

    def run_merged(self, segments, query, stats=None):
        return run_search(segments, query, stats)


class ScanQueryRunnerFactory(TimeseriesQueryRunnerFactory):
    """ScanQueryRunnerFactory (query/scan/ScanQueryRunnerFactory.java:64-96): createRunner(segment) runs one
    segment under the whole limit; the merged runner concatenates the segments' batches and shares the
    running count between them."""
    toolchest = _ToolChest(merge_scan)

    @staticmethod
    def per_segment(segments, query, stats=None):
        return [run_scan([s], query, stats) for s in segments]

    def run_merged(self, segments, query, stats=None):
        return run_scan(segments, query, stats)


FACTORIES = {Q.TimeseriesQuery: TimeseriesQueryRunnerFactory(), Q.TopNQuery: TopNQueryRunnerFactory(),
             Q.GroupByQuery: GroupByQueryRunnerFactory(), Q.SearchQuery: SearchQueryRunnerFactory(),
             Q.ScanQuery: ScanQueryRunnerFactory()}


def run_query(query, segments: Sequence[GpuSegment], stats: Optional[RunStats] = None):
    """QueryRunnerFactoryConglomerate lookup + mergeRunners over the given segments."""
    if isinstance(query, dict):
        query = Q.query_from_json(query)
    f = FACTORIES[type(query)]
    runner = f.mergeRunners([f.createRunner(s) for s in segments])
    if stats is not None:
        runner.stats = stats
    return finalize_results(query, runner.run(query))
