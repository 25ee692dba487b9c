"""Virtual columns, aggregator expressions and expression filters as derived columns.

The reference evaluates a numeric expression per row in three places: ExpressionVirtualColumn
(segment/virtual/ExpressionVirtualColumn.java), the `expression` of the simple aggregator factories
(AggregatorUtil.java:176-288) and ExpressionDimFilter (segment/filter/ExpressionFilter.java:54-66). Here each
distinct expression is evaluated once per segment on the GPU into a derived column (dg_segment_derive_column) and
the query is rewritten to read that column like a stored one, so the engines, the merges and the result
builders see an ordinary query:

  use                                             derived column
  aggregator expression, or fieldName naming      the program's natural type (long or double); the aggregator's
  a virtual column                                selector coercion then does what ExpressionColumnValueSelector.
                                                  getLong / getFloat / getDouble do (ExpressionSelectors.java:66-93)
  selector / in / bound filter on a virtual       cast to the virtual column's outputType: the matcher is chosen by
  column                                          capabilities().getType() (ExpressionVirtualColumn.java:104-107)
  expression filter                               cast to LONG, then the NUMERIC bound `> 0` on it
                                                  (Evals.asBoolean(selector.getLong()): 0.5 does not match)
  groupBy / topN dimension over a virtual column  outputType LONG only, then a LONG column to the engine
                                                  (GroupByQueryEngineV2.java:235-260); any other type is refused

A derived column is named by a digest of its program, so a repeat of the query, or another query with the same
expression, builds nothing, and two queries that use one virtual-column name for different expressions cannot
collide. Each costs 8 B (FLOAT: 4 B) per row of HBM; a segment keeps at most GpuSegment.MAX_DERIVED of them,
least recently used dropped first, never one the running query uses. A GpuSegment serves one querying thread at a
time: the columns of a lowered query are held from lower_query to the end of the engine call only against that
thread's own evictions (GpuSegment.derive), so callers that share a segment between threads serialise their
queries on it.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N
from . import query as Q

_COL_NAMES = {N.COL_LONG: "LONG", N.COL_FLOAT: "FLOAT", N.COL_DOUBLE: "DOUBLE", N.COL_STRING: "STRING",
              N.COL_UNSUPPORTED: "UNSUPPORTED"}
_COL_CODES = {"LONG": N.COL_LONG, "FLOAT": N.COL_FLOAT, "DOUBLE": N.COL_DOUBLE}
_LOWERED = (Q.TimeseriesQuery, Q.TopNQuery, Q.GroupByQuery)


def compile_for_segments(ast, out_type: Optional[str], segments) -> Q.ExprProgram:
    """The expression compiled against every segment's column types, cast to out_type (None: its natural type).
    One call hands the engine one query for all its segments, so the programs must agree."""
    prog = None
    for seg in segments:
        p = Q.compile_expression(ast, lambda name, seg=seg: _COL_NAMES.get(seg.column_type(name)))
        p = p.natural() if out_type is None else p.with_output(out_type)
        if prog is not None and (p.ops, p.inputs, p.out_type) != (prog.ops, prog.inputs, prog.out_type):
            raise N.UnsupportedQuery(2, "expression: its columns' types differ between the call's segments")
        prog = p
    return prog


def lower_query(query, segments: Sequence, stats=None, cancel=None):
    """The query with every expression replaced by a derived column of the given segments (built here unless
    already there). A query without expressions, or one lowered before, is returned as it is.
    stats (RunStats): derived_built / derived_reused / derived_build_ms are added up."""
    if not isinstance(query, _LOWERED) or not Q.query_uses_expressions(query):
        return query
    segments = list(segments)
    if not segments:
        raise N.UnsupportedQuery(2, "expressions need the call's segments")
    vcs: Dict[str, Q.ExpressionVirtualColumn] = {v.name: v for v in query.virtualColumns}
    needed: Dict[str, Q.ExprProgram] = {}

    def stored_only(ast, what: str):
        # the reference binds virtual columns before stored ones; the engine derives from stored columns only, so
        # an expression that names a virtual column is refused by name (never compiled against a stored column
        # of that name, never reported as a missing column)
        for ident in Q.expression_identifiers(ast):
            if ident in vcs:
                raise N.UnsupportedQuery(2, f"{what} references virtual column {ident}")
        return ast

    def need(ast, out_type: Optional[str]) -> str:
        prog = compile_for_segments(ast, out_type, segments)
        name = prog.digest()
        needed[name] = prog
        return name

    def typed(vc: Q.ExpressionVirtualColumn, what: str) -> str:
        if vc.outputType not in _COL_CODES:
            raise N.UnsupportedQuery(2, f"{what} on virtual column {vc.name} of output type {vc.outputType}")
        return need(vc.ast, vc.outputType)

    def lower_filter(f):
        if f is None:
            return None
        if isinstance(f, (Q.AndDimFilter, Q.OrDimFilter)):
            return type(f)([lower_filter(c) for c in f.fields])
        if isinstance(f, Q.NotDimFilter):
            return Q.NotDimFilter(lower_filter(f.field))
        if isinstance(f, Q.ExpressionDimFilter):
            return Q.BoundDimFilter(need(stored_only(f.ast, "expression filter"), "LONG"), lower="0", lowerStrict=True, ordering="numeric")
        vc = vcs.get(getattr(f, "dimension", None))
        if vc is None:
            return f
        if not isinstance(f, (Q.SelectorDimFilter, Q.InDimFilter, Q.BoundDimFilter)):
            raise N.UnsupportedQuery(2, f"filter {type(f).__name__} on virtual column {vc.name}")
        return dataclasses.replace(f, dimension=typed(vc, f"filter {type(f).__name__}"))

    aggs = []
    for a in query.aggregations:
        field, flt = a.fieldName, lower_filter(a.filter)
        if a.expression is not None:
            field = need(stored_only(a.ast, f"the expression of aggregator {a.name}"), None)
        elif field in vcs:
            field = need(vcs[field].ast, None)
        aggs.append(a if (field, flt) == (a.fieldName, a.filter) else Q.AggregatorFactory(a.type, a.name, field, flt))
    changes = dict(filter=lower_filter(query.filter), aggregations=aggs, virtualColumns=[])
    dims = [query.dimension] if isinstance(query, Q.TopNQuery) else list(getattr(query, "dimensions", []))
    derived_dims = dict(getattr(query, "derivedDimensions", {}))
    for d in dims:
        vc = vcs.get(d)
        if vc is None:
            continue
        if vc.outputType != "LONG":
            raise N.UnsupportedQuery(2, f"dimension over virtual column {d} of output type {vc.outputType} "
                                        "(only LONG virtual columns are grouped on the device)")
        derived_dims[d] = need(vc.ast, "LONG")
    if dims:
        changes["derivedDimensions"] = derived_dims
    built = reused = 0
    build_ms = 0.0
    # the context's timeout is one budget for the builds and the query call after them: each build gets what is
    # left of it, and so does the lowered query
    timeout = int((getattr(query, "context", None) or {}).get("timeout", 0) or 0)
    t0 = time.monotonic()

    def left() -> int:
        if timeout <= 0:
            return 0
        ms = timeout - int((time.monotonic() - t0) * 1000.0)
        if ms <= 0:
            raise N.DruidGpuError(N.ERR_TIMEOUT, f"query timeout ({timeout} ms) while its derived columns were built")
        return ms

    for seg in segments:
        for name, prog in needed.items():
            info = seg.derive(name, prog.ops, prog.inputs, _COL_CODES[prog.out_type], in_use=needed, cancel=cancel,
                              timeout_ms=left())
            built += int(info["built"])
            reused += int(not info["built"])
            build_ms += info["build_ms"]
    if stats is not None:
        stats.derived_built += built
        stats.derived_reused += reused
        stats.derived_build_ms += build_ms
    if timeout > 0:
        changes["context"] = dict(query.context, timeout=left())
    return dataclasses.replace(query, **changes)
