"""Device-resident segments (the QueryableIndex / StorageAdapter side of the boundary).

``GpuSegment(path, device)`` maps a Druid v9 segment directory into HBM through
``dg_segment_attach`` (IndexIO.loadIndex, processing/.../segment/IndexIO.java:569-663) and exposes
the StorageAdapter facts the runners need: row count, data interval, min/max time
(StorageAdapter.getMinTime/getMaxTime), column types and dictionaries (lookupName).
"""
from __future__ import annotations

import ctypes
import threading
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _native as N
from . import ordering as O


class GpuContext:
    """One HIP device + stream (``dg_context``); shared by every segment attached to that device."""

    _by_device: Dict[int, "GpuContext"] = {}
    _lock = threading.Lock()

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        N.check(N.lib().dg_context_create(device, ctypes.byref(h)))
        self.device = device
        self.handle = h

    @classmethod
    def get(cls, device: int = 0) -> "GpuContext":
        with cls._lock:
            if device not in cls._by_device:
                cls._by_device[device] = GpuContext(device)
            return cls._by_device[device]

    def set_stream(self, hip_stream_ptr: Optional[int]):
        N.check(N.lib().dg_context_set_stream(self.handle, ctypes.c_void_p(hip_stream_ptr or 0)))


def device_count() -> int:
    n = ctypes.c_int()
    N.lib().dg_device_count(ctypes.byref(n))
    return n.value


class GpuSegment:
    """A Druid segment resident on one GPU (QueryableIndexSegment equivalent)."""

    _ids = 0

    def __init__(self, path: str, device: int = 0, context: Optional[GpuContext] = None):
        self.context = context or GpuContext.get(device)
        h = ctypes.c_void_p()
        N.check(N.lib().dg_segment_attach(self.context.handle, path.encode(), ctypes.byref(h)))
        self._init(h, path)

    @classmethod
    def from_handle(cls, handle: ctypes.c_void_p, context: GpuContext, name: str) -> "GpuSegment":
        """A segment the engine built otherwise (dg_segment_from_rows: an in-memory index)."""
        seg = cls.__new__(cls)
        seg.context = context
        seg._init(handle, name)
        return seg

    def _init(self, h: ctypes.c_void_p, path: str):
        self.handle = h
        self.path = path
        GpuSegment._ids += 1
        self.identifier = f"{path}#{GpuSegment._ids}"
        L = N.lib()
        self.num_rows = int(L.dg_segment_num_rows(h))
        s, e = ctypes.c_int64(), ctypes.c_int64()
        L.dg_segment_interval(h, ctypes.byref(s), ctypes.byref(e))
        self.interval = (s.value, e.value)
        L.dg_segment_time_bounds(h, ctypes.byref(s), ctypes.byref(e))
        self.min_time, self.max_time = s.value, e.value
        self._dicts: Dict[str, List[Optional[str]]] = {}
        self._orders: Dict[Tuple[str, int], O.DictionaryOrder] = {}
        self._types: Dict[str, int] = {}  # a segment's columns never change once attached / built
        self._values: Dict[str, Dict[int, Optional[str]]] = {}  # dim_value lookups already made
        self._derived: "OrderedDict[str, int]" = OrderedDict()  # derived column -> its HBM bytes, LRU first
        self._derive_lock = threading.RLock()  # (derive / drop_derived: the LRU and the engine stay in step)

    # -- StorageAdapter-ish facts ------------------------------------------------------------
    def columns(self) -> List[str]:
        L = N.lib()
        return [L.dg_segment_column_name(self.handle, i).decode() for i in range(L.dg_segment_num_columns(self.handle))]

    def dimensions(self) -> List[str]:
        """StorageAdapter.getAvailableDimensions: index.drd's dimension list (a segment from rows: its
        string columns in the order given)."""
        L = N.lib()
        return [L.dg_segment_dimension_name(self.handle, i).decode()
                for i in range(L.dg_segment_num_dimensions(self.handle))]

    def column_type(self, name: str) -> int:
        t = self._types.get(name)
        if t is None:
            t = self._types[name] = N.lib().dg_segment_column_type(self.handle, name.encode())
        return t

    def device_bytes(self) -> int:
        return int(N.lib().dg_segment_device_bytes(self.handle))

    def long_dim_info(self, column: str) -> Dict:
        """The cached long-dimension encoding of a LONG column (dg_debug_long_dim_info): whether a groupBy
        has built it, its cardinality, the HBM it holds and the device time of its build."""
        built, card, nbytes, ms = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        N.check(N.lib().dg_debug_long_dim_info(self.handle, column.encode(), ctypes.byref(built), ctypes.byref(card),
                                               ctypes.byref(nbytes), ctypes.byref(ms)))
        return {"built": bool(built.value), "cardinality": card.value, "device_bytes": nbytes.value, "build_ms": ms.value}

    def numeric_dim_info(self, column: str) -> Dict:
        """long_dim_info for any numeric column (dg_segment_numeric_dim_info): the encoding the first groupBy or
        topN over the column builds."""
        built, card, nbytes, ms = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        N.check(N.lib().dg_segment_numeric_dim_info(self.handle, column.encode(), ctypes.byref(built),
                                                    ctypes.byref(card), ctypes.byref(nbytes), ctypes.byref(ms)))
        return {"built": bool(built.value), "cardinality": card.value, "device_bytes": nbytes.value, "build_ms": ms.value}

    def numeric_dim_values(self, column: str, ids) -> np.ndarray:
        """The values of a numeric dimension's result ids (dg_segment_numeric_dim_values) in the column's own
        type: int64, float32 or float64 (a NaN is the canonical one)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.zeros(len(ids), dtype=np.uint64)
        N.check(N.lib().dg_segment_numeric_dim_values(self.handle, column.encode(), ids.ctypes.data, len(ids),
                                                      out.ctypes.data))
        t = self.column_type(column)
        if t == N.COL_FLOAT:
            return out.astype(np.uint32).view(np.float32)
        return out.view(np.float64 if t == N.COL_DOUBLE else np.int64)

    def cardinality(self, dim: str) -> int:
        return int(N.lib().dg_segment_dim_cardinality(self.handle, dim.encode()))

    def dictionary(self, dim: str) -> List[Optional[str]]:
        """Sorted dictionary of a string dimension; null (empty) values are None."""
        if dim not in self._dicts:
            if self.column_type(dim) != N.COL_STRING:
                self._dicts[dim] = [None]
            else:
                card = self.cardinality(dim)
                offs = np.zeros(card + 1, dtype=np.int64)
                total = ctypes.c_int64()
                N.check(N.lib().dg_segment_dim_dictionary(self.handle, dim.encode(), None, None, ctypes.byref(total)))
                buf = ctypes.create_string_buffer(max(total.value, 1))
                N.check(N.lib().dg_segment_dim_dictionary(self.handle, dim.encode(), offs.ctypes.data, buf,
                                                          ctypes.byref(total)))
                raw = buf.raw
                vals: List[Optional[str]] = []
                for i in range(card):
                    a, b = int(offs[i]), int(offs[i + 1])
                    vals.append(raw[a:b].decode("utf-8") if b > a else None)
                self._dicts[dim] = vals
        return self._dicts[dim]

    def dim_order(self, dim: str, ordering: str, inverted: bool = False) -> Optional[O.DictionaryOrder]:
        """The dictionary's order under a topN comparator, handed to the engine once
        (dg_segment_set_dim_order); None for a missing dimension (its only value is null)."""
        if self.column_type(dim) != N.COL_STRING:
            return None
        slot = O.order_slot(ordering, inverted)
        key = (dim, slot)
        if key not in self._orders:
            order = O.DictionaryOrder(self.dictionary(dim), ordering, inverted)
            rank = np.ascontiguousarray(order.rank, dtype=np.int32)
            N.check(N.lib().dg_segment_set_dim_order(self.handle, dim.encode(), slot, rank.ctypes.data, len(rank),
                                                     int(order.has_ties)))
            self._orders[key] = order
        return self._orders[key]

    def dim_value(self, dim: str, idx: int) -> Optional[str]:
        """DimensionSelector.lookupName for one id (no full dictionary export)."""
        d = self._dicts.get(dim)
        if d is not None:
            return d[idx]
        seen = self._values.get(dim)
        if seen is not None and idx in seen:
            return seen[idx]
        if self.column_type(dim) != N.COL_STRING:
            return None
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        N.check(N.lib().dg_segment_dim_value(self.handle, dim.encode(), int(idx), ctypes.byref(p), ctypes.byref(n)))
        v = ctypes.string_at(p.value, n.value).decode("utf-8") if n.value > 0 else None
        if seen is None:
            seen = self._values[dim] = {}
        if len(seen) < 65536:  # the ids a query's results name again (topN heads), bounded
            seen[int(idx)] = v
        return v

    # -- derived columns (dg_segment_derive_column) ------------------------------------------------
    MAX_DERIVED = 8  # derived columns kept per segment: each holds 8 B (FLOAT: 4 B) per row of HBM

    def derive(self, name: str, ops, inputs, out_type: int, in_use=(), cancel=None, timeout_ms: int = 0) -> Dict:
        """The derived column `name` = the expression program over this segment's rows, built on the device unless
        an identical one is there. At most MAX_DERIVED are kept: beyond that the least recently used one that is
        not among `in_use` (the running query's) is dropped first. Returns dg_derived_info as a dict
        (built = 0: reused). UnsupportedQuery: a string or missing input, a division by zero in some row.
        One querying thread at a time: `in_use` protects the running query's columns against this call's own
        evictions only. A second thread that derives on the same segment while the first one's engine call has
        not run yet may evict a column the first query names, which the engine would read as a missing column;
        the lock below keeps the bookkeeping whole, it does not pin columns across calls. Callers that share a
        segment between threads serialise their queries on it."""
        with self._derive_lock:
            return self._derive(name, ops, inputs, out_type, in_use, cancel, timeout_ms)

    def _derive(self, name, ops, inputs, out_type, in_use, cancel, timeout_ms) -> Dict:
        held = self._derived
        if name in held:
            held.move_to_end(name)
            return {"built": 0, "type": out_type, "rows": self.num_rows, "device_bytes": held[name],
                    "poisoned_rows": 0, "build_ms": 0.0}
        while len(held) >= self.MAX_DERIVED:
            victim = next((n for n in held if n not in in_use), None)
            if victim is None:
                raise N.UnsupportedQuery(2, f"a query needs more than {self.MAX_DERIVED} derived columns of a segment")
            self.drop_derived(victim)
        e, keep = N.make_expr(ops, inputs, out_type)
        info = N.dg_derived_info()
        N.check(N.lib().dg_segment_derive_column(self.handle, name.encode(), ctypes.byref(e),
                                                 ctypes.pointer(cancel) if cancel is not None else None,
                                                 int(timeout_ms), ctypes.byref(info)))
        held[name] = info.device_bytes
        self._types[name] = out_type
        return info.as_dict()

    def derived_columns(self) -> List[str]:
        """The derived columns held, least recently used first."""
        return list(self._derived)

    def drop_derived(self, name: Optional[str] = None) -> None:
        """Drop one derived column (dg_segment_drop_derived), or all of them: their HBM goes back."""
        with self._derive_lock:
            for n in ([name] if name is not None else list(self._derived)):
                N.check(N.lib().dg_segment_drop_derived(self.handle, n.encode()))
                del self._derived[n]
                self._types.pop(n, None)

    def filter_bitmap(self, flt, query_module) -> Tuple[np.ndarray, int]:
        """Filter.getBitmapResult as a dense row bitset (uint32 words) + cardinality."""
        fp = N.FilterProgram(flt, query_module, [self])
        words = np.zeros((self.num_rows + 31) // 32, dtype=np.uint32)
        cnt = ctypes.c_int64()
        arr = ctypes.cast(fp.array, ctypes.POINTER(N.dg_filter)) if fp.array is not None else None
        N.check(N.lib().dg_filter_bitmap(self.handle, arr, len(fp.nodes), words.ctypes.data, ctypes.byref(cnt)))
        return words, cnt.value

    def close(self):
        if self.handle:
            N.lib().dg_segment_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
