"""Native query model: the JSON query specs of Druid's timeseries / topN / groupBy (v2) path.

Mirrors the reference's query objects closely enough that a Druid native query JSON can be
fed in unchanged (``Query.from_json``):

* granularities: java-util/.../granularity/{Granularity,AllGranularity,PeriodGranularity}.java
  (bucketStart / increment / getIterable, PeriodGranularity.java:222-230,411-428)
* filters: query/filter/{SelectorDimFilter,InDimFilter,BoundDimFilter,AndDimFilter,OrDimFilter,
  NotDimFilter}.java (``toFilter`` / ``optimize``, e.g. InDimFilter.java:132-139)
* aggregators: query/aggregation/{Count,LongSum,DoubleSum,FloatSum,LongMin,LongMax,DoubleMin,
  DoubleMax,FloatMin,FloatMax}AggregatorFactory.java (combine / comparator / initial values)
* queries: query/timeseries/TimeseriesQuery.java, query/topn/TopNQuery.java,
  query/groupby/GroupByQuery.java, query/search/SearchQuery.java; topN metric specs
  NumericTopNMetricSpec / InvertedTopNMetricSpec / DimensionTopNMetricSpec.

* numeric expressions: common/.../math/expr (Expr.g4, Expr, Function, ExprEval, Evals) as a parser, a
  per-segment type checker and a compiler to the postfix programs of dg_segment_derive_column;
  ExpressionVirtualColumn, the aggregators' ``expression`` and ExpressionDimFilter (virtual.py lowers them
  to derived columns before a query runs)

Only the null-handling mode the reference defaults to is modelled
(``druid.generic.useDefaultValueForNull=true``, common/config/NullHandling.java:34,54):
null string == "" and numeric nulls read as 0.
"""
from __future__ import annotations

import datetime as _dt
import functools
import math
import re
import struct
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

# ----------------------------------------------------------------------------------------------
# time helpers
# ----------------------------------------------------------------------------------------------
MIN_INSTANT = -(2 ** 62)   # JodaUtils.MIN_INSTANT (Long.MIN_VALUE / 2)
MAX_INSTANT = 2 ** 62 - 1  # JodaUtils.MAX_INSTANT
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)


def parse_time(s) -> int:
    """ISO-8601 instant (or epoch millis) -> epoch millis (UTC)."""
    if isinstance(s, (int,)):
        return int(s)
    s = str(s).strip()
    if re.fullmatch(r"-?\d+", s) and len(s) > 8:
        return int(s)
    m = re.fullmatch(r"(\d{4})(?:-(\d{2})(?:-(\d{2}))?)?(?:T(\d{2})(?::(\d{2})(?::(\d{2})(?:\.(\d{1,3}))?)?)?)?(Z|[+-]\d{2}:?\d{2})?", s)
    if not m:
        raise ValueError(f"unparseable time {s!r}")
    y, mo, d, h, mi, se, ms, tz = m.groups()
    t = _dt.datetime(int(y), int(mo or 1), int(d or 1), int(h or 0), int(mi or 0), int(se or 0),
                     tzinfo=_dt.timezone.utc)
    millis = int((t - _EPOCH) // _dt.timedelta(milliseconds=1)) + int((ms or "0").ljust(3, "0"))
    if tz and tz != "Z":
        sign = 1 if tz[0] == "+" else -1
        hh, mm = int(tz[1:3]), int(tz[-2:])
        millis -= sign * (hh * 3600 + mm * 60) * 1000
    return millis


def format_time(ms: int) -> str:
    t = _EPOCH + _dt.timedelta(milliseconds=int(ms))
    return t.strftime("%Y-%m-%dT%H:%M:%S.") + f"{int(ms) % 1000:03d}Z"


def parse_interval(s) -> Tuple[int, int]:
    if isinstance(s, (tuple, list)):
        return int(s[0]), int(s[1])
    a, b = str(s).split("/")
    return parse_time(a), parse_time(b)


# ----------------------------------------------------------------------------------------------
# granularity
# ----------------------------------------------------------------------------------------------
_PERIOD_MS = {
    "none": 1, "second": 1000, "minute": 60_000, "five_minute": 300_000, "ten_minute": 600_000,
    "fifteen_minute": 900_000, "thirty_minute": 1_800_000, "hour": 3_600_000, "six_hour": 21_600_000,
    "day": 86_400_000, "week": 604_800_000,
}
_ISO_PERIOD = re.compile(r"P(?:(\d+)W)?(?:(\d+)D)?(?:T(?:(\d+)H)?(?:(\d+)M)?(?:(\d+)S)?)?")


@dataclass(frozen=True)
class Granularity:
    """ALL (period_ms == 0), a fixed-length UTC period with an origin, or a calendar granularity.

    Fixed: bucketStart(t) = t - floorMod(t - origin, period) (PeriodGranularity.truncateMillisPeriod,
    PeriodGranularity.java:411-428, UTC so fixed-length days/hours/weeks); Joda weeks start on
    Monday, so WEEK carries origin 1969-12-29 (Monday) = -3 days.
    Calendar (name "calendar"): any other PeriodGranularity — months / years, a time zone, compound
    periods with calendar fields — bucketed through the Joda restatement of granularity.py; the
    engine receives its bucket starts (dg_scan.bucket_starts).
    """
    period_ms: int = 0
    origin_ms: int = 0
    name: str = "all"
    iso: str = ""                   # calendar: ISO-8601 period
    tz: str = ""                    # calendar: time zone id ("" = UTC)
    origin: Optional[int] = None    # calendar: the spec's origin (None = the zone's local epoch)
    exact_from: Optional[int] = None  # fixed grid of a period spec: exact only for t >= this (None: always)

    @property
    def is_all(self) -> bool:
        return self.period_ms == 0 and self.name != "calendar"

    @property
    def is_calendar(self) -> bool:
        return self.name == "calendar"

    @property
    def calendar(self):
        return _calendar(self.iso, self.origin, self.tz or None)

    def bucket_start(self, t: int) -> int:
        if self.is_calendar:
            return self.calendar.truncate(t)
        if self.is_all:
            return MIN_INSTANT
        return t - ((t - self.origin_ms) % self.period_ms)

    def increment(self, t: int) -> int:
        if self.is_calendar:
            return self.calendar.increment(t)
        if self.is_all:
            return MAX_INSTANT
        return t + self.period_ms

    def bucket_end(self, t: int) -> int:
        return self.increment(self.bucket_start(t))

    def iterable(self, interval: Tuple[int, int]) -> List[Tuple[int, int]]:
        """Granularity.getIterable (Granularity.java:176-240); AllGranularity yields the input."""
        s, e = interval
        if self.is_all:
            return [(s, e)]
        if self.is_calendar:
            b = self.calendar.iterable_starts(s, e)
            return list(zip(b[:-1], b[1:]))
        out = []
        cur = self.bucket_start(s)
        while cur < e:
            out.append((cur, cur + self.period_ms))
            cur += self.period_ms
        return out

    def bucket_starts(self, interval: Tuple[int, int]) -> List[int]:
        """Calendar: starts of the buckets getIterable(interval) yields, then the end of the last."""
        return self.calendar.iterable_starts(*interval)

    def to_json(self):
        if self.is_all:
            return "all"
        if self.is_calendar:
            js = {"type": "period", "period": self.iso}
            if self.tz:
                js["timeZone"] = self.tz
            if self.origin is not None:
                js["origin"] = format_time(self.origin)
            return js
        if self.name in _PERIOD_MS:
            return self.name
        if self.iso:  # a period spec bucketed on its fixed grid
            js = {"type": "period", "period": self.iso}
            if self.tz:
                js["timeZone"] = self.tz
            if self.origin is not None:
                js["origin"] = format_time(self.origin)
            return js
        return {"type": "duration", "duration": self.period_ms, "origin": self.origin_ms}

    @staticmethod
    def period(iso: str, tz: Optional[str] = None, origin=None) -> "Granularity":
        """PeriodGranularity(period, origin, timeZone): the fixed grid when it is exact, else calendar.
        Exact: a period without months / years in UTC or a fixed-offset zone ("+05:30"), where every
        truncate branch (PeriodGranularity.java:222-330) is a floor on the grid of the period from the
        origin (default: the zone's local epoch, 0 - offset; P1W: its Monday). Two quirks of the hours
        branch (:313-326) are not: an origin < 0 off the local hour rounds to the hour (calendar), and
        with an origin <= 0 a timestamp before the origin gets the aligned point AFTER it — exact on the
        grid only at or after the origin, so the grid records `exact_from` and the runners switch to
        the calendar restatement when the data reaches before it (compound periods likewise before 0)."""
        from .granularity import Zone, parse_period
        y, mo, w, d, h, mi, s, ms = parse_period(iso)
        utc = tz in (None, "", "UTC", "Etc/UTC")
        off = 0 if utc else Zone(tz).fixed  # fixed offset in ms, None for a zone with rules
        o = parse_time(origin) if origin is not None else None
        single = sum(1 for v in (y, mo, w, d, h, mi, s, ms) if v) == 1
        hours_branch = bool(h) and single and (h > 1 or o is not None)
        # hours with an origin before 1970 not on the (local) hour: PeriodGranularity.java:313-315 floors to the hour
        quirk = bool(h) and single and o is not None and o < 0 and (o + (off or 0)) % 3_600_000 != 0
        if off is not None and not (y or mo) and not quirk:
            P = ((((w * 7 + d) * 24 + h) * 60 + mi) * 60 + s) * 1000 + ms
            default_origin = (-3 * 86_400_000 if (w == 1 and single) else 0) - off  # P1W: Mondays
            org = o if o is not None else default_origin
            exact_from = None
            if not single:
                # compound: truncateMillisPeriod (PeriodGranularity.java:411-428) = t - (t % P - origin % P,
                # + P once if negative) with Java remainders: the grid's floor only for t >= 0 and a
                # non-negative origin remainder
                if math.fmod(org, P) < 0:
                    return Granularity(0, 0, "calendar", iso.upper(), "" if utc else tz, o)
                exact_from = 0
            elif hours_branch and org <= 0:
                exact_from = org
            return Granularity(P, org, "period", iso.upper(), "" if utc else tz, o, exact_from)
        return Granularity(0, 0, "calendar", iso.upper(), "" if utc else tz, o)

    def calendar_form(self) -> "Granularity":
        """The same PeriodGranularity bucketed through the calendar restatement."""
        return Granularity(0, 0, "calendar", self.iso, self.tz, self.origin)

    @staticmethod
    def of(spec) -> "Granularity":
        if isinstance(spec, Granularity):
            return spec
        if spec is None:
            return ALL
        if isinstance(spec, str):
            k = spec.lower()
            if k == "all":
                return ALL
            if k in _PERIOD_MS:
                return Granularity(_PERIOD_MS[k], -3 * 86_400_000 if k == "week" else 0, k)
            if k in _CALENDAR:  # Granularities.MONTH / QUARTER / YEAR (GranularityType.java)
                return Granularity.period(_CALENDAR[k])
            raise ValueError(f"unsupported granularity {spec!r}")
        t = spec.get("type")
        if t == "all":
            return ALL
        if t == "duration":
            origin = parse_time(spec["origin"]) if spec.get("origin") is not None else 0
            return Granularity(int(spec["duration"]), origin, "duration")
        if t == "period":
            return Granularity.period(spec["period"], spec.get("timeZone"), spec.get("origin"))
        raise ValueError(f"unsupported granularity {spec!r}")


_CALENDAR = {"month": "P1M", "quarter": "P3M", "year": "P1Y"}


@functools.lru_cache(maxsize=64)
def _calendar(iso: str, origin: Optional[int], tz: Optional[str]):
    from .granularity import PeriodGranularity
    return PeriodGranularity(iso, origin, tz)


ALL = Granularity(0, 0, "all")
HOUR = Granularity.of("hour")
DAY = Granularity.of("day")


# ----------------------------------------------------------------------------------------------
# filters
# ----------------------------------------------------------------------------------------------
class DimFilter:
    def to_json(self) -> Dict[str, Any]:
        raise NotImplementedError

    def optimize(self) -> "DimFilter":
        return self

    @staticmethod
    def from_json(js) -> Optional["DimFilter"]:
        if js is None:
            return None
        if isinstance(js, DimFilter):
            return js
        t = js["type"]
        if t == "selector":
            return SelectorDimFilter(js["dimension"], js.get("value"))
        if t == "in":
            return InDimFilter(js["dimension"], list(js["values"]))
        if t == "bound":
            return BoundDimFilter(js["dimension"], js.get("lower"), js.get("upper"),
                                  bool(js.get("lowerStrict", False)), bool(js.get("upperStrict", False)),
                                  _ordering_name(js.get("ordering"), js.get("alphaNumeric", False)))
        if t == "and":
            return AndDimFilter([DimFilter.from_json(f) for f in js["fields"]])
        if t == "or":
            return OrDimFilter([DimFilter.from_json(f) for f in js["fields"]])
        if t == "not":
            return NotDimFilter(DimFilter.from_json(js["field"]))
        if t == "regex":
            return RegexDimFilter(js["dimension"], js["pattern"])
        if t == "search":
            return SearchQueryDimFilter(js["dimension"], dict(js["query"]))
        if t == "like":
            return LikeDimFilter(js["dimension"], js["pattern"], js.get("escape"))
        if t == "expression":
            return ExpressionDimFilter(js["expression"])
        raise ValueError(f"unsupported filter type {t!r}")


def _ordering_name(o, alpha_numeric=False) -> str:
    if o is None:
        return "alphanumeric" if alpha_numeric else "lexicographic"
    if isinstance(o, dict):
        o = o.get("type")
    return str(o).lower()


def _empty_to_null(v):
    return None if v is None or v == "" else str(v)


@dataclass
class SelectorDimFilter(DimFilter):
    dimension: str
    value: Optional[str]

    def to_json(self):
        return {"type": "selector", "dimension": self.dimension, "value": self.value}


@dataclass
class InDimFilter(DimFilter):
    dimension: str
    values: List[Optional[str]]

    def optimize(self):
        # InDimFilter.optimize (InDimFilter.java:132-139): single value -> selector
        vals = sorted({_empty_to_null(v) or "" for v in self.values})
        if len(vals) == 1:
            return SelectorDimFilter(self.dimension, _empty_to_null(vals[0]))
        return InDimFilter(self.dimension, [_empty_to_null(v) for v in vals])

    def to_json(self):
        return {"type": "in", "dimension": self.dimension, "values": list(self.values)}


@dataclass
class BoundDimFilter(DimFilter):
    dimension: str
    lower: Optional[str] = None
    upper: Optional[str] = None
    lowerStrict: bool = False
    upperStrict: bool = False
    ordering: str = "lexicographic"

    def to_json(self):
        return {"type": "bound", "dimension": self.dimension, "lower": self.lower, "upper": self.upper,
                "lowerStrict": self.lowerStrict, "upperStrict": self.upperStrict, "ordering": self.ordering}


@dataclass
class AndDimFilter(DimFilter):
    fields: List[DimFilter]

    def optimize(self):
        fs = [f.optimize() for f in self.fields]
        return fs[0] if len(fs) == 1 else AndDimFilter(fs)

    def to_json(self):
        return {"type": "and", "fields": [f.to_json() for f in self.fields]}


@dataclass
class OrDimFilter(DimFilter):
    fields: List[DimFilter]

    def optimize(self):
        fs = [f.optimize() for f in self.fields]
        return fs[0] if len(fs) == 1 else OrDimFilter(fs)

    def to_json(self):
        return {"type": "or", "fields": [f.to_json() for f in self.fields]}


@dataclass
class NotDimFilter(DimFilter):
    field: DimFilter

    def optimize(self):
        return NotDimFilter(self.field.optimize())

    def to_json(self):
        return {"type": "not", "field": self.field.to_json()}


# ---- predicate filters: evaluated over dictionary values (DimensionPredicateFilter ->
# Filters.matchPredicate, segment/filter/Filters.java:239-290), i.e. the union of the bitmaps of every
# value the predicate accepts; a missing column is all-true iff the predicate accepts null ----
def _java_regex(pattern: str) -> "re.Pattern":
    """java.util.regex.Pattern.compile for the common syntax (Python re; \\p{..} classes and
    possessive quantifiers are not translated)."""
    return re.compile(pattern)


def _region_matches_ignore_case(s: str, i: int, sub: str) -> bool:
    """String.regionMatches(true, i, sub, 0, len): per UTF-16 char, equal after toUpperCase or
    toLowerCase (BMP characters; Python's case tables)."""
    def up(c):
        u = c.upper()
        return u if len(u) == 1 else c

    def low(c):
        u = c.lower()
        return u if len(u) == 1 else c

    for a, b in zip(s[i:i + len(sub)], sub):
        if a == b:
            continue
        ua, ub = up(a), up(b)
        if ua == ub or low(ua) == low(ub):
            continue
        return False
    return True


def contains_ignore_case(s: Optional[str], sub: Optional[str]) -> bool:
    """commons-lang StringUtils.containsIgnoreCase."""
    if s is None or sub is None:
        return False
    return any(_region_matches_ignore_case(s, i, sub) for i in range(len(s) - len(sub) + 1))


@dataclass
class RegexDimFilter(DimFilter):
    """RegexDimFilter -> RegexFilter (segment/filter/RegexFilter.java:44-48): non-null and find()."""
    dimension: str
    pattern: str

    def predicate(self, v: Optional[str]) -> bool:
        return v is not None and _java_regex(self.pattern).search(v) is not None

    def to_json(self):
        return {"type": "regex", "dimension": self.dimension, "pattern": self.pattern}


@dataclass
class SearchQueryDimFilter(DimFilter):
    """SearchQueryDimFilter with a SearchQuerySpec (query/search/*SearchQuerySpec.java accept()):
    contains / insensitive_contains (StringUtils.containsIgnoreCase), fragment (every value
    contained), regex (find), all."""
    dimension: str
    query: Dict[str, Any]

    def predicate(self, v: Optional[str]) -> bool:
        q, t = self.query, self.query.get("type")
        if t == "all":
            return True
        if v is None:
            return False
        if t in ("contains", "insensitive_contains"):
            val = q.get("value")
            if val is None:
                return False
            if t == "contains" and q.get("caseSensitive", False):
                return val in v
            return contains_ignore_case(v, val)
        if t == "fragment":
            vals = q.get("values")
            if vals is None:
                return False
            if q.get("caseSensitive", False):
                return all(x in v for x in set(vals))
            return all(contains_ignore_case(v, x) for x in set(vals))
        if t == "regex":
            return _java_regex(q["pattern"]).search(v) is not None
        raise ValueError(f"unsupported search query spec {t!r}")

    def to_json(self):
        return {"type": "search", "dimension": self.dimension, "query": dict(self.query)}


@dataclass
class LikeDimFilter(DimFilter):
    """LikeDimFilter.LikeMatcher (query/filter/LikeDimFilter.java:75-158): % -> .*, _ -> ., the escape
    character quotes the next one, other characters outside [\\w\\d\\s-] as \\uXXXX; matches()
    over nullToEmpty(value) in default null mode."""
    dimension: str
    pattern: str
    escape: Optional[str] = None

    def _regex(self) -> "re.Pattern":
        esc = self.escape[0] if self.escape else None
        out, escaping = [], False
        for c in self.pattern:
            if esc is not None and c == esc and not escaping:
                escaping = True
            elif c == "%" and not escaping:
                out.append(".*")
            elif c == "_" and not escaping:
                out.append(".")
            else:
                out.append(c if re.fullmatch(r"[A-Za-z0-9_\s-]", c) else "\\u%04x" % ord(c) if ord(c) < 0x10000
                           else re.escape(c))
                escaping = False
        return re.compile("".join(out))

    def predicate(self, v: Optional[str]) -> bool:
        return self._regex().fullmatch("" if v is None else v) is not None

    def to_json(self):
        js = {"type": "like", "dimension": self.dimension, "pattern": self.pattern}
        if self.escape is not None:
            js["escape"] = self.escape
        return js


PREDICATE_FILTERS = (RegexDimFilter, SearchQueryDimFilter, LikeDimFilter)


@dataclass
class ExpressionDimFilter(DimFilter):
    """query/filter/ExpressionDimFilter.java -> segment/filter/ExpressionFilter.java:54-66: a row matches when
    Evals.asBoolean(selector.getLong()) holds, i.e. the expression's value cast to a long is above 0 (0.5 does
    not match). The runners evaluate it into a derived LONG column and filter that with a numeric bound."""
    expression: str

    def __post_init__(self):
        self.ast = parse_expression(self.expression)

    def to_json(self):
        return {"type": "expression", "expression": self.expression}


# ----------------------------------------------------------------------------------------------
# aggregators
# ----------------------------------------------------------------------------------------------
AGG_KINDS = {
    "count": 0, "longSum": 1, "doubleSum": 2, "floatSum": 3, "longMin": 4, "longMax": 5,
    "doubleMin": 6, "doubleMax": 7, "floatMin": 8, "floatMax": 9,
    # query/aggregation/first/*, query/aggregation/last/*: the value at the earliest / latest __time
    "longFirst": 10, "longLast": 11, "doubleFirst": 12, "doubleLast": 13, "floatFirst": 14, "floatLast": 15,
}
AGG_OUTPUT = {0: "long", 1: "long", 4: "long", 5: "long", 2: "double", 6: "double", 7: "double",
              3: "float", 8: "float", 9: "float",
              10: "long", 11: "long", 12: "double", 13: "double", 14: "float", 15: "float", 16: "long"}
FIRST_KINDS = (10, 12, 14)
LAST_KINDS = (11, 13, 15)
PAIR_TIME_KIND = 16  # DG_AGG_PAIR_TIME: the native entry that follows a first/last aggregator (its pair's time)
LONG_MAX = (1 << 63) - 1
LONG_MIN = -(1 << 63)


@dataclass(frozen=True)
class SerializablePair:
    """collections/SerializablePair<Long, Number>: what a first/last BufferAggregator.get returns,
    lhs = the time, rhs = the value at that time. Un-finalized values of the first/last aggregators are
    pairs; AggregatorFactory.finalize_computation returns rhs."""
    lhs: int
    rhs: object

    def __eq__(self, o):
        if not isinstance(o, SerializablePair) or self.lhs != o.lhs or type(self.rhs) is not type(o.rhs):
            return False
        if isinstance(self.rhs, float):  # bit for bit (-0.0 is not 0.0), every NaN equal to every NaN
            if self.rhs != self.rhs or o.rhs != o.rhs:
                return self.rhs != self.rhs and o.rhs != o.rhs
            return struct.pack("<d", self.rhs) == struct.pack("<d", o.rhs)
        return self.rhs == o.rhs

    def __hash__(self):
        return hash((self.lhs, repr(self.rhs)))


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def java_min(a, b):
    """java.lang.Math.min for doubles/floats (NaN-propagating, -0.0 < +0.0)."""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0:
        return b
    return a if a <= b else b


def java_max(a, b):
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0:
        return b
    return a if a >= b else b


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


@dataclass
class AggregatorFactory:
    """An aggregator factory; `filter` set = FilteredAggregatorFactory around it
    (query/aggregation/FilteredAggregatorFactory.java:40-73: the delegate aggregates a row only when
    the filter's ValueMatcher matches it; name, combine and comparator are the delegate's)."""
    type: str
    name: str
    fieldName: Optional[str] = None
    filter: Optional["DimFilter"] = None
    # SimpleLong / SimpleDouble / SimpleFloatAggregatorFactory: the input is an expression instead of a column
    # (sum, min and max factories; the first/last factories have no such field in the reference)
    expression: Optional[str] = None

    def __post_init__(self):
        if self.type not in AGG_KINDS:
            raise ValueError(f"unsupported aggregator type {self.type!r}")
        if self.expression is not None:
            if self.kind == 0 or self.is_pair:
                raise ValueError(f"aggregator type {self.type!r} has no expression field")
            if self.fieldName is not None:
                # SimpleDoubleAggregatorFactory.java:59
                raise ValueError("Must have a valid, non-null fieldName or expression: exactly one of them")
            self.ast = parse_expression(self.expression)
        elif self.kind != 0 and self.fieldName is None:
            raise ValueError("Must have a valid, non-null fieldName or expression")

    @property
    def kind(self) -> int:
        return AGG_KINDS[self.type]

    @property
    def is_pair(self) -> bool:
        """A first/last aggregator: its un-finalized values are SerializablePair(time, value)."""
        return self.kind in FIRST_KINDS or self.kind in LAST_KINDS

    @property
    def output_type(self) -> str:
        return AGG_OUTPUT[self.kind]

    def initial(self):
        """Aggregator reset / BufferAggregator.init values."""
        k = self.kind
        if k in FIRST_KINDS or k in LAST_KINDS:
            # LongFirstBufferAggregator.init: (Long.MAX_VALUE, 0); LongLastBufferAggregator.init: (Long.MIN_VALUE, 0)
            zero = 0 if self.output_type == "long" else 0.0
            return SerializablePair(LONG_MAX if k in FIRST_KINDS else LONG_MIN, zero)
        if k in (0, 1):
            return 0
        if k == 4:
            return (1 << 63) - 1
        if k == 5:
            return -(1 << 63)
        if k in (2, 3):
            return 0.0
        if k in (6, 8):
            return math.inf
        return -math.inf

    def combine(self, a, b):
        """AggregatorFactory.combine (e.g. LongSumAggregator.combineValues, FloatSumAggregator.java:40-43)."""
        k = self.kind
        if k in FIRST_KINDS:  # LongFirstAggregatorFactory.combine (:103-112): the left side wins ties
            return a if a.lhs <= b.lhs else b
        if k in LAST_KINDS:  # LongLastAggregatorFactory.combine (:107): the right side wins ties
            return a if a.lhs > b.lhs else b
        if k in (0, 1):
            return _wrap64(int(a) + int(b))
        if k == 4:
            return min(int(a), int(b))
        if k == 5:
            return max(int(a), int(b))
        if k == 2:
            return float(a) + float(b)
        if k == 3:
            return _f32(_f32(a) + _f32(b))
        if k in (6, 8):
            r = java_min(float(a), float(b))
            return _f32(r) if k == 8 else r
        r = java_max(float(a), float(b))
        return _f32(r) if k == 9 else r

    def finalize_computation(self, v):
        """AggregatorFactory.finalizeComputation: a first/last pair's rhs (LongFirstAggregatorFactory.java:
        finalizeComputation returns ((SerializablePair) object).rhs); every other aggregator's value as is."""
        return v.rhs if isinstance(v, SerializablePair) else v

    def compare_key(self, v):
        """Sort key realising the factory comparator (Long.compare / Doubles.compare; a first/last
        aggregator's VALUE_COMPARATOR compares the pairs' rhs with Longs / Doubles / Floats.compare)."""
        if isinstance(v, SerializablePair):
            v = v.rhs
        if self.output_type == "long":
            return (0, int(v))
        v = float(v)
        if v != v:
            return (1, 0.0)  # Double.compare: NaN is greatest
        if v == 0.0:
            return (0, -0.0 if math.copysign(1.0, v) < 0 else 0.0, 1 if math.copysign(1.0, v) > 0 else 0)
        return (0, v, 0)

    def to_json(self):
        js = {"type": self.type, "name": self.name}
        if self.fieldName is not None:
            js["fieldName"] = self.fieldName
        if self.expression is not None:
            js["expression"] = self.expression
        if self.filter is not None:
            return {"type": "filtered", "filter": self.filter.to_json(), "aggregator": js}
        return js

    @staticmethod
    def from_json(js) -> "AggregatorFactory":
        if isinstance(js, AggregatorFactory):
            return js
        if js["type"] == "filtered":
            inner = AggregatorFactory.from_json(js["aggregator"])
            f = DimFilter.from_json(js["filter"])
            if f is None:
                raise ValueError("filtered aggregator without a filter")
            # FilteredAggregatorFactory(FilteredAggregatorFactory(x, f1), f2) matches f2 and then f1
            both = f if inner.filter is None else AndDimFilter([f, inner.filter])
            return AggregatorFactory(inner.type, inner.name, inner.fieldName, both, inner.expression)
        return AggregatorFactory(js["type"], js["name"], js.get("fieldName"), None, js.get("expression"))


def filtered(agg: AggregatorFactory, flt) -> AggregatorFactory:
    """FilteredAggregatorFactory(agg, filter)."""
    return AggregatorFactory.from_json({"type": "filtered", "filter": flt, "aggregator": agg})


def native_aggregations(aggs: Sequence["AggregatorFactory"]) -> List["AggregatorFactory"]:
    """The aggregator entries of a native call (dg_scan.aggs): every first/last aggregator is followed by
    its DG_AGG_PAIR_TIME entry, whose slot carries the pair's time."""
    out: List[AggregatorFactory] = []
    for a in aggs:
        out.append(a)
        if a.is_pair:
            out.append(_PairTime(a))
    return out


def native_index(aggs: Sequence["AggregatorFactory"]) -> List[int]:
    """Native slot index of every aggregator's value (a pair's time is the slot after it)."""
    out, at = [], 0
    for a in aggs:
        out.append(at)
        at += 2 if a.is_pair else 1
    return out


class _PairTime(AggregatorFactory):
    """The DG_AGG_PAIR_TIME entry of a first/last aggregator: internal to the native calls (no JSON form)."""

    def __init__(self, pair: AggregatorFactory):
        self.type, self.name, self.fieldName, self.filter = "pairTime", pair.name + "\x00time", None, None
        self.expression = None

    @property
    def kind(self) -> int:
        return PAIR_TIME_KIND


def count(name="count"):
    return AggregatorFactory("count", name)


def long_sum(name, field_name=None):
    return AggregatorFactory("longSum", name, field_name or name)


def double_sum(name, field_name=None):
    return AggregatorFactory("doubleSum", name, field_name or name)


def float_sum(name, field_name=None):
    return AggregatorFactory("floatSum", name, field_name or name)


def long_min(name, field_name=None):
    return AggregatorFactory("longMin", name, field_name or name)


def long_max(name, field_name=None):
    return AggregatorFactory("longMax", name, field_name or name)


def double_min(name, field_name=None):
    return AggregatorFactory("doubleMin", name, field_name or name)


def double_max(name, field_name=None):
    return AggregatorFactory("doubleMax", name, field_name or name)


def float_min(name, field_name=None):
    return AggregatorFactory("floatMin", name, field_name or name)


def float_max(name, field_name=None):
    return AggregatorFactory("floatMax", name, field_name or name)


def long_first(name, field_name=None):
    return AggregatorFactory("longFirst", name, field_name or name)


def long_last(name, field_name=None):
    return AggregatorFactory("longLast", name, field_name or name)


def double_first(name, field_name=None):
    return AggregatorFactory("doubleFirst", name, field_name or name)


def double_last(name, field_name=None):
    return AggregatorFactory("doubleLast", name, field_name or name)


def float_first(name, field_name=None):
    return AggregatorFactory("floatFirst", name, field_name or name)


def float_last(name, field_name=None):
    return AggregatorFactory("floatLast", name, field_name or name)


# ----------------------------------------------------------------------------------------------
# post-aggregators (query/aggregation/post/*.java)
# ----------------------------------------------------------------------------------------------
def UnsupportedPostAggregator(msg: str):
    """UnsupportedQuery for a post-aggregator the engine has no program for (javascript, expression,
    hyperUniqueCardinality, a finalizingFieldAccess of anything but an aggregator): the caller keeps its CPU
    engine."""
    from ._native import UnsupportedQuery
    return UnsupportedQuery(2, msg)


# ops of a compiled post-aggregator program (DG_POST_* of include/druidgpu.h)
POST_AGG, POST_CONST_D, POST_CONST_L, POST_L2D, POST_D2L = 0, 1, 2, 3, 4
POST_ADD, POST_SUB, POST_MUL, POST_DIV, POST_QUOT = 5, 6, 7, 8, 9
POST_DMAX, POST_DMIN, POST_LMAX, POST_LMIN = 10, 11, 12, 13
POST_ORDER_NONE, POST_ORDER_DOUBLE, POST_ORDER_LONG, POST_ORDER_NUMERIC_FIRST = 0, 1, 2, 3
POST_MAX_OPS, POST_MAX_STACK = 64, 16
_ARITH_OPS = {"+": POST_ADD, "-": POST_SUB, "*": POST_MUL, "/": POST_DIV, "quotient": POST_QUOT}


def double_bits(d: float) -> int:
    """Double.doubleToLongBits as an unsigned number (every NaN is the canonical one)."""
    if d != d:
        return 0x7FF8000000000000
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def java_d2l(d: float) -> int:
    """Java's (long) double (JLS 5.1.3): NaN -> 0, saturating at Long.MIN_VALUE / MAX_VALUE, else truncation."""
    if d != d:
        return 0
    if d >= 9223372036854775808.0:
        return LONG_MAX
    if d <= -9223372036854775808.0:
        return LONG_MIN
    return int(d)


def java_double_compare(a: float, b: float) -> int:
    """Double.compare: numeric order, -0.0 < 0.0, NaN equal to NaN and greater than everything else."""
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = double_bits(a), double_bits(b)
    x = x - (1 << 64) if x >> 63 else x
    y = y - (1 << 64) if y >> 63 else y
    return (x > y) - (x < y)


def java_double_div(lhs: float, rhs: float) -> float:
    """IEEE lhs / rhs (Python raises on a zero divisor)."""
    if rhs != 0.0 or rhs != rhs:
        return lhs / rhs
    if lhs != lhs or lhs == 0.0:
        return math.nan
    return math.copysign(math.inf, lhs) * math.copysign(1.0, rhs)


def _number_to_double(v) -> float:
    return float(v)  # Number.doubleValue: a long rounds to nearest even, a float widens exactly


def _number_to_long(v) -> int:
    return int(v) if isinstance(v, int) else java_d2l(float(v))  # Number.longValue


class PostAggregator:
    """One post-aggregator: `name`, to_json, compute(event) — the host restatement over a row's values, Python
    floats being IEEE doubles — and emit(ctx), which appends the postfix program of include/druidgpu.h to ctx.ops
    and returns the value's type ("long" / "double")."""
    order = POST_ORDER_DOUBLE

    def compute(self, event: Dict[str, Any]):
        raise NotImplementedError

    def emit(self, ctx: "_PostCompile") -> str:
        raise NotImplementedError

    def dependent_fields(self) -> List[str]:
        return []

    def order_kind(self, ctx: "_PostCompile") -> int:
        """The comparator (getComparator) as a POST_ORDER_* kind."""
        return self.order

    @staticmethod
    def from_json(js) -> "PostAggregator":
        if isinstance(js, PostAggregator):
            return js
        t = js.get("type")
        if t == "arithmetic":
            return ArithmeticPostAggregator(js.get("name"), js["fn"], [PostAggregator.from_json(f) for f in js["fields"]],
                                            js.get("ordering"))
        if t == "fieldAccess":
            return FieldAccessPostAggregator(js.get("name"), js["fieldName"])
        if t == "finalizingFieldAccess":
            return FinalizingFieldAccessPostAggregator(js.get("name"), js["fieldName"])
        if t == "constant":
            return ConstantPostAggregator(js.get("name"), js["value"])
        if t in _GREATEST_LEAST:
            return _GREATEST_LEAST[t](js.get("name"), [PostAggregator.from_json(f) for f in js["fields"]])
        if t in ("javascript", "expression", "hyperUniqueCardinality"):
            raise UnsupportedPostAggregator(f"post-aggregator type {t!r} stays on the CPU engine")
        raise ValueError(f"unknown post-aggregator type {t!r}")


class _PostCompile:
    """State of one compilation: the aggregators' native slots and the earlier post-aggregators a field may
    name (Queries.prepareAggregations: an earlier one is inlined)."""

    def __init__(self, aggregations: Sequence[AggregatorFactory], earlier: Dict[str, PostAggregator]):
        self.aggs = {a.name: (i, a) for a, i in zip(aggregations, native_index(aggregations))}
        self.earlier = earlier
        self.ops: List[Tuple[int, int, int]] = []  # (op, arg, imm)

    def push(self, op: int, arg: int = 0, imm: int = 0):
        self.ops.append((op, arg, imm & ((1 << 64) - 1)))

    def to_double(self, t: str):
        if t == "long":
            self.push(POST_L2D)

    def to_long(self, t: str):
        if t == "double":
            self.push(POST_D2L)


@dataclass
class FieldAccessPostAggregator(PostAggregator):
    """FieldAccessPostAggregator.java: the row's value of `fieldName` as it is."""
    name: Optional[str]
    fieldName: str

    def dependent_fields(self):
        return [self.fieldName]

    def compute(self, event):
        return event[self.fieldName]

    def emit(self, ctx):
        if self.fieldName in ctx.aggs:
            i, a = ctx.aggs[self.fieldName]
            if a.is_pair:  # a SerializablePair is not a Number: the reference's cast fails
                raise ValueError(f"fieldAccess of the first/last aggregator {self.fieldName!r} is a pair, not a number "
                                 "(use finalizingFieldAccess)")
            ctx.push(POST_AGG, i)
            return "long" if a.output_type == "long" else "double"
        if self.fieldName in ctx.earlier:
            return ctx.earlier[self.fieldName].emit(ctx)
        raise ValueError(f"post-aggregator field {self.fieldName!r} names no aggregator and no earlier post-aggregator")

    def order_kind(self, ctx):
        raise ValueError("a fieldAccess post-aggregator has no comparator (FieldAccessPostAggregator.getComparator)")

    def to_json(self):
        return {"type": "fieldAccess", "name": self.name, "fieldName": self.fieldName}


@dataclass
class FinalizingFieldAccessPostAggregator(PostAggregator):
    """FinalizingFieldAccessPostAggregator.java: AggregatorFactory.finalizeComputation of the row's value; its
    comparator is the aggregator's."""
    name: Optional[str]
    fieldName: str

    def dependent_fields(self):
        return [self.fieldName]

    def compute(self, event):
        v = event[self.fieldName]
        return v.rhs if isinstance(v, SerializablePair) else v

    def emit(self, ctx):
        if self.fieldName not in ctx.aggs:
            raise UnsupportedPostAggregator(f"finalizingFieldAccess of {self.fieldName!r}, which is no aggregator")
        i, a = ctx.aggs[self.fieldName]
        ctx.push(POST_AGG, i)  # (a first/last pair's value slot; its time is the slot after it)
        return "long" if a.output_type == "long" else "double"

    def order_kind(self, ctx):
        if self.fieldName not in ctx.aggs:
            raise UnsupportedPostAggregator(f"finalizingFieldAccess of {self.fieldName!r}, which is no aggregator")
        return POST_ORDER_LONG if ctx.aggs[self.fieldName][1].output_type == "long" else POST_ORDER_DOUBLE

    def to_json(self):
        return {"type": "finalizingFieldAccess", "name": self.name, "fieldName": self.fieldName}


@dataclass
class ConstantPostAggregator(PostAggregator):
    """ConstantPostAggregator.java: a number; its comparator calls every two values equal."""
    name: Optional[str]
    value: Any
    order = POST_ORDER_NONE

    def __post_init__(self):
        if isinstance(self.value, bool) or not isinstance(self.value, (int, float)):
            raise ValueError("Constant value must be a number")
        if isinstance(self.value, int) and not LONG_MIN <= self.value <= LONG_MAX:
            raise ValueError("Constant value out of the long range")

    def compute(self, event):
        return self.value

    def emit(self, ctx):
        if isinstance(self.value, int):
            ctx.push(POST_CONST_L, 0, self.value)
            return "long"
        ctx.push(POST_CONST_D, 0, double_bits(self.value))
        return "double"

    def to_json(self):
        return {"type": "constant", "name": self.name, "value": self.value}


@dataclass
class ArithmeticPostAggregator(PostAggregator):
    """ArithmeticPostAggregator.java: a left fold of `fn` over the fields' doubleValue() (:107-124); "/" gives 0
    for a zero divisor (:229-235), "quotient" is IEEE division; ordering None = Double.compare, "numericFirst" =
    Ordering.numericFirst (:277-299)."""
    name: Optional[str]
    fn: str
    fields: List[PostAggregator]
    ordering: Optional[str] = None

    def __post_init__(self):
        self.fields = [PostAggregator.from_json(f) for f in self.fields]
        if self.fn not in _ARITH_OPS:
            raise ValueError(f"Unknown operation[{self.fn}], known operations[{sorted(_ARITH_OPS)}]")
        if len(self.fields) < 2:
            raise ValueError(f"Illegal number of fields[{len(self.fields)}], must be > 1")
        if self.ordering not in (None, "numericFirst"):
            raise ValueError(f"unknown ordering {self.ordering!r}")

    @property
    def order(self):
        return POST_ORDER_NUMERIC_FIRST if self.ordering == "numericFirst" else POST_ORDER_DOUBLE

    def dependent_fields(self):
        return [d for f in self.fields for d in f.dependent_fields()]

    def _apply(self, lhs: float, rhs: float) -> float:
        if self.fn == "+":
            return lhs + rhs
        if self.fn == "-":
            return lhs - rhs
        if self.fn == "*":
            return lhs * rhs
        if self.fn == "/":
            return 0.0 if rhs == 0.0 else lhs / rhs  # (-0.0 == 0.0; a NaN divisor is not zero)
        return java_double_div(lhs, rhs)

    def compute(self, event):
        vals = []
        for f in self.fields:
            v = f.compute(event)
            if isinstance(v, SerializablePair):
                raise ValueError("a first/last pair is not a number (use finalizingFieldAccess)")
            vals.append(_number_to_double(v))
        acc = vals[0]
        for v in vals[1:]:
            acc = self._apply(acc, v)
        return acc

    def emit(self, ctx):
        ctx.to_double(self.fields[0].emit(ctx))
        for f in self.fields[1:]:
            ctx.to_double(f.emit(ctx))
            ctx.push(_ARITH_OPS[self.fn])
        return "double"

    def to_json(self):
        js = {"type": "arithmetic", "name": self.name, "fn": self.fn, "fields": [f.to_json() for f in self.fields]}
        if self.ordering is not None:
            js["ordering"] = self.ordering
        return js


@dataclass
class _GreatestLeast(PostAggregator):
    name: Optional[str]
    fields: List[PostAggregator]
    type_name = ""
    is_long = False
    greatest = True

    def __post_init__(self):
        self.fields = [PostAggregator.from_json(f) for f in self.fields]
        if not self.fields:
            raise ValueError("Illegal number of fields[0], must be > 0")

    @property
    def order(self):
        return POST_ORDER_LONG if self.is_long else POST_ORDER_DOUBLE

    def dependent_fields(self):
        return [d for f in self.fields for d in f.dependent_fields()]

    def compute(self, event):
        # DoubleGreatestPostAggregator.java:77-92 (and its three siblings): folded from the type's least /
        # greatest value, a field replaces the running value when the comparator says strictly greater / less
        if self.is_long:
            acc = LONG_MIN if self.greatest else LONG_MAX
        else:
            acc = -math.inf if self.greatest else math.inf
        for f in self.fields:
            v = f.compute(event)
            if isinstance(v, SerializablePair):
                raise ValueError("a first/last pair is not a number (use finalizingFieldAccess)")
            if self.is_long:
                v = _number_to_long(v)
                c = (v > acc) - (v < acc)
            else:
                v = _number_to_double(v)
                c = java_double_compare(v, acc)
            if (c > 0) if self.greatest else (c < 0):
                acc = v
        return acc

    def emit(self, ctx):
        if self.is_long:
            ctx.push(POST_CONST_L, 0, LONG_MIN if self.greatest else LONG_MAX)
        else:
            ctx.push(POST_CONST_D, 0, double_bits(-math.inf if self.greatest else math.inf))
        for f in self.fields:
            t = f.emit(ctx)
            if self.is_long:
                ctx.to_long(t)
                ctx.push(POST_LMAX if self.greatest else POST_LMIN)
            else:
                ctx.to_double(t)
                ctx.push(POST_DMAX if self.greatest else POST_DMIN)
        return "long" if self.is_long else "double"

    def to_json(self):
        return {"type": self.type_name, "name": self.name, "fields": [f.to_json() for f in self.fields]}


class DoubleGreatestPostAggregator(_GreatestLeast):
    type_name, is_long, greatest = "doubleGreatest", False, True


class DoubleLeastPostAggregator(_GreatestLeast):
    type_name, is_long, greatest = "doubleLeast", False, False


class LongGreatestPostAggregator(_GreatestLeast):
    type_name, is_long, greatest = "longGreatest", True, True


class LongLeastPostAggregator(_GreatestLeast):
    type_name, is_long, greatest = "longLeast", True, False


_GREATEST_LEAST = {c.type_name: c for c in (DoubleGreatestPostAggregator, DoubleLeastPostAggregator,
                                            LongGreatestPostAggregator, LongLeastPostAggregator)}


@dataclass
class PostProgram:
    """A compiled post-aggregator: ops = [(op, arg, imm)] in postfix order, the value's type and the
    comparator's order kind."""
    ops: List[Tuple[int, int, int]]
    out_type: str
    order: int


def compile_post_aggregator(aggregations: Sequence[AggregatorFactory], post_aggregations: Sequence[PostAggregator],
                            name: str, for_order: bool = True) -> PostProgram:
    """The program of the query's post-aggregator `name` over the native slots of `aggregations`. for_order: the
    order kind is the post-aggregator's comparator (ValueError when it has none); otherwise (a having leaf, which
    compares numbers with HavingSpecMetricComparator) the value type's natural order. Programs beyond the ABI's
    length or stack are UnsupportedPostAggregator."""
    earlier: Dict[str, PostAggregator] = {}
    target = None
    for p in post_aggregations:
        if p.name == name:
            target = p
            break
        earlier[p.name] = p
    if target is None:
        raise ValueError(f"no post-aggregator named {name!r}")
    ctx = _PostCompile(aggregations, earlier)
    out_type = target.emit(ctx)
    if for_order:
        order = target.order_kind(ctx)
    else:
        order = POST_ORDER_LONG if out_type == "long" else POST_ORDER_DOUBLE
    if len(ctx.ops) > POST_MAX_OPS:
        raise UnsupportedPostAggregator(f"post-aggregator {name!r} compiles to {len(ctx.ops)} ops (max {POST_MAX_OPS})")
    depth = 0
    for op, _, _ in ctx.ops:
        depth += 1 if op <= POST_CONST_L else (0 if op <= POST_D2L else -1)
        if depth > POST_MAX_STACK:
            raise UnsupportedPostAggregator(f"post-aggregator {name!r} needs more than {POST_MAX_STACK} stack entries")
    return PostProgram(ctx.ops, out_type, order)


def post_program_order_key(order: int, word: int) -> int:
    """The unsigned order key of a program's raw 64-bit value under its order kind (pa_order_key of the engine):
    comparator order = key order."""
    sign = 1 << 63
    if order == POST_ORDER_NONE:
        return 0
    if order == POST_ORDER_LONG:
        return word ^ sign
    d = struct.unpack("<d", struct.pack("<Q", word))[0]
    if d != d:
        return 2 if order == POST_ORDER_NUMERIC_FIRST else (1 << 64) - 1
    if order == POST_ORDER_NUMERIC_FIRST and math.isinf(d):
        return 0 if d < 0 else 1
    return (~word & ((1 << 64) - 1)) if word & sign else (word | sign)


def post_value_word(v, out_type: str) -> int:
    """A post-aggregator value as the raw word a program leaves."""
    return (int(v) & ((1 << 64) - 1)) if out_type == "long" else double_bits(float(v))


def parse_post_aggregations(aggregations: Sequence[AggregatorFactory], post_aggregations) -> List[PostAggregator]:
    """Queries.prepareAggregations: names unique among aggregators and post-aggregators; every field names an
    aggregator or an EARLIER post-aggregator."""
    out = [PostAggregator.from_json(p) for p in (post_aggregations or [])]
    names = {a.name for a in aggregations}
    for p in out:
        if p.name is None:
            raise ValueError("a top-level post-aggregator needs a name")
        for f in p.dependent_fields():
            if f not in names:
                raise ValueError(f"Missing fields [{f}] for postAggregator [{p.name}]")
        if p.name in names:
            raise ValueError(f"[{p.name}] already defined")
        names.add(p.name)
    return out


def compute_post_aggregations(query, event: Dict[str, Any]) -> Dict[str, Any]:
    """The row with every post-aggregator's value added, in order (a later one may read an earlier one)."""
    for p in getattr(query, "postAggregations", None) or []:
        event[p.name] = p.compute(event)
    return event


def post_compare_key(p: PostAggregator, query, v):
    """Sort key realising the post-aggregator's comparator over its computed values."""
    prog = compile_post_aggregator(query.aggregations, query.postAggregations, p.name, True)
    return post_program_order_key(prog.order, post_value_word(v, prog.out_type))


# ----------------------------------------------------------------------------------------------
# topN metric specs
# ----------------------------------------------------------------------------------------------
@dataclass
class TopNMetricSpec:
    """numeric (metric name), inverted(numeric), or dimension ordering (DimensionTopNMetricSpec,
    LexicographicTopNMetricSpec, AlphaNumericTopNMetricSpec; `inverted` = InvertedTopNMetricSpec
    around it)."""
    type: str = "numeric"
    metric: Optional[str] = None
    ordering: str = "lexicographic"
    previous_stop: Optional[str] = None
    inverted: bool = False

    @staticmethod
    def of(spec) -> "TopNMetricSpec":
        if isinstance(spec, TopNMetricSpec):
            return spec
        if isinstance(spec, str):
            return TopNMetricSpec("numeric", spec)
        t = spec.get("type")
        if t == "numeric":
            return TopNMetricSpec("numeric", spec["metric"])
        if t == "inverted":
            inner = TopNMetricSpec.of(spec["metric"])
            if inner.type == "dimension":
                return TopNMetricSpec("dimension", None, inner.ordering, inner.previous_stop, not inner.inverted)
            if inner.type != "numeric":
                raise ValueError("only inverted numeric or dimension metric specs are supported")
            return TopNMetricSpec("inverted", inner.metric)
        if t in ("dimension", "lexicographic", "alphaNumeric"):
            ordering = _ordering_name(spec.get("ordering"), t == "alphaNumeric")
            return TopNMetricSpec("dimension", None, ordering, spec.get("previousStop"))
        raise ValueError(f"unsupported topN metric spec {spec!r}")

    def to_json(self):
        if self.type == "numeric":
            return {"type": "numeric", "metric": self.metric}
        if self.type == "inverted":
            return {"type": "inverted", "metric": {"type": "numeric", "metric": self.metric}}
        js = {"type": "dimension", "ordering": self.ordering, "previousStop": self.previous_stop}
        return {"type": "inverted", "metric": js} if self.inverted else js


# ----------------------------------------------------------------------------------------------
# numeric expressions (common/.../math/expr: Expr.g4, ExprListenerImpl, Expr, Function, ExprEval, Evals)
# ----------------------------------------------------------------------------------------------
def UnsupportedExpression(msg: str):
    """UnsupportedQuery for an expression construct the engine has no program for: the caller keeps its CPU
    engine."""
    from ._native import UnsupportedQuery
    return UnsupportedQuery(2, msg)


# ops of a compiled expression (DG_EXPR_* of include/druidgpu.h)
(EX_INPUT, EX_CONST_L, EX_CONST_D, EX_L2D, EX_D2L, EX_D2F, EX_ADD, EX_SUB, EX_MUL, EX_DIV, EX_MOD, EX_NEG, EX_NOT,
 EX_LT, EX_LE, EX_GT, EX_GE, EX_EQ, EX_NE, EX_AND, EX_OR, EX_SELECT, EX_ABS, EX_CEIL, EX_FLOOR, EX_MIN, EX_MAX,
 EX_IDIV) = range(28)
EXPR_MAX_OPS, EXPR_MAX_STACK, EXPR_MAX_INPUTS = 64, 16, 8
_EX_BINARY = {"+": EX_ADD, "-": EX_SUB, "*": EX_MUL, "/": EX_DIV, "%": EX_MOD, "<": EX_LT, "<=": EX_LE, ">": EX_GT,
              ">=": EX_GE, "==": EX_EQ, "!=": EX_NE, "&&": EX_AND, "||": EX_OR}
# every function the reference knows (Function.java; the macro table's: ExprMacroTable + query/expression/*):
# a name outside this list is a syntax error there, one inside it that the engine lacks is refused
# (names as Parser.FUNCTIONS keys them: lower-cased)
_EX_TRANSCENDENTAL = ("acos", "asin", "atan", "cbrt", "cos", "cosh", "exp", "expm1", "getexponent", "log", "log10",
                      "log1p", "nextup", "rint", "round", "signum", "sin", "sinh", "sqrt", "tan", "tanh", "todegrees",
                      "toradians", "ulp", "atan2", "copysign", "hypot", "remainder", "nextafter", "pow", "scalb")
_EX_STRING_FNS = ("concat", "strlen", "strpos", "substring", "replace", "lower", "upper", "like", "regexp_extract",
                  "lookup", "trim", "ltrim", "rtrim")
_EX_TIME_FNS = ("timestamp", "unix_timestamp", "timestamp_ceil", "timestamp_floor", "timestamp_shift",
                "timestamp_extract", "timestamp_format", "timestamp_parse")
_EX_NULL_FNS = ("nvl", "isnull", "notnull", "case_simple")
_EX_SUPPORTED_FNS = {"abs": 1, "ceil": 1, "floor": 1, "min": 2, "max": 2, "div": 2, "if": 3, "cast": 2,
                     "case_searched": None}

_EX_TOKEN = re.compile(r"""
    (?P<ws>[ \t\r\n]+)
  | (?P<double>[0-9]+\.[0-9]*)
  | (?P<long>[0-9]+)
  | (?P<id>[_$a-zA-Z][_$a-zA-Z0-9]*)
  | (?P<qid>"(?:\\(?:['"\\/bfnrt]|u[0-9a-fA-F]{4})|[^"\\])*")
  | (?P<str>'(?:\\(?:['"\\/bfnrt]|u[0-9a-fA-F]{4})|[^'\\])*')
  | (?P<op><=|>=|==|!=|&&|\|\||[-!^*/%+<>(),])
""", re.X)
_EX_ESCAPES = {"b": "\b", "f": "\f", "n": "\n", "r": "\r", "t": "\t", "'": "'", '"': '"', "\\": "\\", "/": "/"}


def _unescape_java(s: str) -> str:
    """StringEscapeUtils.unescapeJava over the escapes the lexer admits."""
    out, i = [], 0
    while i < len(s):
        c = s[i]
        if c != "\\":
            out.append(c)
            i += 1
        elif s[i + 1] == "u":
            out.append(chr(int(s[i + 2:i + 6], 16)))
            i += 6
        else:
            out.append(_EX_ESCAPES[s[i + 1]])
            i += 2
    return "".join(out)


def _ex_tokens(text: str) -> List[Tuple[str, Any]]:
    out, pos = [], 0
    while pos < len(text):
        m = _EX_TOKEN.match(text, pos)
        if m is None:
            raise ValueError(f"expression {text!r}: unexpected character at {pos}")
        pos = m.end()
        kind = m.lastgroup
        if kind == "ws":
            continue
        v = m.group()
        if kind == "long":  # Long.parseLong (ExprListenerImpl.exitLongExpr): the literal has no sign of its own
            if int(v) > LONG_MAX:
                raise ValueError(f"expression {text!r}: long literal {v} overflows (NumberFormatException)")
            out.append(("long", int(v)))
        elif kind == "double":  # Double.parseDouble: a literal past the range is Infinity
            try:
                out.append(("double", float(v)))
            except OverflowError:
                out.append(("double", math.inf))
        elif kind == "id":
            out.append(("null", None) if v == "null" else ("id", v))
        elif kind == "qid":
            out.append(("id", _unescape_java(v[1:-1])))
        elif kind == "str":
            out.append(("str", _unescape_java(v[1:-1])))
        else:
            out.append(("op", v))
    return out


# binary operators by binding strength, loosest first (Expr.g4: an alternative listed earlier binds tighter;
# every level is left-associative but '^')
_EX_LEVELS = [("&&", "||"), ("<", "<=", ">", ">=", "==", "!="), ("+", "-"), ("*", "/", "%"), ("^",)]


class _ExParser:
    def __init__(self, text: str):
        self.text, self.toks, self.i = text, _ex_tokens(text), 0

    def peek(self):
        return self.toks[self.i] if self.i < len(self.toks) else ("end", None)

    def take(self):
        t = self.peek()
        self.i += 1
        return t

    def fail(self, what):
        raise ValueError(f"expression {self.text!r}: {what}")

    def parse(self):
        e = self.binary(0)
        if self.peek()[0] != "end":
            self.fail(f"unexpected {self.peek()[1]!r}")
        return e

    def binary(self, level):
        if level == len(_EX_LEVELS):
            return self.unary()
        ops = _EX_LEVELS[level]
        left = self.binary(level + 1)
        while self.peek() in [("op", o) for o in ops]:
            op = self.take()[1]
            if op == "^":  # right-associative
                return ("bin", op, left, self.binary(level))
            left = ("bin", op, left, self.binary(level + 1))
        return left

    def unary(self):
        t = self.peek()
        if t in (("op", "-"), ("op", "!")):  # binds tighter than every binary operator: -a ^ b is (-a) ^ b
            self.take()
            return ("un", t[1], self.unary())
        return self.atom()

    def atom(self):
        kind, v = self.take()
        if kind in ("long", "double", "str"):
            return (kind, v)
        if kind == "null":
            return ("null",)
        if kind == "op" and v == "(":
            e = self.binary(0)
            if self.take() != ("op", ")"):
                self.fail("missing ')'")
            return e
        if kind == "id":
            if self.peek() != ("op", "("):
                return ("id", v)
            self.take()
            args = []
            if self.peek() != ("op", ")"):
                args.append(self.binary(0))
                while self.peek() == ("op", ","):
                    self.take()
                    args.append(self.binary(0))
            if self.take() != ("op", ")"):
                self.fail("missing ')' after function arguments")
            # (Parser.getFunction and ExprMacroTable.get look the name up lower-cased: IF(a, b, c) is if(a, b, c))
            return ("fn", v.lower(), args)
        self.fail("unexpected end" if kind == "end" else f"unexpected {v!r}")


def parse_expression(text: str, check: bool = True):
    """Expr.g4 as an AST of tuples: ("long", v) ("double", v) ("str", s) ("null",) ("id", name) ("un", op, e)
    ("bin", op, l, r) ("fn", name, [args]). Syntax errors and unknown function names are ValueError; constructs the
    engine refuses whatever the columns' types are raise UnsupportedQuery here (check_expression; check=False:
    the tree as the grammar reads it, refused constructs included)."""
    if not isinstance(text, str):
        raise ValueError("an expression must be a string")
    ast = _ExParser(text).parse()
    if check:
        check_expression(ast)
    return ast


def check_expression(ast) -> None:
    """The refusals that do not depend on the columns' types, each naming its construct."""
    kind = ast[0]
    if kind == "str":
        raise UnsupportedExpression("expression: string literal (string expressions stay on the CPU)")
    if kind == "null":
        raise UnsupportedExpression("expression: null (the reference types it as a string)")
    if kind == "un":
        check_expression(ast[2])
    elif kind == "bin":
        if ast[1] == "^":
            raise UnsupportedExpression("expression: operator ^ (the device's pow is not Java's bit for bit)")
        check_expression(ast[2])
        check_expression(ast[3])
    elif kind == "fn":
        name, args = ast[1], ast[2]
        if name in _EX_TRANSCENDENTAL:
            raise UnsupportedExpression(f"expression: function {name} (its device result is not Java's bit for bit)")
        if name in _EX_STRING_FNS:
            raise UnsupportedExpression(f"expression: string function {name}")
        if name in _EX_TIME_FNS:
            raise UnsupportedExpression(f"expression: time function {name}")
        if name in _EX_NULL_FNS:
            raise UnsupportedExpression(f"expression: function {name} (null handling stays on the CPU)")
        if name not in _EX_SUPPORTED_FNS:
            raise ValueError(f"expression: unknown function {name!r}")
        want = _EX_SUPPORTED_FNS[name]
        if want is not None and len(args) != want:
            raise ValueError(f"expression: function {name} needs {want} argument{'s' if want > 1 else ''}")
        if name == "case_searched":
            if len(args) < 2:
                raise ValueError("expression: function case_searched must have at least 2 arguments")
            if len(args) % 2 == 0:
                raise UnsupportedExpression("expression: case_searched without an ELSE branch (its value may be null)")
        if name == "cast":
            if args[1][0] != "str":
                raise UnsupportedExpression("expression: cast to a type that is not a literal")
            t = args[1][1].upper()
            if t == "STRING":
                raise UnsupportedExpression("expression: cast to STRING")
            if t not in ("LONG", "DOUBLE"):
                raise ValueError(f"expression: invalid type {args[1][1]!r}")
            check_expression(args[0])
        else:
            for a in args:
                check_expression(a)


def expression_identifiers(ast) -> List[str]:
    """The identifiers of an expression in first-use order (Parser.findRequiredBindings)."""
    out: List[str] = []

    def walk(n):
        if n[0] == "id":
            if n[1] not in out:
                out.append(n[1])
        elif n[0] == "un":
            walk(n[2])
        elif n[0] == "bin":
            walk(n[2])
            walk(n[3])
        elif n[0] == "fn":
            for a in n[2]:
                if a[0] != "str":
                    walk(a)
    walk(ast)
    return out


@dataclass
class ExprProgram:
    """A compiled expression: ops [(op, arg, imm)] over `inputs` (column names), the stack type its value has
    ("long" / "double") and, once with_output gave it one, the derived column's type."""
    ops: List[Tuple[int, int, int]]
    inputs: List[str]
    type: str
    out_type: Optional[str] = None

    def with_output(self, out_type: str) -> "ExprProgram":
        """The program whose value is cast to a LONG, DOUBLE or FLOAT column (ExprEval.asLong / asDouble,
        ExpressionColumnValueSelector.getFloat)."""
        ops = list(self.ops)
        if out_type == "LONG":
            if self.type == "double":
                ops.append((EX_D2L, 0, 0))
        elif out_type in ("DOUBLE", "FLOAT"):
            if self.type == "long":
                ops.append((EX_L2D, 0, 0))
            if out_type == "FLOAT":
                ops.append((EX_D2F, 0, 0))
        else:
            raise UnsupportedExpression(f"expression: output type {out_type}")
        if len(ops) > EXPR_MAX_OPS:
            raise UnsupportedExpression(f"expression: more than {EXPR_MAX_OPS} ops")
        return ExprProgram(ops, list(self.inputs), self.type, out_type)

    def natural(self) -> "ExprProgram":
        return self.with_output("LONG" if self.type == "long" else "DOUBLE")

    def digest(self) -> str:
        """The derived column's name: a digest of (ops, inputs, output type) behind a prefix no Druid column has
        (a control character), so equal expressions share a column and different ones cannot collide."""
        import hashlib
        h = hashlib.sha1(repr((self.ops, self.inputs, self.out_type)).encode()).hexdigest()
        return "\x01expr:" + h[:32]


def compile_expression(ast, column_type) -> ExprProgram:
    """Type-check an expression against one segment's columns and compile it to postfix ops.
    column_type(name) -> "LONG" / "FLOAT" / "DOUBLE", "STRING" or None (no such column); "__time" is LONG."""
    ops: List[Tuple[int, int, int]] = []
    inputs: List[str] = []
    types: Dict[int, str] = {}
    state = {"sp": 0, "max": 0}

    def typeof(n) -> str:
        t = types.get(id(n))
        if t is None:
            t = types[id(n)] = _typeof(n)
        return t

    def _typeof(n) -> str:
        k = n[0]
        if k in ("long", "double"):
            return k
        if k == "id":
            ct = "LONG" if n[1] == "__time" else column_type(n[1])
            if ct is None:
                raise UnsupportedExpression(f"expression: the segment has no column {n[1]} (it would read null)")
            if ct not in ("LONG", "FLOAT", "DOUBLE"):
                raise UnsupportedExpression(f"expression: column {n[1]} is not numeric")
            return "long" if ct == "LONG" else "double"
        if k == "un":
            return typeof(n[2])
        if k == "bin":
            lt, rt = typeof(n[2]), typeof(n[3])
            if n[1] in ("&&", "||"):
                if lt != rt:
                    raise UnsupportedExpression(f"expression: operands of {n[1]} differ in type "
                                                "(the value's type would differ from row to row)")
                return lt
            return "long" if lt == rt == "long" else "double"
        name, args = n[1], n[2]
        if name in ("ceil", "floor"):
            typeof(args[0])
            return "double"
        if name == "abs":
            return typeof(args[0])
        if name in ("min", "max"):
            return "long" if typeof(args[0]) == typeof(args[1]) == "long" else "double"
        if name == "div":
            typeof(args[0]), typeof(args[1])
            return "long"
        if name == "cast":
            typeof(args[0])
            return args[1][1].lower()
        branches = [args[1], args[2]] if name == "if" else [args[i] for i in range(1, len(args), 2)] + [args[-1]]
        conds = [args[0]] if name == "if" else [args[i] for i in range(0, len(args) - 1, 2)]
        for c in conds:
            typeof(c)
        ts = {typeof(b) for b in branches}
        if len(ts) != 1:
            raise UnsupportedExpression(f"expression: branches of {'if' if name == 'if' else 'case'} differ in type "
                                        "(the value's type would differ from row to row)")
        return ts.pop()

    def push(op, arg=0, imm=0, pops=0):
        ops.append((op, arg, imm & ((1 << 64) - 1)))
        state["sp"] += 1 - pops
        state["max"] = max(state["max"], state["sp"])

    def emit_as(n, want: str):
        emit(n)
        if typeof(n) != want:
            push(EX_L2D if want == "double" else EX_D2L, pops=1)

    def constant(n):
        """The value of a subexpression without identifiers, or None."""
        if expression_identifiers(n):
            return None
        sub = compile_expression(n, lambda name: None)
        return run_expression(sub.ops, [])

    def emit(n):
        k = n[0]
        if k == "long":
            push(EX_CONST_L, imm=n[1])
        elif k == "double":
            push(EX_CONST_D, imm=double_bits(n[1]))
        elif k == "id":
            typeof(n)
            if n[1] not in inputs:
                inputs.append(n[1])
            push(EX_INPUT, arg=inputs.index(n[1]))
        elif k == "un":
            emit(n[2])
            push(EX_NEG if n[1] == "-" else EX_NOT, pops=1)
        elif k == "bin":
            op, t = n[1], typeof(n)
            operand = t if op in ("&&", "||") else ("long" if typeof(n[2]) == typeof(n[3]) == "long" else "double")
            if op in ("/", "%") and operand == "long":
                zero_divisor(n[2], n[3])
            emit_as(n[2], operand)
            emit_as(n[3], operand)
            push(_EX_BINARY[op], pops=2)
        else:
            name, args = n[1], n[2]
            if name in ("abs", "ceil", "floor"):
                emit_as(args[0], "double" if name != "abs" else typeof(args[0]))
                push({"abs": EX_ABS, "ceil": EX_CEIL, "floor": EX_FLOOR}[name], pops=1)
            elif name in ("min", "max", "div"):
                operand = "long" if typeof(args[0]) == typeof(args[1]) == "long" else "double"
                if name == "div" and operand == "long":
                    zero_divisor(args[0], args[1])
                emit_as(args[0], operand)
                emit_as(args[1], operand)
                push({"min": EX_MIN, "max": EX_MAX, "div": EX_IDIV}[name], pops=2)
            elif name == "cast":
                emit_as(args[0], typeof(n))
            else:  # if / case_searched: c1 ? a1 : (c2 ? a2 : ... else)
                typeof(n)
                rest = list(args)

                def chain(rest):
                    if len(rest) == 1:
                        emit(rest[0])
                        return
                    emit(rest[0])
                    emit(rest[1])
                    chain(rest[2:])
                    push(EX_SELECT, pops=3)
                chain(rest)

    def zero_divisor(l, r):
        # Parser.flatten evaluates a constant subexpression while parsing: a long division by zero throws there
        if not expression_identifiers(l) and not expression_identifiers(r):
            c = constant(r)
            if c is not None and c[0] == 0:
                raise UnsupportedExpression("expression: a constant subexpression divides a long by zero "
                                            "(ArithmeticException while parsing)")

    t = typeof(ast)
    emit(ast)
    if len(inputs) > EXPR_MAX_INPUTS:
        raise UnsupportedExpression(f"expression: more than {EXPR_MAX_INPUTS} input columns")
    if len(ops) > EXPR_MAX_OPS:
        raise UnsupportedExpression(f"expression: more than {EXPR_MAX_OPS} ops")
    if state["max"] > EXPR_MAX_STACK:
        raise UnsupportedExpression(f"expression: more than {EXPR_MAX_STACK} operands alive at once")
    return ExprProgram(ops, inputs, t)


def _java_ldiv(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return _wrap64(q if (a < 0) == (b < 0) else -q)


def _java_lmod(a: int, b: int) -> int:
    return a - b * (abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1))


def java_fmod(x: float, y: float) -> float:
    """Java's double % (JLS 15.17.3) = C fmod."""
    if x != x or y != y or math.isinf(x) or y == 0.0:
        return math.nan
    if math.isinf(y):
        return x
    return math.fmod(x, y)


def _java_ceil_floor(x: float, up: bool) -> float:
    if x != x or math.isinf(x):
        return x
    r = float(math.ceil(x) if up else math.floor(x))
    return math.copysign(r, x) if r == 0.0 else r


def _bits_double(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def run_expression(ops: Sequence[Tuple[int, int, int]], row: Sequence[Tuple[str, Any]]):
    """The evaluator of csrc/dg_expr.h in Python, for one row: row[k] = ("LONG" | "DOUBLE" | "FLOAT", value) of
    input k. Returns (word, poisoned): the final 64-bit word (a long as unsigned, a double's canonical bits, a
    D2F result's float32 bits) and whether it depends on a long division by zero."""
    M = (1 << 64) - 1
    st: List[Tuple[str, Any, bool]] = []  # (type, value, poisoned); a long as a signed int, a double as a float

    def truth(e):
        return e[1] > 0

    for op, arg, imm in ops:
        if op == EX_INPUT:
            t, v = row[arg]
            st.append(("long", _wrap64(int(v)), False) if t == "LONG" else
                      ("double", _f32(v) if t == "FLOAT" else float(v), False))
        elif op == EX_CONST_L:
            st.append(("long", _wrap64(imm), False))
        elif op == EX_CONST_D:
            st.append(("double", _bits_double(imm), False))
        elif op in (EX_L2D, EX_D2L, EX_D2F, EX_NEG, EX_NOT, EX_ABS, EX_CEIL, EX_FLOOR):
            t, v, p = st.pop()
            if op == EX_L2D:
                st.append(("double", float(v), p))
            elif op == EX_D2L:
                st.append(("long", java_d2l(v), p))
            elif op == EX_D2F:
                f = struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0] if v != v else _f32_round(v)
                st.append(("float", f, p))
            elif op == EX_NEG:
                st.append((t, _wrap64(-v) if t == "long" else -v, p))
            elif op == EX_NOT:
                b = not truth((t, v))
                st.append((t, int(b) if t == "long" else float(b), p))
            elif op == EX_ABS:
                st.append((t, _wrap64(abs(v)) if t == "long" else abs(v), p))
            else:
                st.append((t, _java_ceil_floor(v, op == EX_CEIL), p))
        elif op == EX_SELECT:
            b, a, c = st.pop(), st.pop(), st.pop()
            pick = a if truth(c) else b
            st.append((pick[0], pick[1], c[2] or pick[2]))
        else:
            b, a = st.pop(), st.pop()
            t, x, y, p = a[0], a[1], b[1], a[2] or b[2]
            if op in (EX_AND, EX_OR):
                right = truth(a) if op == EX_AND else not truth(a)
                pick = b if right else a
                st.append((pick[0], pick[1], a[2] or (right and b[2])))
            elif t == "long":
                if op in (EX_DIV, EX_IDIV, EX_MOD) and y == 0:
                    st.append(("long", 0, True))
                    continue
                r = {EX_ADD: lambda: x + y, EX_SUB: lambda: x - y, EX_MUL: lambda: x * y,
                     EX_DIV: lambda: _java_ldiv(x, y), EX_IDIV: lambda: _java_ldiv(x, y),
                     EX_MOD: lambda: _java_lmod(x, y), EX_LT: lambda: int(x < y), EX_LE: lambda: int(x <= y),
                     EX_GT: lambda: int(x > y), EX_GE: lambda: int(x >= y), EX_EQ: lambda: int(x == y),
                     EX_NE: lambda: int(x != y), EX_MIN: lambda: min(x, y), EX_MAX: lambda: max(x, y)}[op]()
                st.append(("long", _wrap64(r), p))
            else:
                cmp = java_double_compare(x, y)
                if op == EX_IDIV:
                    st.append(("long", java_d2l(java_double_div(x, y)), p))
                    continue
                r = {EX_ADD: lambda: x + y, EX_SUB: lambda: x - y, EX_MUL: lambda: x * y,
                     EX_DIV: lambda: java_double_div(x, y), EX_MOD: lambda: java_fmod(x, y),
                     EX_LT: lambda: float(cmp < 0), EX_LE: lambda: float(cmp <= 0), EX_GT: lambda: float(cmp > 0),
                     EX_GE: lambda: float(cmp >= 0), EX_EQ: lambda: float(x == y), EX_NE: lambda: float(x != y),
                     EX_MIN: lambda: java_min(x, y) if y == y else y,
                     EX_MAX: lambda: java_max(x, y) if y == y else y}[op]()
                st.append(("double", r, p))
    t, v, p = st.pop()
    if t == "long":
        return v & M, p
    if t == "float":
        return (0x7FC00000 if v != v else struct.unpack("<I", struct.pack("<f", v))[0]), p
    return double_bits(v), p


def _f32_round(d: float) -> float:
    """Java's (float) double: round to nearest even, past the range an infinity (struct.pack raises there)."""
    try:
        return _f32(d)
    except OverflowError:
        return math.copysign(math.inf, d)


@dataclass
class ExpressionVirtualColumn:
    """segment/virtual/ExpressionVirtualColumn.java: a column computed from an expression over the segment's
    columns; outputType defaults to FLOAT (:59)."""
    name: str
    expression: str
    outputType: str = "FLOAT"

    def __post_init__(self):
        if not self.name:
            raise ValueError("a virtual column needs a name")
        self.outputType = str(self.outputType or "FLOAT").upper()
        if self.outputType not in DIMENSION_OUTPUT_TYPES:
            raise ValueError(f"unknown outputType {self.outputType!r}")
        self.ast = parse_expression(self.expression)

    def to_json(self):
        return {"type": "expression", "name": self.name, "expression": self.expression, "outputType": self.outputType}

    @staticmethod
    def from_json(js) -> "ExpressionVirtualColumn":
        if isinstance(js, ExpressionVirtualColumn):
            return js
        if js.get("type") != "expression":
            raise ValueError(f"unsupported virtual column type {js.get('type')!r}")
        return ExpressionVirtualColumn(js["name"], js["expression"], js.get("outputType") or "FLOAT")


def parse_virtual_columns(specs) -> List[ExpressionVirtualColumn]:
    """VirtualColumns.create (segment/VirtualColumns.java:60-90): no duplicate names, no __time; a virtual column
    that references another one is refused (the engine derives a column from stored columns only)."""
    out = [ExpressionVirtualColumn.from_json(v) for v in (specs or [])]
    names = [v.name for v in out]
    if len(set(names)) != len(names):
        raise ValueError("duplicate virtual column names")
    if "__time" in names:
        raise ValueError("a virtual column cannot be named __time")
    for v in out:
        for ident in expression_identifiers(v.ast):
            if ident in names:
                raise UnsupportedExpression(f"virtual column {v.name} references virtual column {ident}")
    return out


def _with_virtual_columns(js, query):
    """virtualColumns only when there are some: a query without them serializes as it always did."""
    if query.virtualColumns:
        js["virtualColumns"] = [v.to_json() for v in query.virtualColumns]
    return js


def query_uses_expressions(query) -> bool:
    """The query needs derived columns: a virtual column, an aggregator expression or an expression filter."""
    def in_filter(f):
        if f is None:
            return False
        if isinstance(f, ExpressionDimFilter):
            return True
        if isinstance(f, (AndDimFilter, OrDimFilter)):
            return any(in_filter(c) for c in f.fields)
        return in_filter(f.field) if isinstance(f, NotDimFilter) else False
    return bool(getattr(query, "virtualColumns", None)) or in_filter(query.filter) or \
        any(a.expression is not None or in_filter(a.filter) for a in query.aggregations)


# ----------------------------------------------------------------------------------------------
# queries
# ----------------------------------------------------------------------------------------------
@dataclass
class BaseQuery:
    dataSource: str = "ds"
    intervals: List[Tuple[int, int]] = field(default_factory=lambda: [(MIN_INSTANT, MAX_INSTANT)])
    granularity: Granularity = ALL
    filter: Optional[DimFilter] = None
    aggregations: List[AggregatorFactory] = field(default_factory=list)
    context: Dict[str, Any] = field(default_factory=dict)

    def __post_init__(self):
        self.intervals = [parse_interval(i) for i in self.intervals]
        if len(self.intervals) != 1:
            raise ValueError("exactly one query interval is supported (TopNQueryEngine.java:75-77)")
        self.granularity = Granularity.of(self.granularity)
        self.filter = DimFilter.from_json(self.filter)
        self.aggregations = [AggregatorFactory.from_json(a) for a in self.aggregations]
        names = [a.name for a in self.aggregations]
        if len(set(names)) != len(names):
            raise ValueError("duplicate aggregator names")

    @property
    def interval(self) -> Tuple[int, int]:
        return self.intervals[0]

    def effective_filter(self) -> Optional[DimFilter]:
        return self.filter.optimize() if self.filter is not None else None

    def _base_json(self, qtype):
        js = {"queryType": qtype, "dataSource": self.dataSource,
              "intervals": [f"{format_time(s)}/{format_time(e)}" for s, e in self.intervals],
              "granularity": self.granularity.to_json(),
              "aggregations": [a.to_json() for a in self.aggregations]}
        if self.filter is not None:
            js["filter"] = self.filter.to_json()
        if self.context:
            js["context"] = dict(self.context)
        return js


def _with_post_aggregations(js, query):
    """postAggregations only when there are some: a query without them serializes as it always did."""
    if query.postAggregations:
        js["postAggregations"] = [p.to_json() for p in query.postAggregations]
    return js


@dataclass
class TimeseriesQuery(BaseQuery):
    descending: bool = False
    postAggregations: List = field(default_factory=list)
    virtualColumns: List = field(default_factory=list)

    def __post_init__(self):
        super().__post_init__()
        self.postAggregations = parse_post_aggregations(self.aggregations, self.postAggregations)
        self.virtualColumns = parse_virtual_columns(self.virtualColumns)

    @property
    def skip_empty_buckets(self) -> bool:
        return bool(self.context.get("skipEmptyBuckets", False))

    def to_json(self):
        js = self._base_json("timeseries")
        js["descending"] = self.descending
        return _with_virtual_columns(_with_post_aggregations(js, self), self)


@dataclass
class TopNQuery(BaseQuery):
    """dimension: the column's name; it may be given as a DefaultDimensionSpec, whose outputType
    (query/dimension/DefaultDimensionSpec.java:68-78, STRING when absent) becomes dimension_type."""
    dimension: str = ""
    metric: Any = None
    threshold: int = 10
    dimension_type: str = "STRING"
    postAggregations: List = field(default_factory=list)
    virtualColumns: List = field(default_factory=list)
    # set by the runners (virtual.lower_query), never serialized: the derived column that stands for a dimension
    # over a virtual column in the native calls; results keep the dimension's own name
    derivedDimensions: Dict[str, str] = field(default_factory=dict)

    def __post_init__(self):
        super().__post_init__()
        self.virtualColumns = parse_virtual_columns(self.virtualColumns)
        if isinstance(self.dimension, dict):
            if self.dimension.get("extractionFn") is not None:
                raise ValueError("extraction functions are out of scope")
            if self.dimension.get("outputType") is not None:
                self.dimension_type = self.dimension["outputType"]
            self.dimension = self.dimension["dimension"]
        self.dimension_type = str(self.dimension_type).upper()
        if self.dimension_type not in DIMENSION_OUTPUT_TYPES:
            raise ValueError(f"unknown outputType {self.dimension_type!r}")
        self.postAggregations = parse_post_aggregations(self.aggregations, self.postAggregations)
        self.metric = TopNMetricSpec.of(self.metric)
        if self.metric.type in ("numeric", "inverted") and self.metric.metric not in {a.name for a in self.aggregations}:
            if self.metric.metric in {p.name for p in self.postAggregations}:
                self.metric_program()  # (ValueError: no comparator; UnsupportedQuery: no program)
            else:
                raise ValueError("topN metric must name an aggregator")

    @property
    def native_dimension(self) -> str:
        """The column the native calls group by: the dimension, or the derived column that stands for it."""
        return self.derivedDimensions.get(self.dimension, self.dimension)

    def metric_program(self) -> Optional["PostProgram"]:
        """The program of the post-aggregator a numeric / inverted metric spec names (NumericTopNMetricSpec.
        getComparator takes the post-aggregator's comparator), or None when it names an aggregator."""
        if self.metric.type not in ("numeric", "inverted") or self.metric.metric in {a.name for a in self.aggregations}:
            return None
        prog = compile_post_aggregator(self.aggregations, self.postAggregations, self.metric.metric, True)
        if prog.order == POST_ORDER_NONE:
            raise UnsupportedPostAggregator("topN ranked by a constant post-aggregator (every value ties)")
        return prog

    @property
    def min_topn_threshold(self) -> int:
        # TopNQueryConfig.minTopNThreshold = 1000 (TopNQueryConfig.java:32), context override
        return int(self.context.get("minTopNThreshold", 1000))

    @property
    def segment_threshold(self) -> int:
        """Per-segment threshold after TopNQueryQueryToolChest.preMergeQueryDecoration (:553-561)."""
        return max(self.threshold, self.min_topn_threshold)

    def to_json(self):
        js = self._base_json("topN")
        dim = self.dimension
        if self.dimension_type != "STRING":
            dim = {"type": "default", "dimension": dim, "outputName": dim, "outputType": self.dimension_type}
        js.update({"dimension": dim, "metric": self.metric.to_json(), "threshold": self.threshold})
        return _with_virtual_columns(_with_post_aggregations(js, self), self)


@dataclass
class OrderByColumnSpec:
    """groupby/orderby/OrderByColumnSpec.java: column, direction, dimensionOrder (StringComparator)."""
    dimension: str
    direction: str = "ascending"
    dimensionOrder: str = "lexicographic"

    @staticmethod
    def from_json(js) -> "OrderByColumnSpec":
        if isinstance(js, str):
            return OrderByColumnSpec(js)
        d = str(js.get("direction", "ascending")).lower()
        if d in ("asc", "ascending"):
            d = "ascending"
        elif d in ("desc", "descending"):
            d = "descending"
        else:
            raise ValueError(f"Unknown direction[{d}]")
        order = js.get("dimensionOrder", "lexicographic") or "lexicographic"
        if isinstance(order, dict):
            order = order.get("type", "lexicographic")
        order = str(order).lower()
        if order not in ("lexicographic", "alphanumeric", "numeric", "strlen"):
            raise ValueError(f"unsupported dimensionOrder {order!r}")
        return OrderByColumnSpec(js["dimension"], d, order)

    def to_json(self):
        return {"dimension": self.dimension, "direction": self.direction, "dimensionOrder": self.dimensionOrder}


@dataclass
class DefaultLimitSpec:
    """groupby/orderby/DefaultLimitSpec.java: ORDER BY columns + LIMIT (None = Integer.MAX_VALUE)."""
    columns: List[OrderByColumnSpec] = field(default_factory=list)
    limit: Optional[int] = None

    @staticmethod
    def from_json(js) -> Optional["DefaultLimitSpec"]:
        if js is None:
            return None
        t = js.get("type", "default")
        if t == "noop":
            return None
        if t != "default":
            raise ValueError(f"unsupported limitSpec {t!r}")
        limit = js.get("limit")
        if limit is not None and int(limit) <= 0:
            raise ValueError(f"limit[{limit}] must be >0")
        return DefaultLimitSpec([OrderByColumnSpec.from_json(c) for c in js.get("columns") or []],
                                None if limit is None else int(limit))

    def to_json(self):
        js = {"type": "default", "columns": [c.to_json() for c in self.columns]}
        if self.limit is not None:
            js["limit"] = self.limit
        return js


@dataclass
class HavingSpec:
    """groupby/having/*HavingSpec.java as a tree: type in greaterThan / lessThan / equalTo
    (aggregation, value), dimSelector (dimension, value), and / or (specs), not (specs[0]), always,
    never."""
    type: str
    aggregation: Optional[str] = None
    value: Any = None
    dimension: Optional[str] = None
    specs: List["HavingSpec"] = field(default_factory=list)

    @staticmethod
    def from_json(js) -> Optional["HavingSpec"]:
        if js is None:
            return None
        t = js["type"]
        if t in ("greaterThan", "lessThan", "equalTo"):
            return HavingSpec(t, aggregation=js["aggregation"], value=js["value"])
        if t == "dimSelector":
            if js.get("extractionFn") is not None:
                raise ValueError("extraction functions are out of scope")
            return HavingSpec(t, dimension=js["dimension"], value=js.get("value"))
        if t in ("and", "or"):
            return HavingSpec(t, specs=[HavingSpec.from_json(x) for x in js["havingSpecs"]])
        if t == "not":
            return HavingSpec(t, specs=[HavingSpec.from_json(js["havingSpec"])])
        if t in ("always", "never"):
            return HavingSpec(t)
        raise ValueError(f"unsupported having {t!r}")

    def to_json(self):
        if self.type in ("greaterThan", "lessThan", "equalTo"):
            return {"type": self.type, "aggregation": self.aggregation, "value": self.value}
        if self.type == "dimSelector":
            return {"type": self.type, "dimension": self.dimension, "value": self.value}
        if self.type in ("and", "or"):
            return {"type": self.type, "havingSpecs": [x.to_json() for x in self.specs]}
        if self.type == "not":
            return {"type": "not", "havingSpec": self.specs[0].to_json()}
        return {"type": self.type}


# ValueType names a DimensionSpec's outputType may carry (segment/column/ValueType.java); the engine groups
# with STRING and LONG and refuses the others
DIMENSION_OUTPUT_TYPES = ("STRING", "LONG", "FLOAT", "DOUBLE")


@dataclass
class GroupByQuery(BaseQuery):
    """dimensions: the grouping columns' names; a dimension may be given as a DefaultDimensionSpec
    ({"type": "default", "dimension": ..., "outputType": "STRING" | "LONG"},
    query/dimension/DefaultDimensionSpec.java:68-78, outputType defaults to STRING). dimensionTypes: the
    output type of every dimension, parallel to `dimensions`."""
    dimensions: List[str] = field(default_factory=list)
    limitSpec: Optional[DefaultLimitSpec] = None
    having: Optional[HavingSpec] = None
    dimensionTypes: Optional[List[str]] = None
    postAggregations: List = field(default_factory=list)
    virtualColumns: List = field(default_factory=list)
    derivedDimensions: Dict[str, str] = field(default_factory=dict)  # (as TopNQuery's)

    def __post_init__(self):
        super().__post_init__()
        self.virtualColumns = parse_virtual_columns(self.virtualColumns)
        if isinstance(self.limitSpec, dict):
            self.limitSpec = DefaultLimitSpec.from_json(self.limitSpec)
        if isinstance(self.having, dict):
            self.having = HavingSpec.from_json(self.having)
        given = list(self.dimensionTypes) if self.dimensionTypes is not None else None
        if given is not None and len(given) != len(self.dimensions):
            raise ValueError("dimensionTypes must name one output type per dimension")
        dims, types = [], []
        for i, d in enumerate(self.dimensions):
            t = given[i] if given is not None else "STRING"
            if isinstance(d, dict):
                if d.get("type", "default") != "default":
                    raise ValueError(f"unsupported dimension spec {d.get('type')!r}")
                if d.get("extractionFn") is not None:
                    raise ValueError("extraction functions are out of scope")
                if d.get("outputName") not in (None, d["dimension"]):
                    raise ValueError("renamed dimensions (outputName) are out of scope")
                if d.get("outputType") is not None:
                    t = d["outputType"]
                dims.append(d["dimension"])
            else:
                dims.append(d)
            t = str(t).upper()
            if t not in DIMENSION_OUTPUT_TYPES:
                raise ValueError(f"unknown outputType {t!r}")
            types.append(t)
        self.dimensions = dims
        self.dimensionTypes = types
        self.postAggregations = parse_post_aggregations(self.aggregations, self.postAggregations)
        if any(p.name in dims for p in self.postAggregations):
            raise ValueError("a post-aggregator has the name of a dimension")

    @property
    def native_dimensions(self) -> List[str]:
        """The columns the native calls group by (TopNQuery.native_dimension)."""
        return [self.derivedDimensions.get(d, d) for d in self.dimensions]

    def post_aggregator(self, name: str) -> Optional["PostAggregator"]:
        for p in self.postAggregations:
            if p.name == name:
                return p
        return None

    def dimension_type(self, name: str) -> str:
        """The output type of the grouping dimension `name` (STRING for anything else)."""
        return self.dimensionTypes[self.dimensions.index(name)] if name in self.dimensions else "STRING"

    def _ctx_bool(self, key: str, default: bool) -> bool:
        v = (self.context or {}).get(key, default)
        if isinstance(v, str):  # QueryContexts.parseBoolean: Boolean.parseBoolean of a string
            return v.strip().lower() == "true"
        return bool(v)

    def force_hash_aggregation(self) -> bool:
        """GroupByQueryConfig.CTX_KEY_FORCE_HASH_AGGREGATION (GroupByQueryConfig.java:35-40,179-200)."""
        return self._ctx_bool("forceHashAggregation", False)

    def buffer_grouper_max_size(self) -> int:
        """The context's bufferGrouperMaxSize (GroupByQueryConfig.CTX_KEY_BUFFER_GROUPER_MAX_SIZE): the most
        groups a grouper may hold; 0 = not set (Integer.MAX_VALUE in the reference)."""
        v = (self.context or {}).get("bufferGrouperMaxSize")
        if v is None or isinstance(v, bool):
            return 0
        return max(int(v), 0)

    def order_by_dims(self) -> Optional[List[int]]:
        """Dimension index of every ORDER BY column (OrderByColumnSpec.getDimIndexForOrderBy), or None
        when one sorts on a non-grouping field (DefaultLimitSpec.sortingOrderHasNonGroupingFields)."""
        idx = []
        for c in (self.limitSpec.columns if self.limitSpec else []):
            if c.dimension not in self.dimensions:
                return None
            idx.append(self.dimensions.index(c.dimension))
        return idx

    def apply_limit_push_down(self) -> bool:
        """GroupByQuery.determineApplyLimitPushDown / validateAndGetForceLimitPushDown
        (query/groupby/GroupByQuery.java:352-416): a limited DefaultLimitSpec ordered by grouping
        dimensions only, no having spec, applyLimitPushDown not switched off in the context. A forced
        push-down (forceLimitPushDown) that sorts on aggregators is not pushed here: the reference
        then truncates every segment's grouper by partial aggregates (approximate); this engine
        returns the exact ordering instead."""
        ls = self.limitSpec
        force = self._ctx_bool("forceLimitPushDown", False)
        if force:
            if ls is None:
                raise ValueError("When forcing limit push down, a limit spec must be provided.")
            if ls.limit is None:
                raise ValueError("When forcing limit push down, the provided limit spec must have a limit.")
            if self.having is not None:
                raise ValueError("Cannot force limit push down when a having spec is present.")
        if ls is None or ls.limit is None:
            return False
        if not force and (not self._ctx_bool("applyLimitPushDown", True) or self.having is not None):
            return False
        return self.order_by_dims() is not None

    def to_json(self):
        js = self._base_json("groupBy")
        if all(t == "STRING" for t in self.dimensionTypes):
            js["dimensions"] = list(self.dimensions)
        else:  # DefaultDimensionSpec JSON: the output types travel with the dimensions
            js["dimensions"] = [{"type": "default", "dimension": d, "outputName": d, "outputType": t}
                                for d, t in zip(self.dimensions, self.dimensionTypes)]
        if self.limitSpec is not None:
            js["limitSpec"] = self.limitSpec.to_json()
        if self.having is not None:
            js["having"] = self.having.to_json()
        return _with_virtual_columns(_with_post_aggregations(js, self), self)


SEARCH_SPEC_TYPES = ("contains", "insensitive_contains", "fragment", "regex", "all")
SEARCH_SORTS = ("lexicographic", "alphanumeric", "numeric", "strlen")
SEARCH_STRATEGIES = ("useIndexes", "cursorOnly")
MAX_SEARCH_LIMIT = 1000  # SearchQueryConfig.maxSearchLimit (query/search/SearchQueryConfig.java)


@dataclass
class SearchQuery(BaseQuery):
    """SearchQuery (query/search/SearchQuery.java:52-73): which values of the search dimensions match
    the SearchQuerySpec, and in how many rows. ``searchDimensions``: names or default dimension specs
    (empty = every dimension of the segment, SearchStrategy.getDimsToSearch); ``query``: a
    SearchQuerySpec JSON (a bare string is the builder's insensitive_contains; None = all); ``sort``:
    the SearchSortSpec's StringComparator; ``limit``: 0 reads as 1000."""
    searchDimensions: List[Any] = field(default_factory=list)
    query: Any = None
    sort: Any = "lexicographic"
    limit: int = 1000

    def __post_init__(self):
        super().__post_init__()
        if self.aggregations:
            raise ValueError("a search query has no aggregations")
        dims = self.searchDimensions
        if dims is None:
            dims = []
        if isinstance(dims, (str, dict)):
            dims = [dims]
        specs = []
        for d in dims:
            if isinstance(d, dict):
                if d.get("extractionFn") is not None or d.get("type", "default") not in ("default",):
                    raise ValueError("extraction functions are out of scope")
                specs.append((d["dimension"], d.get("outputName") or d["dimension"]))
            else:
                specs.append((str(d), str(d)))
        self.dimension_specs: List[Tuple[str, str]] = specs
        self.searchDimensions = [d for d, _ in specs]
        q = self.query
        if q is None:
            q = {"type": "all"}
        elif isinstance(q, str):
            q = {"type": "insensitive_contains", "value": q}
        q = dict(q)
        if q.get("type") not in SEARCH_SPEC_TYPES:
            raise ValueError(f"unsupported search query spec {q.get('type')!r}")
        if q["type"] == "regex":
            _java_regex(q["pattern"])
        self.query = q
        self._spec = SearchQueryDimFilter("", q)
        self.sort = _ordering_name(self.sort.get("type") if isinstance(self.sort, dict) else self.sort)
        if self.sort not in SEARCH_SORTS:
            raise ValueError(f"unsupported search sort {self.sort!r}")
        self.limit = int(self.limit)
        if self.limit == 0:
            self.limit = 1000
        if self.limit < 0:
            raise ValueError("limit must be positive")
        st = self.context.get("searchStrategy", "useIndexes")
        if st not in SEARCH_STRATEGIES + ("auto",):
            raise ValueError(f"unknown searchStrategy {st!r}")

    def accept(self, value: Optional[str]) -> bool:
        """SearchQuerySpec.accept (query/search/*SearchQuerySpec.java)."""
        return self._spec.predicate(value)

    @property
    def strategy(self) -> str:
        """SearchStrategySelector.strategize: useIndexes (default) or cursorOnly. ``auto`` picks between
        them with a cost model (AutoStrategy.java) that is not restated here."""
        st = self.context.get("searchStrategy", "useIndexes")
        if st == "auto":
            from ._native import UnsupportedQuery
            raise UnsupportedQuery(2, "searchStrategy auto (its cost model is not restated)")
        return st

    def _dims_json(self):
        return [d if d == o else {"type": "default", "dimension": d, "outputName": o} for d, o in self.dimension_specs]

    def to_json(self):
        js = self._base_json("search")
        js.pop("aggregations", None)
        js.update({"searchDimensions": self._dims_json(), "query": dict(self.query), "sort": {"type": self.sort},
                   "limit": self.limit})
        return js


SCAN_RESULT_FORMATS = ("list", "compactedList")
SCAN_LEGACY_TIMESTAMP = "timestamp"  # ScanQueryEngine.LEGACY_TIMESTAMP_KEY
SCAN_TIME_COLUMN = "__time"


@dataclass
class ScanQuery(BaseQuery):
    """ScanQuery (query/scan/ScanQuery.java:53-77): the rows themselves. ``resultFormat`` list (default) or
    compactedList; ``batchSize`` 0 reads as 20480, ``limit`` 0 as unlimited (:70-71), negative values are
    IllegalArgumentExceptions (:72-73). Never descending (the constructor passes false, :67). ``legacy``
    None reads as ScanQueryConfig's default, false (withNonNullLegacy, :137-140)."""
    virtualColumns: Any = None
    resultFormat: Optional[str] = None
    batchSize: int = 0
    limit: int = 0
    columns: Optional[List[str]] = None
    legacy: Optional[bool] = None

    def __post_init__(self):
        super().__post_init__()
        if self.aggregations:
            raise ValueError("a scan query has no aggregations")
        if not self.granularity.is_all:
            raise ValueError("a scan query has no granularity (its cursor is at ALL, ScanQueryEngine.java:132)")
        if self.virtualColumns:
            from ._native import UnsupportedQuery
            raise UnsupportedQuery(2, "virtual columns are out of scope")
        self.virtualColumns = []
        self.resultFormat = "list" if self.resultFormat is None else str(self.resultFormat)
        if self.resultFormat == "valueVector":
            # the reference refuses it itself (ScanQueryEngine.java:186-188: UOE)
            from ._native import UnsupportedQuery
            raise UnsupportedQuery(2, "resultFormat[valueVector] is not supported")
        if self.resultFormat not in SCAN_RESULT_FORMATS:
            raise ValueError(f"resultFormat[{self.resultFormat}] is not supported")
        self.batchSize = int(self.batchSize or 0)
        self.limit = int(self.limit or 0)
        if self.batchSize == 0:
            self.batchSize = 4096 * 5
        if self.batchSize <= 0:
            raise ValueError("batchSize must be greater than 0")
        if self.limit < 0:
            raise ValueError("limit must be greater than 0")
        self.columns = [str(c) for c in (self.columns or [])]
        self.legacy = bool(self.legacy) if self.legacy is not None else False

    @property
    def row_limit(self) -> Optional[int]:
        """None = unlimited (limit 0 reads as Long.MAX_VALUE)."""
        return self.limit if self.limit > 0 else None

    def column_list(self, dimensions: Sequence[str], metrics: Sequence[str]) -> List[str]:
        """The result's column list for one segment (ScanQueryEngine.java:85-113): ``columns`` exactly
        (legacy: ``timestamp`` first when absent), or __time (legacy: ``timestamp``) followed by the
        segment's dimensions and metrics, without duplicates."""
        if self.columns:
            out = list(self.columns)
            if self.legacy and SCAN_LEGACY_TIMESTAMP not in out:
                out.insert(0, SCAN_LEGACY_TIMESTAMP)
            return out
        out = []
        for c in [SCAN_LEGACY_TIMESTAMP if self.legacy else SCAN_TIME_COLUMN, *dimensions, *metrics]:
            if c not in out:
                out.append(c)
        if self.legacy and SCAN_TIME_COLUMN in out:
            out.remove(SCAN_TIME_COLUMN)
        return out

    def to_json(self):
        js = self._base_json("scan")
        js.pop("aggregations", None)
        js.pop("granularity", None)
        js.update({"virtualColumns": [], "resultFormat": self.resultFormat, "batchSize": self.batchSize,
                   "limit": self.limit, "columns": list(self.columns), "legacy": self.legacy})
        return js


@dataclass
class ScanResultValue:
    """ScanResultValue (query/scan/ScanResultValue.java): one batch of one segment's rows. ``events``: a
    list of dicts (list) or of lists in ``columns`` order (compactedList)."""
    segmentId: str
    columns: List[str]
    events: List[Any]

    def to_json(self):
        return {"segmentId": self.segmentId, "columns": list(self.columns), "events": self.events}


def query_from_json(js: Dict[str, Any]):
    qt = js["queryType"]
    if qt == "scan":
        return ScanQuery(dataSource=js.get("dataSource", "ds"), intervals=js["intervals"], filter=js.get("filter"),
                         context=js.get("context", {}) or {}, virtualColumns=js.get("virtualColumns"),
                         resultFormat=js.get("resultFormat"), batchSize=int(js.get("batchSize", 0) or 0),
                         limit=int(js.get("limit", 0) or 0), columns=js.get("columns"), legacy=js.get("legacy"))
    common = dict(dataSource=js.get("dataSource", "ds"), intervals=js["intervals"],
                  granularity=js.get("granularity", "all"), filter=js.get("filter"),
                  aggregations=js.get("aggregations", []), context=js.get("context", {}) or {})
    post = js.get("postAggregations") or []
    virt = js.get("virtualColumns") or []
    if qt == "timeseries":
        return TimeseriesQuery(descending=bool(js.get("descending", False)), postAggregations=post,
                               virtualColumns=virt, **common)
    if qt == "topN":
        return TopNQuery(dimension=js["dimension"], metric=js["metric"], threshold=int(js["threshold"]),
                         postAggregations=post, virtualColumns=virt, **common)
    if qt == "groupBy":
        return GroupByQuery(dimensions=js.get("dimensions", []), limitSpec=js.get("limitSpec"),
                            having=js.get("having"), dimensionTypes=js.get("dimensionTypes"), postAggregations=post,
                            virtualColumns=virt, **common)
    if js.get("virtualColumns"):
        from ._native import UnsupportedQuery
        raise UnsupportedQuery(2, f"virtual columns on a {qt} query are out of scope")
    if qt == "search":
        return SearchQuery(searchDimensions=js.get("searchDimensions") or [], query=js.get("query"),
                           sort=js.get("sort") or "lexicographic", limit=int(js.get("limit", 0) or 0), **common)
    raise ValueError(f"unsupported queryType {qt!r}")


@dataclass
class Result:
    """Result<T> (query/Result.java): timestamp + value (dict for timeseries, list for topN)."""
    timestamp: int
    value: Any

    def to_json(self):
        return {"timestamp": format_time(self.timestamp), "result": self.value}


@dataclass
class Row:
    """groupBy MapBasedRow: timestamp + event."""
    timestamp: int
    event: Dict[str, Any]

    def to_json(self):
        return {"version": "v1", "timestamp": format_time(self.timestamp), "event": self.event}
