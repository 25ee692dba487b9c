// dg_filter_plan.cpp — filter planning on the host, once per call: the filter's strings under Java's rules
// (dg_javatext.h) against the segment's dictionaries (BitmapIndexSelector semantics). Nothing here touches the
// device; the engine's build_bitset turns the finished FilterPlan into launches.
#include "dg_filter_plan.h"

#include <algorithm>

#include "dg_javatext.h"

namespace dg {

// dictionary search (GenericIndexed.indexOf, GenericIndexed.java:308-333)
int index_of(const DictColumn* c, const char* value) {
  const bool vnull = value == nullptr || value[0] == 0;  // NullHandling.emptyToNullIfNeeded
  const std::string v = vnull ? std::string() : std::string(value);
  int lo = 0, hi = (int)c->dict.size() - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    int r = cmp_nullable(c->dict_null[mid], c->dict[mid], vnull, v);
    if (r == 0) return mid;
    if (r < 0) lo = mid + 1;
    else hi = mid - 1;
  }
  return -(lo + 1);
}

// BoundFilter.doesMatch (BoundFilter.java:249-275), default null mode
static bool bound_matches(const dg_filter& f, const char* value /* NULL = null */) {
  const bool has_lower = f.lower != nullptr, has_upper = f.upper != nullptr;
  if (!value) {
    const bool lower_null = !has_lower || f.lower[0] == 0;
    const bool upper_null = !has_upper || f.upper[0] == 0;
    return (!has_lower || (lower_null && !f.lower_strict)) && (!has_upper || !upper_null || !f.upper_strict);
  }
  auto cmp = [&](const char* x, const char* y) {
    if (f.ordering == DG_ORDER_NUMERIC) return numeric_compare(x, y);
    return cmp_nullable(x == nullptr, x ? x : "", y == nullptr, y ? y : "");
  };
  const int lc = has_lower ? cmp(value, f.lower) : 1;
  const int uc = has_upper ? cmp(f.upper, value) : 1;
  if (f.lower_strict && f.upper_strict) return lc > 0 && uc > 0;
  if (f.lower_strict) return lc > 0 && uc >= 0;
  if (f.upper_strict) return lc >= 0 && uc > 0;
  return lc >= 0 && uc >= 0;
}

static bool leaf_matches_null(const dg_filter& f) {
  if (f.kind == DG_F_SELECTOR) return f.n_values < 1 || !f.values || !f.values[0] || !f.values[0][0];
  if (f.kind == DG_F_IN) {
    for (int i = 0; i < f.n_values; ++i)
      if (!f.values[i] || !f.values[i][0]) return true;
    return false;
  }
  return bound_matches(f, nullptr);
}

// The row predicate of a selector / in / bound filter on a numeric column, as the reference builds
// its ValueMatcher. Default null mode: a numeric row is never null, so null-matching predicates
// (nullValueMatcher) select nothing.
static int plan_numeric_leaf(const dg_filter& f, const DictColumn* c, PredLeaf* L) {
  memset(&L->p, 0, sizeof L->p);
  L->col = c;
  NumPred& p = L->p;
  p.kind = PRED_FALSE;
  const bool is_long = c->type == DG_COL_LONG, is_float = c->type == DG_COL_FLOAT;
  auto add_value = [&](const char* v) {  // one selector / IN value
    if (!v || !*v) return;  // emptyToNullIfNeeded -> null: no numeric row matches
    if (is_long) {
      long long x;
      if (exact_long(v, &x)) L->set.push_back(x);
    } else if (is_float) {
      float x;
      if (guava_try_parse_float(v, &x)) L->set.push_back(float_bits(x));
    } else {
      double x;
      if (guava_try_parse_double(v, &x)) L->set.push_back(double_bits(x));
    }
  };
  if (f.kind == DG_F_SELECTOR || f.kind == DG_F_IN) {
    // SelectorFilter -> {Long,Float,Double}ValueMatcherColumnSelectorStrategy.makeValueMatcher(value)
    // (convertObjectToLong = getExactLongFromDecimalString, Floats/Doubles.tryParse + *ToIntBits);
    // InFilter -> InDimFilter.get{Long,Float,Double}PredicateSupplier (the same parsing, a set)
    const int nv = f.kind == DG_F_SELECTOR ? std::min(f.n_values, 1) : f.n_values;
    for (int k = 0; k < nv; ++k) add_value(f.values ? f.values[k] : nullptr);
    std::sort(L->set.begin(), L->set.end());
    L->set.erase(std::unique(L->set.begin(), L->set.end()), L->set.end());
    if (!L->set.empty()) p.kind = is_long ? PRED_LONG_SET : PRED_BITS_SET;
    return DG_OK;
  }
  // BoundFilter: NUMERIC ordering -> BoundDimFilter.{long,float,double}PredicateSupplier
  // (BoundDimFilter.java:341-652); other orderings compare String.valueOf(value) (BoundFilter
  // makeLongPredicate etc.: doesMatch) — for long columns under LEXICOGRAPHIC (UTF-8 bytes)
  // the bounds are kept as given (BoundDimFilter.java:73-76; hasLowerBound = lower != null): "" is a
  // bound, unparseable as a number
  const char* lo = f.lower;
  const char* hi = f.upper;
  p.lo_strict = f.lower_strict;
  p.hi_strict = f.upper_strict;
  if (f.ordering != DG_ORDER_NUMERIC) {
    if (!is_long || f.ordering != DG_ORDER_LEXICOGRAPHIC)
      return set_error(DG_ERR_UNSUPPORTED, "bound ordering %d on numeric column %s (String.valueOf formatting)",
                       f.ordering, c->name.c_str());
    p.kind = PRED_LONG_LEX;
    p.has_lo = lo != nullptr;
    p.has_hi = hi != nullptr;
    L->lo = lo ? lo : "";
    L->hi = hi ? hi : "";
    return DG_OK;
  }
  if (is_long) {
    bool nothing = false;
    long long lv = 0, hv = 0;
    if (lo) {
      if (guava_try_parse_long(lo, &lv)) {
        p.has_lo = 1;
      } else {
        Decimal d;
        if (!parse_big_decimal(lo, &d)) {
          p.has_lo = 0;  // unparseable: below every number
        } else {
          const int r = decimal_to_long(d, f.lower_strict ? 1 : 2, &lv);
          if (r == 1) p.has_lo = 1;
          else if (r == 2) nothing = true;  // positive lower bound above every long
        }
      }
    }
    if (hi) {
      if (guava_try_parse_long(hi, &hv)) {
        p.has_hi = 1;
      } else {
        Decimal d;
        if (!parse_big_decimal(hi, &d)) {
          nothing = true;  // unparseable upper bound: below every number
        } else {
          const int r = decimal_to_long(d, f.upper_strict ? 2 : 1, &hv);
          if (r == 1) p.has_hi = 1;
          else if (r == -2) nothing = true;
        }
      }
    }
    p.kind = nothing ? PRED_FALSE : PRED_LONG_RANGE;
    p.lo = lv;
    p.hi = hv;
    return DG_OK;
  }
  bool nothing = false;
  double lv = 0, hv = 0;
  if (lo) {
    if (is_float) {
      float x;
      p.has_lo = guava_try_parse_float(lo, &x);
      lv = x;
    } else {
      p.has_lo = guava_try_parse_double(lo, &lv);
    }
  }
  if (hi) {
    bool ok;
    if (is_float) {
      float x;
      ok = guava_try_parse_float(hi, &x);
      hv = x;
    } else {
      ok = guava_try_parse_double(hi, &hv);
    }
    p.has_hi = ok;
    nothing = !ok;
  }
  p.kind = nothing ? PRED_FALSE : PRED_ORD_RANGE;
  p.lo = (int64_t)dcmp_key(lv);
  p.hi = (int64_t)dcmp_key(hv);
  return DG_OK;
}

static int plan_node(ColumnLookup find, const void* seg, const dg_filter* nodes, int n, int* pos, FilterPlan* fp) {
  if (*pos >= n) return set_error(DG_ERR_ARG, "truncated filter");
  const dg_filter& f = nodes[(*pos)++];
  switch (f.kind) {
    case DG_F_AND:
    case DG_F_OR: {
      if (f.n_children < 1) return set_error(DG_ERR_ARG, "empty and/or filter");
      for (int c = 0; c < f.n_children; ++c) {
        int rc = plan_node(find, seg, nodes, n, pos, fp);
        if (rc) return rc;
        if (c > 0) fp->prog.push_back(f.kind == DG_F_AND ? -3 : -4);
      }
      return DG_OK;
    }
    case DG_F_NOT: {
      int rc = plan_node(find, seg, nodes, n, pos, fp);
      if (rc) return rc;
      fp->prog.push_back(-5);
      return DG_OK;
    }
    case DG_F_SELECTOR:
    case DG_F_IN:
    case DG_F_BOUND: {
      if (!f.dimension) return set_error(DG_ERR_ARG, "filter without dimension");
      const DictColumn* c = find(seg, f.dimension);
      if (!c) {
        // missing column: allTrue iff the filter matches null (ColumnSelectorBitmapIndexSelector.java:212-218)
        fp->prog.push_back(leaf_matches_null(f) ? -1 : -2);
        return DG_OK;
      }
      if (c->type == DG_COL_LONG || c->type == DG_COL_FLOAT || c->type == DG_COL_DOUBLE) {
        // no bitmap index: a row post-filter (QueryableIndexStorageAdapter.java:244-260, FilteredOffset)
        PredLeaf L;
        int rc = plan_numeric_leaf(f, c, &L);
        if (rc) return rc;
        if (L.p.kind == PRED_FALSE) {
          fp->prog.push_back(-2);
          return DG_OK;
        }
        fp->prog.push_back((int32_t)fp->leaf_ids.size());
        fp->leaf_ids.emplace_back();
        fp->leaf_col.push_back(nullptr);
        fp->leaf_pred.push_back((int32_t)fp->preds.size());
        fp->preds.push_back(std::move(L));
        return DG_OK;
      }
      if (c->type != DG_COL_STRING)
        return set_error(DG_ERR_UNSUPPORTED, "filter on %s needs a bitmap index", f.dimension);
      std::vector<int32_t> ids;
      if (f.kind == DG_F_SELECTOR) {
        int i = index_of(c, f.n_values > 0 && f.values ? f.values[0] : nullptr);
        if (i >= 0) ids.push_back(i);
      } else if (f.kind == DG_F_IN) {
        for (int k = 0; k < f.n_values; ++k) {
          int i = index_of(c, f.values[k]);
          if (i >= 0) ids.push_back(i);
        }
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      } else if (f.ordering == DG_ORDER_LEXICOGRAPHIC) {
        // BoundFilter.getStartEndIndexes (BoundFilter.java:141-174)
        const int card = (int)c->dict.size();
        int start, end;
        if (!f.lower) start = 0;
        else {
          int found = index_of(c, f.lower);
          start = found >= 0 ? (f.lower_strict ? found + 1 : found) : -(found + 1);
        }
        if (!f.upper) end = card;
        else {
          int found = index_of(c, f.upper);
          end = found >= 0 ? (f.upper_strict ? found : found + 1) : -(found + 1);
        }
        if (end < start) end = start;
        for (int i = start; i < end; ++i) ids.push_back(i);
      } else if (f.ordering == DG_ORDER_NUMERIC) {
        // predicate over every dictionary value (Filters.matchPredicate, Filters.java:239-290)
        for (int i = 0; i < (int)c->dict.size(); ++i)
          if (bound_matches(f, c->dict_null[i] ? nullptr : c->dict[i].c_str())) ids.push_back(i);
      } else {
        return set_error(DG_ERR_UNSUPPORTED, "bound ordering %d", f.ordering);
      }
      if (ids.empty()) {
        fp->prog.push_back(-2);
        return DG_OK;
      }
      if (!c->has_bitmaps) {
        // no bitmap index (an in-memory segment): the matching ids become a row predicate, as
        // IncrementalIndexStorageAdapter's cursors evaluate filter.makeMatcher per row
        PredLeaf L;
        memset(&L.p, 0, sizeof L.p);
        L.p.kind = PRED_ID_SET;
        L.col = c;
        L.set.assign((c->dict.size() + 63) / 64, 0);
        for (int32_t i : ids) L.set[i >> 6] |= (int64_t)(1ull << (i & 63));
        L.p.has_lo = c->multi_value && !c->dict.empty() && c->dict_null[0] && !ids.empty() && ids[0] == 0;
        fp->prog.push_back((int32_t)fp->leaf_ids.size());
        fp->leaf_ids.emplace_back();
        fp->leaf_col.push_back(nullptr);
        fp->leaf_pred.push_back((int32_t)fp->preds.size());
        fp->preds.push_back(std::move(L));
        return DG_OK;
      }
      fp->prog.push_back((int32_t)fp->leaf_ids.size());
      fp->leaf_ids.push_back(std::move(ids));
      fp->leaf_col.push_back(c);
      fp->leaf_pred.push_back(-1);
      return DG_OK;
    }
    default:
      return set_error(DG_ERR_ARG, "unknown filter kind %d", f.kind);
  }
}

int plan_filter(ColumnLookup find, const void* segment, const dg_filter* nodes, int n, FilterPlan* fp) {
  int pos = 0;
  int rc = plan_node(find, segment, nodes, n, &pos, fp);
  if (rc) return rc;
  if (pos != n) return set_error(DG_ERR_ARG, "filter has %d trailing nodes", n - pos);
  if (fp->prog.size() > 64) return set_error(DG_ERR_UNSUPPORTED, "filter program too long");
  // stack depth check (kernel stack of 16)
  int depth = 0, maxd = 0;
  for (int op : fp->prog) {
    if (op >= -2) depth++;
    else if (op != -5) depth--;
    maxd = std::max(maxd, depth);
  }
  if (maxd > 16) return set_error(DG_ERR_UNSUPPORTED, "filter nesting too deep");
  return DG_OK;
}

}  // namespace dg
