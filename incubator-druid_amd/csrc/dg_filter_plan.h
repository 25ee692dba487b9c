// dg_filter_plan.h — filter planning (dg_filter_plan.cpp): a filter's prefix nodes resolved against a segment's
// dictionaries into a postfix program over leaf bitsets, and the row predicate of a leaf without a bitmap index,
// one evaluator for the device kernel (k_num_pred) and for host C++. No HIP include: a plain C++ compiler builds
// it too (tests/filter_plan_main.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/druidgpu.h"

#if defined(__HIPCC__)
#define DG_FP_HD __host__ __device__ inline
#else
#define DG_FP_HD inline
#endif

namespace dg {

// Row predicate of a filter on a numeric column: the reference evaluates it per row as a post-filter
// (QueryableIndexStorageAdapter.makeCursors :244-260 -> FilteredOffset.java:40-105) through the
// column's ValueMatcher ({Long,Float,Double}ValueMatcherColumnSelectorStrategy, the filters'
// DruidLong/Float/DoublePredicate); here it becomes one more row bitset of the filter program.
enum PredKind : int32_t {
  PRED_FALSE = 0,       // matches no row (unparseable selector value, empty IN, ALWAYS_FALSE bounds)
  PRED_LONG_RANGE = 1,  // long column: [lo, hi] with strictness (makeLongPredicateFromBounds)
  PRED_LONG_SET = 2,    // long column: value in the sorted set (IN / selector)
  PRED_ORD_RANGE = 3,   // float/double column: Double.compare range on (double) value, as ordered keys
  PRED_BITS_SET = 4,    // float/double column: floatToIntBits / doubleToLongBits in the sorted set
  PRED_LONG_LEX = 5,    // long column: String.valueOf(value) vs UTF-8 bound strings (LEXICOGRAPHIC)
  PRED_ID_SET = 6,      // string column without a bitmap index: row id's bit in `set` (64-bit words)
};
struct NumPred {
  int32_t kind;
  int32_t has_lo, has_hi, lo_strict, hi_strict;
  int32_t nset;
  int64_t lo, hi;         // LONG_RANGE: bounds; ORD_RANGE: ordered keys (uint64 bit patterns)
  const int64_t* set;     // LONG_SET / BITS_SET: sorted values / canonical bit patterns
  const uint8_t* lo_str;  // LONG_LEX: bound bytes
  const uint8_t* hi_str;
  int32_t lo_len, hi_len;
};

// ------------------------------------------------------------------------------------------------
// the row predicate on an already loaded value (FilteredOffset + ValueMatcher, see NumPred)
// ------------------------------------------------------------------------------------------------
DG_FP_HD int64_t float_bits(float f) {  // Float.floatToIntBits
  if (f != f) return 0x7fc00000ll;
  uint32_t u;
  memcpy(&u, &f, 4);
  return (int64_t)u;
}

DG_FP_HD int64_t double_bits(double d) {  // Double.doubleToLongBits
  if (d != d) return 0x7ff8000000000000ll;
  int64_t u;
  memcpy(&u, &d, 8);
  return u;
}

// Double.compare order as unsigned keys: -0.0 < 0.0, every NaN equal and greatest
DG_FP_HD uint64_t dcmp_key(double d) {
  if (d != d) return ~0ull;
  uint64_t u;
  memcpy(&u, &d, 8);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

DG_FP_HD bool in_sorted(const int64_t* set, int n, int64_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (set[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && set[lo] == x;
}

// UnsignedBytes.lexicographicalComparator of String.valueOf(x) (ASCII) against a UTF-8 string
DG_FP_HD int lex_cmp_long(int64_t x, const uint8_t* b, int blen) {
  char buf[20];
  int n = 0;
  uint64_t u = x < 0 ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
  do {
    buf[n++] = (char)('0' + (int)(u % 10));
    u /= 10;
  } while (u);
  const int len = n + (x < 0 ? 1 : 0);
  for (int i = 0; i < len && i < blen; ++i) {
    const int c = x < 0 ? (i == 0 ? '-' : buf[n - i]) : buf[n - 1 - i];
    if (c != b[i]) return c < (int)b[i] ? -1 : 1;
  }
  return (len > blen) - (len < blen);
}

DG_FP_HD bool range_ok(int lc, int uc, const NumPred& p) {
  // lc = compare(value, lower), uc = compare(upper, value)
  const bool lok = !p.has_lo || (p.lo_strict ? lc > 0 : lc >= 0);
  const bool uok = !p.has_hi || (p.hi_strict ? uc > 0 : uc >= 0);
  return lok && uok;
}

// PRED_ID_SET: whether dictionary id `id` is in the set
DG_FP_HD bool pred_has_id(const NumPred& p, uint32_t id) { return ((uint64_t)p.set[id >> 6] >> (id & 63)) & 1ull; }

// a long column's value
DG_FP_HD bool pred_long(const NumPred& p, int64_t x) {
  if (p.kind == PRED_LONG_RANGE) return range_ok((x > p.lo) - (x < p.lo), (p.hi > x) - (p.hi < x), p);
  if (p.kind == PRED_LONG_SET) return in_sorted(p.set, p.nset, x);
  if (p.kind == PRED_LONG_LEX) {
    const int lc = p.has_lo ? lex_cmp_long(x, p.lo_str, p.lo_len) : 1;
    const int uc = p.has_hi ? -lex_cmp_long(x, p.hi_str, p.hi_len) : 1;
    return range_ok(lc, uc, p);
  }
  return false;
}

// a float or double column's value: its canonical bits (float_bits / double_bits) and the value as a double
DG_FP_HD bool pred_fp(const NumPred& p, int64_t bits, double d) {
  if (p.kind == PRED_BITS_SET) return in_sorted(p.set, p.nset, bits);
  if (p.kind == PRED_ORD_RANGE) {
    const uint64_t k = dcmp_key(d), klo = (uint64_t)p.lo, khi = (uint64_t)p.hi;
    return range_ok((k > klo) - (k < klo), (khi > k) - (khi < k), p);
  }
  return false;
}

// ------------------------------------------------------------------------------------------------
// filter planning: prefix nodes -> postfix program over leaf bitsets
// ------------------------------------------------------------------------------------------------
// What the planner reads of a column (the engine's Column derives from it).
struct DictColumn {
  std::string name;
  int type = DG_COL_MISSING;
  // dictionary-encoded string column
  std::vector<std::string> dict;
  std::vector<uint8_t> dict_null;      // 1 = null / empty value
  bool has_bitmaps = false;
  bool multi_value = false;            // a row holds a list of ids (an empty one: the null value)
};

struct PredLeaf {
  NumPred p;
  std::vector<int64_t> set;
  std::string lo, hi;
  const DictColumn* col;
};

// prog: a leaf's index (>= 0), -1 = every row, -2 = no row, -3 / -4 / -5 = AND / OR / NOT
struct FilterPlan {
  std::vector<int32_t> prog;
  std::vector<std::vector<int32_t>> leaf_ids;  // dictionary ids whose bitmaps are OR-ed
  std::vector<const DictColumn*> leaf_col;     // null: a row-predicate leaf (leaf_pred)
  std::vector<int32_t> leaf_pred;              // index into preds, -1 for bitmap leaves
  std::vector<PredLeaf> preds;
};

// error reporting: defined by whoever links the planner (the engine: dg_engine.cpp)
int set_error(int code, const char* fmt, ...);

// GenericIndexed.indexOf over the column's dictionary: the id, or -(insertion point) - 1
int index_of(const DictColumn* c, const char* value);

// the column of a segment by name, null when the segment has none
typedef const DictColumn* (*ColumnLookup)(const void* segment, const char* name);

// Plans the n nodes of a filter into *fp (empty on entry), within the filter kernel's limits.
int plan_filter(ColumnLookup find, const void* segment, const dg_filter* nodes, int n, FilterPlan* fp);

}  // namespace dg
