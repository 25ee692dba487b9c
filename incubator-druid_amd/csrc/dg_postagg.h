// dg_postagg.h — the post-aggregator evaluator: one function for the device kernels (k_post_eval) and for host
// C++, so the two cannot drift apart. No HIP include: a plain C++ compiler builds it too.
//
// A post-aggregator (query/aggregation/post/*.java) arrives as a postfix program over one cell's aggregator
// slots, type-checked by the caller: every op's operand types are static, so the stack holds raw 64-bit words.
//   PA_AGG arg            push aggregator slot `arg`: a long kind pushes the int64, a double kind the double, a
//                         float kind the exactly widened float32 (Number.doubleValue of a Float)
//   PA_CONST_D / _L imm   push the constant (ConstantPostAggregator.java)
//   PA_L2D                (double) long, round to nearest even (Number.doubleValue of a Long)
//   PA_D2L                Java's (long) double: NaN -> 0, saturating (Number.longValue of a Double; JLS 5.1.3)
//   PA_ADD PA_SUB PA_MUL  IEEE fp64, rounded after each op (ArithmeticPostAggregator.java:206-228)
//   PA_DIV                rhs == 0.0 ? 0.0 : lhs / rhs (:229-235; -0.0 is zero, a NaN rhs is not)
//   PA_QUOT               lhs / rhs (:236-242)
//   PA_DMAX PA_DMIN       Double.compare(b, a) > 0 ? b : a, < 0 for DMIN (DoubleGreatestPostAggregator.java:77-92,
//                         DoubleLeastPostAggregator): NaN greatest, -0.0 < 0.0
//   PA_LMAX PA_LMIN       Long.compare (LongGreatestPostAggregator.java:76-93, LongLeastPostAggregator)
// Every NaN on the stack is the canonical one (Double.doubleToLongBits: Java cannot tell NaNs apart, and the
// payload an fp64 unit gives 0.0 / 0.0 differs between processors), so values compare bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DG_PA_HD __host__ __device__ inline
#else
#define DG_PA_HD inline
#endif

namespace dg {

enum {
  PA_AGG = 0,
  PA_CONST_D = 1,
  PA_CONST_L = 2,
  PA_L2D = 3,
  PA_D2L = 4,
  PA_ADD = 5,
  PA_SUB = 6,
  PA_MUL = 7,
  PA_DIV = 8,
  PA_QUOT = 9,
  PA_DMAX = 10,
  PA_DMIN = 11,
  PA_LMAX = 12,
  PA_LMIN = 13,
  PA_N_OPS = 14
};
// the comparator of a program's top-level post-aggregator
enum { PA_ORDER_NONE = 0, PA_ORDER_DOUBLE = 1, PA_ORDER_LONG = 2, PA_ORDER_NUMERIC_FIRST = 3 };
// what a slot holds (PA_AGG; the engine derives it from the aggregator's kind)
enum { PA_SLOT_LONG = 0, PA_SLOT_DOUBLE = 1, PA_SLOT_FLOAT = 2 };
// value type on the stack (the checker)
enum { PA_T_LONG = 0, PA_T_DOUBLE = 1 };

constexpr int kPostAggMaxOps = 64;
constexpr int kPostAggMaxStack = 16;
constexpr uint64_t kPaNaN = 0x7ff8000000000000ull;
constexpr uint64_t kPaSign = 0x8000000000000000ull;

// A checked program in the form the evaluator runs (passed to kernels by value).
struct PostAggProg {
  int32_t n;
  int32_t order;                      // PA_ORDER_*
  int8_t op[kPostAggMaxOps];          // PA_*
  int8_t cls[kPostAggMaxOps];         // PA_AGG: PA_SLOT_*
  int16_t arg[kPostAggMaxOps];        // PA_AGG: the slot
  uint64_t imm[kPostAggMaxOps];       // PA_CONST_*
};

DG_PA_HD double pa_as_double(uint64_t u) {
  union {
    uint64_t u;
    double d;
  } x;
  x.u = u;
  return x.d;
}
DG_PA_HD uint64_t pa_bits(double d) {  // Double.doubleToLongBits
  union {
    uint64_t u;
    double d;
  } x;
  x.d = d;
  return d != d ? kPaNaN : x.u;
}
DG_PA_HD double pa_widen_float(uint32_t u) {
  union {
    uint32_t u;
    float f;
  } x;
  x.u = u;
  return (double)x.f;
}
// Java's (long) double. The plain C++ cast is undefined out of range.
DG_PA_HD int64_t pa_d2l(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
// Double.compare as an unsigned key: NaN greatest, -0.0 < 0.0
DG_PA_HD uint64_t pa_double_key(double d) {
  if (d != d) return ~0ull;
  const uint64_t u = pa_bits(d);
  return (u & kPaSign) ? ~u : (u | kPaSign);
}
// The order key of a program's value under its order kind: comparator order = unsigned key order.
//   DOUBLE         Double.compareTo
//   LONG           Long.compare
//   NUMERIC_FIRST  ArithmeticPostAggregator.Ordering.numericFirst (:277-299): -inf < +inf < NaN < every finite
//                  value (a finite double's key is at least 2^52)
//   NONE           ConstantPostAggregator's always-equal comparator: one key
DG_PA_HD uint64_t pa_order_key(int order, uint64_t v) {
  switch (order) {
    case PA_ORDER_LONG: return v ^ kPaSign;
    case PA_ORDER_DOUBLE: return pa_double_key(pa_as_double(v));
    case PA_ORDER_NUMERIC_FIRST: {
      const double d = pa_as_double(v);
      if (d != d) return 2;
      if (d == -__builtin_inf()) return 0;
      if (d == __builtin_inf()) return 1;
      return pa_double_key(d);
    }
    default: return 0;
  }
}

// Static check of a program over n_slots slots: stack discipline, ops, slot indices, operand types. Returns 0 and
// the result's type (PA_T_*), or a negative code: -1 length, -2 unknown op, -3 slot index, -4 stack underflow,
// -5 stack overflow, -6 operand type, -7 does not end with exactly one value, -8 order kind does not fit the type.
// slot_cls[s] = PA_SLOT_* of slot s, or -1 for a slot a program may not read.
inline int pa_check(const PostAggProg& p, const int8_t* slot_cls, int n_slots, int* out_type) {
  if (p.n < 1 || p.n > kPostAggMaxOps) return -1;
  int8_t ty[kPostAggMaxStack];
  int sp = 0;
  for (int i = 0; i < p.n; ++i) {
    const int op = p.op[i];
    if (op < 0 || op >= PA_N_OPS) return -2;
    if (op == PA_AGG || op == PA_CONST_D || op == PA_CONST_L) {
      if (op == PA_AGG && (p.arg[i] < 0 || p.arg[i] >= n_slots || slot_cls[p.arg[i]] < 0)) return -3;
      if (sp == kPostAggMaxStack) return -5;
      ty[sp++] = op == PA_CONST_L || (op == PA_AGG && slot_cls[p.arg[i]] == PA_SLOT_LONG) ? PA_T_LONG : PA_T_DOUBLE;
    } else if (op == PA_L2D || op == PA_D2L) {
      if (sp < 1) return -4;
      if (ty[sp - 1] != (op == PA_L2D ? PA_T_LONG : PA_T_DOUBLE)) return -6;
      ty[sp - 1] = op == PA_L2D ? PA_T_DOUBLE : PA_T_LONG;
    } else {
      if (sp < 2) return -4;
      const int want = op == PA_LMAX || op == PA_LMIN ? PA_T_LONG : PA_T_DOUBLE;
      if (ty[sp - 1] != want || ty[sp - 2] != want) return -6;
      --sp;
    }
  }
  if (sp != 1) return -7;
  if (p.order < PA_ORDER_NONE || p.order > PA_ORDER_NUMERIC_FIRST) return -8;
  if (p.order == PA_ORDER_LONG && ty[0] != PA_T_LONG) return -8;
  if ((p.order == PA_ORDER_DOUBLE || p.order == PA_ORDER_NUMERIC_FIRST) && ty[0] != PA_T_DOUBLE) return -8;
  if (out_type) *out_type = ty[0];
  return 0;
}

// The value of a CHECKED program (pa_check) for one cell; load(slot) returns the cell's ABI-encoded slot.
// Each op is rounded on its own, as the reference's are: a * b + c is never contracted into an FMA, whatever
// the including translation unit's flags say (the pragma covers this function only).
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
template <class Load>
DG_PA_HD uint64_t pa_eval(const PostAggProg& p, Load load) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  uint64_t st[kPostAggMaxStack];
  int sp = 0;
  for (int i = 0; i < p.n; ++i) {
    const int op = p.op[i];
    switch (op) {
      case PA_AGG: {
        const uint64_t v = load((int)p.arg[i]);
        st[sp++] = p.cls[i] == PA_SLOT_LONG     ? v
                   : p.cls[i] == PA_SLOT_DOUBLE ? pa_bits(pa_as_double(v))
                                                : pa_bits(pa_widen_float((uint32_t)v));
        break;
      }
      case PA_CONST_D: st[sp++] = pa_bits(pa_as_double(p.imm[i])); break;
      case PA_CONST_L: st[sp++] = p.imm[i]; break;
      case PA_L2D: st[sp - 1] = pa_bits((double)(int64_t)st[sp - 1]); break;
      case PA_D2L: st[sp - 1] = (uint64_t)pa_d2l(pa_as_double(st[sp - 1])); break;
      case PA_LMAX:
      case PA_LMIN: {
        const int64_t b = (int64_t)st[--sp], a = (int64_t)st[sp - 1];
        st[sp - 1] = (uint64_t)((op == PA_LMAX ? b > a : b < a) ? b : a);
        break;
      }
      case PA_DMAX:
      case PA_DMIN: {
        const uint64_t b = st[--sp], a = st[sp - 1];
        const uint64_t kb = pa_double_key(pa_as_double(b)), ka = pa_double_key(pa_as_double(a));
        st[sp - 1] = (op == PA_DMAX ? kb > ka : kb < ka) ? b : a;
        break;
      }
      default: {
        const double rhs = pa_as_double(st[--sp]), lhs = pa_as_double(st[sp - 1]);
        double r;
        if (op == PA_ADD) r = lhs + rhs;
        else if (op == PA_SUB) r = lhs - rhs;
        else if (op == PA_MUL) r = lhs * rhs;
        else if (op == PA_DIV) r = rhs == 0.0 ? 0.0 : lhs / rhs;
        else r = lhs / rhs;
        st[sp - 1] = pa_bits(r);
        break;
      }
    }
  }
  return st[0];
}
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

}  // namespace dg
