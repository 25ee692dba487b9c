// dg_expr.h — the numeric expression evaluator: one function for the device kernel (k_expr_eval) and for host
// C++, so the two cannot drift apart. No HIP include: a plain C++ compiler builds it too.
//
// A numeric expression (common/src/main/java/org/apache/druid/math/expr/) arrives as a postfix program over up
// to kExprMaxInputs stored columns of one segment, type-checked by the caller and again by ex_check: every
// value's type is static, long or double, so the stack holds raw 64-bit words. Null handling is
// replaceWithDefault only (a numeric column has no null there).
//   EX_INPUT arg          push input column `arg` as ExpressionSelectors.createBindings types it
//                         (ExpressionSelectors.java:66-93): a LONG column or __time pushes the long, a DOUBLE
//                         column the double, a FLOAT column its exactly widened float32
//   EX_CONST_L / _D imm   push the constant (LongExpr / DoubleExpr, Expr.java:71-140)
//   EX_L2D                (double) long (ExprEval.LongExprEval.asDouble)
//   EX_D2L                Java's (long) double: NaN -> 0, saturating (ExprEval.DoubleExprEval.asLong; JLS 5.1.3)
//   EX_D2F                (float) double, stored as float32 bits: only as the last op of a FLOAT output
//                         (ExpressionColumnValueSelector.getFloat)
//   EX_ADD SUB MUL DIV MOD   BinaryEvalOpExprBase.eval (Expr.java:358-401): long op long in wrapping 64-bit
//                         arithmetic, else both sides as doubles in IEEE arithmetic, % as fmod (:403-528).
//                         Long / and % follow Java: MIN / -1 = MIN, MIN % -1 = 0 (JLS 15.17.2-3); a zero
//                         divisor throws ArithmeticException there and POISONS the value here (below)
//   EX_NEG                UnaryMinusExpr (Expr.java:263-299): on a long (wrapping) or a double
//   EX_NOT                UnaryNotExpr (Expr.java:301-326): !Evals.asBoolean(x) (x > 0, Evals.java) in the
//                         operand's type
//   EX_LT LE GT GE        longs directly, doubles by Double.compare (Expr.java:530-636): NaN greatest, -0.0 < 0.0
//   EX_EQ EX_NE           longs directly, doubles by the primitive == / != (Expr.java:638-688): NaN != NaN,
//                         -0.0 == 0.0. Comparisons give 1 / 0 as a long for longs, 1.0 / 0.0 as a double otherwise
//   EX_AND EX_OR          selects, not booleans (Expr.java:690-720): asBoolean(l) ? r : l, and asBoolean(l) ? l : r
//   EX_SELECT             pops c, a, b: asBoolean(c) ? a : b (Function.ConditionFunc, Function.java:704-722;
//                         case_searched with an ELSE, :727-754, is a chain of them)
//   EX_ABS                Math.abs on a long (abs(MIN) = MIN) or a double (Function.Abs, :125-144)
//   EX_CEIL EX_FLOOR      on a double (SingleParamMath.eval(long) widens, Function.java:88-91)
//   EX_MIN EX_MAX         Math.min / Math.max on longs or doubles (Function.java:617-657): NaN wins, -0.0 < 0.0
//   EX_IDIV               Function.Div (:251-270): long / long (a zero divisor poisons), else (long)(x / y)
// Operands of a binary op, of EX_AND / EX_OR and the two branches of EX_SELECT have one type: the caller
// inserts EX_L2D where the reference's asDouble would convert, and refuses branches of different types
// (the reference does not promote them: the type would differ from row to row).
//
// Every NaN on the stack is the canonical one (Double.doubleToLongBits), so values compare bit for bit.
//
// Poison. The reference throws ArithmeticException for a long zero divisor only on rows its cursor visits and
// only in branches it evaluates: if(b != 0, a / b, 0) never throws. The device evaluates both branches, so
// the exception is a flag per stack entry (one bit each in a 32-bit word): an op ORs its operands' bits,
// EX_SELECT / EX_AND / EX_OR take the condition's bit and the CHOSEN branch's only. A row whose final value
// is poisoned stores 0 and is counted; the build that finds one registers nothing.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define DG_EX_HD __host__ __device__ inline
#else
#define DG_EX_HD inline
#endif

namespace dg {

enum {
  EX_INPUT = 0,
  EX_CONST_L = 1,
  EX_CONST_D = 2,
  EX_L2D = 3,
  EX_D2L = 4,
  EX_D2F = 5,
  EX_ADD = 6,
  EX_SUB = 7,
  EX_MUL = 8,
  EX_DIV = 9,
  EX_MOD = 10,
  EX_NEG = 11,
  EX_NOT = 12,
  EX_LT = 13,
  EX_LE = 14,
  EX_GT = 15,
  EX_GE = 16,
  EX_EQ = 17,
  EX_NE = 18,
  EX_AND = 19,
  EX_OR = 20,
  EX_SELECT = 21,
  EX_ABS = 22,
  EX_CEIL = 23,
  EX_FLOOR = 24,
  EX_MIN = 25,
  EX_MAX = 26,
  EX_IDIV = 27,
  EX_N_OPS = 28
};
// value type on the stack
enum { EX_T_LONG = 0, EX_T_DOUBLE = 1 };
// an input column's / the output's type: the values of DG_COL_LONG / DG_COL_FLOAT / DG_COL_DOUBLE
enum { EX_COL_LONG = 1, EX_COL_FLOAT = 2, EX_COL_DOUBLE = 3 };

constexpr int kExprMaxOps = 64;
constexpr int kExprMaxStack = 16;
constexpr int kExprMaxInputs = 8;
constexpr uint64_t kExNaN = 0x7ff8000000000000ull;
constexpr uint64_t kExSign = 0x8000000000000000ull;

// an op as the C-ABI hands it in (dg_expr_op)
struct ExOp {
  int32_t op;
  int32_t arg;
  uint64_t imm;
};

// A checked program in the form the evaluator runs (passed to the kernel by value).
struct ExprProg {
  int32_t n;
  int32_t n_inputs;
  int32_t out_type;                  // EX_COL_*
  int32_t pad;
  int8_t op[kExprMaxOps];            // EX_*
  int8_t ty[kExprMaxOps];            // the op's operand type (EX_T_*); EX_INPUT: the column's EX_COL_*
  int8_t arg[kExprMaxOps];           // EX_INPUT: the input
  uint64_t imm[kExprMaxOps];         // EX_CONST_*
};

DG_EX_HD double ex_as_double(uint64_t u) {
  union {
    uint64_t u;
    double d;
  } x;
  x.u = u;
  return x.d;
}
DG_EX_HD uint64_t ex_bits(double d) {  // Double.doubleToLongBits
  union {
    uint64_t u;
    double d;
  } x;
  x.d = d;
  return d != d ? kExNaN : x.u;
}
DG_EX_HD double ex_widen_float(uint32_t u) {
  union {
    uint32_t u;
    float f;
  } x;
  x.u = u;
  return (double)x.f;
}
DG_EX_HD uint32_t ex_float_bits(double d) {  // (float) d as float32 bits, NaN canonical
  union {
    uint32_t u;
    float f;
  } x;
  x.f = (float)d;
  return d != d ? 0x7fc00000u : x.u;
}
// Java's (long) double. The plain C++ cast is undefined out of range.
DG_EX_HD int64_t ex_d2l(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
// Double.compare as an unsigned key: NaN greatest, -0.0 < 0.0
DG_EX_HD uint64_t ex_double_key(uint64_t canonical_bits) {
  return (canonical_bits & kExSign) ? ~canonical_bits : (canonical_bits | kExSign);
}
// Evals.asBoolean of a stack word of type ty
DG_EX_HD bool ex_truth(int ty, uint64_t v) { return ty == EX_T_LONG ? (int64_t)v > 0 : ex_as_double(v) > 0.0; }

// Static check of a program over n_inputs input columns of types in_type[] (EX_COL_*) with output type
// out_type, and its checked form *out. Returns 0, or a negative code: -1 length, -2 unknown op, -3 input index or
// input type, -4 stack underflow, -5 stack overflow, -6 operand type, -7 does not end with exactly one value,
// -8 the result's type does not fit the output type, -9 EX_D2F anywhere but last in a FLOAT output,
// -10 input count, -11 output type.
inline int ex_check(const ExOp* ops, int n, const int32_t* in_type, int n_inputs, int out_type, ExprProg* out) {
  if (n < 1 || n > kExprMaxOps || !ops) return -1;
  if (n_inputs < 0 || n_inputs > kExprMaxInputs) return -10;
  if (out_type != EX_COL_LONG && out_type != EX_COL_FLOAT && out_type != EX_COL_DOUBLE) return -11;
  for (int k = 0; k < n_inputs; ++k)
    if (in_type[k] != EX_COL_LONG && in_type[k] != EX_COL_FLOAT && in_type[k] != EX_COL_DOUBLE) return -3;
  ExprProg p = {};
  p.n = n;
  p.n_inputs = n_inputs;
  p.out_type = out_type;
  int8_t ty[kExprMaxStack];
  int sp = 0;
  bool is_float = false;  // the top of the stack holds float32 bits (after EX_D2F)
  for (int i = 0; i < n; ++i) {
    const int op = ops[i].op;
    if (op < 0 || op >= EX_N_OPS) return -2;
    if (is_float) return -9;
    p.op[i] = (int8_t)op;
    p.imm[i] = ops[i].imm;
    switch (op) {
      case EX_INPUT:
        if (ops[i].arg < 0 || ops[i].arg >= n_inputs) return -3;
        if (sp == kExprMaxStack) return -5;
        p.arg[i] = (int8_t)ops[i].arg;
        p.ty[i] = (int8_t)in_type[ops[i].arg];
        ty[sp++] = in_type[ops[i].arg] == EX_COL_LONG ? EX_T_LONG : EX_T_DOUBLE;
        break;
      case EX_CONST_L:
      case EX_CONST_D:
        if (sp == kExprMaxStack) return -5;
        ty[sp++] = op == EX_CONST_L ? EX_T_LONG : EX_T_DOUBLE;
        break;
      case EX_L2D:
      case EX_D2L:
      case EX_D2F:
      case EX_CEIL:
      case EX_FLOOR:
        if (sp < 1) return -4;
        if (ty[sp - 1] != (op == EX_L2D ? EX_T_LONG : EX_T_DOUBLE)) return -6;
        if (op == EX_D2F) {
          if (i != n - 1 || out_type != EX_COL_FLOAT) return -9;
          is_float = true;
        }
        p.ty[i] = ty[sp - 1];
        if (op == EX_L2D) ty[sp - 1] = EX_T_DOUBLE;
        if (op == EX_D2L) ty[sp - 1] = EX_T_LONG;
        break;
      case EX_NEG:
      case EX_NOT:
      case EX_ABS:
        if (sp < 1) return -4;
        p.ty[i] = ty[sp - 1];
        break;
      case EX_SELECT:
        if (sp < 3) return -4;
        if (ty[sp - 1] != ty[sp - 2]) return -6;
        p.ty[i] = ty[sp - 3];  // the condition's type
        ty[sp - 3] = ty[sp - 1];
        sp -= 2;
        break;
      default:  // binary
        if (sp < 2) return -4;
        if (ty[sp - 1] != ty[sp - 2]) return -6;
        p.ty[i] = ty[sp - 1];
        --sp;
        if (op == EX_IDIV) ty[sp - 1] = EX_T_LONG;
        break;
    }
  }
  if (sp != 1) return -7;
  if (out_type == EX_COL_FLOAT ? !is_float : ty[0] != (out_type == EX_COL_LONG ? EX_T_LONG : EX_T_DOUBLE)) return -8;
  if (out) *out = p;
  return 0;
}

// Java's long / and %, the divisor not zero
DG_EX_HD int64_t ex_ldiv(int64_t a, int64_t b) { return b == -1 ? (int64_t)(0ull - (uint64_t)a) : a / b; }
DG_EX_HD int64_t ex_lmod(int64_t a, int64_t b) { return b == -1 ? 0 : a % b; }

// The value of a CHECKED program (ex_check) for one row. load(k) returns the row's raw value of input k (a
// float32 in the low 4 bytes); st.get(slot) / st.set(slot, word) is the operand stack (a plain array on the
// host, a lane-major LDS column on the device: a private array indexed by the stack pointer would live in
// scratch memory). *poisoned = the final value depends on a long division by zero. Each op is rounded on its
// own, as the reference's are: a * b + c is never contracted into an FMA, whatever the including translation
// unit's flags say (the pragma covers this function only).
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
template <class Stack, class Load>
DG_EX_HD uint64_t ex_eval(const ExprProg& p, Stack& st, Load load, bool* poisoned) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  uint32_t pz = 0;  // bit s: stack entry s is poisoned
  int sp = 0;
  for (int i = 0; i < p.n; ++i) {
    const int op = p.op[i];
    const int t = p.ty[i];
    if (op <= EX_CONST_D) {  // pushes
      uint64_t v;
      if (op == EX_INPUT) {
        const uint64_t raw = load((int)p.arg[i]);
        v = t == EX_COL_LONG ? raw : t == EX_COL_DOUBLE ? ex_bits(ex_as_double(raw)) : ex_bits(ex_widen_float((uint32_t)raw));
      } else {
        v = op == EX_CONST_L ? p.imm[i] : ex_bits(ex_as_double(p.imm[i]));
      }
      pz &= ~(1u << sp);
      st.set(sp++, v);
      continue;
    }
    if (op <= EX_D2F || op == EX_NEG || op == EX_NOT || (op >= EX_ABS && op <= EX_FLOOR)) {  // unary: the bit stays
      const uint64_t a = st.get(sp - 1);
      uint64_t r;
      switch (op) {
        case EX_L2D: r = ex_bits((double)(int64_t)a); break;
        case EX_D2L: r = (uint64_t)ex_d2l(ex_as_double(a)); break;
        case EX_D2F: r = (uint64_t)ex_float_bits(ex_as_double(a)); break;
        case EX_NEG: r = t == EX_T_LONG ? 0ull - a : ex_bits(-ex_as_double(a)); break;
        case EX_NOT: r = t == EX_T_LONG ? (uint64_t)!ex_truth(t, a) : ex_bits(ex_truth(t, a) ? 0.0 : 1.0); break;
        case EX_ABS: r = t == EX_T_LONG ? ((int64_t)a < 0 ? 0ull - a : a) : ex_bits(fabs(ex_as_double(a))); break;
        case EX_CEIL: r = ex_bits(ceil(ex_as_double(a))); break;
        default: r = ex_bits(floor(ex_as_double(a))); break;  // EX_FLOOR
      }
      st.set(sp - 1, r);
      continue;
    }
    if (op == EX_SELECT) {
      const uint64_t b = st.get(sp - 1), a = st.get(sp - 2), c = st.get(sp - 3);
      const bool take = ex_truth(t, c);
      const uint32_t pc = (pz >> (sp - 3)) & 1u, pa = (pz >> (sp - 2)) & 1u, pb = (pz >> (sp - 1)) & 1u;
      sp -= 2;
      st.set(sp - 1, take ? a : b);
      pz = (pz & ~(1u << (sp - 1))) | ((pc | (take ? pa : pb)) << (sp - 1));
      continue;
    }
    // binary
    const uint64_t b = st.get(sp - 1), a = st.get(sp - 2);
    const uint32_t pb = (pz >> (sp - 1)) & 1u, pa = (pz >> (sp - 2)) & 1u;
    --sp;
    uint64_t r = 0;
    uint32_t pr = pa | pb;
    if (op == EX_AND || op == EX_OR) {
      const bool l = ex_truth(t, a);
      const bool right = op == EX_AND ? l : !l;
      r = right ? b : a;
      pr = pa | (right ? pb : 0u);
    } else if (t == EX_T_LONG) {
      const int64_t x = (int64_t)a, y = (int64_t)b;
      switch (op) {
        case EX_ADD: r = a + b; break;
        case EX_SUB: r = a - b; break;
        case EX_MUL: r = a * b; break;
        case EX_DIV:
        case EX_IDIV:
          if (y == 0) pr = 1u;
          else r = (uint64_t)ex_ldiv(x, y);
          break;
        case EX_MOD:
          if (y == 0) pr = 1u;
          else r = (uint64_t)ex_lmod(x, y);
          break;
        case EX_LT: r = x < y; break;
        case EX_LE: r = x <= y; break;
        case EX_GT: r = x > y; break;
        case EX_GE: r = x >= y; break;
        case EX_EQ: r = x == y; break;
        case EX_NE: r = x != y; break;
        case EX_MIN: r = (uint64_t)(x < y ? x : y); break;
        default: r = (uint64_t)(x > y ? x : y); break;  // EX_MAX
      }
    } else {
      const double x = ex_as_double(a), y = ex_as_double(b);
      const uint64_t ka = ex_double_key(a), kb = ex_double_key(b);  // (the stack's NaNs are canonical)
      switch (op) {
        case EX_ADD: r = ex_bits(x + y); break;
        case EX_SUB: r = ex_bits(x - y); break;
        case EX_MUL: r = ex_bits(x * y); break;
        case EX_DIV: r = ex_bits(x / y); break;
        case EX_MOD: r = ex_bits(fmod(x, y)); break;
        case EX_IDIV: r = (uint64_t)ex_d2l(x / y); break;
        case EX_LT: r = ex_bits(ka < kb ? 1.0 : 0.0); break;
        case EX_LE: r = ex_bits(ka <= kb ? 1.0 : 0.0); break;
        case EX_GT: r = ex_bits(ka > kb ? 1.0 : 0.0); break;
        case EX_GE: r = ex_bits(ka >= kb ? 1.0 : 0.0); break;
        case EX_EQ: r = ex_bits(x == y ? 1.0 : 0.0); break;
        case EX_NE: r = ex_bits(x != y ? 1.0 : 0.0); break;
        // Math.min / Math.max: a NaN operand wins (its key is the greatest: for min it is picked by hand)
        case EX_MIN: r = (x != x || y != y) ? kExNaN : (ka < kb ? a : b); break;
        default: r = ka > kb ? a : b; break;  // EX_MAX
      }
    }
    st.set(sp - 1, r);
    pz = (pz & ~(1u << (sp - 1))) | (pr << (sp - 1));
  }
  *poisoned = (pz & 1u) != 0;
  return st.get(0);
}
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

// the host's operand stack
struct ExprHostStack {
  uint64_t w[kExprMaxStack];
  uint64_t get(int s) const { return w[s]; }
  void set(int s, uint64_t v) { w[s] = v; }
};

}  // namespace dg
