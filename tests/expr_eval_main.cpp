// expr_eval_main.cpp — a stand-alone driver of csrc/dg_expr.h for tests/test_expr.py, built with the system
// compiler and -fsanitize=undefined: the header is the one the device kernel compiles, so what the sanitizer
// and the comparison with the Python values establish here holds for the host side of k_expr_eval's evaluator.
//
// stdin, one case per line: out_type n_inputs n_ops, then n_inputs x (column type, the row's raw value in
// hex), then n_ops x (op, arg, imm in hex).
// stdout, one line per case: ex_check's code, the value's word in hex (0 when the checker refused), 1 when the
// value is poisoned.
#include <stdio.h>

#include <vector>

#include "dg_expr.h"

int main() {
  int out_type, n_in, n_ops;
  while (scanf("%d %d %d", &out_type, &n_in, &n_ops) == 3) {
    if (n_in < 0 || n_in > 64 || n_ops < 0 || n_ops > 1024) return 2;
    std::vector<int32_t> types((size_t)n_in + 1);
    std::vector<uint64_t> words((size_t)n_in + 1);
    for (int k = 0; k < n_in; ++k) {
      unsigned long long w;
      if (scanf("%d %llx", &types[k], &w) != 2) return 2;
      words[k] = w;
    }
    std::vector<dg::ExOp> ops((size_t)n_ops + 1);
    for (int i = 0; i < n_ops; ++i) {
      unsigned long long imm;
      if (scanf("%d %d %llx", &ops[i].op, &ops[i].arg, &imm) != 3) return 2;
      ops[i].imm = imm;
    }
    dg::ExprProg prog;
    const int rc = dg::ex_check(ops.data(), n_ops, types.data(), n_in, out_type, &prog);
    uint64_t v = 0;
    bool poisoned = false;
    if (rc == 0) {
      dg::ExprHostStack st;
      v = dg::ex_eval(prog, st, [&](int k) { return words[(size_t)k]; }, &poisoned);
      if (poisoned) v = 0;  // (what k_expr_eval stores for such a row)
    }
    printf("%d %llx %d\n", rc, (unsigned long long)v, poisoned ? 1 : 0);
  }
  return 0;
}
