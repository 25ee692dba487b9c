// dg_expr.hip — the HIP kernel (gfx950 / CDNA4, wave64) that evaluates a numeric expression (dg_expr.h) over
// every row of one segment into a derived column: a flat LONG, DOUBLE or FLOAT column in HBM that every
// consumer then reads through the ordinary ColView (dg_segment_derive_column, dg_engine.cpp).
//
//   k_expr_eval   one row per lane, grid-stride over the rows        the inputs' bytes read + 8 B (FLOAT: 4 B)
//                                                                    written per row
//
// The operand stack is a lane-major LDS column st[slot][256 lanes] (32 KiB per workgroup; lane l of a wave
// touches word l of a slot's row: conflict-free), not a private array: one indexed by the stack pointer would
// live in scratch memory, and this kernel runs once per row of the segment. The program and the input views
// are kernel arguments, read with scalar loads by the uniform op loop. Each lane issues one 8-byte (4-byte)
// store, so a wave writes one contiguous span. The loop is bounded by the host-known row count and every
// load and store is guarded by it; poisoned rows are counted in LDS and added to the call's counter with one
// atomic per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"
#include "dg_expr.h"

namespace dg {

constexpr int kExT = 256;  // threads per workgroup

struct ExprLdsStack {
  uint64_t* col;  // this lane's word of slot 0; slot s is kExT words further
  __device__ __forceinline__ uint64_t get(int s) const { return col[s * kExT]; }
  __device__ __forceinline__ void set(int s, uint64_t v) { col[s * kExT] = v; }
};

template <int OUT>
__global__ __launch_bounds__(kExT) void k_expr_eval(ExprProg p, ExprInputs in, int64_t nrows, void* __restrict__ out,
                                                    unsigned long long* __restrict__ poisoned) {
  __shared__ uint64_t s_st[kExprMaxStack * kExT];
  __shared__ uint32_t s_poisoned;
  if (threadIdx.x == 0) s_poisoned = 0;
  __syncthreads();
  ExprLdsStack st{s_st + threadIdx.x};
  uint32_t mine = 0;
  for (int64_t base = (int64_t)blockIdx.x * kExT; base < nrows; base += (int64_t)gridDim.x * kExT) {
    const int64_t r = base + threadIdx.x;
    if (r >= nrows) continue;
    bool bad = false;
    uint64_t v = ex_eval(
        p, st,
        [&](int k) -> uint64_t {
          const uint8_t* q = cv_ptr(in.v[k], r);
          return in.v[k].kind == VIEW_FLOAT ? (uint64_t) * reinterpret_cast<const uint32_t*>(q)
                                            : *reinterpret_cast<const uint64_t*>(q);
        },
        &bad);
    if (bad) {
      v = 0;
      ++mine;
    }
    if (OUT == EX_COL_FLOAT) static_cast<uint32_t*>(out)[r] = (uint32_t)v;
    else static_cast<uint64_t*>(out)[r] = v;
  }
  if (mine) atomicAdd(&s_poisoned, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_poisoned) atomicAdd(poisoned, (unsigned long long)s_poisoned);
}

// workgroups: one per 256 rows up to four per compute unit (the LDS stacks of four fit a CU beside another
// stream's kernels); the CU count is the device's own
static unsigned expr_grid(int64_t nrows) {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!cus[dev]) {
    hipDeviceProp_t prop;
    cus[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 64;
  }
  const int64_t tiles = std::max<int64_t>((nrows + kExT - 1) / kExT, 1);
  return (unsigned)std::min<int64_t>(tiles, (int64_t)cus[dev] * 4);
}

void launch_expr_eval(const ExprProg& p, const ExprInputs& in, int64_t nrows, void* out, unsigned long long* poisoned,
                      hipStream_t s) {
  if (nrows <= 0) return;
  const dim3 g(expr_grid(nrows)), b(kExT);
  if (p.out_type == EX_COL_FLOAT) hipLaunchKernelGGL(k_expr_eval<EX_COL_FLOAT>, g, b, 0, s, p, in, nrows, out, poisoned);
  else hipLaunchKernelGGL(k_expr_eval<EX_COL_LONG>, g, b, 0, s, p, in, nrows, out, poisoned);
}

}  // namespace dg
