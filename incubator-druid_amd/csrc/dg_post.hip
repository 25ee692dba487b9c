// dg_post.hip — HIP kernels (gfx950 / CDNA4, wave64) of the groupBy post-processing step
// (dg_result_post_process): GroupByQuery.postProcess = the having spec, then DefaultLimitSpec.build
// (query/groupby/orderby/DefaultLimitSpec.java:122-290) over a result resident in HBM.
//
//   k_post_having     having tree (the HavingSpec classes of query/groupby/having) as a postfix program over each
//                     group's slots -> selection bitset, one ballot per 64 groups (as k_num_pred)
//   k_post_eval       post-aggregator programs (dg_postagg.h) over each group's slots -> value columns
//   k_post_sort_word  one 64-bit word of the comparator chain (makeComparator :190-260) per element,
//                     read through the element's group reference
//
// Both are HBM-bound integer kernels: one group per lane, neighbouring lanes hold neighbouring groups
// of the slot-major [1 + n_aggs][cap] records, so every slot read of the having pass and of the first
// (identity / survivor referenced) word load is a contiguous span per wave. Later words of a multi-word
// order are loaded through the permuted references (a gather). Every loop is bounded by a count the
// host knows (n) or by the survivor count clamped to it; every index is checked against n first.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"

namespace dg {

// The aggregator's own comparator as an unsigned key over its ABI-encoded slot: Long.compare for long
// outputs, Doubles.compare (every NaN equal and greatest, -0.0 < 0.0) for double outputs, the same over
// the exactly widened float32 of float outputs (HavingSpecMetricComparator.java:36-80 compares doubles
// the same way; DefaultLimitSpec.metricOrdering uses AggregatorFactory.getComparator).
// A post column (kind = kPostColKind + its order kind) compares under the program's order kind.
__device__ __forceinline__ uint64_t post_order_key(int kind, uint64_t v) {
  if (kind >= kPostColKind) return pa_order_key(kind - kPostColKind, v);
  switch (kind) {
    case DG_AGG_COUNT:
    case DG_AGG_LONG_SUM:
    case DG_AGG_LONG_MIN:
    case DG_AGG_LONG_MAX: return v ^ kSign;
    case DG_AGG_DOUBLE_SUM:
    case DG_AGG_DOUBLE_MIN:
    case DG_AGG_DOUBLE_MAX: {
      const double d = __longlong_as_double((long long)v);
      return d != d ? ~0ull : ord_key(d);
    }
    default: {
      const float f = __uint_as_float((uint32_t)v);
      return f != f ? ~0ull : ord_key((double)f);
    }
  }
}

// a float output's key in 32 bits: the same fold over the float32 itself (monotone in the widened double)
__device__ __forceinline__ uint32_t post_order_key32(uint64_t v) {
  const uint32_t u = (uint32_t)v;
  const float f = __uint_as_float(u);
  if (f != f) return ~0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_post_having(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ slots,
                                                     int64_t cap, int64_t n, PostHaving p, const uint64_t* __restrict__ post,
                                                     uint32_t* __restrict__ sel) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t g = base + threadIdx.x;
    const bool live = g < n;
    uint64_t st = 0;  // the operand stack, top in bit 0 (depth <= kPostMaxStack, checked by the host)
    for (int i = 0; i < p.n; ++i) {  // (p is uniform: every lane takes the same branch)
      const int op = p.op[i];
      if (op == DG_HAVING_ALWAYS || op == DG_HAVING_NEVER) {
        st = (st << 1) | (op == DG_HAVING_ALWAYS ? 1ull : 0ull);
      } else if (op == DG_HAVING_NOT) {
        st ^= 1ull;
      } else if (op == DG_HAVING_AND || op == DG_HAVING_OR) {
        const int k = p.arg[i];
        const uint64_t m = (1ull << k) - 1ull;
        const uint64_t v = op == DG_HAVING_AND ? (st & m) == m : (st & m) != 0;
        st = ((st >> k) << 1) | v;
      } else if (op == DG_HAVING_AGG_RANGE) {
        uint64_t v = 0;
        if (live) {
          const uint64_t* col = p.kind[i] >= kPostColKind ? post : slots;  // (arg: the column / the slot row)
          const uint64_t k = post_order_key(p.kind[i], col[(size_t)p.arg[i] * cap + g]);
          v = k >= p.lo[i] && k <= p.hi[i];
        }
        st = (st << 1) | v;
      } else {  // DG_HAVING_DIM_EQ
        uint64_t v = 0;
        if (live) v = ((keys[g] >> p.arg[i]) & ((1ull << p.kind[i]) - 1ull)) == p.lo[i];
        st = (st << 1) | v;
      }
    }
    const uint64_t b = __ballot(live && (st & 1ull));
    const int64_t w = (g - lane) >> 5;  // first word of this wave's 64 groups
    if (g - lane < n) {
      if (lane == 0) sel[w] = (uint32_t)b;
      if (lane == 32 && live) sel[w + 1] = (uint32_t)(b >> 32);
    }
  }
}

void launch_post_having(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t n, const PostHaving& p,
                        const uint64_t* post, uint32_t* sel, hipStream_t s) {
  if (n <= 0) return;
  const int64_t blocks = std::min<int64_t>(16384, (n + 255) / 256);
  hipLaunchKernelGGL(k_post_having, dim3((unsigned)blocks), dim3(256), 0, s, keys, slots, cap, n, p, post, sel);
}

__global__ __launch_bounds__(256) void k_post_sort_word(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ slots,
                                                        int64_t cap, int64_t n, const unsigned long long* __restrict__ info,
                                                        const uint32_t* __restrict__ refs_in, PostWord w,
                                                        const uint64_t* __restrict__ post,
                                                        uint64_t* __restrict__ kout, uint32_t* __restrict__ refs_out,
                                                        uint32_t* __restrict__ n_out) {
  int64_t count = n;
  if (info) count = std::min<int64_t>((int64_t)info[1], n);
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) n_out[0] = (uint32_t)count;
  for (int64_t i = t; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t g = refs_in ? (int64_t)refs_in[i] : i;
    if (g >= n) g = n - 1;  // (references are group numbers below n; never read past the result)
    uint64_t word = 0, key = 0;
    bool have_key = false;
    for (int f = 0; f < w.nfields; ++f) {
      const PostField& pf = w.f[f];
      const uint64_t m = pf.bits >= 64 ? ~0ull : (1ull << pf.bits) - 1ull;
      uint64_t v;
      if (pf.type == POST_F_KEY) {
        if (!have_key) {
          key = keys[g];
          have_key = true;
        }
        v = (key >> pf.in_shift) & m;
        if (pf.rank) v = (uint64_t)(uint32_t)pf.rank[v];
      } else if (pf.type == POST_F_AGG64) {
        const uint64_t* col = pf.kind >= kPostColKind ? post : slots;  // (slot: the column / the slot row)
        v = post_order_key(pf.kind, col[(size_t)pf.slot * cap + g]);
      } else {
        v = (uint64_t)post_order_key32(slots[(size_t)pf.slot * cap + g]);
      }
      if (pf.desc) v = m - v;
      word |= v << pf.out_shift;
    }
    kout[i] = word;
    if (refs_out) refs_out[i] = (uint32_t)g;
  }
}

void launch_post_sort_word(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t n,
                           const unsigned long long* info, const uint32_t* refs_in, const PostWord& w,
                           const uint64_t* post, uint64_t* kout, uint32_t* refs_out, uint32_t* n_out, hipStream_t s) {
  const int64_t blocks = std::min<int64_t>(16384, std::max<int64_t>(1, (n + 255) / 256));
  hipLaunchKernelGGL(k_post_sort_word, dim3((unsigned)blocks), dim3(256), 0, s, keys, slots, cap, n, info, refs_in, w, post,
                     kout, refs_out, n_out);
}

// Post-aggregator columns of a resident result (dg_result_post_aggregate): one group per lane, neighbouring
// lanes hold neighbouring groups, so every slot read and the column store are contiguous per wave. The
// programs are uniform across lanes (no divergence); the operand stack is per lane. The grid-stride loop is
// bounded by n, and only groups below n are read or written (cap >= n).
__global__ __launch_bounds__(256) void k_post_eval(const uint64_t* __restrict__ slots, int64_t cap, int64_t n,
                                                   const PostAggProg* __restrict__ progs, int ncols,
                                                   uint64_t* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
    for (int c = 0; c < ncols; ++c) {
      const uint64_t v = pa_eval(progs[c], [&](int slot) { return slots[(size_t)(1 + slot) * cap + g]; });
      out[(size_t)c * cap + g] = v;
    }
  }
}

void launch_post_eval(const uint64_t* slots, int64_t cap, int64_t n, const PostAggProg* d_progs, int ncols, uint64_t* out,
                      hipStream_t s) {
  if (n <= 0 || ncols <= 0) return;
  const int64_t blocks = std::min<int64_t>(16384, (n + 255) / 256);
  hipLaunchKernelGGL(k_post_eval, dim3((unsigned)blocks), dim3(256), 0, s, slots, cap, n, d_progs, ncols, out);
}

}  // namespace dg
