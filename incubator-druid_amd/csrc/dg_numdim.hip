// dg_numdim.hip — HIP kernels (gfx950 / CDNA4, wave64) of the numeric-dimension encoding: a LONG, FLOAT
// or DOUBLE column becomes what a dictionary-encoded string column is, a sorted value list (nd_vals) plus
// one id per row (nd_ids), so the groupBy (LONG) and the topN (all three) run over it as over any
// dimension (the reference keys such a dimension by the long itself, Float.floatToIntBits or
// Double.doubleToLongBits: LongGroupByColumnSelectorStrategy, GroupByQueryEngineV2.java:235-260;
// NumericTopNColumnSelectorStrategy.java:81-151). Built once per (segment, column) by the first groupBy
// or topN over the column (Column::nd_*, dg_engine.cpp build_num_dim).
//
// A row's value is its signed 64-bit key (nd_value): the long itself, or for a float / double the
// canonical bits b (every NaN -> 0x7fc00000 / 0x7ff8000000000000, as floatToIntBits / doubleToLongBits
// give) folded to b ^ ((b >> 31 or 63) & 0x7fff…), widened to int64. Ascending keys are Float.compare /
// Double.compare order (-0.0 < 0.0, NaN greatest), equal keys are equal bits, and the fold is its own
// inverse, so nd_vals holds keys and the export folds them back.
//
//   k_nd_minmax        the column's smallest and largest value                      8 B read per row
//   k_nd_words         word[r] = (uint64)(v[r] - min): the sort's keys              8 B read + 8 B written
//   (launch_radix_sort over bits_for(max - min) key bits, dg_sort.hip)
//   k_nd_unique_count  run heads of the sorted words per tile of kSortTile          8 B read
//   k_nd_scan          tile counts -> exclusive offsets, their total = cardinality  (one workgroup)
//   k_nd_unique_emit   nd_vals[k] = word of the k-th run head + min                 8 B read, 8 B per value written
//   k_nd_encode        nd_ids[r] = lower bound of v[r] in nd_vals                   8 B read + 4 B written,
//                                                                                   log2(card) value-list probes
//
// Every kernel is a plain HBM-bound integer pass; nothing waits on another workgroup, every loop is
// bounded by a length the host passes (rows, tiles, cardinality) and every store is guarded by it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"

namespace dg {

constexpr int kNdT = 256;                   // threads per workgroup
constexpr int kNdPer = kSortTile / kNdT;    // elements per thread of a tile
static_assert(kNdPer * kNdT == kSortTile, "whole tiles");

template <int KIND>
__device__ __forceinline__ int64_t nd_value(const ColView& v, int64_t r) {
  const uint8_t* p = cv_ptr(v, r);
  if (KIND == VIEW_FLOAT) {
    const float x = *reinterpret_cast<const float*>(p);
    const int32_t b = x != x ? 0x7fc00000 : __float_as_int(x);
    return (int64_t)(b ^ ((b >> 31) & 0x7fffffff));
  }
  if (KIND == VIEW_DOUBLE) {
    const double x = *reinterpret_cast<const double*>(p);
    const int64_t b = x != x ? 0x7ff8000000000000ll : (int64_t)__double_as_longlong(x);
    return b ^ ((b >> 63) & 0x7fffffffffffffffll);
  }
  return *reinterpret_cast<const int64_t*>(p);
}

// mm[0] = min, mm[1] = max over the rows, as order-preserving unsigned keys (value ^ sign); the host
// initialises mm to {~0, 0}. One atomic pair per workgroup.
template <int KIND>
__global__ __launch_bounds__(kNdT) void k_nd_minmax(ColView v, int64_t nrows, unsigned long long* __restrict__ mm) {
  __shared__ uint64_t s_lo[kNdT / 64], s_hi[kNdT / 64];
  uint64_t lo = ~0ull, hi = 0ull;
  for (int64_t r = (int64_t)blockIdx.x * kNdT + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kNdT) {
    const uint64_t k = (uint64_t)nd_value<KIND>(v, r) ^ kSign;
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNdT / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    if (lo <= hi) {  // (a workgroup with no rows holds the identities)
      atomicMin(&mm[0], (unsigned long long)lo);
      atomicMax(&mm[1], (unsigned long long)hi);
    }
  }
}

// The subtraction wraps in 64 bits and is exact for every range (Long.MIN_VALUE .. Long.MAX_VALUE gives
// words 0 .. 2^64 - 1): the words order like the values (keys).
template <int KIND>
__global__ __launch_bounds__(kNdT) void k_nd_words(ColView v, int64_t nrows, int64_t vmin, uint64_t* __restrict__ words) {
  for (int64_t r = (int64_t)blockIdx.x * kNdT + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kNdT)
    words[r] = (uint64_t)nd_value<KIND>(v, r) - (uint64_t)vmin;
}

// A head is a word that differs from its predecessor; a tile's first word is compared with the last word
// of the tile before it, read from memory (element 0 is a head).
__device__ __forceinline__ uint32_t nd_head(const uint64_t* __restrict__ w, int64_t i) {
  return (i == 0 || w[i] != w[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(kNdT) void k_nd_unique_count(const uint64_t* __restrict__ w, int64_t n,
                                                          uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_tmp[kNdT / 64];
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  uint32_t c = 0;
#pragma unroll 4
  for (int q = 0; q < kNdPer; ++q) {
    const int64_t i = base + q * kNdT + threadIdx.x;
    if (i < n) c += nd_head(w, i);
  }
  uint32_t total;
  block_scan_u32<kNdT>(c, &total, s_tmp);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// cnt[0 .. ntiles) -> exclusive offsets in place, info[0] = their sum (one workgroup; ntiles = rows / 4096)
__global__ __launch_bounds__(kNdT) void k_nd_scan(uint32_t* __restrict__ cnt, int64_t ntiles,
                                                  unsigned long long* __restrict__ info) {
  __shared__ uint32_t s_tmp[kNdT / 64];
  uint64_t carry = 0;
  for (int64_t base = 0; base < ntiles; base += kNdT) {
    const int64_t i = base + threadIdx.x;
    const uint32_t c = i < ntiles ? cnt[i] : 0u;
    uint32_t total;
    const uint32_t x = block_scan_u32<kNdT>(c, &total, s_tmp);
    if (i < ntiles) cnt[i] = (uint32_t)(carry + x);
    carry += total;
  }
  if (threadIdx.x == 0) info[0] = carry;
}

// vals[k] = the k-th distinct value, ascending; k < card (the total k_nd_scan found) guards the store
__global__ __launch_bounds__(kNdT) void k_nd_unique_emit(const uint64_t* __restrict__ w, int64_t n,
                                                         const uint32_t* __restrict__ tile_off, int64_t vmin,
                                                         int64_t* __restrict__ vals, int64_t card) {
  __shared__ uint32_t s_tmp[kNdT / 64];
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  int64_t k0 = tile_off[blockIdx.x];
  for (int q = 0; q < kNdPer; ++q) {  // (the trip count and the barriers inside are uniform)
    const int64_t i = base + q * kNdT + threadIdx.x;
    const uint32_t h = i < n ? nd_head(w, i) : 0u;
    uint32_t total;
    const uint32_t x = block_scan_u32<kNdT>(h, &total, s_tmp);
    const int64_t k = k0 + x;
    if (h && k < card) vals[k] = (int64_t)(w[i] + (uint64_t)vmin);
    k0 += total;
  }
}

// ids[r] = index of v[r] in vals (every row's value is in the list: the lower bound is its position)
template <int KIND>
__global__ __launch_bounds__(kNdT) void k_nd_encode(ColView v, int64_t nrows, const int64_t* __restrict__ vals,
                                                    uint32_t card, uint32_t* __restrict__ ids) {
  for (int64_t r = (int64_t)blockIdx.x * kNdT + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kNdT) {
    const int64_t x = nd_value<KIND>(v, r);
    uint32_t lo = 0, len = card;
    while (len > 0) {
      const uint32_t h = len >> 1;
      if (vals[lo + h] < x) {
        lo += h + 1;
        len -= h + 1;
      } else {
        len = h;
      }
    }
    ids[r] = lo < card ? lo : card - 1u;
  }
}

static unsigned nd_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + kNdT - 1) / kNdT, 1), 2048); }

void launch_nd_minmax(const ColView& v, int64_t nrows, unsigned long long* mm, hipStream_t s) {
  if (nrows <= 0) return;
  const dim3 g(nd_grid(nrows)), b(kNdT);
  if (v.kind == VIEW_FLOAT) hipLaunchKernelGGL(k_nd_minmax<VIEW_FLOAT>, g, b, 0, s, v, nrows, mm);
  else if (v.kind == VIEW_DOUBLE) hipLaunchKernelGGL(k_nd_minmax<VIEW_DOUBLE>, g, b, 0, s, v, nrows, mm);
  else hipLaunchKernelGGL(k_nd_minmax<VIEW_LONG>, g, b, 0, s, v, nrows, mm);
}

void launch_nd_words(const ColView& v, int64_t nrows, int64_t vmin, uint64_t* words, hipStream_t s) {
  if (nrows <= 0) return;
  const dim3 g(nd_grid(nrows)), b(kNdT);
  if (v.kind == VIEW_FLOAT) hipLaunchKernelGGL(k_nd_words<VIEW_FLOAT>, g, b, 0, s, v, nrows, vmin, words);
  else if (v.kind == VIEW_DOUBLE) hipLaunchKernelGGL(k_nd_words<VIEW_DOUBLE>, g, b, 0, s, v, nrows, vmin, words);
  else hipLaunchKernelGGL(k_nd_words<VIEW_LONG>, g, b, 0, s, v, nrows, vmin, words);
}

void launch_nd_unique_count(const uint64_t* words, int64_t n, uint32_t* tile_cnt, unsigned long long* info, hipStream_t s) {
  if (n <= 0) return;
  const int nt = sort_tiles(n);
  hipLaunchKernelGGL(k_nd_unique_count, dim3(nt), dim3(kNdT), 0, s, words, n, tile_cnt);
  hipLaunchKernelGGL(k_nd_scan, dim3(1), dim3(kNdT), 0, s, tile_cnt, (int64_t)nt, info);
}

void launch_nd_unique_emit(const uint64_t* words, int64_t n, const uint32_t* tile_off, int64_t vmin, int64_t* vals,
                           int64_t card, hipStream_t s) {
  if (n <= 0 || card <= 0) return;
  hipLaunchKernelGGL(k_nd_unique_emit, dim3(sort_tiles(n)), dim3(kNdT), 0, s, words, n, tile_off, vmin, vals, card);
}

void launch_nd_encode(const ColView& v, int64_t nrows, const int64_t* vals, uint32_t card, uint32_t* ids, hipStream_t s) {
  if (nrows <= 0 || card == 0) return;
  const dim3 g(nd_grid(nrows)), b(kNdT);
  if (v.kind == VIEW_FLOAT) hipLaunchKernelGGL(k_nd_encode<VIEW_FLOAT>, g, b, 0, s, v, nrows, vals, card, ids);
  else if (v.kind == VIEW_DOUBLE) hipLaunchKernelGGL(k_nd_encode<VIEW_DOUBLE>, g, b, 0, s, v, nrows, vals, card, ids);
  else hipLaunchKernelGGL(k_nd_encode<VIEW_LONG>, g, b, 0, s, v, nrows, vals, card, ids);
}

}  // namespace dg
