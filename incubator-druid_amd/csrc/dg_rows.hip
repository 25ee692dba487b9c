// dg_rows.hip — HIP kernels (gfx950 / CDNA4, wave64) of the scan query (dg_rows_run): the raw-row
// counterpart of the aggregating engines (query/scan/ScanQueryEngine.java:59-264: one ascending cursor
// over filter AND interval, every selected row's column values, at most `limit` rows).
//
//   k_rows_count    set bits of each tile of the selection bitset            the cursor's offset (the rows the
//   k_rows_scan     tile counts -> exclusive offsets, total, keep            filter and the interval select, in
//   k_rows_emit     the first `keep` selected rows as ascending u32 numbers  row order), cut at the limit (:125,:170)
//   k_rows_gather   kept rows x fixed-width columns -> contiguous outputs    getColumnValue (:238-250) over the
//   k_rows_mv_len   value-list lengths of the kept rows, summed per tile     column selectors; a multi-value row is
//   k_rows_mv_copy  kept rows' value lists -> offsets + concatenated ids     its id list (DimensionSelector.java:167-182)
//
// The compaction is a count / scan / emit triple over tiles of kRowsTileWords bitset words (one word
// per thread): nothing waits on another workgroup, every loop is bounded by a length the host knows
// (nrows, keep capacity, tile counts). Bits at or past nrows in the last word are masked off; a rank at
// or past `keep` writes nothing, so the row list never holds more than its capacity.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"

namespace dg {

// word w of the selection restricted to rows below nrows (w < ceil(nrows / 32))
__device__ __forceinline__ uint32_t rows_word(const uint32_t* __restrict__ S, int64_t w, int64_t nrows) {
  const int64_t nwords = (nrows + 31) >> 5;
  if (w >= nwords) return 0u;
  uint32_t v = S[w];
  if (w == nwords - 1 && (nrows & 31)) v &= (1u << (nrows & 31)) - 1u;
  return v;
}

__global__ __launch_bounds__(kRowsTileWords) void k_rows_count(const uint32_t* __restrict__ S, int64_t nrows,
                                                                uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_tmp[kRowsTileWords / 64];
  const int64_t w = (int64_t)blockIdx.x * kRowsTileWords + threadIdx.x;
  uint32_t total;
  block_scan_u32<kRowsTileWords>(__popc(rows_word(S, w, nrows)), &total, s_tmp);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// cnt[0 .. n) -> exclusive offsets in place; info[0] = their sum, info[1] = min(sum, cap). One workgroup:
// n is a tile count (rows / 8192, or kept rows / 256), so the loop is short.
__global__ __launch_bounds__(256) void k_rows_scan(uint32_t* __restrict__ cnt, int64_t n, uint64_t cap,
                                                   unsigned long long* __restrict__ info) {
  __shared__ uint32_t s_tmp[4];
  uint64_t carry = 0;
  for (int64_t base = 0; base < n; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < n ? cnt[i] : 0u;
    uint32_t total;
    const uint32_t x = block_scan_u32<256>(v, &total, s_tmp);
    if (i < n) cnt[i] = (uint32_t)(carry + x);
    carry += total;
  }
  if (threadIdx.x == 0) {
    info[0] = carry;
    info[1] = carry < cap ? carry : cap;
  }
}

// rows[rank] = row number of the rank-th selected row, for rank < keep = info[1]; info[2] / info[3] = the
// first / last kept row (the block range the gather decodes)
__global__ __launch_bounds__(kRowsTileWords) void k_rows_emit(const uint32_t* __restrict__ S, int64_t nrows,
                                                               const uint32_t* __restrict__ tile_off,
                                                               unsigned long long* __restrict__ info,
                                                               uint32_t* __restrict__ rows) {
  __shared__ uint32_t s_tmp[kRowsTileWords / 64];
  const uint64_t keep = info[1];
  const uint64_t base = tile_off[blockIdx.x];
  if (base >= keep) return;  // (uniform over the workgroup: before any barrier)
  const int64_t w = (int64_t)blockIdx.x * kRowsTileWords + threadIdx.x;
  uint32_t bits = rows_word(S, w, nrows);
  uint32_t total;
  uint64_t rank = base + block_scan_u32<kRowsTileWords>(__popc(bits), &total, s_tmp);
  while (bits && rank < keep) {
    const int b = __ffs(bits) - 1;
    bits &= bits - 1;
    const uint32_t row = (uint32_t)(w * 32 + b);
    rows[rank] = row;
    if (rank == 0) info[2] = row;
    if (rank == keep - 1) info[3] = row;
    ++rank;
  }
}

void launch_rows_select(const uint32_t* S, int64_t nrows, uint64_t cap, uint32_t* tile_cnt, unsigned long long* info,
                        uint32_t* rows, hipStream_t s) {
  if (nrows <= 0) return;
  const int64_t nwords = (nrows + 31) / 32;
  const unsigned ntiles = (unsigned)((nwords + kRowsTileWords - 1) / kRowsTileWords);
  hipLaunchKernelGGL(k_rows_count, dim3(ntiles), dim3(kRowsTileWords), 0, s, S, nrows, tile_cnt);
  hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(256), 0, s, tile_cnt, (int64_t)ntiles, cap, info);
  hipLaunchKernelGGL(k_rows_emit, dim3(ntiles), dim3(kRowsTileWords), 0, s, S, nrows, tile_cnt, info, rows);
}

// ------------------------------------------------------------------------------------------------
// Gather: workgroup (x, y) takes kept rows x * 256 .. of table entry y. Neighbouring lanes hold
// neighbouring kept rows of ONE column: the row numbers ascend, so a wave's loads walk one block of the
// column forwards (one contiguous span when the selection is dense, ascending 64-byte segments when it
// is sparse) and its stores are one contiguous span of the column's output.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_gather(const RowsCol* __restrict__ cols, const uint32_t* __restrict__ rows,
                                                     int64_t keep) {
  const RowsCol c = cols[blockIdx.y];
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < keep; k += (int64_t)gridDim.x * 256) {
    const int64_t r = rows ? (int64_t)rows[k] : k;
    if (c.v.kind == VIEW_IDS) {
      reinterpret_cast<int32_t*>(c.out)[k] = (int32_t)load_id(c.v, r);
    } else if (c.v.width == 8) {
      reinterpret_cast<uint64_t*>(c.out)[k] = *reinterpret_cast<const uint64_t*>(cv_ptr(c.v, r));
    } else {
      reinterpret_cast<uint32_t*>(c.out)[k] = *reinterpret_cast<const uint32_t*>(cv_ptr(c.v, r));
    }
  }
}

void launch_rows_gather(const RowsCol* d_cols, int ncols, const uint32_t* rows, int64_t keep, hipStream_t s) {
  if (ncols <= 0 || keep <= 0) return;
  const unsigned gx = (unsigned)std::min<int64_t>((keep + 255) / 256, 65536);
  hipLaunchKernelGGL(k_rows_gather, dim3(gx, (unsigned)ncols), dim3(256), 0, s, d_cols, rows, keep);
}

// ------------------------------------------------------------------------------------------------
// Multi-value columns: kept row k's list is vals[offs[r] .. offs[r + 1]) (r its row number). The offsets
// were validated by the call's k_mv_check; they are still clamped to the values stored.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mv_span(const RowsMv& m, int64_t k, uint32_t* b, uint32_t* len) {
  const int64_t r = m.rows ? (int64_t)m.rows[k] : k;
  uint32_t lo = load_id(m.offs, r), hi = load_id(m.offs, r + 1);
  if (hi > (uint64_t)m.nvals) hi = (uint32_t)m.nvals;
  if (lo > hi) lo = hi;
  *b = lo;
  *len = hi - lo;
}

__global__ __launch_bounds__(256) void k_rows_mv_len(RowsMv m) {
  __shared__ uint32_t s_tmp[4];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t b = 0, len = 0;
  if (k < m.keep) mv_span(m, k, &b, &len);
  uint32_t total;
  block_scan_u32<256>(len, &total, s_tmp);
  if (threadIdx.x == 0) m.tile_off[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_rows_mv_copy(RowsMv m) {
  __shared__ uint32_t s_tmp[4];
  __shared__ uint32_t s_off[256], s_b[256];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t b = 0, len = 0;
  if (k < m.keep) mv_span(m, k, &b, &len);
  uint32_t total;
  const uint32_t x = block_scan_u32<256>(len, &total, s_tmp);
  const int64_t base = m.tile_off[blockIdx.x];
  s_off[threadIdx.x] = x;
  s_b[threadIdx.x] = b;
  if (k < m.keep) {
    m.out_offs[k] = base + x;
    if (k == m.keep - 1) m.out_offs[m.keep] = base + x + len;
  }
  __syncthreads();
  // value j of the tile belongs to the last row whose exclusive offset is <= j (rows of length 0 share an
  // offset with their successor and are passed over)
  for (uint32_t j = threadIdx.x; j < total; j += 256) {
    int lo = 0, hi = 255;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_off[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    const int64_t o = base + j;
    if (o < m.out_cap) m.out_ids[o] = (int32_t)load_id(m.vals, (int64_t)s_b[lo] + (j - s_off[lo]));
  }
}

void launch_rows_mv_len(const RowsMv& m, unsigned long long* info, hipStream_t s) {
  if (m.keep <= 0) return;
  const int64_t ntiles = (m.keep + 255) / 256;
  hipLaunchKernelGGL(k_rows_mv_len, dim3((unsigned)ntiles), dim3(256), 0, s, m);
  hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(256), 0, s, m.tile_off, ntiles, ~0ull, info);
}

void launch_rows_mv_copy(const RowsMv& m, hipStream_t s) {
  if (m.keep <= 0) return;
  hipLaunchKernelGGL(k_rows_mv_copy, dim3((unsigned)((m.keep + 255) / 256)), dim3(256), 0, s, m);
}

}  // namespace dg
