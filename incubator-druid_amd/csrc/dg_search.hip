// dg_search.hip — HIP kernels (gfx950 / CDNA4) of the search query (dg_search_run).
//
//   k_search_time_and       rows inside the query interval AND the filter   UseIndexesStrategy.makeTimeFilteredBitmap
//                                                                           (query/search/UseIndexesStrategy.java:143-219)
//   k_search_concise_count  |Concise bitmap AND selection| per accepted value IndexOnlyExecutor.execute (:236-281):
//   k_search_roaring_count  |Roaring bitmap AND selection| per accepted value bitmapFactory.intersection(...).size()
//   k_search_hist           accepted value occurrences of the selected rows StringSearchColumnSelectorStrategy
//   k_search_gather         the accepted ids' counters in output order      .updateSearchResultSet (SearchQueryRunner.java:118-141)
//
// The bitmap kernels never build the intersection: every Concise word / Roaring container adds the
// popcount of its rows inside the selection bitset S (null = every row below nrows). Counts are summed
// with integer adds (one atomicAdd per job), so they do not depend on the order the jobs run in.
// Every loop is bounded by a length the host read at attach (bitmap bytes, piece tables, nrows);
// nothing waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"

namespace dg {

// ------------------------------------------------------------------------------------------------
// the selection bitset: word w of S restricted to rows below nrows (words outside [0, ceil(nrows/32))
// are never read: the filter's bitset has nothing defined there)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sel_word(const uint32_t* __restrict__ S, int64_t w, int64_t nrows) {
  const int64_t nwords = (nrows + 31) >> 5;
  if (w < 0 || w >= nwords) return 0u;
  uint32_t v = S ? S[w] : 0xFFFFFFFFu;
  if (w == nwords - 1 && (nrows & 31)) v &= (1u << (nrows & 31)) - 1u;
  return v;
}

__device__ __forceinline__ uint32_t sel_bit(const uint32_t* __restrict__ S, int64_t r, int64_t nrows) {
  if (r < 0 || r >= nrows) return 0u;
  return S ? (S[r >> 5] >> (r & 31)) & 1u : 1u;
}

// mask of word w's bits that lie in rows [lo, hi) (lo < hi)
__device__ __forceinline__ uint32_t range_mask(int64_t w, int64_t lo, int64_t hi) {
  const int64_t b0 = w << 5;
  uint32_t m = 0xFFFFFFFFu;
  if (lo > b0) m &= 0xFFFFFFFFu << (lo - b0);
  if (hi < b0 + 32) m &= 0xFFFFFFFFu >> (b0 + 32 - hi);
  return m;
}

// |S AND [lo, hi)| by the words first, first + step, ... of the range (step lanes share one range)
__device__ __forceinline__ uint32_t sel_range_strided(const uint32_t* __restrict__ S, int64_t lo, int64_t hi,
                                                      int64_t nrows, int first, int step) {
  if (lo < 0) lo = 0;
  if (hi > nrows) hi = nrows;
  if (hi <= lo) return 0u;
  uint32_t c = 0;
  const int64_t w1 = (hi - 1) >> 5;
  for (int64_t w = (lo >> 5) + first; w <= w1; w += step) c += __popc(sel_word(S, w, nrows) & range_mask(w, lo, hi));
  return c;
}

// rows a lane may walk alone; longer ranges are shared by its wave or workgroup
constexpr int64_t kSearchShortRows = 64 * 32;

// Ranges too long for one lane, shared by the wave: every lane with `mine` set hands its [lo, hi) to
// all 64 lanes in turn (at most 64 rounds, each ceil(range words / 64) steps)
__device__ __forceinline__ uint32_t wave_long_ranges(const uint32_t* __restrict__ S, bool mine, int64_t lo, int64_t hi,
                                                     int64_t nrows, int lane) {
  uint32_t c = 0;
  uint64_t pending = __ballot(mine);
  while (pending) {
    const int src = __ffsll((unsigned long long)pending) - 1;
    pending &= pending - 1;
    const int64_t l = __shfl(lo, src, 64), h = __shfl(hi, src, 64);
    c += sel_range_strided(S, l, h, nrows, lane, 64);
  }
  return c;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// block-wide (256 threads) exclusive scan of int64 (as dg_kernels.hip's)
__device__ __forceinline__ int64_t search_block_scan(int64_t v, int64_t* total, int64_t* s_tmp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_tmp[wave] = x;
  __syncthreads();
  int64_t wave_off = 0, tot = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) wave_off += s_tmp[w];
    tot += s_tmp[w];
  }
  __syncthreads();
  *total = tot;
  return wave_off + x - v;
}

// ------------------------------------------------------------------------------------------------
// S = filter bitset AND rows whose time lies in [t_lo, t_hi): one ballot per 64 rows writes two bitset
// words per wave (as k_num_pred). Tagged __time blocks (load_time) stay undecoded. The rows selected
// are counted into *count (one atomic per workgroup).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_search_time_and(ColView time, const uint32_t* __restrict__ in, int64_t nrows,
                                                         int64_t t_lo, int64_t t_hi, uint32_t* __restrict__ out,
                                                         unsigned long long* __restrict__ count) {
  __shared__ unsigned long long s_c[4];
  const int lane = threadIdx.x & 63;
  unsigned long long local = 0;
  const int64_t ntiles = (nrows + 255) >> 8;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * 256 + threadIdx.x;
    bool m = false;
    if (r < nrows) {
      const int64_t t = load_time(time, r);
      m = t >= t_lo && t < t_hi && (!in || ((in[r >> 5] >> (r & 31)) & 1u));
    }
    const uint64_t b = __ballot(m);
    const int64_t w = (r - lane) >> 5;  // first word of this wave's 64 rows
    if (r - lane < nrows) {
      if (lane == 0) {
        out[w] = (uint32_t)b;
        local += __popcll((unsigned long long)b);
      }
      if (lane == 32 && r < nrows) out[w + 1] = (uint32_t)(b >> 32);
    }
  }
  local = wave_sum(local);
  if (lane == 0) s_c[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long c = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    if (c) atomicAdd(count, c);
  }
}

void launch_search_time_and(ColView time, const uint32_t* in, int64_t nrows, int64_t t_lo, int64_t t_hi, uint32_t* out,
                            unsigned long long* d_count, hipStream_t s) {
  if (nrows <= 0) return;
  const int64_t ntiles = (nrows + 255) / 256;
  hipLaunchKernelGGL(k_search_time_and, dim3((unsigned)std::min<int64_t>(ntiles, 1024)), dim3(256), 0, s, time, in, nrows,
                     t_lo, t_hi, out, d_count);
}

// ------------------------------------------------------------------------------------------------
// Concise: |bitmap AND S|. The words are walked as k_concise_or walks them (big-endian; literal = MSB 1
// + 31 bits; fill = bit 30 fill value, bits 25-29 flipped bit + 1, bits 0-24 blocks - 1; the flipped bit
// is in the first block; ConciseSetUtils.java:45-75,149-281); a word adds the popcount of S over its
// rows instead of OR-ing them. Jobs [0, n_small) hold at most 64 words and take one wave each, four per
// workgroup; the others one workgroup each, 256 words per step.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t concise_span(uint32_t w) {
  return (w & 0x80000000u) ? 31 : 31ll * ((int64_t)(w & 0x01FFFFFFu) + 1);
}

// the rows of word w at row offset o inside S; a one-fill longer than kSearchShortRows is left to the
// caller (*long_lo / *long_hi, returns true) minus its flipped bit, which is settled here
__device__ __forceinline__ bool concise_word_count(const uint32_t* __restrict__ S, int64_t nrows, uint32_t w, int64_t o,
                                                   int64_t span, unsigned long long* c) {
  if (w & 0x80000000u) {
    const int64_t wi = o >> 5;
    const int sh = (int)(o & 31);
    const uint64_t both = (uint64_t)sel_word(S, wi, nrows) | ((uint64_t)sel_word(S, wi + 1, nrows) << 32);
    *c += __popc((uint32_t)(both >> sh) & (w & 0x7FFFFFFFu));
    return false;
  }
  const int flip = (int)((w >> 25) & 0x1Fu) - 1;
  if ((w & 0x40000000u) == 0) {
    if (flip >= 0) *c += sel_bit(S, o + flip, nrows);
    return false;
  }
  if (flip >= 0) *c -= sel_bit(S, o + flip, nrows);  // (the range's count below holds it; sums wrap back)
  if (span > kSearchShortRows) return true;
  *c += sel_range_strided(S, o, o + span, nrows, 0, 1);
  return false;
}

__global__ __launch_bounds__(256) void k_search_concise_count(const SearchJob* __restrict__ jobs, int n_small, int n_jobs,
                                                              unsigned long long* __restrict__ counts) {
  __shared__ int64_t s_tmp[8];
  __shared__ unsigned long long s_c[4];
  __shared__ int64_t s_qlo[256], s_qhi[256];
  __shared__ int s_nq;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int small_blocks = (n_small + 3) >> 2;
  if ((int)blockIdx.x < small_blocks) {
    // ---- one wave per bitmap of at most 64 words ----
    const int j = blockIdx.x * 4 + wave;
    if (j >= n_small) return;
    const SearchJob job = jobs[j];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(job.data);
    const int nw = min(job.len >> 2, 64);
    uint32_t w = 0;
    int64_t span = 0;
    if (lane < nw) {
      w = __builtin_bswap32(words[lane]);
      span = concise_span(w);
    }
    int64_t x = span;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    const int64_t o = job.row0 + x - span;
    unsigned long long c = 0;
    bool lng = false;
    if (lane < nw) lng = concise_word_count(job.S, job.nrows, w, o, span, &c);
    c += wave_long_ranges(job.S, lng, o, o + span, job.nrows, lane);
    c = wave_sum(c);
    if (lane == 0 && c) atomicAdd(counts + job.slot, c);
    return;
  }
  // ---- one workgroup per longer bitmap (or piece of a split one) ----
  const int j = n_small + ((int)blockIdx.x - small_blocks);
  if (j >= n_jobs) return;
  const SearchJob job = jobs[j];
  const uint32_t* words = reinterpret_cast<const uint32_t*>(job.data);
  const int nw = job.len >> 2;
  int64_t carry = job.row0;
  unsigned long long c = 0;
  if (threadIdx.x == 0) s_nq = 0;
  __syncthreads();
  for (int basew = 0; basew < nw; basew += 256) {
    const int i = basew + threadIdx.x;
    uint32_t w = 0;
    int64_t span = 0;
    if (i < nw) {
      w = __builtin_bswap32(words[i]);
      span = concise_span(w);
    }
    int64_t total;
    const int64_t o = carry + search_block_scan(span, &total, s_tmp);
    if (i < nw && concise_word_count(job.S, job.nrows, w, o, span, &c)) {
      const int q = atomicAdd(&s_nq, 1);  // at most 256 per step: one per thread
      s_qlo[q] = o;
      s_qhi[q] = o + span;
    }
    carry += total;
    __syncthreads();
    // the step's long one-fills: the whole workgroup popcounts each
    const int nq = s_nq;
    for (int q = 0; q < nq; ++q) c += sel_range_strided(job.S, s_qlo[q], s_qhi[q], job.nrows, threadIdx.x, 256);
    __syncthreads();
    if (threadIdx.x == 0) s_nq = 0;
    // (the next step's first barrier, inside the scan, orders this reset before its queueing)
  }
  c = wave_sum(c);
  if (lane == 0) s_c[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    if (t) atomicAdd(counts + job.slot, t);
  }
}

void launch_search_concise_count(const SearchJob* d_jobs, int n_small, int n_jobs, unsigned long long* d_counts,
                                 hipStream_t s) {
  if (n_jobs <= 0) return;
  const int blocks = (n_small + 3) / 4 + (n_jobs - n_small);
  hipLaunchKernelGGL(k_search_concise_count, dim3(blocks), dim3(256), 0, s, d_jobs, n_small, n_jobs, d_counts);
}

// ------------------------------------------------------------------------------------------------
// Roaring (portable format, RoaringFormatSpec): |bitmap AND S|. Jobs [0, n_whole) are whole bitmaps: one
// workgroup each, thread 0 walks the headers into LDS as k_roaring_or does (checking every container
// against the bitmap's bytes), then the waves take containers round-robin. The others are single
// containers of bitmaps split at attach (row0, info as BmPiece), one wave each, four per workgroup.
// ------------------------------------------------------------------------------------------------
constexpr int kSearchMaxContainers = 4096;

__device__ __forceinline__ uint32_t s_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t s_rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// one container by one wave: d = its data (inside the bitmap's bytes, checked by the caller), rows from row0
__device__ __forceinline__ unsigned long long container_count(const uint8_t* __restrict__ d, int64_t row0, bool run,
                                                              int card, const uint32_t* __restrict__ S, int64_t nrows,
                                                              int lane) {
  unsigned long long c = 0;
  if (run) {
    const int nruns = (int)s_rd16(d);
    for (int base = 0; base < nruns; base += 64) {  // (uniform trip count: the shared ranges need every lane)
      const int r = base + lane;
      int64_t st = 0, ln = 0;
      if (r < nruns) {
        st = row0 + s_rd16(d + 2 + 4 * r);
        ln = (int64_t)s_rd16(d + 4 + 4 * r) + 1;
      }
      const bool lng = ln > kSearchShortRows;
      if (r < nruns && !lng) c += sel_range_strided(S, st, st + ln, nrows, 0, 1);
      c += wave_long_ranges(S, lng, st, st + ln, nrows, lane);
    }
  } else if (card <= 4096) {
    for (int k = lane; k < card; k += 64) c += sel_bit(S, row0 + s_rd16(d + 2 * k), nrows);
  } else {
    const int64_t w0 = row0 >> 5;
    for (int k = lane; k < 2048; k += 64) c += __popc(s_rd32(d + 4 * k) & sel_word(S, w0 + k, nrows));
  }
  return c;
}

__global__ __launch_bounds__(256) void k_search_roaring_count(const SearchJob* __restrict__ jobs, int n_whole, int n_jobs,
                                                              unsigned long long* __restrict__ counts,
                                                              int32_t* __restrict__ err) {
  __shared__ int32_t s_key[kSearchMaxContainers];
  __shared__ int32_t s_card[kSearchMaxContainers];
  __shared__ int32_t s_off[kSearchMaxContainers];
  __shared__ uint8_t s_run[kSearchMaxContainers];
  __shared__ int32_t s_n;
  __shared__ unsigned long long s_c[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.x >= n_whole) {
    // ---- one container per wave ----
    const int j = n_whole + ((int)blockIdx.x - n_whole) * 4 + wave;
    if (j >= n_jobs) return;
    const SearchJob job = jobs[j];
    const bool run = job.info < 0;
    const int card = (job.info & 0x7FFFFFFF) + 1;
    // the piece's bytes were sized at attach; a run container's own count must still fit them
    if (run && (job.len < 2 || 2 + 4 * (int)s_rd16(job.data) > job.len)) {
      if (lane == 0) atomicOr(err, 2);
      return;
    }
    unsigned long long c = wave_sum(container_count(job.data, job.row0, run, card, job.S, job.nrows, lane));
    if (lane == 0 && c) atomicAdd(counts + job.slot, c);
    return;
  }
  const SearchJob job = jobs[blockIdx.x];
  const uint8_t* p = job.data;
  const int nbytes = job.len;
  if (threadIdx.x == 0) {
    int n = 0;
    bool ok = nbytes >= 8;
    if (ok) {
      const uint32_t cookie = s_rd32(p);
      int pos = 4;
      const uint8_t* runbits = nullptr;
      bool has_off = true;
      if ((cookie & 0xFFFFu) == 12347u) {
        n = (int)(cookie >> 16) + 1;
        runbits = p + pos;
        pos += (n + 7) / 8;
        has_off = n >= 4;
      } else if (cookie == 12346u) {
        n = (int)s_rd32(p + 4);
        pos = 8;
      } else {
        ok = false;
      }
      ok = ok && n >= 0 && n <= kSearchMaxContainers;
      // the descriptive header and the offset header lie inside the bitmap
      ok = ok && (int64_t)pos + 4ll * n * (has_off ? 2 : 1) <= nbytes;
      if (ok) {
        const uint8_t* desc = p + pos;
        pos += 4 * n;
        const uint8_t* offs = has_off ? p + pos : nullptr;
        if (has_off) pos += 4 * n;
        int64_t cur = pos;
        for (int c = 0; c < n && ok; ++c) {
          s_key[c] = (int)s_rd16(desc + 4 * c);
          s_card[c] = (int)s_rd16(desc + 4 * c + 2) + 1;
          s_run[c] = runbits ? ((runbits[c >> 3] >> (c & 7)) & 1) : 0;
          const int64_t start = offs ? (int64_t)s_rd32(offs + 4 * c) : cur;
          int64_t sz;
          if (s_run[c]) {
            if (start < pos || start + 2 > nbytes) {
              ok = false;
              break;
            }
            sz = 2 + 4 * (int64_t)s_rd16(p + start);
          } else if (s_card[c] <= 4096) {
            sz = 2 * s_card[c];
          } else {
            sz = 8192;
          }
          if (start < pos || start + sz > nbytes) {
            ok = false;
            break;
          }
          s_off[c] = (int32_t)start;
          cur = start + sz;
        }
      }
    }
    if (!ok) {
      atomicOr(err, 2);
      n = 0;
    }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  unsigned long long c = 0;
  for (int k = wave; k < n; k += 4)
    c += container_count(p + s_off[k], (int64_t)s_key[k] << 16, s_run[k] != 0, s_card[k], job.S, job.nrows, lane);
  c = wave_sum(c);
  if (lane == 0) s_c[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    if (t) atomicAdd(counts + job.slot, t);
  }
}

void launch_search_roaring_count(const SearchJob* d_jobs, int n_whole, int n_jobs, unsigned long long* d_counts,
                                 int32_t* d_err, hipStream_t s) {
  if (n_jobs <= 0) return;
  const int blocks = n_whole + (n_jobs - n_whole + 3) / 4;
  hipLaunchKernelGGL(k_search_roaring_count, dim3(blocks), dim3(256), 0, s, d_jobs, n_whole, n_jobs, d_counts, d_err);
}

// ------------------------------------------------------------------------------------------------
// Cursor plan: every accepted value occurrence of the rows S selects adds one to its dictionary id's
// counter (a multi-value row [a, a] adds two). Dictionaries of at most kSearchLdsCard values count in
// LDS (each workgroup flushes its non-zero counters once), larger ones with global integer atomics.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool accepted(const uint64_t* __restrict__ accept, uint32_t id, uint32_t card) {
  return id < card && ((accept[id >> 6] >> (id & 63)) & 1ull);
}

__global__ __launch_bounds__(256) void k_search_hist(SearchHist h) {
  __shared__ uint32_t s_cnt[kSearchLdsCard];
  const bool lds = h.card <= (uint32_t)kSearchLdsCard;
  if (lds) {
    for (uint32_t i = threadIdx.x; i < h.card; i += 256) s_cnt[i] = 0;
    __syncthreads();
  }
  const int64_t ntiles = (h.nrows + 255) >> 8;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * 256 + threadIdx.x;
    if (r >= h.nrows || !sel_bit(h.S, r, h.nrows)) continue;
    if (h.offs.kind != VIEW_ABSENT) {
      uint32_t b = load_id(h.offs, r), e = load_id(h.offs, r + 1);
      if (e > h.nvals) e = (uint32_t)h.nvals;  // (corrupt row lists raise the call's error word; stay inside)
      for (uint32_t k = b; k < e; ++k) {
        const uint32_t id = load_id(h.vals, k);
        if (!accepted(h.accept, id, h.card)) continue;
        if (lds) atomicAdd(&s_cnt[id], 1u);
        else atomicAdd(h.hist + id, 1ull);
      }
    } else {
      const uint32_t id = load_id(h.vals, r);
      if (!accepted(h.accept, id, h.card)) continue;
      if (lds) atomicAdd(&s_cnt[id], 1u);
      else atomicAdd(h.hist + id, 1ull);
    }
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < h.card; i += 256) {
      const uint32_t v = s_cnt[i];
      if (v) atomicAdd(h.hist + i, (unsigned long long)v);
    }
  }
}

// out[k] = hist[ids[k]]: the accepted ids' counters in the call's output order
__global__ __launch_bounds__(256) void k_search_gather(const unsigned long long* __restrict__ hist,
                                                       const int32_t* __restrict__ ids, int n,
                                                       unsigned long long* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = hist[ids[k]];
}

void launch_search_hist(const SearchHist& h, const int32_t* d_ids, int n_ids, unsigned long long* d_out, hipStream_t s) {
  if (n_ids <= 0) return;
  if (h.nrows > 0) {
    // LDS counters: few workgroups, so few flushes (each up to card atomics); global counters: one tile each
    const int64_t ntiles = (h.nrows + 255) / 256;
    const int64_t cap = h.card <= (uint32_t)kSearchLdsCard ? 512 : 4096;
    hipLaunchKernelGGL(k_search_hist, dim3((unsigned)std::min<int64_t>(ntiles, cap)), dim3(256), 0, s, h);
  }
  hipLaunchKernelGGL(k_search_gather, dim3((n_ids + 255) / 256), dim3(256), 0, s, h.hist, d_ids, n_ids, d_out);
}

}  // namespace dg
