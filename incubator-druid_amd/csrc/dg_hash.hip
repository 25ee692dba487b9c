// dg_hash.hip — groupBy v2 as an HBM open-addressing hash grouper (gfx950), the opt-in alternative to
// the sort of dg_sort.hip.
//
// Replaces, for the merged result of the segments of one call:
//   BufferHashGrouper.aggregate over ByteBufferHashTable.findBucketWithAutoGrowth
//     (query/groupby/epinephelinae/BufferHashGrouper.java:38-133, ByteBufferHashTable.java:286-327,
//     AbstractBufferHashGrouper.java:119-171), with bufferGrouperMaxSize (GroupByQueryConfig.java:35-40)
//     and Groupers.HASH_TABLE_FULL (Groupers.java:36-40) when the table cannot take another group.
// It runs after the keygen of dg_sort.hip (one [key | element reference] word per selected element,
// the aggregators' inputs in the payload records):
//   insert   one workgroup per tile of kHashTile elements aggregates the tile into an LDS
//            open-addressing table first (LDS atomics, combine_op semantics), then upserts every
//            occupied LDS entry into the HBM table: one atomicCAS claim on the key (linear probing from
//            a mixed hash) and one atomic per slot — per (tile, group) instead of per element. An
//            element that finds the LDS table full (load factor 0.7) without its key goes to the
//            HBM table directly. No workgroup waits for another: no look-back, no spinning; a probe
//            sequence ends after `capacity` steps.
//   collect  occupied table positions -> [key | position] sort words, one atomic per workgroup;
//   (sort)   launch_radix_sort of dg_sort.hip over those words: groups, not rows;
//   emit     the sorted words' table records -> the result's keys and slot-major values (finalized).
// Integer results are exact; doubleSum partials combine in arrival order (last bits vary run to run).
// floatSum plans are not eligible (the fp32 row-order recurrence needs the sorted runs).
#include <hip/hip_runtime.h>

#include "dg_device.h"

namespace dg {

constexpr int kHT = 256;                  // threads of the hash kernels
constexpr int kHSPT = kHashTile / kHT;    // 16 elements per thread
// LDS table: 32 KiB of the CU's 160 KiB, so four to five insert workgroups (16-20 waves) share a CU and
// the LDS atomics of one hide the HBM upserts of another; entries of 8 * (2 + naggs) bytes (key, rows,
// values): 1024 entries for one or two aggregators, 128 for kMaxAggs
constexpr int kHashLdsBytes = 32 << 10;
// The LDS table is full at ByteBufferHashTable's max load factor, 0.7 of its entries: from then on it
// takes no new key (an absent key's probe sequence then stays ~6 entries long instead of walking a
// packed table), and an element whose key it does not hold goes to the HBM table. The limit is read
// before a claim and counted after it, so concurrent claims can pass it by a few entries; a probe
// sequence ends after min(entries, kHashLdsProbes) positions in any case.
constexpr int kHashLdsProbes = 128;
constexpr int kCollectPer = 8;            // table positions per thread of a collect workgroup

inline int hash_lds_entries(int naggs) {
  int e = 1;
  while (2 * e * (2 + naggs) * 8 <= kHashLdsBytes) e <<= 1;
  return e;
}

// splitmix64 finalizer: dictionary ids and bucket indices are dense small integers
__device__ __forceinline__ uint64_t hash_mix(uint64_t k) {
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}

__global__ __launch_bounds__(kHT) void k_gb_hash_fill(uint64_t* __restrict__ keys, uint64_t* __restrict__ slots,
                                                      int64_t capacity, AggPlan plan,
                                                      unsigned long long* __restrict__ ctr) {
  const int64_t stride = (int64_t)gridDim.x * kHT;
  for (int64_t i = (int64_t)blockIdx.x * kHT + threadIdx.x; i < capacity; i += stride) {
    keys[i] = kHashEmpty;
    slots[i] = 0;  // rows
    for (int a = 0; a < plan.n; ++a) slots[(size_t)(1 + a) * capacity + i] = identity_of(plan.op[a], plan.kind[a]);
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) ctr[threadIdx.x] = 0;
}

// One record (key, rows, val(a) per aggregator: device slot encoding) into the HBM table. False when the
// table cannot take it (probe bound or max_groups reached): the error bit is set and nothing is added.
template <class Val>
__device__ __forceinline__ bool hash_upsert(const HashTable& ht, const AggPlan& plan, uint64_t key, uint64_t rows,
                                            int32_t* __restrict__ err, Val&& val) {
  const uint64_t mask = (uint64_t)ht.capacity - 1ull;
  uint64_t h = hash_mix(key) & mask;
  bool found = false;
  for (int64_t p = 0; p < ht.capacity; ++p, h = (h + 1ull) & mask) {
    // a position only ever goes from empty to one key, so a stale read can only show `empty`, which
    // the CAS then settles
    uint64_t cur = __atomic_load_n(&ht.keys[h], __ATOMIC_RELAXED);
    if (cur == kHashEmpty) {
      cur = atomicCAS(reinterpret_cast<unsigned long long*>(&ht.keys[h]), (unsigned long long)kHashEmpty,
                      (unsigned long long)key);
      if (cur == kHashEmpty) {  // claimed: a new group
        const unsigned long long g = atomicAdd(&ht.ctr[0], 1ull) + 1ull;
        if (g > (unsigned long long)ht.max_groups) break;
        found = true;
        break;
      }
    }
    if (cur == key) {
      found = true;
      break;
    }
  }
  if (!found) {
    atomicOr(err, kErrTableFull);
    return false;
  }
  atomicAdd(reinterpret_cast<unsigned long long*>(&ht.slots[h]), (unsigned long long)rows);
  for (int a = 0; a < plan.n; ++a) {
    const uint64_t v = val(a);
    if (v != identity_of(plan.op[a], plan.kind[a])) atomic_op(plan.op[a], &ht.slots[(size_t)(1 + a) * ht.capacity + h], v);
  }
  return true;
}

// LDS: s_mem[0 .. E) keys, then [1 + naggs][E] slots (slot-major, so a wave's atomics on one slot of
// neighbouring entries fall into different banks)
__global__ __launch_bounds__(kHT) void k_gb_hash_insert(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ refs,
                                                        int kshift, const uint32_t* __restrict__ n_ptr,
                                                        const uint64_t* __restrict__ payload, int pw, HashTable ht,
                                                        AggPlan plan, int lds_entries, int32_t* __restrict__ err) {
  extern __shared__ uint64_t s_mem[];
  __shared__ uint32_t s_cnt[2];  // flushed entries, direct elements
  __shared__ uint32_t s_used;    // claimed LDS entries
  __shared__ int32_t s_stop;
  const int E = lds_entries;
  uint64_t* s_keys = s_mem;
  uint64_t* s_slots = s_mem + E;
  const uint32_t n = *n_ptr;
  const int64_t base = (int64_t)blockIdx.x * kHashTile;
  if (base >= (int64_t)n) return;
  if (threadIdx.x == 0) {
    s_stop = __atomic_load_n(err, __ATOMIC_RELAXED) & kErrTableFull;  // the table is full: stop inserting
    s_cnt[0] = s_cnt[1] = 0;
    s_used = 0;
  }
  for (int e = threadIdx.x; e < E; e += kHT) {
    s_keys[e] = kHashEmpty;
    s_slots[e] = 0;
    for (int a = 0; a < plan.n; ++a) s_slots[(1 + a) * E + e] = identity_of(plan.op[a], plan.kind[a]);
  }
  __syncthreads();
  if (s_stop) return;
  bool ok = true;
  uint32_t ndirect = 0, nflush = 0;
  for (int q = 0; q < kHSPT; ++q) {
    const int64_t i = base + q * kHT + threadIdx.x;
    if (i >= (int64_t)n || !ok) continue;
    const uint64_t w = keys[i];
    const uint64_t key = refs ? w : (kshift ? w >> kshift : w);
    const uint32_t ref = refs ? refs[i] : (uint32_t)(w & ((1ull << kshift) - 1ull));
    const uint64_t* rec = payload + (size_t)ref * (size_t)pw;
    uint32_t h = (uint32_t)(hash_mix(key) >> 40) & (uint32_t)(E - 1);
    bool found = false;
    const int nprobe = E < kHashLdsProbes ? E : kHashLdsProbes;
    const uint32_t limit = (uint32_t)E * 7u / 10u;
    for (int p = 0; p < nprobe; ++p, h = (h + 1u) & (uint32_t)(E - 1)) {
      // (an entry only ever goes from empty to one key: the CAS is needed on an empty one alone)
      uint64_t cur = __atomic_load_n(&s_keys[h], __ATOMIC_RELAXED);
      if (cur == kHashEmpty) {
        if (__atomic_load_n(&s_used, __ATOMIC_RELAXED) >= limit) break;  // full: the key is not in the table
        cur = atomicCAS(reinterpret_cast<unsigned long long*>(&s_keys[h]), (unsigned long long)kHashEmpty,
                        (unsigned long long)key);
        if (cur == kHashEmpty) {
          atomicAdd(&s_used, 1u);
          found = true;
          break;
        }
      }
      if (cur == key) {
        found = true;
        break;
      }
    }
    if (found) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&s_slots[h]), 1ull);
      for (int a = 0; a < plan.n; ++a) {
        const uint64_t v = rec[a];
        if (v != identity_of(plan.op[a], plan.kind[a])) atomic_op(plan.op[a], &s_slots[(1 + a) * E + h], v);
      }
    } else {  // the direct path
      ++ndirect;
      ok = hash_upsert(ht, plan, key, 1ull, err, [&](int a) { return rec[a]; });
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += kHT) {
    const uint64_t key = s_keys[e];
    if (key == kHashEmpty || !ok) continue;
    ++nflush;
    ok = hash_upsert(ht, plan, key, s_slots[e], err, [&](int a) { return s_slots[(1 + a) * E + e]; });
  }
  if (nflush) atomicAdd(&s_cnt[0], nflush);
  if (ndirect) atomicAdd(&s_cnt[1], ndirect);
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&ht.ctr[1 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// occupied positions of kHT * kCollectPer consecutive table positions -> sort words at the offset one
// atomic per workgroup reserves (the words' order is the sort's business)
__global__ __launch_bounds__(kHT) void k_gb_hash_collect(const uint64_t* __restrict__ tkeys, int64_t capacity, int pbits,
                                                         uint64_t* __restrict__ okeys, uint32_t* __restrict__ orefs,
                                                         uint32_t* __restrict__ out_n, int64_t ng) {
  __shared__ uint32_t s_tmp[kHT / 64];
  __shared__ uint32_t s_base;
  const int64_t base = (int64_t)blockIdx.x * (kHT * kCollectPer);
  uint64_t k[kCollectPer];
  uint32_t c = 0;
#pragma unroll
  for (int u = 0; u < kCollectPer; ++u) {
    const int64_t pos = base + u * kHT + threadIdx.x;
    k[u] = pos < capacity ? tkeys[pos] : kHashEmpty;
    c += k[u] != kHashEmpty ? 1u : 0u;
  }
  uint32_t tot;
  const uint32_t ex = block_scan_u32<kHT>(c, &tot, s_tmp);
  if (tot == 0) return;
  if (threadIdx.x == 0) s_base = atomicAdd(out_n, tot);
  __syncthreads();
  int64_t idx = (int64_t)s_base + ex;
#pragma unroll
  for (int u = 0; u < kCollectPer; ++u) {
    if (k[u] == kHashEmpty) continue;
    const uint64_t pos = (uint64_t)(base + u * kHT + threadIdx.x);
    if (idx < ng) {  // (the host sized the words for the groups the insert counted)
      if (orefs) {
        okeys[idx] = k[u];
        orefs[idx] = (uint32_t)pos;
      } else {
        okeys[idx] = (k[u] << pbits) | pos;
      }
    }
    ++idx;
  }
}

__global__ __launch_bounds__(kHT) void k_gb_hash_emit(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srefs,
                                                      int pbits, int64_t ng, const uint64_t* __restrict__ tslots,
                                                      int64_t capacity, AggPlan plan, uint64_t* __restrict__ out_keys,
                                                      uint64_t* __restrict__ out_slots, int64_t cap) {
  const int64_t stride = (int64_t)gridDim.x * kHT;
  for (int64_t g = (int64_t)blockIdx.x * kHT + threadIdx.x; g < ng; g += stride) {
    const uint64_t w = skeys[g];
    const uint64_t pos = srefs ? (uint64_t)srefs[g] : w & ((1ull << pbits) - 1ull);
    out_keys[g] = srefs ? w : w >> pbits;
    out_slots[g] = tslots[pos];
    for (int a = 0; a < plan.n; ++a)
      out_slots[(size_t)(1 + a) * cap + g] = finalize_dev(plan.kind[a], tslots[(size_t)(1 + a) * capacity + pos]);
  }
}

void launch_gb_hash_fill(const HashTable& ht, AggPlan plan, hipStream_t s) {
  const int64_t blocks = std::min<int64_t>(16384, (ht.capacity + kHT - 1) / kHT);
  hipLaunchKernelGGL(k_gb_hash_fill, dim3((unsigned)blocks), dim3(kHT), 0, s, ht.keys, ht.slots, ht.capacity, plan, ht.ctr);
}

void launch_gb_hash_insert(const SortBufs* sb, int64_t elem_cap, const HashTable& ht, AggPlan plan, int32_t* err,
                           hipStream_t s) {
  if (elem_cap <= 0) return;
  const int E = hash_lds_entries(plan.n);
  const size_t lds = (size_t)E * (2 + plan.n) * 8;
  const int64_t tiles = (elem_cap + kHashTile - 1) / kHashTile;
  hipLaunchKernelGGL(k_gb_hash_insert, dim3((unsigned)tiles), dim3(kHT), lds, s, sb->keys[sb->cur], sb->refs[sb->cur],
                     sb->ref_bits, sb->n, sb->payload, sb->pw, ht, plan, E, err);
}

void launch_gb_hash_collect(const HashTable& ht, SortBufs* gsb, int64_t ng, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(gsb->n, 0, 16, s);
  if (e != hipSuccess) {
    note_launch_error(e);
    return;
  }
  const int64_t per = (int64_t)kHT * kCollectPer;
  const int64_t blocks = (ht.capacity + per - 1) / per;
  hipLaunchKernelGGL(k_gb_hash_collect, dim3((unsigned)blocks), dim3(kHT), 0, s, ht.keys, ht.capacity, ht.log2_capacity,
                     gsb->keys[gsb->cur], gsb->refs[gsb->cur], gsb->n, ng);
}

void launch_gb_hash_emit(const SortBufs* gsb, int64_t ng, const HashTable& ht, AggPlan plan, uint64_t* out_keys,
                         uint64_t* out_slots, int64_t cap, hipStream_t s) {
  if (ng <= 0) return;
  const int64_t blocks = std::min<int64_t>(16384, (ng + kHT - 1) / kHT);
  hipLaunchKernelGGL(k_gb_hash_emit, dim3((unsigned)blocks), dim3(kHT), 0, s, gsb->keys[gsb->cur], gsb->refs[gsb->cur],
                     ht.log2_capacity, ng, ht.slots, ht.capacity, plan, out_keys, out_slots, cap);
}

}  // namespace dg
