// dg_firstlast.hip — HIP kernels (gfx950 / CDNA4, wave64) of the first / last aggregators
// (query/aggregation/first/*, query/aggregation/last/*: "the value at the earliest / latest timestamp").
//
// Row update of the reference's buffer aggregators, a 16-byte (time, value) pair per cell:
//   Long/Double/FloatFirstBufferAggregator.aggregate (first/LongFirstBufferAggregator.java:48-56):
//     if (time < firstTime) { firstTime = time; firstValue = valueSelector.getLong(); }   init (Long.MAX_VALUE, 0)
//     strict <: of the rows sharing the smallest time, the one the cursor reaches first wins;
//   Long/Double/FloatLastBufferAggregator.aggregate (last/LongLastBufferAggregator.java:50-56):
//     if (time >= lastTime) { lastTime = time; lastValue = valueSelector.getLong(); }     init (Long.MIN_VALUE, 0)
//     >=: of the rows sharing the largest time, the one the cursor reaches last wins.
// "Reached first / last" is the cursor's order: position p(r) = r under an ascending cursor and
// nrows - 1 - r under a descending one (timeseries and topN; groupBy always scans ascending). So the
// winner of a cell is the arg-min (first) or arg-max (last) of the pair (row time, cursor position), and
// inside one call that pair packs into one 64-bit key:
//
//   key(r) = (((t(r) - t0) << rb) | p(r)) + 1        t0 = smallest row time, rb = bits of the largest p
//
// The + 1 and the host's budget bits(tmax - t0) + rb <= 63 keep every key inside [1, 2^63], away from
// both slot identities (~0 for a minimum, 0 for a maximum). The keys are stored as int64 (key ^ sign), so
// the existing longMin / longMax input encoding (value ^ sign) hands the aggregation kernels the unsigned
// key: every aggregation path finds the winner with the OP_MIN_U64 / OP_MAX_U64 it already has.
//
//   k_fl_keys     one segment's key column from its decoded __time       8 B read + 8 B written per row
//   k_fl_resolve  winning keys -> the value at the winning row           per (cell, first/last slot): 8 B read,
//                                                                        one gathered value, 8 B written
//
// groupBy merges a call's segments in one sort: there p is the call-wide row reference row_base + r, so
// earlier segments win first-ties and later ones last-ties — a left fold of the factories' combine
// (LongFirstAggregatorFactory.java:103-112: lhs.time <= rhs.time ? lhs : rhs;
// LongLastAggregatorFactory.java:107: lhs.time > rhs.time ? lhs : rhs) in segment order.
//
// Both kernels are plain passes: nothing waits on another workgroup, every loop is bounded by a length
// the host passes and every load and store is guarded by it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dg_device.h"

namespace dg {

constexpr int kFlT = 256;

// grid: (x = strided rows, y = job). One 8-byte load and one 8-byte store per lane.
__global__ __launch_bounds__(kFlT) void k_fl_keys(const FlKeyJob* __restrict__ jobs) {
  const FlKeyJob& j = jobs[blockIdx.y];
  const int64_t n = j.nrows;
  const bool timed = j.time.kind != VIEW_ABSENT;
  for (int64_t r = (int64_t)blockIdx.x * kFlT + threadIdx.x; r < n; r += (int64_t)gridDim.x * kFlT) {
    // the row's real time: this view decodes every block (no representative times, see load_time)
    const int64_t t = timed ? *reinterpret_cast<const int64_t*>(cv_ptr(j.time, r)) : j.t0;
    const uint64_t p = (uint64_t)(j.desc ? j.p0 - r : j.p0 + r);
    const uint64_t key = ((((uint64_t)t - (uint64_t)j.t0) << j.rb) | p) + 1;
    j.keys[r] = (int64_t)(key ^ kSign);
  }
}

void launch_fl_keys(const FlKeyJob* d_jobs, int njobs, int64_t max_rows, hipStream_t s) {
  if (njobs <= 0 || max_rows <= 0) return;
  const int64_t blocks = std::min<int64_t>((max_rows + kFlT - 1) / kFlT, 4096);
  hipLaunchKernelGGL(k_fl_keys, dim3((unsigned)blocks, (unsigned)njobs), dim3(kFlT), 0, s, d_jobs);
}

// grid: (x = strided (cell, slot) pairs, y = job). The slot holds the winning key — as the accumulator
// tables keep it (abi == 0: the device encoding, the key itself) or as the groupBy reduce left it
// (abi == 1: finalized like a longMin / longMax, key ^ sign) — and receives the pair's value: the
// selector call of the aggregator's own type on the winning row (getLong / getDouble / getFloat with
// agg_input_at's coercions; a column the segment lacks reads 0), in the encoding of a sum of that type
// (okind = DG_AGG_LONG_SUM / DOUBLE_SUM / FLOAT_SUM: int64, double bits, float widened to double bits), or
// finalized to the ABI's (abi == 1). A cell still at its identity (no row reached the aggregator) gives
// 0, the reference's init value.
__global__ __launch_bounds__(kFlT) void k_fl_resolve(const FlResolveJob* __restrict__ jobs) {
  const FlResolveJob& j = jobs[blockIdx.y];
  const int64_t ncells = j.n_ptr ? min((int64_t)*j.n_ptr, j.ncells) : j.ncells;
  const int64_t total = ncells * j.nslots;
  for (int64_t x = (int64_t)blockIdx.x * kFlT + threadIdx.x; x < total; x += (int64_t)gridDim.x * kFlT) {
    const int64_t cell = x / j.nslots;
    const int k = (int)(x % j.nslots);
    uint64_t* slot = j.cells + cell * j.cell_stride + (int64_t)(1 + j.slot[k]) * j.slot_stride;
    const uint64_t key = j.abi ? *slot ^ kSign : *slot;
    const int okind = j.okind[k];
    uint64_t out = 0;
    if (key != 0ull && key != ~0ull) {
      const uint64_t ref = (key - 1) & ((1ull << j.rb) - 1ull);
      // the segment holding row reference `ref`: the last one whose row_base <= ref
      int lo = 0, len = j.nsegs;
      while (len > 1) {
        const int h = len >> 1;
        if ((uint64_t)j.segs[lo + h].row_base <= ref) {
          lo += h;
          len -= h;
        } else {
          len = h;
        }
      }
      const FlSeg& sg = j.segs[lo];
      const int64_t p = (int64_t)ref - (int64_t)sg.row_base;
      const int64_t r = sg.desc ? (int64_t)sg.nrows - 1 - p : p;
      if (r >= 0 && r < (int64_t)sg.nrows) {
        const ColView& v = sg.val[k];
        out = agg_input_at(okind, v.kind, v.kind != VIEW_ABSENT ? cv_ptr(v, r) : nullptr);
      }
    }
    *slot = j.abi ? finalize_dev(okind, out) : out;
  }
}

void launch_fl_resolve(const FlResolveJob* d_jobs, int njobs, int64_t max_pairs, hipStream_t s) {
  if (njobs <= 0 || max_pairs <= 0) return;
  const int64_t blocks = std::min<int64_t>((max_pairs + kFlT - 1) / kFlT, 4096);
  hipLaunchKernelGGL(k_fl_resolve, dim3((unsigned)blocks, (unsigned)njobs), dim3(kFlT), 0, s, d_jobs);
}

}  // namespace dg
