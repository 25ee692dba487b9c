// dg_internal.h — structures shared by the host engine (dg_segment.cpp, dg_engine.cpp) and the
// HIP kernels (dg_kernels.hip). Device-side descriptors are plain PODs copied into HBM per call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/druidgpu.h"
#include "dg_expr.h"
#include "dg_filter_plan.h"
#include "dg_postagg.h"

namespace dg {

constexpr int kMaxAggs = 16;
constexpr int kBlockBytes = 65536;  // CompressedPools.BUFFER_SIZE (segment/CompressedPools.java:39)

// stored codecs (CompressionStrategy ids, data/CompressionStrategy.java:48-107)
enum Codec : int32_t { CODEC_LZF = 0x00, CODEC_LZ4 = 0x01, CODEC_UNCOMPRESSED = 0xFF, CODEC_NONE = 0xFE };

// value kinds a kernel can read from a column view
enum ViewKind : int32_t { VIEW_ABSENT = 0, VIEW_LONG = 1, VIEW_FLOAT = 2, VIEW_DOUBLE = 3, VIEW_IDS = 4 };

// accumulator slot ops (all slots are 8 bytes)
enum SlotOp : int32_t { OP_ADD_I64 = 0, OP_ADD_F64 = 1, OP_MIN_U64 = 2, OP_MAX_U64 = 3 };

// A column as the kernels see it: value(row) lives at blocks[row >> log2_per] + (row & mask) * width.
// flags: kViewBigEndian = dictionary ids stored big-endian (uncompressed VSizeColumnarInts);
// kViewFused = an aggregator's input whose tagged blocks (low pointer bit) the decoder already
// aggregated (Lz4Job.red_*): the scan takes the aggregator's identity for their rows.
struct ColView {
  const uint8_t* const* blocks;
  int32_t log2_per;
  int32_t width;
  int32_t kind;
  int32_t pad;  // flags
};
constexpr int32_t kViewBigEndian = 1;
constexpr int32_t kViewFused = 2;

// LZ4 sequence checkpoints: built once per block at attach (lz4_index_block), one entry per
// kLzSeqPerCp sequences (2 * kLzSeqPerCp for the rare block with more than kLzMaxCps * kLzSeqPerCp
// sequences) = the compressed offset where that sequence's token starts. They let the decoder
// parse every interval of a block in parallel (one interval per thread); the bytes stay LZ4.
constexpr int kLzSeqPerCp = 8;
constexpr int kLzMaxSeqPerCp = 2 * kLzSeqPerCp;  // the decoder's per-thread register budget
constexpr int kLzMaxCps = 1024;                  // one interval per decoder thread

// One LZ4 block to decode (compressed bytes are 16-byte aligned in the device image).
struct Lz4Job {
  const uint8_t* src;
  uint8_t* dst;
  const uint32_t* cp;  // checkpoints of this block
  int32_t src_len;
  int32_t expect_len;  // bytes that must come out (>= rows * width of the block)
  int32_t ncp;         // number of checkpoints; < 0: the block failed validation at attach
  int32_t dec_len;     // decoded length found at attach
  int32_t wide;        // checkpoints every 2 * kLzSeqPerCp sequences (decoded by the wide kernel)
  int32_t light;       // few sequences, short copy chains: decoded by the light kernel (k_lz4_light);
                       // > 0: sequences per light checkpoint (cp[ncp .. ncp + nfine) = the light checkpoints)
  int32_t nfine;       // light checkpoints (one per light-decoder thread)
  // 0: the block's bytes go to dst contiguously (a decode slot). > 0: the block holds 8-byte values
  // and value v goes to dst + v * vstride (a column of the groupBy payload records, written in place);
  // bytes past expect_len are then not written (they would land in the next segment's records)
  int32_t vstride;
  // run block (k_lz4_run): the block's run index (lz4_run_index) and its shape; null: another decoder
  const uint8_t* rx;
  int32_t run_n;    // intervals (one per k_lz4_run thread)
  int32_t run_far;  // bytes of the far-copy table after the intervals
  // flow block (wide & kLzFlow): its schedule (lz4_flow_schedule) and highest level
  const uint8_t* lvl;
  int32_t nlvl;
  // Decode fused with a timeseries aggregator (the block's rows share one bucket, no filter): instead
  // of writing its 8-byte values the decoder folds them with red_op (agg_input_raw(red_kind,
  // red_vkind, value)) and combines the block's result into the bucket's slot *red_dst atomically.
  // Null: the block is written out.
  uint64_t* red_dst;
  int32_t red_op;
  int32_t red_kind;
  int32_t red_vkind;
  int32_t red_code;  // kRed*: the fold in the value's own type (generic: agg_input_raw + combine_op)
  // a filtered scan's fold (round 6): only the rows whose bit is set in the segment's row bitset
  // red_bits (null: every row) fold; value v of the block is row red_row0 + v
  const uint32_t* red_bits;
  int64_t red_row0;
};
// A run of one column's LZ4 blocks of one decoder kind, decoded in one launch. Built per call in O(1)
// from the column's attach-time tables: block k = list[i] for i in [i0, i0 + n) (the column's blocks of
// that kind, ascending), its job = desc[k] (every query-independent Lz4Job field, expect_len = the bytes
// of its rows) with dst = dst_base + k * dst_step (null dst_base: a fused fold writes nothing), vstride
// and the fused fold (red_*) from the task.
struct Lz4Task {
  const Lz4Job* desc;
  const int32_t* list;
  int32_t i0, n;
  uint8_t* dst_base;
  int64_t dst_step;
  uint64_t* red_dst;
  int32_t vstride, red_op, red_kind, red_vkind, red_code;
  int32_t red_rpb;           // rows per block (the fold's row of value v of block k: k * red_rpb + v)
  const uint32_t* red_bits;  // the fold's row bitset (null: every row)
};
// A decoder launch: blocks [0, njobs) are per-block jobs, the rest belong to tasks (task_of[b - njobs] =
// the task of block b, task_first[t] = the launch block of task t's first block).
struct Lz4Launch {
  const Lz4Job* jobs;
  const Lz4Task* tasks;
  const int32_t* task_of;
  const int32_t* task_first;
  int32_t njobs;
  int32_t pad;
};
// decoder kinds of a block under the default routes (the partition run_decodes_only launches by)
enum : int32_t { kKindRun = 0, kKindGen0 = 1, kKindLight = 5, kKinds = 6 };  // kKindGen0 + wide: general

// folds of a fused decode (Lz4Job.red_code): int64 sum / max / min of a long column, double sum of a
// double column in their native types (converted to the slot encoding once per block); others generic
enum : int32_t { kRedGeneric = 0, kRedLongSum = 1, kRedDoubleSum = 2, kRedLongMax = 3, kRedLongMin = 4 };

// Light blocks (literal-heavy: random ids, high-entropy values): at most kLtMaxCps checkpoint
// intervals and copy chains of at most kLtMaxDepth hops. k_lz4_light decodes them with a small
// sequence table in LDS (many blocks per CU), resolving every output byte back to its literal.
constexpr int kLtMaxCps = 256;
#ifndef DG_LT_THREADS  // (A/B builds)
#define DG_LT_THREADS 512
#endif
constexpr int kLtThreads = DG_LT_THREADS;  // light-decoder threads (at most one light checkpoint interval each)
constexpr int kLtMaxDepth = 16;

// Run blocks: LZ4 blocks of 8-byte value runs (sequential longs, timestamps, constant columns) whose
// matches copy from at most 8 bytes back, except a few far copies. The attach-time run index cuts the
// block into intervals of >= kRunTarget output bytes at sequence boundaries and stores, per interval,
// its token offset, its output start and the 8 output bytes before it (its window); every far copy's
// bytes are listed once. k_lz4_run then decodes each interval independently in one thread: the last
// 8 output bytes ride in a register, a near copy is a shift of it, and every aligned 8-byte value is
// emitted as it completes. Index layout per block (16-byte aligned): u64 win[n], u32 tok[n] (token
// offset | far-table offset << 17), u16 out[n], zero pad to 16, the far table, zero pad to 16.
// Interval length and threads of the run decoder: one thread's serial chain is its interval, so the
// block's latency follows it; 96-byte intervals over 768 threads (round 6, same box: configs[4]a 8.03
// -> 7.46 ms, topN and the headline within noise to -3 %; 128 / 64 bytes close behind,
// profiles/r06_v51_ab_run.log) against 256 bytes over 256 threads before. (A/B builds override both.)
#ifndef DG_RUN_TARGET
#define DG_RUN_TARGET 96
#define DG_RUN_THREADS 768
#endif
constexpr int kRunThreads = DG_RUN_THREADS;  // one interval per thread (kBlockBytes / kRunTarget intervals at most)
constexpr int kRunTarget = DG_RUN_TARGET;    // output bytes per interval, at least (the last one excepted)
constexpr int kRunFarMax = 4096;   // far-copy bytes a run block may list
constexpr int kRunMaxRun = 1024;   // longest literal run / match of a run block (one thread's serial work)
constexpr int kRunLdsMax = 40960;  // staged input + far table of one run block (four workgroups per CU)
static_assert(kBlockBytes / kRunTarget <= kRunThreads, "one interval per k_lz4_run thread");
inline int run_index_bytes(int nint, int nfar) { return ((14 * nint + 15) & ~15) + ((nfar + 15) & ~15); }
inline int run_lds_bytes(int n, int nfar) { return ((n + 15) & ~15) + 16 + ((nfar + 15) & ~15) + 16; }
// Run index of one validated LZ4 block decoding to dec_len bytes, appended to *idx (16-byte aligned);
// returns false (nothing appended) when the block is not a run block.
bool lz4_run_index(const uint8_t* in, int n, int dec_len, std::vector<uint8_t>* idx, int* nint, int* nfar);
// Literal-only LZ4 block (a single sequence of literals, as LZ4 writes incompressible data): the
// offset of its literal bytes (= its decoded image), or -1.
int lz4_literal_start(const uint8_t* in, int n);
// Host decode of a validated LZ4 block into out (kBlockBytes); returns the decoded length or -1.
int lz4_decode_host(const uint8_t* in, int n, uint8_t* out);
// Decoder routes a query may take (read once per column): kRouteRun = run blocks go to k_lz4_run
// (off with DG_NO_RUN_DECODE), kRouteFlow = flow blocks go to k_lz4_decode_flow (off with
// DG_NO_FLOW_DECODE); same-box A/B and the tests of the other decoders turn them off
constexpr int kRouteRun = 1, kRouteFlow = 2;
int decode_routes();
struct BlockColumn;
// the job of LZ4 block k of a column (dst, expect and the routes given; no fused fold)
Lz4Job lz4_job(const BlockColumn& b, int32_t k, uint8_t* dst, int32_t expect, int routes);

// Flow blocks (Lz4Job.wide & kLzFlow, set at attach): general blocks of at most kLzMaxCps intervals
// that are not distance-8 class chains (at most a quarter of their bytes copied from 8 back) and whose
// copy chains are at most kFlowMaxDepth hops deep. The attach-time schedule ranks every match by its
// copy-chain level; k_lz4_decode_flow writes the literals into a byte image in LDS, then the matches
// level by level, each level's matches spread evenly over the threads.
constexpr int kLzFlow = 2;
constexpr int kFlowSideWgs = 192;  // persistent flow-decoder workgroups beside the groupBy sort (dg_engine.cpp)
constexpr int kFlowMaxDepth = 64;
constexpr int kFlowRecBytes = 48;  // schedule bytes per checkpoint interval (lz4_flow_schedule)
constexpr int kCompSlack = 64;     // bytes of zeros before and after a column's packed LZ4 blocks

// One LZF block (compress-lzf chunk stream, CompressionStrategy.LZFDecompressor) -> dst.
struct LzfJob {
  const uint8_t* src;
  uint8_t* dst;
  int32_t src_len;
  int32_t expect_len;  // bytes that must come out
};

// Expansion of one block of a DELTA / TABLE long column (CompressionFactory.LongEncodingFormat,
// CompressionFactory.java:153-188): `rows` values of `bits` bits packed MSB-first
// (VSizeLongSerde deserializers, VSizeLongSerde.java:416-657) -> little-endian int64 at dst.
struct VsJob {
  const uint8_t* src;   // packed block (decoded LZ4 slot, uncompressed block or NONE range)
  int64_t* dst;         // size_per int64 slots
  const int64_t* table; // TABLE: table values; DELTA: nullptr
  int64_t base;         // DELTA: base (DeltaLongEncodingReader.read, :63-66)
  int32_t rows;
  int32_t bits;
  int32_t table_n;
  int32_t pad;
};

// Host-side validating parse of one LZ4 block (lz4-java safe-decompressor semantics): appends the
// block's checkpoints to *cps and returns the decoded length, or -1 for a malformed block.
// *wide: bit 0 = the block keeps every other checkpoint (more than kLzMaxCps * kLzSeqPerCp sequences),
// kLzFlow = a flow block (decoded by k_lz4_decode_flow).
// *light (optional): the block qualifies for the light decoder (kLtMaxCps / kLtMaxDepth).
// *light = g > 0 when light: the block's checkpoints are followed by *nfine light checkpoints, one
// every g sequences (g the fewest sequences per checkpoint that fit the light decoder's threads).
// levels (optional): a flow block's schedule is appended (lz4_flow_schedule: per checkpoint interval
// kLzSeqPerCp u16 ranks of its matches in (level, position) order and kLzSeqPerCp u16 forwarded
// distances; then the u16 start of every level's ranks, padded to 16 bytes) and *nlvl = its highest
// level; without it no block is a flow block.
int lz4_index_block(const uint8_t* in, int n, std::vector<uint32_t>* cps, int* wide, int* light = nullptr,
                    int* nfine = nullptr, std::vector<uint8_t>* levels = nullptr, int* nlvl = nullptr);

struct AggPlan {
  int32_t n;
  int32_t kind[kMaxAggs];   // DG_AGG_*
  int32_t op[kMaxAggs];     // SlotOp
};

// One segment's share of a scan kernel.
struct ScanJob {
  int32_t nrows;
  int32_t tile_begin;       // first global tile index of this segment
  const uint32_t* bitset;   // null: every row passes the filter
  ColView time;             // VIEW_ABSENT when the time column is not needed
  int64_t t_lo, t_hi;       // rows with t in [t_lo, t_hi)
  int64_t bucket0;          // start of the first bucket (calendar: its index in `bounds`)
  int64_t period;           // 0 = ALL (single bucket); calendar: 1
  const int64_t* bounds;    // calendar granularity: ascending bucket starts (null: period grid)
  int32_t nbounds;
  int32_t desc;             // descending cursors (floatSum recurrence runs backwards)
  int32_t nbuckets;         // timeseries: buckets; topN: table keys (cardinality, x buckets when key_card)
  int32_t key_card;         // topN over granularity buckets: key = bucket * key_card + id (0: key = id)
  ColView vals[kMaxAggs];   // input column per aggregator
  const uint32_t* agg_bits[kMaxAggs];  // FilteredAggregatorFactory row matcher per aggregator (null: all rows)
  ColView key;              // topN: dimension ids (a multi-value dimension: its value stream)
  ColView key_off;          // topN over a multi-value dimension: row value offsets (VIEW_ABSENT otherwise)
  uint64_t* out;            // accumulator table of this segment
  // one-bucket timeseries (round 6): the tiles' records [tiles][1 + naggs], stored plainly and folded
  // into `out` by k_scan_combine — hundreds of tiles' atomics on one record serialised (configs[0]:
  // 1,464 on one line) — null: per-tile atomics into `out`
  uint64_t* part;
};

// groupBy by sort (dg_sort.hip) and the floatSum row-order pass. One job per segment of the call.
// A selected row becomes (key, row ref): key = [seg slot | bucket | merged id of every dimension],
// most significant field first, so ascending keys are the reference's merged row order
// (timestamp, then dimension values in Java String order, nulls first); the row ref is the row's
// index over the call's segments (row_base + row), so a stable sort keeps equal keys in
// (segment, row) order.
constexpr int kMaxGroupDims = 8;

struct GbJob {
  int32_t nrows;
  int32_t tile_begin;           // first keygen tile (kTileRows rows) of this segment
  uint32_t row_base;            // row ref of row 0
  int32_t ndims;
  const uint32_t* bitset;       // null: every row passes the filter
  ColView time;                 // VIEW_ABSENT when the time column is not needed
  int64_t t_lo, t_hi;           // rows with t in [t_lo, t_hi)
  int64_t bucket0;              // origin of the bucket index (shared by the call's segments in a merge)
  int64_t period;               // 0 = ALL; calendar: 1 (bucket index = position in `bounds`)
  const int64_t* bounds;        // calendar granularity: ascending bucket starts (null: period grid)
  int32_t nbounds;
  int32_t desc;                 // descending cursors: the floatSum pass runs each cell backwards
  int32_t seg_slot, seg_shift;  // key field of the segment (0 / 0 when the groups are merged)
  int32_t bucket_shift, bucket_bits;
  ColView dims[kMaxGroupDims];           // dictionary ids (a multi-value dimension: its value stream)
  ColView moff[kMaxGroupDims];           // multi-value dimension: row value offsets (VIEW_ABSENT otherwise)
  int32_t multi;                         // some dimension is multi-value: rows explode into groupings
  int32_t skip_empty;                    // an empty value list yields no element (topN) instead of null (groupBy)
  uint32_t inplace;                      // row-ref mode: payload columns the LZ4 decoder wrote (bit a)
  const int32_t* remap[kMaxGroupDims];  // local dictionary id -> merged id (null: identity)
  int32_t null_gid[kMaxGroupDims];      // merged id of the null value (a missing dimension's rows)
  int32_t dim_shift[kMaxGroupDims];
  int32_t dim_bits[kMaxGroupDims];
  ColView vals[kMaxAggs];
  const uint32_t* agg_bits[kMaxAggs];  // FilteredAggregatorFactory row matcher per aggregator
  // floatSum sink of the per-segment engines (timeseries / topN): slot (bucket * fs_mul + id) of this
  // segment's [keys][1 + naggs] accumulator table
  uint64_t* fs_out;
  int64_t fs_mul;
};

// Device buffers of one sort-based grouping; *_n are device words (counts known only on the device).
struct SortBufs {
  uint64_t* keys[2];      // packed (refs null): [key | row ref in the low ref_bits bits]; else keys
  uint32_t* refs[2];      // row refs when the key and the ref do not fit one word, else null
  int ref_bits;           // packed: bits of the element index (the sort key starts there); else 0
  uint64_t* payload;      // the aggregators' inputs of each element (device slot encoding): [cap][pw]
                          // by element reference
  int row_refs;           // element reference = the row's index over the call (one element per row,
                          // payload columns may be decoded in place); else the element index
  int pw;
  int cur;                // which of the ping-pong buffers holds the result
  uint32_t* tile_cnt;     // keygen tiles: selected rows, then their offsets
  uint32_t* n;            // [0] selected rows, [1] groups
  uint64_t* lb_status;    // radix look-back status per (tile, digit) of one pass: flag in the top two bits,
                          // the tile's digit count or inclusive prefix below (prefixes reach n: 64-bit)
  uint32_t* bin_total;    // [kRsMaxPasses][kMaxBins] digit totals + [kRsMaxPasses] tile counters
  uint32_t* run_cnt;      // per sort tile: run heads, then their offsets
  int64_t cap;            // element capacity (rows of the call)
  int ntiles_sort;        // sort tiles of `cap`
  // One-clear control memory (sort_ctl_bind; the groupBy call): `n`, `bin_total`, a look-back status
  // region per radix pass and the reduce's own lie in one contiguous region [ctl, ctl + ctl_bytes) that
  // launch_sort_ctl_clear zeroes with a single memset before the call's decodes, instead of a memset in
  // front of every pass and three in front of the reduce. lb_status is then null. ctl_clean: what is
  // still zeroed (kCtlSort: the passes' part, kCtlReduce: the reduce's); each user takes its bit, so
  // a second sort or reduce over the same buffers clears its part itself, as the unbound layout does.
  uint8_t* ctl;
  size_t ctl_bytes;
  uint64_t* pass_status[8];  // [kRsMaxPasses]
  uint64_t* red_status;
  int ctl_key_bits;  // the sort the pass regions were laid out for: key bits [defer_bits, defer_bits + ctl_key_bits)
  int ctl_clean;
  // Deferred low key bits (the groupBy sort plan): launch_radix_sort / launch_gb_sort_generated
  // order the words by key bits [defer_bits, key_bits) only (ties in element order) and launch_gb_reduce
  // finishes the order inside runs of equal prefix in LDS. 0: the classic sort over every key bit.
  int defer_bits;
};
constexpr int kCtlSort = 1, kCtlReduce = 2;

// ---------------------------------------------------------------------------------------------
// Host-side objects
// ---------------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset();
  bool alloc(size_t bytes);
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// A block-layout column (numeric values or dictionary ids) resident in HBM.
struct BlockColumn {
  int32_t total = 0;      // rows
  int32_t size_per = 0;   // rows per block (power of two)
  int32_t log2_per = 0;
  int32_t width = 0;      // bytes per value
  int32_t codec = 0;
  int32_t nblocks = 0;
  int32_t big_endian = 0;  // VSizeColumnarInts ids (uncompressed dimension)
  // DELTA / TABLE long encodings: blocks hold `vbits`-bit packed values (0 = plain LONGS);
  // `width` stays 8, the width of the expanded view the kernels read
  int32_t vbits = 0;
  int32_t table_n = 0;
  int64_t delta_base = 0;
  DevBuf table;                        // TABLE: int64[table_n]
  int64_t stored_bytes = 0;            // on-HBM bytes of all blocks (algorithmic bytes of a full scan)
  std::vector<int64_t> comp_off;       // host copy: offset of block b inside comp
  std::vector<int32_t> comp_len;
  std::vector<int64_t> cp_off;         // LZ4: first checkpoint of block b inside cps
  std::vector<int32_t> cp_n;           // LZ4: checkpoints of block b (-1: malformed block)
  std::vector<uint8_t> cp_wide;        // LZ4: block b keeps a checkpoint every 2 * kLzSeqPerCp sequences
  std::vector<uint8_t> cp_light;       // LZ4: block b goes to the light decoder (sequences per light checkpoint)
  std::vector<int32_t> cp_fine;        // LZ4: light checkpoints of block b (after its cp_n checkpoints)
  std::vector<int32_t> dec_len;        // LZ4: decoded bytes of block b
  bool time_col = false;               // the __time column: min8 / max8 are recorded at attach
  std::vector<int64_t> min8, max8;     // __time LZ4 LONGS: smallest / largest row time of block b (host
                                       // decode at attach; the cursor's uniform-block skip needs no
                                       // assumption on the row order inside a block)
  int64_t index_bytes = 0;             // LZ4: bytes of the index a query reads (checkpoints; run index
                                       // of run blocks instead)
  std::vector<int64_t> lit_off;        // LZ4: literal-only block b's literal bytes inside comp (16-byte
                                       // aligned: its decoded image, viewed in place), -1 otherwise;
                                       // empty: no literal-only block
  std::vector<int64_t> run_off;        // LZ4: block b's run index inside runx (-1: not a run block)
  std::vector<int32_t> run_n;          // LZ4: its intervals
  std::vector<int32_t> run_far;        // LZ4: its far-copy bytes
  DevBuf runx;                         // LZ4: run indexes of the run blocks
  std::vector<int64_t> lvl_off;        // LZ4: flow block b's level schedule inside lvls (-1: none)
  std::vector<int32_t> lvl_n;          // LZ4: its highest level
  DevBuf lvls;                         // LZ4: level schedules of the flow blocks
  DevBuf comp;                         // LZ4: packed compressed blocks (16-byte aligned)
  DevBuf cps;                          // LZ4: uint32 checkpoints of every block
  DevBuf raw;                          // UNCOMPRESSED: 64 KiB slot per block; NONE: flat values
  DevBuf block_ptrs;                   // const uint8_t*[nblocks]: raw slots (UNCOMPRESSED/NONE)
  // LZ4 decode tables (attach time, default routes): every block's query-independent job (device,
  // Lz4Job[nblocks]) and, per decoder kind, the blocks of that kind ascending (host + device, at
  // kind_at[kind] in kind_dev) with the prefix sums of their stored bytes / run-index or checkpoint
  // bytes. Literal-only and empty blocks are in no list.
  DevBuf job_desc;
  DevBuf kind_dev;
  std::vector<int32_t> kind_list[kKinds];
  std::vector<int32_t> kind_pos[kKinds];    // [k] = blocks of the kind below block k (nblocks + 1): O(1) ranges
  std::vector<int64_t> kind_bytes[kKinds];  // [i] = stored bytes of list[0 .. i)
  int64_t kind_at[kKinds] = {0, 0, 0, 0, 0, 0};
};

// A piece of a long serialized bitmap: Concise = a run of whole words starting at row `row0`;
// Roaring = one container (info = cardinality - 1 | 1 << 31 for a run container).
struct BmPiece {
  int64_t off;   // byte offset of the piece's data inside the column's bm_bytes
  int64_t row0;  // first row the piece covers
  int32_t len;   // bytes
  int32_t info;  // Roaring container: (card - 1) | run << 31; Concise: 0
};
constexpr int kConcisePieceWords = 4096;  // Concise bitmaps above 2x this are cut into pieces of it
constexpr int kRoaringSplitBytes = 32768; // Roaring bitmaps above this are cut into containers

constexpr int kOrderSlots = 8;

// (name, type, dict, dict_null, has_bitmaps and multi_value: DictColumn, what the filter planner reads)
struct Column : DictColumn {
  BlockColumn data;
  std::vector<uint64_t> dict_hash;     // value_hash of every dictionary value (cross-segment merges)
  int bitmap_roaring = 0;
  BlockColumn mv_off;                  // multi_value: rows + 1 value offsets (4-byte ints); row r's values:
                                       // data[mv_off[r] .. mv_off[r + 1])
  std::vector<int64_t> bm_off;         // byte offset of each bitmap inside bm_bytes (4-byte aligned)
  std::vector<int32_t> bm_len;
  DevBuf bm_bytes;
  // long bitmaps split at attach so one bitmap's expansion spreads over many workgroups: bitmap i's
  // pieces are bm_pieces[bm_piece_first[i] .. bm_piece_first[i + 1]) (empty = not split); empty
  // vector = no bitmap of the column is split
  std::vector<int32_t> bm_piece_first;
  std::vector<BmPiece> bm_pieces;
  // dictionary orders handed in by dg_segment_set_dim_order (slot = 2 * DG_ORDER_* + inverted):
  // rank of every dictionary id under the StringComparator, comparator-equal values share a rank
  DevBuf order_rank[kOrderSlots];
  std::vector<int32_t> order_host[kOrderSlots];
  int32_t order_ties[kOrderSlots] = {};
  bool order_set[kOrderSlots] = {};
  // topN bin index (built by the first topN over the column on the device, then reused): the rows
  // grouped by dictionary-id bin (id >> kTopnIxShift), each with its id's low bits (TopnIx)
  DevBuf tix_perm, tix_lid, tix_base;
  bool tix_ready = false;
  // value counts (built by the first groupBy whose first sort digit lies in this dimension's key field,
  // then reused): u32[cardinality], entry v = the segment's rows whose dictionary id is v — what the
  // per-value bitmap index stores. The sort's first-pass digit totals are summed from them (CountJob).
  // Ready only after a call that succeeded and whose counts summed to the segment's rows; a mismatch
  // marks the column never eligible (vcnt_never), so it is not rebuilt by every call.
  DevBuf vcnt;
  bool vcnt_ready = false;
  bool vcnt_never = false;
  // numeric-dimension encoding of a LONG, FLOAT or DOUBLE column (built on the device by the first groupBy
  // or topN over the column, then reused; dg_numdim.hip): nd_vals = int64[nd_card], the column's distinct
  // keys ascending (a LONG's key is the value, a FLOAT's / DOUBLE's the order-preserving fold of its
  // canonical bits, nd_key_bits; nd_host: its host copy, read back once); nd_ids = uint32[rows], row r's
  // index into nd_vals, viewed by the groupBy and the topN as ONE block of little-endian 4-byte ids
  // (nd_ptr: the one-entry block table in HBM, log2_per = kNdLog2Per). Ready only after a build that ran
  // to its end. nd_text: LONG only, position of every id in String.compareTo order of the decimal text
  // (long_text_key), derived on the host by the first topN that needs it.
  DevBuf nd_vals, nd_ids, nd_ptr;
  std::vector<int64_t> nd_host;
  std::vector<int32_t> nd_text;
  int64_t nd_card = 0;
  double nd_build_ms = 0;
  bool nd_ready = false;
  // a derived column (dg_segment_derive_column): `data` is a flat CODEC_NONE column the expression kernel wrote
  // (dg_expr.hip), registered under a name the caller chose and kept until dropped or until the segment is
  // released; the program it was built from tells an identical request from a colliding one
  bool derived = false;
  std::vector<ExOp> ex_ops;
  std::vector<std::string> ex_inputs;
};
constexpr int kNdLog2Per = 31;  // rows of a segment are int32: every row lies in block 0

inline bool is_numeric_type(int type) { return type == DG_COL_LONG || type == DG_COL_FLOAT || type == DG_COL_DOUBLE; }

// The value of a numeric-dimension key in the aggregate slot encoding (int64 / double bits / float32 bits
// in the low 4 bytes): the fold b ^ ((b >> 31 or 63) & 0x7fff…) is its own inverse.
inline uint64_t nd_key_bits(int type, int64_t key) {
  if (type == DG_COL_DOUBLE) return (uint64_t)(key ^ ((key >> 63) & 0x7fffffffffffffffll));
  if (type == DG_COL_FLOAT) {
    const int32_t k = (int32_t)key;
    return (uint64_t)(uint32_t)(k ^ ((k >> 31) & 0x7fffffff));
  }
  return (uint64_t)key;
}

// Merged dictionary of one dimension over a set of segments (the union of their sorted
// dictionaries in Java String order, nulls first) + each segment's local id -> merged id table in
// HBM. GroupByMergingQueryRunnerV2 merges rows by dimension VALUE (:188-246); the engine merges by
// merged id instead, which orders exactly like the values. Built on the host once per
// (segment set, dimension) and cached in the context, like a datasource-level dictionary.
struct MergedDict {
  std::vector<uint64_t> uids;  // attach serials of the segments, in call order
  std::string dim;
  std::vector<std::string> values;
  std::vector<uint8_t> is_null;
  int32_t null_gid = -1;                        // merged id of null (-1: no null value)
  std::vector<std::unique_ptr<DevBuf>> remap;   // per segment: int32[card] (empty = identity)
  // A long dimension (the column is LONG in every segment): the merged values are `longs` (values /
  // is_null stay empty, a long column has no null), in the order of the dimension's output type —
  // DG_COL_LONG: ascending; DG_COL_STRING: Java String order of their decimal text (long_text_less).
  bool is_long = false;
  int32_t out_type = DG_COL_STRING;  // DimensionSpec.getOutputType
  std::vector<int64_t> longs;
  size_t card() const { return is_long ? longs.size() : values.size(); }
};

// Java String.compareTo of String.valueOf(a) and String.valueOf(b) without forming the text: '-' sorts
// before every digit, so negatives come first; two magnitudes compare as their digit strings do, i.e. as
// the numbers padded with zeros on the right to 19 digits
// (a magnitude has at most 19, and 10^19 - 1 fits 64 bits), the shorter first when those are equal.
struct LongTextKey {
  int neg;           // 0 for "-…" (sorts first), 1 otherwise
  uint64_t mag;  // the magnitude's digits followed by zeros up to 19 digits
  int len;           // digits of the magnitude
  bool operator<(const LongTextKey& o) const {
    if (neg != o.neg) return neg < o.neg;
    if (mag != o.mag) return mag < o.mag;
    return len < o.len;
  }
};
inline LongTextKey long_text_key(int64_t v) {
  LongTextKey k;
  k.neg = v < 0 ? 0 : 1;
  uint64_t m = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;  // (|Long.MIN_VALUE| = 2^63 fits)
  int len = 1;
  for (uint64_t t = m; t >= 10; t /= 10) ++len;
  uint64_t a = m;
  for (int i = len; i < 19; ++i) a *= 10;
  k.mag = a;
  k.len = len;
  return k;
}
inline bool long_text_less(int64_t a, int64_t b) { return long_text_key(a) < long_text_key(b); }

struct Context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::mutex mu;
  // grow-only scratch arenas reused across calls
  DevBuf scratch[6];
  DevBuf pinned_dummy;
  hipEvent_t ev[8] = {};
  // side stream: the groupBy payload columns decode on it while the main stream builds and sorts the
  // keys (the two only meet at the reduce); side_ev[0] = its inputs are staged, [1..2] = decode span
  hipStream_t side = nullptr;
  hipEvent_t side_ev[3] = {};
  // the general LZ4 decoder's own span on each stream: [0, 1] main, [2, 3] side (its roofline
  // figures, dg_metrics)
  hipEvent_t gen_ev[4] = {};
  // a small call's short decoders (run, light) on the side stream beside the general decoder:
  // [0] their jobs are staged, [1] they are done (no timing)
  hipEvent_t ovl_ev[2] = {};
  // dg_context_set_limit(DG_LIMIT_GROUP_ELEMENTS): most sort elements one groupBy call may build
  uint64_t max_elements = ~0ull;
  // dg_context_set_limit(DG_LIMIT_GROUPER / DG_LIMIT_GROUPER_MAX_GROUPS): the default grouper of the
  // context's groupBy calls and their bufferGrouperMaxSize (0: unlimited)
  int32_t grouper = DG_GROUPER_SORT;
  int64_t max_groups = 0;
  // the last groupBy call's source of its first sort pass's digit totals (dg_debug_groupby_totals_source):
  // 0 = k_rs_hist0 (or no sort), 1 = the segments' value counts
  int32_t gb_totals_source = 0;
  // the last groupBy call's sort plan (dg_debug_groupby_sort_plan): global radix passes of the plan,
  // deferred key bits, 1 when a run overflowed and the classic sort ran after it
  int32_t gb_sort_plan[3] = {0, 0, 0};
  // query shapes (segments, dimensions, granularity) whose deferred sort overflowed: they take the
  // classic plan at once (most recent last, bounded like dict_cache)
  std::vector<std::string> gb_classic_shapes;
  std::vector<std::shared_ptr<MergedDict>> dict_cache;  // most recent last
  // device blocks of groupBy results: live (size by pointer) and released for reuse
  std::map<void*, size_t> block_size;
  std::vector<std::pair<void*, size_t>> free_blocks;
};

struct Segment {
  Context* ctx = nullptr;
  uint64_t uid = 0;  // attach serial (never reused: a cache key that outlives the segment)
  std::string dir;
  int64_t nrows = 0;
  int64_t istart = 0, iend = 0;
  int64_t min_time = 0, max_time = 0;
  int bitmap_roaring = 0;
  std::vector<std::unique_ptr<Column>> columns;
  // derived columns (dg_segment_derive_column): found by name like the stored ones, not listed among them
  std::vector<std::unique_ptr<Column>> derived;
  std::map<std::string, Column*> by_name;
  // the dimension list (index.drd's `dims`, StorageAdapter.getAvailableDimensions; a segment from rows:
  // its string columns in the order given): the scan query's default column list puts them first
  std::vector<std::string> dims;
  int64_t device_bytes = 0;
  Column* find(const std::string& n) const {
    auto it = by_name.find(n);
    return it == by_name.end() ? nullptr : it->second;
  }
};

// 64-bit hash of a dimension value (FNV-1a + avalanche); identity across segments' dictionaries
constexpr uint64_t kNullValueHash = 0x6e756c6c2d76616cull;
inline uint64_t value_hash(const std::string& v) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char ch : v) h = (h ^ ch) * 0x100000001b3ull;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h == kNullValueHash ? h + 1 : h;
}

// error reporting (set_error: declared in dg_filter_plan.h, defined in dg_engine.cpp)
#define DG_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess) return ::dg::set_error(DG_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(_e)); \
  } while (0)

// segment loading (dg_segment.cpp)
int load_segment(Context* ctx, const char* dir, Segment** out);
int segment_from_rows(Context* ctx, int64_t nrows, const int64_t* ts, int64_t istart, int64_t iend,
                      const dg_row_column* cols, int ncols, Segment** out);

// a failed enqueue inside a void launcher (e.g. the memset of look-back status): recorded per thread,
// returned as DG_ERR_DEVICE by the call's finish_call (dg_engine.cpp)
void note_launch_error(hipError_t e);
hipError_t take_launch_error();

// kernel launchers (dg_kernels.hip)
constexpr int kLz4ProfWords = 32;  // per-block phase stamps of the decoder (diagnostic builds of the call)
// blocks of one kind: wide (2 * kLzSeqPerCp sequences per checkpoint) or not
// flow blocks (wide & kLzFlow): flow_wgs > 0 caps the grid at that many persistent workgroups
void launch_lz4_decode(const Lz4Launch& L, int nblocks, int wide, int32_t* d_err, hipStream_t s, uint64_t* d_prof = nullptr,
                       int flow_wgs = 0);
void launch_lz4_light(const Lz4Launch& L, int nblocks, int32_t* d_err, hipStream_t s, uint64_t* d_prof = nullptr);
// run blocks (rx set); stage: 0 = read the input from L1/L2 (64 KiB of LDS per block, two per CU: beside
// another stream's LDS-heavy kernels), 1 = stage it in LDS when the launch is small (latency mode),
// 2 = stage it (a launch that has the GPU to itself)
void launch_lz4_run(const Lz4Launch& L, int nblocks, int stage, int32_t* d_err, hipStream_t s);
void launch_lzf_decode(const LzfJob* d_jobs, int njobs, int32_t* d_err, hipStream_t s);
void launch_vsize_expand(const VsJob* d_jobs, int njobs, int32_t max_rows, int32_t* d_err, hipStream_t s);
// one multi-value dimension's decoded row lists, validated before use (bit 2 of the error word)
struct MvCheck {
  ColView vals;
  ColView offs;
  int64_t rows;
  int64_t nvals;  // values stored (the offsets may not pass it)
  int64_t card;   // dictionary size (every value id must be below it)
};
// measurement probes (dg_debug_probe)
void launch_probe_copy(const void* in, void* out, int64_t bytes, hipStream_t s);
void launch_probe_chain(uint32_t* word, int n, hipStream_t s);
void launch_probe_gather(const uint64_t* words, const void* rec, int64_t n, uint64_t* out, hipStream_t s);
void launch_probe_fill(uint64_t* words, void* rec, int64_t n, hipStream_t s);
// DG_PROBE_SORT: n words sorted iters times by launch_radix_sort (events around the sort only);
// DG_PROBE_SORT_DEFER=d: key bits [d, 34) only, the check then on the sorted prefix
int probe_sort(int64_t n, int iters, double* ms, hipStream_t st);
void launch_mv_check(const MvCheck* d_jobs, int njobs, int32_t* d_err, hipStream_t s);
// VSizeLongSerde.getSerializedSize (VSizeLongSerde.java:61-65)
inline int64_t vsize_serialized(int bits, int64_t n) { return (bits * n + 7) / 8 + 4; }
// Concise words [off, off + len) whose first word starts at row row0 (null: 0), OR-ed into sets[target]
void launch_concise_or(const uint8_t* bm_base, const int64_t* d_off, const int32_t* d_len, const int32_t* d_target,
                       const int64_t* d_row0, int nbitmaps, uint32_t* const* d_sets, int64_t limit_bits, hipStream_t s);
// single Roaring containers (pieces): data at off, rows from row0, info as BmPiece; four per workgroup
void launch_roaring_pieces(const uint8_t* bm_base, const int64_t* d_off, const int64_t* d_row0, const int32_t* d_info,
                           const int32_t* d_target, int npieces, uint32_t* const* d_sets, int64_t limit_bits,
                           hipStream_t s);
void launch_roaring_or(const uint8_t* bm_base, const int64_t* d_off, const int32_t* d_len, const int32_t* d_target,
                       int nbitmaps, uint32_t* const* d_sets, int32_t* d_err, int64_t limit_bits, hipStream_t s);
void launch_filter_eval(const int32_t* d_prog, int prog_len, uint32_t* const* d_sets, uint32_t* out, int64_t nrows,
                        unsigned long long* d_count, hipStream_t s);
// ---- search query (dg_search.hip) ----
// One intersect-and-count job: a serialized bitmap (or a piece of one split at attach) of an accepted
// dictionary value, counted inside the selection bitset S of its segment into counts[slot].
struct SearchJob {
  const uint8_t* data;  // the bitmap's / piece's bytes in HBM
  const uint32_t* S;    // selection bitset of the segment's rows; null = every row
  int64_t nrows;        // rows of the segment (rows at or beyond it count nothing)
  int64_t row0;         // first row the piece covers (0 for a whole bitmap)
  int32_t len;          // bytes
  int32_t info;         // Roaring container piece: BmPiece::info
  int32_t slot;         // index into the call's counts
  int32_t pad;
};
constexpr int kSearchLdsCard = 8192;  // dictionaries up to this count in LDS (k_search_hist)
// the cursor plan of one (segment, dimension): occurrences of accepted ids over the rows S selects
struct SearchHist {
  ColView vals;            // dictionary ids (multi-value: the value lists)
  ColView offs;            // multi-value: rows + 1 offsets into vals; VIEW_ABSENT otherwise
  const uint32_t* S;       // null = every row
  const uint64_t* accept;  // bit per dictionary id
  unsigned long long* hist;  // [card] counters, zeroed
  int64_t nrows;
  int64_t nvals;           // multi-value: values stored
  uint32_t card;
  uint32_t pad;
};
// out = `in` (null = all rows) AND rows whose time lies in [t_lo, t_hi); *d_count += rows selected
void launch_search_time_and(ColView time, const uint32_t* in, int64_t nrows, int64_t t_lo, int64_t t_hi, uint32_t* out,
                            unsigned long long* d_count, hipStream_t s);
// jobs [0, n_small): at most 64 words, one wave each; [n_small, n_jobs): one workgroup each
void launch_search_concise_count(const SearchJob* d_jobs, int n_small, int n_jobs, unsigned long long* d_counts,
                                 hipStream_t s);
// jobs [0, n_whole): whole bitmaps, one workgroup each; [n_whole, n_jobs): single containers, one wave each
void launch_search_roaring_count(const SearchJob* d_jobs, int n_whole, int n_jobs, unsigned long long* d_counts,
                                 int32_t* d_err, hipStream_t s);
// the histogram of one (segment, dimension) and the gather of its accepted ids' counters into d_out[0, n_ids)
void launch_search_hist(const SearchHist& h, const int32_t* d_ids, int n_ids, unsigned long long* d_out, hipStream_t s);
// ---- scan query (dg_rows.hip) ----
// Tile of the selection -> row number compaction: kRowsTileWords 32-bit bitset words, one per thread
// (8192 rows per workgroup).
constexpr int kRowsTileWords = 256;
constexpr int kRowsTileRows = kRowsTileWords * 32;
// one fixed-width column of a gather launch: the kept rows' values go to out[0 .. keep) as int64 / double
// (8-byte views), float32 (4-byte views) or int32 dictionary ids (id views of any stored width)
struct RowsCol {
  ColView v;
  void* out;
};
// one multi-value column of one segment: the kept rows' value lists
struct RowsMv {
  ColView vals;          // the value ids
  ColView offs;          // rows + 1 offsets into vals
  const uint32_t* rows;  // kept row numbers (null: rows 0 .. keep - 1)
  int64_t keep;
  int64_t nvals;         // values stored (offsets are clamped to it)
  uint32_t* tile_off;    // [ceil(keep / 256)] values per tile of 256 kept rows, then their exclusive offsets
  int64_t* out_offs;     // [keep + 1] list starts in out_ids (k_rows_mv_copy)
  int32_t* out_ids;      // [out_cap]
  int64_t out_cap;
};
// S -> the first min(|S|, cap) selected rows, ascending, in rows; tile_cnt: ceil(ceil(nrows / 32) /
// kRowsTileWords) words; info (zeroed): [0] = |S|, [1] = rows kept, [2] / [3] = first / last kept row
void launch_rows_select(const uint32_t* S, int64_t nrows, uint64_t cap, uint32_t* tile_cnt, unsigned long long* info,
                        uint32_t* rows, hipStream_t s);
// every table entry's column gathered at the kept rows (rows null: rows 0 .. keep - 1) in one launch
void launch_rows_gather(const RowsCol* d_cols, int ncols, const uint32_t* rows, int64_t keep, hipStream_t s);
// m.tile_off = per-tile value counts scanned to offsets, info[0] = values of the kept rows
void launch_rows_mv_len(const RowsMv& m, unsigned long long* info, hipStream_t s);
void launch_rows_mv_copy(const RowsMv& m, hipStream_t s);
// ---- long-dimension encoding (dg_numdim.hip; Column::nd_*) ----
// mm (host-initialised to {~0, 0}): [0] = min, [1] = max of the rows as (value ^ sign) keys
void launch_nd_minmax(const ColView& v, int64_t nrows, unsigned long long* mm, hipStream_t s);
// words[r] = (uint64)(v[r] - vmin)
void launch_nd_words(const ColView& v, int64_t nrows, int64_t vmin, uint64_t* words, hipStream_t s);
// run heads of the n sorted words: tile_cnt (sort_tiles(n) entries) = the heads per tile of kSortTile,
// scanned to exclusive offsets; info[0] = their total, the cardinality
void launch_nd_unique_count(const uint64_t* words, int64_t n, uint32_t* tile_cnt, unsigned long long* info, hipStream_t s);
// vals[k] = word of the k-th run head + vmin, for k < card
void launch_nd_unique_emit(const uint64_t* words, int64_t n, const uint32_t* tile_off, int64_t vmin, int64_t* vals,
                           int64_t card, hipStream_t s);
// ids[r] = lower bound of v[r] in vals[0 .. card)
void launch_nd_encode(const ColView& v, int64_t nrows, const int64_t* vals, uint32_t card, uint32_t* ids, hipStream_t s);
// ---- derived columns (dg_expr.hip; Column::derived) ----
// the decoded views of a program's input columns (EX_INPUT arg indexes them)
struct ExprInputs {
  ColView v[kExprMaxInputs];
};
// out[r] = the checked program over row r for r < nrows (8-byte words; a FLOAT output: 4-byte float32); a row
// whose value depends on a long division by zero stores 0 and adds one to *poisoned (zeroed by the caller)
void launch_expr_eval(const ExprProg& p, const ExprInputs& in, int64_t nrows, void* out, unsigned long long* poisoned,
                      hipStream_t s);
// ---- first / last aggregators (dg_firstlast.hip) ----
// One segment's key column: keys[r] = ((((t(r) - t0) << rb) | p(r)) + 1) ^ sign, p(r) = p0 + r (ascending
// cursor; groupBy: p0 = the segment's row_base) or p0 - r (descending: p0 = nrows - 1).
struct FlKeyJob {
  ColView time;   // the segment's __time, every block decoded (VIEW_ABSENT: every row at t0)
  int64_t* keys;  // [nrows]
  int64_t t0;
  int64_t nrows;
  int64_t p0;
  int32_t rb;
  int32_t desc;
};
void launch_fl_keys(const FlKeyJob* d_jobs, int njobs, int64_t max_rows, hipStream_t s);
// A segment of a resolve: its rows' references are [row_base, row_base + nrows) and val[k] is the value
// column of the job's k-th first/last slot in this segment (VIEW_ABSENT: the segment lacks it).
struct FlSeg {
  uint32_t row_base;
  int32_t nrows;
  int32_t desc;
  int32_t pad;
  ColView val[kMaxAggs];
};
// Cells whose first/last slots hold winning keys: slot a of cell c at
// cells[c * cell_stride + (1 + a) * slot_stride] (accumulator tables: cell_stride = 1 + naggs, slot_stride = 1;
// a groupBy result: 1 and its capacity). n_ptr (optional): the cell count known on the device only.
struct FlResolveJob {
  uint64_t* cells;
  int64_t ncells;
  int64_t cell_stride, slot_stride;
  const uint32_t* n_ptr;
  const FlSeg* segs;  // ascending row_base
  int32_t nsegs;
  int32_t rb;
  int32_t abi;        // the slots are finalized (a groupBy result) and stay so
  int32_t nslots;
  int32_t slot[kMaxAggs];   // aggregator index of the k-th first/last slot
  int32_t okind[kMaxAggs];  // DG_AGG_LONG_SUM / DOUBLE_SUM / FLOAT_SUM: the value's type
};
void launch_fl_resolve(const FlResolveJob* d_jobs, int njobs, int64_t max_pairs, hipStream_t s);
// The row predicate of a filter leaf without a bitmap index (NumPred, dg_filter_plan.h) over a column:
// out: bitset words of rows [0, nrows) (bit r of word r >> 5); v: the decoded numeric column
// voff: row value offsets of a multi-value id column (VIEW_ABSENT otherwise); PRED_ID_SET over a
// multi-value column: has_lo = whether an empty row (the null value) matches
void launch_num_pred(ColView v, ColView voff, int64_t nrows, NumPred p, uint32_t* out, hipStream_t s);
// one record of accumulator slots, passed by value (a kernel argument: no staging copy)
struct SlotInit {
  uint64_t v[kMaxAggs + 1];
};
void launch_fill_u64(uint64_t* p, int64_t n_rows_of_slots, int slots_per_row, const SlotInit& init, hipStream_t s);
void launch_scan_agg(const ScanJob* d_jobs, const int32_t* d_tile_job, int ntiles, AggPlan plan, int topn, hipStream_t s);
// the tiles' records of the jobs with `part` folded into `out` (one workgroup per job, tree order)
void launch_scan_combine(const ScanJob* d_jobs, int njobs, AggPlan plan, hipStream_t s);
// topN aggregation with LDS-private dictionary-id ranges: workgroup (p, s) owns ids
// [p * range, (p + 1) * range) of segment s, scans every row of the segment and writes its range of
// the record table with plain stores (no HBM atomics). Applicable when the table needs at most
// kMaxIdRanges ranges; the caller skips the table fill.
constexpr int kPartLdsBytes = 144 * 1024;
constexpr int kMaxIdRanges = 64;
constexpr int kPartTargetGroups = 256;  // one workgroup per CU (the LDS table fills the CU)
inline int64_t topn_part_range(int naggs) { return kPartLdsBytes / (8 * (naggs + 1)); }
// row splits per (segment, id range); each split writes its own [card][1 + naggs] partial table
int topn_part_splits(int64_t max_card, int naggs, int njobs);
void launch_topn_part(const ScanJob* d_jobs, int njobs, int64_t max_card, AggPlan plan, int splits, hipStream_t s);
// topN aggregation by dictionary-id bins of 2^shift ids (radix partition of the rows, then one
// LDS table per bin); see dg_kernels.hip. bin_first[seg] = first global bin of segment seg,
// bin_seg[b] = segment of global bin b; hist/base/cursor: nbins words (hist zeroed by the caller);
// lid/vals: cap selected-row slots (vals is naggs x cap).
// topN bin index of a dimension column (Column::tix_*): bin b's rows are perm[base[b] .. base[b + 1])
// (base has bins + 1 entries), lid = each row's dictionary id & (2^shift - 1)
struct TopnIx {
  const uint32_t* perm;
  const uint16_t* lid;
  const uint32_t* base;
};
constexpr int kTopnIxShift = 8;  // ids per index bin: 256
void launch_topn_ix_build(const ScanJob* d_jobs, int seg, int64_t nrows, int shift, int nbins, uint32_t* d_cnt,
                          uint32_t* d_cursor, uint32_t* base, uint32_t* perm, uint16_t* lid, hipStream_t s);
void launch_topn_ix_reduce(const ScanJob* d_jobs, const TopnIx* d_ix, const int32_t* d_bin_first,
                           const int32_t* d_bin_seg, int nbins, int shift, AggPlan plan, hipStream_t s);
int topn_bin_shift(int naggs);
void launch_topn_bins(const ScanJob* d_jobs, const int32_t* d_tile_job, int ntiles, const int32_t* d_bin_first,
                      const int32_t* d_bin_seg, int nbins, int shift, uint32_t* d_hist, uint32_t* d_base,
                      uint32_t* d_cursor, AggPlan plan, uint16_t* d_lid, uint64_t* d_vals, int64_t cap, hipStream_t s);
// topN selection of one segment: K-th largest metric key (8-bit radix select over all touched ids,
// many workgroups per segment), candidate ids (key >= K-th) in id order, and the candidates'
// records gathered into a compact buffer for one read-back.
struct TopnSelJob {
  const uint64_t* table;  // [card][1 + naggs] accumulator records
  int64_t card;
  uint64_t* state;        // [0] = K-th key, [1] = aggregated rows, [2] = touched ids (zeroed by the host)
  int32_t* cand;          // candidate ids (capacity card)
  int32_t* ncand;
  uint64_t* gathered;     // [gather_cap][2 + naggs]: id, then the record of cand[0 .. gather_cap)
  uint64_t* keys;         // [card] metric keys (0 = untouched)
  uint32_t* hist;         // [8][256] radix histograms (zeroed by the host)
  uint64_t* rstate;       // [9][4] the radix choice after k levels: prefix, mask, keys still to take, done
                          // (k_topn_radix level k writes entry k, so each level replays one histogram)
  int32_t* blkcnt;        // [ceil(card / 1024)] candidates per workgroup
  uint16_t* order;        // [gather_cap] gather positions in builder order (filled when ncand <= 4096)
  int32_t gather_cap;
  // DimensionTopNMetricSpec: key of a touched id = its dictionary rank (smaller first), eligible when
  // lo <= id < hi and rank >= min_rank; rank == nullptr: every id has rank 0 (missing dimension)
  int32_t dim_mode;
  const int32_t* rank;
  int32_t lo, hi;
  int32_t min_rank;
  int32_t pad;
};
constexpr int kSelBlock = 1024;
constexpr int kTopnOrderCap = 4096;  // k_topn_order sorts at most this many candidates
// A topN ranked by a post-aggregator (dg_topn_run_post): the checked program and the output-side kind of every
// slot of a record (device encoding -> finalize_dev -> the ABI slot the program reads).
struct TopnMetricProg {
  PostAggProg p;
  int32_t okind[kMaxAggs];
};
// d_prog (device memory; NULL = the aggregator `metric`): the keys are the program's order keys instead
void launch_topn_select(const TopnSelJob* d_jobs, int njobs, int64_t max_card, int naggs, int metric, int metric_op,
                        int inverted, int threshold, const TopnMetricProg* d_prog, hipStream_t s);

constexpr int kTileRows = 2048;

// dg_sort.hip
// radix digits of up to 8 bits (9-bit digits on 4096-element tiles measured slower: 64-byte store runs);
// DG_RS_DIGIT_BITS: A/B builds
#ifndef DG_RS_DIGIT_BITS
#define DG_RS_DIGIT_BITS 8
#endif
constexpr int kMaxDigitBits = DG_RS_DIGIT_BITS;
constexpr int kMaxBins = 1 << kMaxDigitBits;
// longest run of equal sorted prefix the groupBy reduce orders in LDS (its halo on each side of a tile),
// and the planner's bound on the expected elements per prefix
constexpr int kDeferMaxRun = 64;
constexpr int kDeferLambda = kDeferMaxRun / 4;
// ... and on what the planner defers unasked: 1 / kDeferPlanInvLambda elements per prefix. The reduce pays
// for every element inside a run (its walk, and a second payload gather for a displaced one): measured on
// the headline, 0.04 per prefix leaves a gain of the pass saved, 0.64 none, 10 costs 2 ms.
constexpr int kDeferPlanInvLambda = 8;
constexpr int kRsMaxPasses = 8;  // 64 key bits at >= 8 bits per digit (rows of SortBufs::bin_total)
constexpr int kSortTile = 4096;  // elements per radix / run tile (256 threads x 16)
// groupBy reduce: waves per sort tile (each reduces its own 4096 / kRedWaves elements; one carry /
// open slot per wave)
#ifndef DG_RED_WAVES
#define DG_RED_WAVES 16
#endif
constexpr int kRedWaves = DG_RED_WAVES;
constexpr int kMaxCallSegs = 1024;  // segments of one sort-based call (row-ref bases live in LDS)
inline int sort_tiles(int64_t n) { return (int)std::max<int64_t>(1, (n + kSortTile - 1) / kSortTile); }
// selected rows -> (key, element index) in (segment, row) order + their aggregator inputs in
// sb->payload; sb->n[0] = selected rows
// selected rows (groupings of rows with multi-value dimensions) per keygen tile, and their total
void launch_gb_count(const GbJob* d_jobs, const int32_t* d_tile_job, int ntiles, uint32_t* tile_cnt, uint32_t* total,
                     bool multi, hipStream_t s);
// multi-value element count: per-tile counts (0xFFFFFFFF = saturated) and their 64-bit total
void launch_gb_count_total(const GbJob* d_jobs, const int32_t* d_tile_job, int ntiles, uint32_t* tile_cnt,
                           unsigned long long* total, hipStream_t s);
// all_rows >= 0: every row of the call's jobs is an element (no filter bitset, every row's time
// inside the interval, no multi-value dimension) and all_rows is their count: no count pass before
// the keygen
void launch_gb_keygen(const GbJob* d_jobs, const int32_t* d_tile_job, int ntiles, SortBufs* sb, AggPlan plan,
                      hipStream_t s, bool multi = false, int64_t all_rows = -1);
// The first pass's digit totals without a read of the elements: when every row of every segment is an
// element (all_rows) and the first digit's key bits lie inside the lowest key field, a single-value
// dimension's, the totals are a function of the segments' cached value counts (Column::vcnt) and the
// merged-dictionary maps. One CountJob per segment of the call; counts null = the segment lacks the
// dimension (its nrows rows carry null_gid) or has no rows.
struct CountJob {
  const uint32_t* counts;  // [card]: rows per dictionary id
  const int32_t* remap;    // local id -> merged id (null: identity)
  uint32_t card;
  uint32_t nrows;          // rows of a segment without the dimension (counts null)
  int32_t null_gid;
  int32_t pad;
};
struct CountTotals {
  const CountJob* jobs;  // device
  int njobs;
  int dim_shift;  // the field's shift inside the key
  uint32_t max_card;  // largest dictionary of the jobs (sizes the grid)
  uint32_t n;     // elements of the call (stored to sb->n[0] by the totals kernel)
};
constexpr int32_t kErrDictId = 16;  // bit of the call's device error word: a dictionary id >= its cardinality
constexpr int32_t kErrLzf = 32;     // bit of the call's device error word: k_lzf_decode refused a block
// bits of the first digit of a sort over key_bits key bits (0: no pass), and its passes
int radix_first_digit_bits(int key_bits);
int radix_pass_count(int key_bits);
// counts[v] = rows of `ids` below nrows whose id is v (counts zeroed here); an id >= card is not counted
// and raises kErrDictId; *sum = the counts' total (64-bit)
void launch_value_counts(const ColView& ids, int64_t nrows, uint32_t card, uint32_t* counts, unsigned long long* sum,
                         int32_t* d_err, hipStream_t s);
// stable LSD radix sort of sb->keys/refs[cur] on key bits [sb->defer_bits, key_bits); ct: the first pass's digit
// totals come from the value counts instead of k_rs_hist0
void launch_radix_sort(SortBufs* sb, int key_bits, hipStream_t s, const CountTotals* ct = nullptr);
// The one-clear control layout of SortBufs (its comment): sort_ctl_bytes = the region's size for a sort
// of key_bits key bits (those above sb->defer_bits) over sb->cap elements, sort_ctl_bind points n / bin_total / pass_status /
// red_status into it (lb_status becomes null), launch_sort_ctl_clear zeroes it and marks it clean.
size_t sort_ctl_bytes(const SortBufs* sb, int key_bits);
void sort_ctl_bind(SortBufs* sb, int key_bits, void* mem, size_t bytes);
void launch_sort_ctl_clear(SortBufs* sb, hipStream_t s);
// The keygen fused into the first radix pass: for a call whose every row is an element in row order
// (launch_gb_keygen's all_rows case) with no time view, single-value little-endian id views (or
// missing dimensions) and every payload column decoded in place, the sort word of element e is a
// function of e and the job table alone. launch_gb_sort_generated sets sb->n[0] = rows and sorts as
// launch_radix_sort does, its first pass (and that pass's digit totals) forming the words in
// registers from the id columns: no k_gb_keygen launch, no write and two reads of the words less.
// A job with a payload column the decoder did not write in place (a literal-only LZ4 block is viewed,
// not decoded) still needs its payload records: launch_gb_keygen_payload runs k_gb_keygen over that
// job's tiles [tile0, tile0 + ntiles) for the payload alone (an all_rows, row-ref call).
// radix_sort_generates: what the sort itself needs for it (packed words by row ref, at least one pass).
// Every id view of such a call holds at least 2^kRsGenMinBlockLog2 rows per block (64-KiB blocks of
// ids of at most 4 bytes hold 2^14), so a wave's share of a sort tile spans two blocks at the most.
constexpr int kRsGenMinBlockLog2 = 13;
bool radix_sort_generates(const SortBufs* sb, int key_bits, int64_t rows);
void launch_gb_keygen_payload(const GbJob* d_jobs, const int32_t* d_tile_job, int tile0, int ntiles, SortBufs* sb,
                              AggPlan plan, hipStream_t s);
void launch_gb_sort_generated(const GbJob* d_jobs, int njobs, int64_t rows, SortBufs* sb, int key_bits, hipStream_t s,
                              const CountTotals* ct = nullptr);
// run heads of the sorted keys: sb->run_cnt = per-tile offsets, sb->n[1] = runs
void launch_run_heads(SortBufs* sb, hipStream_t s);
// head_pos[g] = first sorted element of run g (after launch_run_heads)
void launch_run_mark(SortBufs* sb, uint32_t* head_pos, hipStream_t s);
// groupBy merge of the sorted rows: one record per run, out_keys[g] and slot s of group g at
// out_slots[s * cap + g] (SoA) in the ABI slot encoding; head_pos (null unless a floatSum needs it)
// = first sorted element of run g; floatSum slots are left to launch_fsum_runs. carry_g / open_g:
// sort_tiles(cap) entries, carry_slots: sort_tiles(cap) * (1 + naggs).
// sb->defer_bits > 0 (packed words): each tile first orders the runs of equal sorted prefix it holds; a
// run longer than kDeferMaxRun sets sb->n[2] and the result is then not to be used (the caller sorts
// classically and reduces again).
void launch_gb_reduce(SortBufs* sb, AggPlan plan, uint64_t* out_keys, uint64_t* out_slots, int64_t cap,
                      uint32_t* head_pos, int64_t* carry_g, uint64_t* carry_slots, int64_t* open_g, hipStream_t s);
// floatSum aggregator `agg` as the reference computes it: a float32 sum in row order per run and
// segment (FloatSumBufferAggregator.aggregate), segments combined in order with float adds
// (FloatSumAggregator.combine). groupBy: into out_slots[(1 + agg) * cap + g]; per-segment engines
// (out_slots == null): into the job's fs_out table.
void launch_fsum_runs(const GbJob* d_jobs, int njobs, int ntiles, SortBufs* sb, AggPlan plan, int agg,
                      const uint32_t* head_pos, uint64_t* out_slots, int64_t cap, hipStream_t s, int desc = 0);
// device slot encoding -> ABI encoding (finalize) of the aggregator slots [1 + a][cap] of n_ptr[0] groups
void launch_slots_finalize(uint64_t* slots, const uint32_t* n_ptr, int64_t cap, AggPlan plan, hipStream_t s);
// SoA slots [rec][cap] -> AoS records [n][rec]
void launch_soa_to_aos(const uint64_t* soa, int64_t cap, int64_t n, int rec, uint64_t* aos, hipStream_t s);
// a result laid out for `cap` records compacted to its n groups: keys [n], slots [rec][n] (16-byte copies)
void launch_result_compact(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t n, int rec, uint64_t* keys2,
                           uint64_t* slots2, hipStream_t s);
// dg_hash.hip — the opt-in hash grouper (BufferHashGrouper.java:38-133 over ByteBufferHashTable.java:286-327):
// an open-addressing table in HBM, empty key = ~0ull (keys of <= 63 bits), linear probing from a mixed hash.
constexpr uint64_t kHashEmpty = ~0ull;
constexpr int32_t kErrTableFull = 8;  // bit of the call's device error word (CallScratch::d_err)
constexpr int kHashTile = 4096;       // keygen elements per insert workgroup
struct HashTable {
  uint64_t* keys;           // [capacity]
  uint64_t* slots;          // [1 + naggs][capacity] (slot-major): rows, then the values in the device slot encoding
  int64_t capacity;         // power of two
  int log2_capacity;
  int64_t max_groups;       // bufferGrouperMaxSize: a claim beyond it fails the call (Groupers.HASH_TABLE_FULL)
  unsigned long long* ctr;  // [0] groups claimed, [1] LDS entries flushed, [2] elements that bypassed a full LDS table
};
// table slots for max_groups groups: the next power of two >= max_groups / 0.7 (ByteBufferHashTable's
// default max load factor, AbstractBufferHashGrouper.DEFAULT_MAX_LOAD_FACTOR)
inline int64_t hash_capacity(int64_t max_groups) {
  int64_t c = 1;
  while (c * 7 < max_groups * 10) c <<= 1;
  return c;
}
// The grouper and group limit of one call: explicit opts first, then (grouper only) the DG_GROUPER
// environment switch ("hash" / "sort", anything else ignored), then the context's defaults.
// max_groups 0 = unlimited.
struct GrouperChoice {
  int32_t grouper;
  int64_t max_groups;
};
inline GrouperChoice resolve_grouper(const dg_groupby_opts* opts, int32_t ctx_grouper, int64_t ctx_max_groups,
                                     const char* env) {
  GrouperChoice c{ctx_grouper, ctx_max_groups > 0 ? ctx_max_groups : 0};
  if (env && !strcmp(env, "hash")) c.grouper = DG_GROUPER_HASH;
  else if (env && !strcmp(env, "sort")) c.grouper = DG_GROUPER_SORT;
  if (opts && opts->grouper >= 0) c.grouper = opts->grouper;
  if (opts && opts->max_groups > 0) c.max_groups = opts->max_groups;
  return c;
}
// keys = empty, slots = the aggregators' identities, counters = 0
void launch_gb_hash_fill(const HashTable& ht, AggPlan plan, hipStream_t s);
// the keygen's elements (sb, at most elem_cap of them) aggregated per tile in LDS and upserted into ht;
// err: the call's device error word (kErrTableFull)
void launch_gb_hash_insert(const SortBufs* sb, int64_t elem_cap, const HashTable& ht, AggPlan plan, int32_t* err,
                           hipStream_t s);
// occupied positions -> gsb's sort words [key | position] (or keys + refs), gsb->n[0] = their count (<= ng)
void launch_gb_hash_collect(const HashTable& ht, SortBufs* gsb, int64_t ng, hipStream_t s);
// the sorted words' table records -> out_keys[g], out_slots[s * cap + g] (rows, then ABI-encoded values)
void launch_gb_hash_emit(const SortBufs* gsb, int64_t ng, const HashTable& ht, AggPlan plan, uint64_t* out_keys,
                         uint64_t* out_slots, int64_t cap, hipStream_t s);

// groups [start, start + count): key fields -> bucket index and merged ids (int32 per dimension)
struct KeyLayout {
  int32_t ndims;
  int32_t bucket_shift, bucket_bits;
  int32_t dim_shift[kMaxGroupDims];
  int32_t dim_bits[kMaxGroupDims];
};
void launch_gb_unpack(const uint64_t* keys, int64_t start, int64_t count, KeyLayout lay, int64_t* bucket, int32_t* ids,
                      hipStream_t s);
// groups [start, start + count) packed for one device-to-host copy: times, ids, AoS values (see dg_sort.hip)
void launch_gb_fetch_pack(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t start, int64_t count,
                          KeyLayout lay, int naggs, int64_t universal, int64_t bucket0, int64_t period,
                          const int64_t* bounds, int64_t* times, int32_t* ids, uint64_t* vals, hipStream_t s);
// cross-device merge: keys of layout lin -> layout lout (bucket index + bucket_delta, ids through maps)
struct RekeyMaps {
  const int32_t* m[kMaxGroupDims];
};
void launch_gb_rekey(const uint64_t* in, int64_t n, KeyLayout lin, KeyLayout lout, int64_t bucket_delta,
                     RekeyMaps maps, uint64_t* out, hipStream_t s);
void launch_lower_bound(const uint64_t* keys, int64_t n, const uint64_t* split, int nsplit, int64_t* pos, hipStream_t s);
// sort input of a merge (refs = record index, sb->n[0] = n)
void launch_merge_load(const uint64_t* keys, int64_t n, SortBufs* sb, hipStream_t s);
// limit push-down: key fields (bucket, dimensions) re-packed most significant first in the push-down
// order; a field's value goes through its rank table (if any) and is complemented when descending
struct LimitOrder {
  int32_t nfields;
  int32_t in_shift[kMaxGroupDims + 1];
  int32_t bits[kMaxGroupDims + 1];
  int32_t out_shift[kMaxGroupDims + 1];
  int32_t desc[kMaxGroupDims + 1];
  const int32_t* rank[kMaxGroupDims + 1];
};
void launch_limit_load(const uint64_t* keys, int64_t n, const LimitOrder& o, SortBufs* sb, hipStream_t s);
// the first m elements of the sorted order: keys[ref] and the [rec][cap] slot-major records -> [rec][ocap]
void launch_limit_gather(const SortBufs* sb, int64_t m, const uint64_t* keys, const uint64_t* slots, int64_t cap,
                         int rec, uint64_t* okeys, uint64_t* oslots, int64_t ocap, hipStream_t s);
// dg_post.hip — groupBy post-processing on a resident result (dg_result_post_process): the having
// tree as a postfix program over the groups' ABI-encoded slots and key fields, and the limit spec's
// comparator chain as 64-bit sort words.
constexpr int kPostMaxOps = DG_HAVING_MAX_OPS;
constexpr int kPostMaxStack = 32;  // operands alive at once (a bit stack in one register pair)
struct PostHaving {
  int32_t n;
  int32_t op[kPostMaxOps];    // DG_HAVING_*
  int32_t arg[kPostMaxOps];   // AND / OR: operands; AGG_RANGE: slot row (1 + aggregator); DIM_EQ: the field's shift
  int32_t kind[kPostMaxOps];  // AGG_RANGE: DG_AGG_*; DIM_EQ: the field's bits
  uint64_t lo[kPostMaxOps];   // AGG_RANGE: the closed order-key interval; DIM_EQ: lo = the id
  uint64_t hi[kPostMaxOps];
};
// sel[ceil(n / 32) + 2]: bit g = the program accepts group g (bits at or past n clear)
// (post: the result's post-aggregator columns [n_cols][cap], read by AGG_RANGE ops of kind >= kPostColKind)
void launch_post_having(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t n, const PostHaving& p,
                        const uint64_t* post, uint32_t* sel, hipStream_t s);
// One sort word: fields most significant first, each a key field (bucket / dimension id, through its
// rank table if any), an aggregator's 64-bit order key or a float aggregator's 32-bit one;
// a descending field is complemented within its bits.
constexpr int kPostWordFields = 16;
enum { POST_F_KEY = 0, POST_F_AGG64 = 1, POST_F_AGG32 = 2 };
struct PostField {
  int32_t type;      // POST_F_*
  int32_t bits;
  int32_t in_shift;  // key field: its shift inside the group's key
  int32_t out_shift;
  int32_t desc;
  int32_t slot;      // aggregator field: slot row (1 + aggregator)
  int32_t kind;      // aggregator field: DG_AGG_*
  int32_t pad;
  const int32_t* rank;
};
struct PostWord {
  int32_t nfields;
  int32_t bits;  // of the whole word (the sort's key_bits)
  PostField f[kPostWordFields];
};
// kout[i] = word w of group g = refs_in ? refs_in[i] : i, for i < count (count = info ? info[1] : n);
// refs_out (if given) [i] = g; n_out[0] = count
void launch_post_sort_word(const uint64_t* keys, const uint64_t* slots, int64_t cap, int64_t n,
                           const unsigned long long* info, const uint32_t* refs_in, const PostWord& w,
                           const uint64_t* post, uint64_t* kout, uint32_t* refs_out, uint32_t* n_out, hipStream_t s);
// Post-aggregator columns (dg_result_post_aggregate): out[c][g] = program c over group g's slots, g < n;
// d_progs: ncols checked programs in device memory. A field / having kind of kPostColKind + PA_ORDER_* names a
// post column in place of an aggregator slot.
constexpr int kPostColKind = 64;
void launch_post_eval(const uint64_t* slots, int64_t cap, int64_t n, const PostAggProg* d_progs, int ncols, uint64_t* out,
                      hipStream_t s);
// one record per run of the sorted merge input, partial values combined in order (device encoding,
// SoA slots [rec][cap])
void launch_merge_reduce(SortBufs* sb, const uint32_t* head_pos, const uint64_t* in_slots, AggPlan plan, int64_t cap,
                         uint64_t* out_keys, uint64_t* out_slots, hipStream_t s);

}  // namespace dg
