/*
 * druidgpu.h — C-ABI of the MI355X segment scan-and-aggregate engine.
 *
 * This is the drop-in boundary a JNI shim binds. Every entry point replaces
 * one reference interface on the historical's per-segment query path (paths relative to the
 * reference root; processing/... = processing/src/main/java/org/apache/druid/...):
 *
 *   dg_segment_attach        <- IndexIO.loadIndex / V9IndexLoader.load (processing/.../segment/IndexIO.java:569-663)
 *                               + Segment.asQueryableIndex/asStorageAdapter (processing/.../segment/Segment.java:30-35)
 *   dg_segment_release       <- QueryableIndex.close / ReferenceCountingSegment (SmooshedFileMapper.close)
 *   dg_segment_time_bounds   <- StorageAdapter.getMinTime / getMaxTime (processing/.../segment/StorageAdapter.java:33-80)
 *   dg_segment_dim_*         <- StorageAdapter.getDimensionCardinality, DimensionSelector.lookupName,
 *                               GenericIndexed.get (processing/.../segment/data/GenericIndexed.java:479-492)
 *   dg_filter_bitmap         <- Filter.getBitmapResult over BitmapIndexSelector
 *                               (processing/.../query/filter/Filter.java:28-110; segment/filter/{Selector,In,Bound,
 *                               And,Or,Not}Filter.java) as used by QueryableIndexStorageAdapter.makeCursors (:244-299)
 *   dg_timeseries_run        <- TimeseriesQueryRunnerFactory.createRunner(segment).run
 *                               (processing/.../query/timeseries/TimeseriesQueryRunnerFactory.java:93-105,
 *                               TimeseriesQueryEngine.java:40-111)
 *   dg_topn_run              <- TopNQueryRunnerFactory.createRunner(segment).run (query/topn/TopNQueryRunnerFactory.java:61-90,
 *                               TopNQueryEngine.java:60-160 -> PooledTopNAlgorithm + TopNNumericResultBuilder)
 *   dg_topn_run_opts         <- the same over a LONG / FLOAT / DOUBLE column: TopNQueryEngine.getMapFn (:141-148) ->
 *                               DimExtractionTopNAlgorithm + NumericTopNColumnSelectorStrategy
 *                               (query/topn/types/NumericTopNColumnSelectorStrategy.java:81-171)
 *   dg_segment_set_dim_order <- StringComparator.compare over one dictionary (query/ordering/StringComparators.java),
 *                               the order DimensionTopNMetricSpec / TopNLexicographicResultBuilder ranks values by
 *   dg_topn_merge            <- TopNBinaryFn.apply fold of QueryRunnerFactory.mergeRunners (query/topn/TopNBinaryFn.java:75-135)
 *   dg_groupby_run           <- GroupByStrategyV2.process -> GroupByQueryEngineV2.process per segment
 *                               (query/groupby/strategy/GroupByStrategyV2.java:472-477, epinephelinae/GroupByQueryEngineV2.java:91-187)
 *                               + GroupByStrategyV2.mergeRunners -> GroupByMergingQueryRunnerV2.run (:170-290)
 *   dg_groupby_run_opts      <- the same under GroupByQueryConfig's forceHashAggregation / bufferGrouperMaxSize
 *                               (query/groupby/GroupByQueryConfig.java:35-40): BufferHashGrouper over ByteBufferHashTable
 *                               (epinephelinae/BufferHashGrouper.java:38-133, ByteBufferHashTable.java:286-327)
 *   dg_groupby_run_dims      <- the same with DimensionSpec.getOutputType per dimension (query/dimension/
 *                               DefaultDimensionSpec.java:68-78): LONG columns grouped by value as
 *                               GroupByStrategyFactory -> LongGroupByColumnSelectorStrategy does
 *                               (epinephelinae/GroupByQueryEngineV2.java:235-260)
 *   dg_search_run            <- SearchQueryRunnerFactory.createRunner(segment).run: the counting of SearchQueryRunner.run
 *                               (query/search/SearchQueryRunner.java:207-260) under UseIndexesStrategy.getExecutionPlan
 *                               (UseIndexesStrategy.java:66-109): IndexOnlyExecutor.execute (:236-281) over
 *                               makeTimeFilteredBitmap (:143-219), or CursorBasedExecutor with
 *                               StringSearchColumnSelectorStrategy.updateSearchResultSet (SearchQueryRunner.java:118-141)
 *   dg_rows_run / dg_rowset_* <- ScanQueryRunnerFactory.createRunner(segment).run: ScanQueryEngine.process
 *                               (query/scan/ScanQueryEngine.java:59-264) over the call's segments with the shared
 *                               limit of mergeRunners (ScanQueryRunnerFactory.java:64-96); the rowset is the
 *                               columnar form of the ScanResultValue batches (ScanResultValue.java)
 *   dg_topn_run_post / dg_topn_merge_post
 *                            <- the same two for a NumericTopNMetricSpec that names a post-aggregator:
 *                               TopNNumericResultBuilder.addEntry (query/topn/TopNNumericResultBuilder.java:112-183)
 *                               and TopNBinaryFn (TopNBinaryFn.java:65-71,97-110) compute it before they rank
 *   dg_result_post_aggregate <- the post-aggregators GroupByQuery.postProcess decides on, which
 *                               GroupByStrategyV2.mergeResults (strategy/GroupByStrategyV2.java:286-300) computes first
 *                               (query/aggregation/post/{Arithmetic,FieldAccess,FinalizingFieldAccess,Constant,
 *                               DoubleGreatest,DoubleLeast,LongGreatest,LongLeast}PostAggregator.java)
 *   dg_result_*              <- the merged grouper's sorted iterator (ConcurrentGrouper.iterator(true))
 *   dg_result_export / dg_keys_partition / dg_merge
 *                            <- QueryRunnerFactory.mergeRunners across devices (query/QueryRunnerFactory.java:62):
 *                               GroupByMergingQueryRunnerV2 semantics over the devices' merged groups
 *   dg_groupby_merge_devices <- the same within one process: the library moves key ranges between devices itself
 *   dg_timeseries_merge      <- TimeseriesBinaryFn fold of runners' results (query/timeseries/TimeseriesBinaryFn.java:67-70)
 *   dg_records_pack          <- BufferAggregator.get* record layout (query/aggregation/BufferAggregator.java:35-199)
 *
 * Segment arrays: every *_run takes n_segs segments that are attached to the SAME context (device)
 * and runs them as one batched launch sequence; results stay per segment, exactly as the
 * reference's per-segment runners return them (cross-segment merging is QueryRunnerFactory.mergeRunners,
 * done by the host layer / RCCL, see incubator-druid_amd/runners.py and distributed.py).
 *
 * Conventions: 0 = DG_OK, otherwise a DG_ERR_* code and dg_last_error() (thread-local) describes it.
 * All output buffers are caller-allocated host memory. No callbacks into the caller. Every entry
 * point is safe to call concurrently for different segments; calls on one context serialize on
 * that context's HIP stream. Only the reference's default null mode is implemented
 * (druid.generic.useDefaultValueForNull=true, common/config/NullHandling.java:34,54): anything else
 * is the caller's problem (the Java shim keeps its CPU path, DG_ERR_UNSUPPORTED).
 */
#ifndef DRUIDGPU_H
#define DRUIDGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_ABI_VERSION 16

/* status codes (the JNI shim maps them to the reference's exceptions) */
#define DG_OK 0
#define DG_ERR_FORMAT 1      /* IAE / ISE on malformed segment bytes (GenericIndexed.java:131-149) */
#define DG_ERR_UNSUPPORTED 2 /* shape not implemented on GPU: caller keeps its CPU engine */
#define DG_ERR_OOM 3         /* device allocation failed */
#define DG_ERR_INTERRUPTED 4 /* QueryInterruptedException (BaseQuery.checkInterrupted, BaseQuery.java:46-51) */
#define DG_ERR_TABLE_FULL 5  /* Groupers.HASH_TABLE_FULL (Groupers.java:36-40) */
#define DG_ERR_ARG 6         /* IllegalArgumentException */
#define DG_ERR_DEVICE 7      /* HIP runtime failure */
#define DG_ERR_NOT_FOUND 8   /* SegmentMissingException (TimeseriesQueryEngine.java:42-46) */
#define DG_ERR_TIMEOUT 9     /* QueryInterruptedException(TimeoutException): "Query timeout" (ChainedExecutionQueryRunner.java:164-167,
                                QueryInterruptedException.java:46) */

/* column types (ValueType, processing/.../segment/column/ValueType.java) */
#define DG_COL_MISSING 0
#define DG_COL_LONG 1
#define DG_COL_FLOAT 2
#define DG_COL_DOUBLE 3
#define DG_COL_STRING 4      /* single- or multi-value (V3, legacy compressed or uncompressed multi-value:
                                filters, topN per value and groupBy explode all run on it) */
#define DG_COL_UNSUPPORTED 5 /* complex column / unsupported codec */

/* aggregator kinds (query/aggregation/...AggregatorFactory.java) */
#define DG_AGG_COUNT 0
#define DG_AGG_LONG_SUM 1
#define DG_AGG_DOUBLE_SUM 2
#define DG_AGG_FLOAT_SUM 3
#define DG_AGG_LONG_MIN 4
#define DG_AGG_LONG_MAX 5
#define DG_AGG_DOUBLE_MIN 6
#define DG_AGG_DOUBLE_MAX 7
#define DG_AGG_FLOAT_MIN 8
#define DG_AGG_FLOAT_MAX 9
/* First / last aggregators (query/aggregation/first/{Long,Double,Float}FirstAggregatorFactory.java,
 * query/aggregation/last/{Long,Double,Float}LastAggregatorFactory.java): the value at the earliest /
 * latest __time of the cell's rows. The reference's buffer is a 16-byte (time, value) pair
 * (SerializablePair<Long, ...>): first/LongFirstBufferAggregator.java:48-56 updates it when
 * time < firstTime (init (Long.MAX_VALUE, 0): of the rows sharing the smallest time the one the cursor
 * reaches first wins), last/LongLastBufferAggregator.java:50-56 when time >= lastTime (init
 * (Long.MIN_VALUE, 0): of the rows sharing the largest time the one the cursor reaches last wins); a
 * descending scan (dg_scan.descending, timeseries and topN) reverses the cursor. Here the pair is two
 * aggregator entries: the first/last entry's slot holds the pair's value (rhs: int64, double, or float32 in
 * the low 4 bytes; an empty cell holds 0) and the entry directly after it MUST be DG_AGG_PAIR_TIME, whose
 * int64 slot holds the pair's time (lhs: the smallest / largest __time of the cell's rows; an empty cell
 * holds Long.MAX_VALUE / Long.MIN_VALUE). The DG_AGG_PAIR_TIME entry has a NULL field and no filter of
 * its own: it inherits its pair's (a FilteredAggregatorFactory wraps the whole pair). A DG_AGG_PAIR_TIME
 * anywhere else, or a first/last entry without it, is DG_ERR_ARG. A pair therefore costs two of the 16
 * aggregator entries of a call. dg_records_pack lays the reference's 16-byte [time][value] record out with
 * the two entries' offsets. Merges combine a pair by the factories' rule
 * (LongFirstAggregatorFactory.java:103-112: lhs.time <= rhs.time ? lhs : rhs;
 * LongLastAggregatorFactory.java:107: lhs.time > rhs.time ? lhs : rhs) and order by the value
 * (getComparator: Longs / Doubles / Floats.compare of rhs). A call whose times and rows do not fit the
 * engine's 63-bit (time, cursor position) key — bits(max time - min time) + bits(rows - 1) > 63 — is
 * DG_ERR_UNSUPPORTED, as are the device-side groupBy merges (dg_keyspace_bits, dg_result_export, dg_merge,
 * dg_groupby_merge_devices) of these kinds. */
#define DG_AGG_LONG_FIRST 10
#define DG_AGG_LONG_LAST 11
#define DG_AGG_DOUBLE_FIRST 12
#define DG_AGG_DOUBLE_LAST 13
#define DG_AGG_FLOAT_FIRST 14
#define DG_AGG_FLOAT_LAST 15
#define DG_AGG_PAIR_TIME 16

/* filter node kinds (query/filter/...DimFilter.java -> segment/filter/...Filter.java) */
#define DG_F_AND 1
#define DG_F_OR 2
#define DG_F_NOT 3
#define DG_F_SELECTOR 4
#define DG_F_IN 5
#define DG_F_BOUND 6

/* string orderings (query/ordering/StringComparators.java): bound filters use LEXICOGRAPHIC / NUMERIC,
 * dimension-ordered topN all four */
#define DG_ORDER_LEXICOGRAPHIC 0
#define DG_ORDER_NUMERIC 1
#define DG_ORDER_ALPHANUMERIC 2
#define DG_ORDER_STRLEN 3

typedef struct dg_context dg_context;
typedef struct dg_segment dg_segment;
typedef struct dg_result dg_result;

/*
 * One filter node. A filter is an array of nodes in prefix order: an AND/OR node is followed by
 * its n_children subtrees, a NOT node by exactly one subtree. Strings are NUL-terminated UTF-8;
 * a NULL value pointer means the null value ("" in default null mode). A leaf on a string column
 * runs on its bitmap index; a leaf on a long / float / double column (no bitmap index) is the
 * reference's row post-filter (QueryableIndexStorageAdapter.java:244-260, FilteredOffset.java:40-105)
 * with its ValueMatcher semantics: selector / in values parsed as getExactLongFromDecimalString or
 * Floats/Doubles.tryParse, NUMERIC bounds as BoundDimFilter's long / float / double predicates,
 * LEXICOGRAPHIC bounds on long columns over String.valueOf(value); other orderings on numeric
 * columns -> DG_ERR_UNSUPPORTED.
 */
typedef struct {
  int32_t kind;
  int32_t n_children;
  const char* dimension;
  const char* const* values; /* SELECTOR: values[0]; IN: values[0..n_values) */
  int32_t n_values;
  const char* lower;         /* BOUND: NULL = no bound */
  const char* upper;
  int32_t lower_strict;
  int32_t upper_strict;
  int32_t ordering;          /* DG_ORDER_* */
} dg_filter;

/* AggregatorFactory (name is the caller's business; field is the input column, NULL for count).
 * filter / n_filter: FilteredAggregatorFactory (query/aggregation/FilteredAggregatorFactory.java:56-73,
 * FilteredBufferAggregator.java:45-50): the aggregator takes a cursor row only when the filter
 * (same node encoding as dg_scan.filter) matches it; NULL / 0 = unfiltered. */
typedef struct {
  int32_t kind;
  const char* field;
  const dg_filter* filter;
  int32_t n_filter;
} dg_agg;

/*
 * The scan common to all three query types (what makeCursors receives:
 * CursorFactory.makeCursors(filter, interval, virtualColumns, gran, descending, metrics),
 * processing/.../segment/CursorFactory.java:32-42).
 * Granularity: period_ms == 0 is ALL; otherwise a fixed-length UTC period with bucket starts at
 * origin_ms + k * period_ms (PeriodGranularity.truncateMillisPeriod, PeriodGranularity.java:411-428).
 * Calendar granularities (months, years, periods in a time zone, compound periods: PeriodGranularity
 * with Joda chronology arithmetic, PeriodGranularity.java:212-410) are given as the bucket list
 * gran.getIterable(interval) yields (Granularity.java:176-240): bucket_starts[0..n_bucket_starts)
 * = the starts followed by the end of the last bucket (strictly ascending, the last end at or past the
 * interval end; the first start may lie after the interval start, rows before it are in no bucket),
 * period_ms = 0; bucket k = [bucket_starts[k], bucket_starts[k + 1]). The Java shim computes it
 * with the query's own Granularity object. In dg_keyspace / dg_merge such a granularity is the
 * grid period_ms = 1 over bucket indices into that list.
 * seg_bounds (calendar only, optional): per segment of the call two instants, {gran.bucketStart(s),
 * gran.bucketEnd(maxTime)} with s = max(interval start, minTime): where the segment's iterable starts
 * and where its dataInterval ends (QueryableIndexStorageAdapter.java:367-372). Both truncate from
 * the origin, so they can leave the listed buckets: bucketEnd past the end of the listed bucket that
 * holds maxTime (an origin whose day clamps: P1M from Jan 31), bucketStart after s (the hours branch
 * before its origin, PeriodGranularity.java:313-326: rows in [s, bucketStart(s)) are in no cursor).
 * NULL = the listed bucket ends and no clipping at the start.
 * descending: CursorFactory.makeCursors(..., descending) (QueryableIndexStorageAdapter.java:378-424):
 * cursors in descending time order and each cursor's rows last to first (order-dependent floatSum);
 * timeseries / topN write their per-segment buckets in that order. groupBy ignores it (its engine
 * always asks for ascending cursors, GroupByQueryEngineV2.java:108-115).
 */
typedef struct {
  int64_t interval_start; /* [start, end) epoch millis */
  int64_t interval_end;
  int64_t period_ms;
  int64_t origin_ms;
  const dg_filter* filter; /* NULL / n_filter == 0: no filter */
  int32_t n_filter;
  const dg_agg* aggs;
  int32_t n_aggs;
  /* optional cancellation flag (Thread.interrupt / QueryWatcher cancel, BaseQuery.checkInterrupted,
     BaseQuery.java:46-51): polled between every launch group and while the call waits for the device;
     non-zero => DG_ERR_INTERRUPTED. Work already queued on the device finishes before the call
     returns, so the context is ready for its next call. */
  const volatile int32_t* cancel;
  const int64_t* bucket_starts;   /* calendar granularity (see above); NULL = period_ms grid */
  int32_t n_bucket_starts;
  int32_t descending;
  const int64_t* seg_bounds;      /* calendar granularity: 2 per segment (see above), or NULL */
  /* since ABI 14: the query context's "timeout" in ms (QueryContexts.getTimeout, ChainedExecutionQueryRunner
     futures.get(timeout), ChainedExecutionQueryRunner.java:150-167), measured from the call's start and
     checked where `cancel` is; <= 0: none. Past it => DG_ERR_TIMEOUT. */
  int64_t timeout_ms;
} dg_scan;

/* QueryMetrics counters (query/QueryMetrics.java:295-306) + device timings */
typedef struct {
  int64_t segment_rows;      /* reportSegmentRows */
  int64_t pre_filtered_rows; /* reportPreFilteredRows: rows passing the bitmap filter */
  int64_t selected_rows;     /* rows aggregated (filter AND interval) */
  int64_t bytes_read;        /* algorithmic HBM bytes of the column blocks / bitmaps scanned */
  double bitmap_ms;          /* reportBitmapConstructionTime (device time) */
  double decode_ms;          /* column decode kernels */
  double aggregate_ms;       /* aggregation kernels (all of them, groupBy: keygen + sort + reduce) */
  double total_ms;           /* whole call, host wall */
  /* groupBy phases (device time) and their element counts */
  double keygen_ms;          /* selected rows -> (key, row ref) */
  double sort_ms;            /* radix passes (hash grouper: the table insert) */
  double reduce_ms;          /* run heads + segmented reduce + floatSum pass + finalize (hash grouper: the group-count
                                read-back, collect, group sort and emit) */
  int32_t sort_passes;
  int32_t key_bits;
  int64_t groups;            /* groupBy: merged groups; topN: the candidates its selection kept over every result
                                list (ids whose metric key >= the list's K-th largest key) */
  /* groupBy: payload columns decoded in place on the side stream, overlapping the key build + sort */
  double decode_side_ms;     /* device time of those decodes (their own stream) */
  int64_t bytes_side;        /* their algorithmic bytes (part of bytes_read) */
  /* the general LZ4 decoder (token-dense blocks: 8-byte value runs, noisy doubles), both streams: device
     time of its launches, the stored bytes and number of the blocks it decoded, and its launches */
  double lz4_general_ms;
  int64_t lz4_general_bytes;
  int32_t lz4_general_blocks;
  int32_t lz4_general_launches;
  /* filter bitmaps: serialized bitmap bytes read + row bitsets written and read (since ABI 11) */
  int64_t bitmap_bytes;
  /* since ABI 12: the groupBy reduce kernels alone (reduce_ms also holds the wait for the side-stream
     payload decode) */
  double reduce_kernel_ms;
  /* since ABI 13: timeseries LZ4 blocks whose decode was fused with their aggregator (the decoder
     folded the block's values into its bucket's slot and wrote no decoded image) */
  int64_t lz4_fused_blocks;
  /* the wall time the general decoder ran on either stream (the union of its main- and side-stream
     spans; lz4_general_ms is their sum) */
  double lz4_general_wall_ms;
  /* since ABI 16: of the general decoder's blocks, those decoded by its flow kernel (k_lz4_decode_flow)
     and their stored bytes; the rest went to k_lz4_decode */
  int64_t lz4_flow_blocks;
  int64_t lz4_flow_bytes;
} dg_metrics;

/* Aggregate values are returned in 8-byte slots: int64 for count/long*, double for double*,
 * and for float* a float32 in the first 4 bytes of the slot (rest zero). */

/* ---- library / context ---- */
const char* dg_last_error(void);
int dg_abi_version(void);
int dg_device_count(int* out);
int dg_context_create(int device, dg_context** out);
void dg_context_release(dg_context* ctx);
/* Bind the context's work to an existing HIP stream (e.g. torch's current stream); NULL resets. */
int dg_context_set_stream(dg_context* ctx, void* hip_stream);
/* Resource limits of the context's calls (the processing-buffer budget a historical configures,
 * DruidProcessingConfig / GroupByQueryConfig; exceeding one is answered DG_ERR_UNSUPPORTED before any
 * buffer is sized, so the Java factory keeps its CPU engine). value <= 0 restores the default.
 *   DG_LIMIT_GROUP_ELEMENTS: sort elements of one groupBy call (rows, or for multi-value dimensions
 *   rows x the product of their value-list lengths, GroupByQueryEngineV2.java:480-540); never more
 *   than 2^32 - 64 (element indices are 32-bit). */
#define DG_LIMIT_GROUP_ELEMENTS 1
/*   DG_LIMIT_GROUPER: the grouper dg_groupby_run uses, a DG_GROUPER_* value (the context's
 *   forceHashAggregation default, GroupByQueryConfig.java:35-40,179-200); <= 0: the sort.
 *   DG_LIMIT_GROUPER_MAX_GROUPS: bufferGrouperMaxSize, the most groups one groupBy call may build; a
 *   call that finds more fails with DG_ERR_TABLE_FULL; <= 0: unlimited. */
#define DG_LIMIT_GROUPER 2
#define DG_LIMIT_GROUPER_MAX_GROUPS 3
int dg_context_set_limit(dg_context* ctx, int32_t which, int64_t value);

/* ---- segments ---- */
int dg_segment_attach(dg_context* ctx, const char* segment_dir, dg_segment** out);
void dg_segment_release(dg_segment* seg);
/* In-memory (realtime) segment: the rows of an IncrementalIndex queried like a persisted segment
 * (IncrementalIndexStorageAdapter, processing/.../segment/incremental/IncrementalIndexStorageAdapter.java:
 * the index's facts in its iteration order, TimeAndDims order: time ascending). Rows are copied into
 * HBM as flat columns (__time from `timestamps`); a string dimension comes as the index's
 * DimensionDictionary (values by id in insertion order, NULL or "" = null) plus one id per row and is
 * re-sorted into the sorted-dictionary form (SortedDimensionDictionary) the engines use. Such a
 * segment has no bitmap index: string filters run as row predicates on the ids (the adapter's
 * ValueMatchers; a multi-value row matches when one of its values does, an empty row as null).
 * Multi-value dimension: offsets[n_rows + 1] into ids (StringDimensionIndexer's encoded rows, values
 * in the row's order; an empty row = no values). Released with dg_segment_release. */
typedef struct {
  const char* name;
  int32_t type;            /* DG_COL_LONG / DG_COL_FLOAT / DG_COL_DOUBLE / DG_COL_STRING */
  int32_t card;            /* STRING: dictionary size */
  const char* const* dict; /* STRING: value of every id */
  const int32_t* ids;      /* STRING: [n_rows] ids into dict (multi-value: [offsets[n_rows]]) */
  const void* values;      /* numeric: [n_rows] int64 / float / double */
  const int32_t* offsets;  /* STRING multi-value: [n_rows + 1] row starts into ids; NULL = one id per row */
} dg_row_column;
int dg_segment_from_rows(dg_context* ctx, int64_t n_rows, const int64_t* timestamps, int64_t interval_start,
                         int64_t interval_end, const dg_row_column* columns, int32_t n_columns, dg_segment** out);
int64_t dg_segment_num_rows(const dg_segment* seg);
int dg_segment_interval(const dg_segment* seg, int64_t* start, int64_t* end);
int dg_segment_time_bounds(const dg_segment* seg, int64_t* min_time, int64_t* max_time);
int dg_segment_num_columns(const dg_segment* seg);
const char* dg_segment_column_name(const dg_segment* seg, int index);
int dg_segment_column_type(const dg_segment* seg, const char* column);
int64_t dg_segment_device_bytes(const dg_segment* seg);
int32_t dg_segment_dim_cardinality(const dg_segment* seg, const char* dim);
/* lookupName: *len = -1 for null (empty) values */
int dg_segment_dim_value(const dg_segment* seg, const char* dim, int32_t id, const char** out, int32_t* len);
/* Bulk dictionary export: offsets[card + 1] (byte offsets into bytes), bytes (size offsets[card]).
 * Call with bytes == NULL to get *total_bytes first. */
int dg_segment_dim_dictionary(const dg_segment* seg, const char* dim, int64_t* offsets, char* bytes,
                              int64_t* total_bytes);
/* Hand the engine one dictionary order (kept in HBM with the segment, set once per segment):
 * slot = 2 * DG_ORDER_* + inverted (InvertedTopNMetricSpec over DimensionTopNMetricSpec);
 * rank[id] for every dictionary id (card of them): position of the value under the comparator,
 * comparator-equal values share a rank (has_ties != 0 then). The ordering is the caller's
 * StringComparator (the JNI shim sorts the dictionary with the Java comparator itself). */
int dg_segment_set_dim_order(dg_segment* seg, const char* dim, int32_t slot, const int32_t* rank, int32_t card,
                             int32_t has_ties);

/* ---- scan pieces ---- */
/* Filter.getBitmapResult: row bitset (uint32 words, bit r = row r) of the filter, into out_words
 * (ceil(num_rows / 32) words); *out_count = cardinality of the result. */
int dg_filter_bitmap(dg_segment* seg, const dg_filter* filter, int32_t n_filter, uint32_t* out_words,
                     int64_t* out_count);

/* ---- timeseries ---- */
/* Per segment i: out_n_buckets[i] cursors (one per granularity bucket of the segment's actual
 * interval, TimeseriesQueryEngine emits each even when empty); bucket k of segment i is at
 * index i * bucket_cap + k of out_bucket_time / out_bucket_rows, and its aggregate slots at
 * (i * bucket_cap + k) * n_aggs. out_bucket_rows = rows aggregated (skipEmptyBuckets decision). */
int dg_timeseries_run(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, int32_t bucket_cap,
                      int32_t* out_n_buckets, int64_t* out_bucket_time, int64_t* out_bucket_rows,
                      uint64_t* out_values, dg_metrics* metrics);

/* ---- topN ---- */
typedef struct {
  const char* dimension;
  int32_t metric_agg; /* index into scan->aggs of the NumericTopNMetricSpec metric */
  int32_t inverted;   /* InvertedTopNMetricSpec */
  int32_t threshold;  /* per-segment threshold, i.e. max(query threshold, minTopNThreshold) */
  /* DimensionTopNMetricSpec / LexicographicTopNMetricSpec / AlphaNumericTopNMetricSpec
   * (query/topn/DimensionTopNMetricSpec.java): dim_order = order slot set with
   * dg_segment_set_dim_order (metric_agg / inverted ignored), -1 = metric ordering. */
  int32_t dim_order;
  const char* previous_stop;  /* NULL = none; LEXICOGRAPHIC skips to it (computeStartEnd) */
  const int32_t* min_rank;    /* per segment: values need rank >= min_rank[i], i.e. after previousStop
                                 under the comparator (NULL = no previousStop) */
  /* non-ALL granularity (scan->period_ms != 0): one result list per cursor (granularity bucket) */
  int32_t bucket_cap;         /* list slots per segment (>= its bucket count) */
  int64_t* out_bucket_time;   /* [n_segs * bucket_cap] bucket start of every list */
} dg_topn;

/* Per segment i and cursor b (b = 0 for ALL granularity, where bucket_cap counts as 1): list
 * L = i * bucket_cap + b holds out_n[L] entries (-1: no cursor), ordered as
 * TopNNumericResultBuilder.build() (or, for a dimension order, TopNLexicographicResultBuilder.build())
 * returns them; entry j at index L * threshold + j: dictionary id (segment-local) and n_aggs slots. */
int dg_topn_run(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_topn* topn,
                int32_t* out_n, int32_t* out_ids, uint64_t* out_values, dg_metrics* metrics);

/* topN over a numeric dimension. TopNQueryEngine.getMapFn (query/topn/TopNQueryEngine.java:141-148) sends a
 * LONG, FLOAT or DOUBLE column to DimExtractionTopNAlgorithm with a NumericTopNColumnSelectorStrategy
 * (types/TopNColumnSelectorStrategyFactory.java:43-69), which aggregates the rows into a map keyed by the long
 * itself, Float.floatToIntBits(v) or Double.doubleToLongBits(v) (types/NumericTopNColumnSelectorStrategy.java:
 * 81-151): every NaN is one value, -0.0 and 0.0 are two. The engine dictionary-encodes the column on the device
 * at its first use (the encoding dg_groupby_run_dims builds for a LONG dimension, shared with it; see
 * dg_segment_numeric_dim_info) and runs the topN over the ids: result ids index the column's distinct values in
 * ascending Long / Float / Double.compareTo order, and dg_segment_numeric_dim_values gives their values.
 *
 *   output_type  DimensionSpec.getOutputType. Supported: a LONG column with DG_COL_LONG or DG_COL_STRING (the
 *                entries carry String.valueOf(value)), a FLOAT column with DG_COL_FLOAT, a DOUBLE column with
 *                DG_COL_DOUBLE. Metric ties are broken by the output value's compareTo (TopNNumericResultBuilder.
 *                java:94-107,185-191,219-236): numerically, or for DG_COL_STRING by String.compareTo of the decimal
 *                text. A dimension-ordered spec (topn->dim_order; TopNLexicographicResultBuilder.java:66-125
 *                compares Objects.toString(value)) is supported on a LONG column for DG_ORDER_NUMERIC and
 *                DG_ORDER_LEXICOGRAPHIC, plain and inverted; the engine derives the ranks itself
 *                (dg_segment_set_dim_order refuses a numeric column).
 *   out_cut_ties The reference offers the map's entries to the builder in its hash map's iteration order
 *                (updateDimExtractionResults, NumericTopNColumnSelectorStrategy.java:154-171), and the builder
 *                refuses an entry whose metric equals the full queue's minimum: every value above the K-th largest
 *                metric is in its result and none below, but WHICH of the values tied with the K-th it keeps is
 *                arbitrary. The engine offers the values in ascending order of the output type's comparator (as a
 *                string dimension's ids are) and reports here, per list, how many values whose metric equals the
 *                last entry's are not in the list. 0: the list is what the reference returns under any order.
 *
 * DG_ERR_UNSUPPORTED before any launch, naming the column: any other (column, output) pair (the reference
 * aggregates by the OUTPUT type's key there, which is many-to-one), a column that is numeric in some of the
 * call's segments with a cursor and a string or missing in others, previous_stop on a numeric dimension,
 * DG_ORDER_ALPHANUMERIC / DG_ORDER_STRLEN on a numeric dimension, any dimension ordering on FLOAT / DOUBLE (it
 * would need Float.toString), a numeric output type on a string column. A string dimension with
 * DG_COL_STRING is dg_topn_run. */
typedef struct {
  int32_t output_type;    /* DG_COL_STRING | DG_COL_LONG | DG_COL_FLOAT | DG_COL_DOUBLE; 0 = DG_COL_STRING */
  int32_t reserved;
  int32_t* out_cut_ties;  /* optional [n_segs * bucket_cap]: per list, values whose metric equals the last
                             entry's and that are not in the list; 0 for a short list, a dimension-ordered
                             spec and a string dimension */
} dg_topn_opts;
/* dg_topn_run with options (opts == NULL: dg_topn_run itself). */
int dg_topn_run_opts(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_topn* topn,
                     const dg_topn_opts* opts, int32_t* out_n, int32_t* out_ids, uint64_t* out_values,
                     dg_metrics* metrics);
/* Values of result ids of a numeric dimension: out[k] = the value of ids[k] as an 8-byte slot in the aggregate
 * slot encoding (LONG: int64; DOUBLE: the double; FLOAT: the float32 in the first 4 bytes), what
 * convertAggregatorStoreKeyToColumnValue gives for the map key; a NaN is the canonical one. DG_ERR_ARG: not a
 * numeric column, no encoding built yet, or an id outside it. */
int dg_segment_numeric_dim_values(dg_segment* seg, const char* column, const int32_t* ids, int32_t n, uint64_t* out);
/* The cached encoding of a numeric column (dg_debug_long_dim_info for LONG, FLOAT and DOUBLE columns; that call
 * keeps its LONG-only contract): *built, *cardinality, *device_bytes (ids 4 B per row + 8 B per value, part of
 * dg_segment_device_bytes), *build_ms. Any output may be NULL. DG_ERR_NOT_FOUND: no such column; DG_ERR_ARG: not
 * a numeric column. */
int dg_segment_numeric_dim_info(dg_segment* seg, const char* column, int32_t* built, int64_t* cardinality,
                                int64_t* device_bytes, double* build_ms);

/* TopNBinaryFn fold (query/topn/TopNBinaryFn.java:75-135) of per-segment topN lists, as
 * TopNQueryQueryToolChest.mergeResults applies it over the per-segment runners' results
 * (QueryRunnerFactory.mergeRunners): lists in merge order (result timestamp, then segment index),
 * pairwise: union by dimension value with AggregatorFactory.combine, then TopNNumericResultBuilder with
 * the query threshold; the final list is truncated to the query threshold. ALL granularity.
 *   keys: segment mode (segs != NULL, one per list): segment-local dictionary ids, values compared by
 *         string through segs[i]'s dictionary; global mode (segs == NULL): ids of one cluster-wide
 *         dictionary whose order is Java String order, nulls first.
 * Output: out_n entries (<= topn->threshold), entry j taken from list out_list[j] with key out_keys[j]
 * and n_aggs slots in dg_topn_run's encoding. topn->threshold here is the QUERY threshold. */
typedef struct {
  int32_t n_lists;
  const int32_t* list_n;   /* entries of list i; <= 0: empty (no cursor) */
  int32_t stride;          /* entry j of list i is at index i * stride + j */
  const int64_t* keys;
  const uint64_t* values;  /* n_aggs slots per entry */
} dg_topn_lists;

int dg_topn_merge(dg_segment* const* segs, const dg_scan* scan, const dg_topn* topn, const dg_topn_lists* in,
                  int32_t* out_n, int32_t* out_list, int64_t* out_keys, uint64_t* out_values);
/* dg_topn_merge with options (opts == NULL: dg_topn_merge itself; out_cut_ties is not used). Segment mode over a
 * numeric dimension (the pairs of dg_topn_run_opts, the same refusals): TopNBinaryFn keys its map by the value
 * object, so keys (ids into each segment's value list) are one value when the values' map keys are equal, and
 * the builder breaks metric ties by the output type's compareTo (DG_COL_STRING on a LONG column: String.compareTo
 * of the decimal text). Global mode: the keys are the caller's and compare as signed 64-bit integers, whatever
 * the output type (a LONG dimension's values themselves). */
int dg_topn_merge_opts(dg_segment* const* segs, const dg_scan* scan, const dg_topn* topn, const dg_topn_lists* in,
                       const dg_topn_opts* opts, int32_t* out_n, int32_t* out_list, int64_t* out_keys,
                       uint64_t* out_values);

/* ---- search ----
 * Per-value hit counts of a search query (query/search/SearchQueryRunner.java:207-260). The caller
 * evaluates SearchQuerySpec.accept over the dictionaries it exports with dg_segment_dim_dictionary (the
 * Java shim with its own spec objects and extraction functions) and passes, per search dimension and
 * segment, the accepted segment-local dictionary ids; the engine counts, for each, the rows it occurs in
 * inside the selection S = filter AND rows whose time lies in [interval_start, interval_end):
 *   DG_SEARCH_PLAN_INDEX   IndexOnlyExecutor.execute (UseIndexesStrategy.java:236-281): |bitmap(id) AND S|, or the
 *                          bitmap's size when there is no filter and the interval covers the segment's rows. A
 *                          multi-value row counts once per distinct value. Taken for a dimension with a bitmap index
 *                          when the filter is null or runs on bitmap indexes alone (UseIndexesStrategy.java:87-98).
 *                          The interval rows are found by a per-row time test, which equals the reference's binary
 *                          search over __time (makeTimeFilteredBitmap, :164-219) on time-sorted segments, the only
 *                          kind IndexMergerV9 writes.
 *   DG_SEARCH_PLAN_CURSOR  CursorBasedExecutor: every occurrence of an accepted value in a selected row counts one
 *                          (StringSearchColumnSelectorStrategy, SearchQueryRunner.java:118-141: a row [a, a] counts 2).
 *                          Taken when a filter leaf is a row post-filter (a numeric column), when the segment has no
 *                          bitmap index (dg_segment_from_rows), or with DG_SEARCH_CURSOR_ONLY (CursorOnlyStrategy).
 *                          The counts are those of the full scan: the reference's early exit once its map holds
 *                          `limit` hits (:135-137) stops at a row the counts then depend on, so a caller that finds
 *                          at least `limit` distinct hits under this plan keeps its CPU engine.
 *   DG_SEARCH_PLAN_NONE    the column is missing in the segment or no id was passed: nothing to count.
 * scan supplies the filter, the interval, cancel and timeout_ms; its aggregators and granularity are ignored
 * (n_aggs == 0 is allowed). out_counts is flat in (segment, dimension, id) order, the sum of every n_ids
 * entries; zero counts are the caller's to drop, and the limit, the comparator-keyed map and the `remain`
 * arithmetic of SearchQueryRunner.run are the caller's too (out_plan[seg * n_dims + d] tells which limit rule
 * applies). Errors before any launch: ids not strictly ascending or not below the cardinality -> DG_ERR_ARG; a
 * LONG / FLOAT / DOUBLE column as a search dimension -> DG_ERR_UNSUPPORTED (its values have no dictionary).
 * Metrics: segment_rows, pre_filtered_rows, selected_rows, bitmap_bytes, bytes_read (serialized bitmap bytes +
 * N/8 of selection per accepted value, or the columns scanned), bitmap_ms (the selection), aggregate_ms (the
 * counting), decode_ms, total_ms. */
#define DG_SEARCH_USE_INDEXES 0   /* UseIndexesStrategy: index plan where the reference takes it, else cursor */
#define DG_SEARCH_CURSOR_ONLY 1
#define DG_SEARCH_PLAN_NONE   0   /* column missing in this segment / nothing accepted */
#define DG_SEARCH_PLAN_INDEX  1
#define DG_SEARCH_PLAN_CURSOR 2
typedef struct {
  const char* dimension;
  const int32_t* const* ids;  /* [n_segs] accepted segment-local dictionary ids, strictly ascending */
  const int32_t* n_ids;       /* [n_segs] */
} dg_search_dim;
typedef struct { const dg_search_dim* dims; int32_t n_dims; int32_t strategy; } dg_search;
int dg_search_run(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_search* s,
                  int64_t* out_counts, int32_t* out_plan, dg_metrics* metrics);

/* ---- scan (raw rows) ----
 * The rows a scan query returns (query/scan/ScanQuery.java:53-77, ScanQueryEngine.process :59-264): one
 * ascending cursor per segment at ALL granularity over filter AND interval (:126-135), the rows in cursor
 * (= row) order, at most `limit` of them over the call's segments taken in the order given: segment s keeps
 * its first min(selected_s, limit - kept before s) selected rows (the response context's count, :68-73,:125;
 * ScanQueryRunnerFactory.mergeRunners :64-96 concatenates in runner order). A segment reached once the limit
 * is full launches nothing and is not counted in metrics.segment_rows. dg_scan is the cursor struct, so the
 * query is dg_rows: `scan` supplies the filter, the interval, cancel and timeout_ms; its aggregators,
 * granularity and `descending` are ignored (the reference's constructor passes descending = false, :67).
 * columns: the caller's column list (:85-113 is the caller's rule); "__time" names the time column. A name a
 * segment lacks is DG_COL_MISSING there (null in every row, nothing to fetch); a complex column
 * (DG_COL_UNSUPPORTED) is DG_ERR_UNSUPPORTED before any launch. The values are what the column selectors'
 * getObject returns (getColumnValue, :238-250), columnar per (segment, column) and resident in HBM until
 * fetched page by page or released, like a dg_result:
 *   LONG and __time  int64            FLOAT  float32            DOUBLE  float64
 *   STRING, single-value: int32 segment-local dictionary ids (lookupName is the caller's, through
 *     dg_segment_dim_dictionary: SimpleDictionaryEncodedColumn.java:302-305, null for the empty string)
 *   STRING, multi-value: the page's ids concatenated + count + 1 offsets relative to the page (the caller
 *     applies DimensionSelector.defaultGetObject, DimensionSelector.java:167-182: null / the value / the list).
 *     out_values == NULL writes the offsets only (out_offsets[count] = the ids the page holds).
 * With no filter and an interval covering the segment's rows there is no selection bitset: the kept rows are
 * 0 .. keep - 1 and no compaction runs. Only the column blocks holding kept rows are decoded (the block
 * range [first kept row, last kept row]); a multi-value column is decoded whole.
 * dg_rowset_rows: rows kept of segment seg (seg < 0: of all). dg_rowset_column_info: *type = DG_COL_*,
 * *multi, *n_values = values held (rows kept; multi-value: ids). Out-of-range seg / col / start / count and
 * a NULL out_offsets for a multi-value column -> DG_ERR_ARG.
 * Metrics: segment_rows, pre_filtered_rows, selected_rows (filter AND interval in the segments scanned,
 * before the limit), bitmap_bytes, bytes_read (stored bytes of the blocks decoded + bitmaps), bitmap_ms (the
 * selection), decode_ms, aggregate_ms (compaction + gather kernels), total_ms.
 * dg_segment_num_dimensions / dg_segment_dimension_name: StorageAdapter.getAvailableDimensions (index.drd's
 * dimension list; a segment from rows: its string columns in the order given), which the default column
 * list of a scan puts before the metrics (:96-106). */
typedef struct { const char* const* columns; int32_t n_columns; int64_t limit; /* <= 0: none */ } dg_rows;
typedef struct dg_rowset dg_rowset;
int dg_rows_run(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_rows* spec, dg_rowset** out,
                dg_metrics* metrics);
int64_t dg_rowset_rows(const dg_rowset* rs, int32_t seg);
int dg_rowset_column_info(const dg_rowset* rs, int32_t seg, int32_t col, int32_t* type, int32_t* multi,
                          int64_t* n_values);
int dg_rowset_fetch(dg_rowset* rs, int32_t seg, int32_t col, int64_t start, int64_t count, void* out_values,
                    int64_t* out_offsets);
void dg_rowset_release(dg_rowset* rs);
int dg_segment_num_dimensions(const dg_segment* seg);
const char* dg_segment_dimension_name(const dg_segment* seg, int index);

/* ---- groupBy (v2) ---- */
/* GroupByStrategyV2.mergeRunners over the call's segments: every segment's rows grouped
 * (GroupByQueryEngineV2.process, epinephelinae/GroupByQueryEngineV2.java:91-187) and merged by
 * (bucket, dimension values) like GroupByMergingQueryRunnerV2 (:170-290), in that order. A call
 * with one segment is that segment's runner (createRunner(segment).run). The groups stay in HBM in
 * the dg_result until fetched (page by page for large results). */
typedef struct {
  const char* const* dimensions;
  int32_t n_dims;
} dg_groupby;

int dg_groupby_run(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_groupby* g,
                   dg_result** out, dg_metrics* metrics);
/* The grouper of one call (since ABI 16). DG_GROUPER_SORT: the call's elements sorted by key and
 * reduced run by run. DG_GROUPER_HASH: BufferHashGrouper (epinephelinae/BufferHashGrouper.java:38-133)
 * over an open-addressing table in HBM (ByteBufferHashTable.java:286-327: linear probing, max load factor
 * 0.7), sized for max_groups, its groups sorted afterwards: the same result, a footprint and a sort
 * sized by the groups. forceHashAggregation / bufferGrouperMaxSize of GroupByQueryConfig.java:35-40 map
 * to `grouper` / `max_groups`. Like forceHashAggregation, `grouper` is a preference that never changes
 * results: a plan with a floatSum aggregator (its fp32 row-order recurrence needs the sorted rows), a
 * key of 64 bits or a table of more than 2^31 slots runs the sort (dg_result_grouper_info tells).
 * max_groups: the table holds next_pow2(max_groups / 0.7) slots, max_groups capped at the call's
 * elements and at 2^key_bits; a call that finds more distinct groups fails with DG_ERR_TABLE_FULL
 * (Groupers.HASH_TABLE_FULL, there is no spilling), under either grouper, and leaves the context usable.
 * dg_groupby_run(...) = dg_groupby_run_opts(..., NULL, ...). Environment DG_GROUPER=hash|sort overrides
 * the context's default grouper per call (same-box A/B runs), never an explicit opts->grouper. */
#define DG_GROUPER_SORT 0
#define DG_GROUPER_HASH 1
typedef struct {
  int32_t grouper;      /* DG_GROUPER_*; -1 = the context's default */
  int32_t reserved;
  int64_t max_groups;   /* bufferGrouperMaxSize; <= 0 = the context's default (unlimited) */
} dg_groupby_opts;
int dg_groupby_run_opts(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_groupby* g,
                        const dg_groupby_opts* opts /* NULL = defaults */, dg_result** out, dg_metrics* metrics);

/* groupBy with a DimensionSpec output type per dimension (DefaultDimensionSpec.getOutputType,
 * query/dimension/DefaultDimensionSpec.java:68-78; every Druid SQL GROUP BY over a long column asks for
 * LONG). dg_groupby_run / dg_groupby_run_opts are this call with every output_type DG_COL_STRING.
 *
 * A dimension that is a LONG column in every segment of the call is grouped by its values, as
 * GroupByQueryEngineV2.GroupByStrategyFactory does through LongGroupByColumnSelectorStrategy
 * (epinephelinae/GroupByQueryEngineV2.java:235-260). The first such call dictionary-encodes the column on
 * the device (its distinct values ascending + one id per row) and the segment keeps the encoding
 * (dg_debug_long_dim_info); the segments' value lists are merged like string dictionaries. The merged
 * ids, and so the result's rows, are ordered by the output type:
 *   DG_COL_LONG    ascending numeric order (LongRowBasedKeySerdeHelper = Longs.compare,
 *                  RowBasedGrouperHelper.java:1389-1437)
 *   DG_COL_STRING  the rows carry String.valueOf(value) (convertRowTypesToOutputTypes,
 *                  GroupByQueryEngineV2.java:689-698; DimensionHandlerUtils.convertObjectToString :245-251)
 *                  and order as strings: "-5" < "10" < "9"
 * Refused with DG_ERR_UNSUPPORTED before any launch, naming the column: a dimension that is LONG in some
 * of the call's segments and a string or missing in others, a FLOAT or DOUBLE dimension, output type LONG
 * on a string (or everywhere missing) column, any other output type. */
typedef struct {
  const char* dimension;
  int32_t output_type; /* DG_COL_STRING | DG_COL_LONG */
  int32_t reserved;
} dg_dimension;
int dg_groupby_run_dims(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_dimension* dims,
                        int32_t n_dims, const dg_groupby_opts* opts /* NULL = defaults */, dg_result** out,
                        dg_metrics* metrics);
/* What dimension `dim` of a groupBy result is: *column_type = DG_COL_STRING | DG_COL_LONG (what the
 * dimension's ids index: strings, or the longs of dg_result_dim_longs), *output_type as the query asked
 * (the ValueType convertRowTypesToOutputTypes gives the row's value, GroupByQueryEngineV2.java:689-698).
 * A dg_merge result has the caller's dictionaries: DG_ERR_ARG. */
int dg_result_dim_type(const dg_result* res, int32_t dim, int32_t* column_type, int32_t* output_type);
/* A long dimension's merged dictionary: out[dg_result_dim_cardinality(res, dim)] in merged-id order (the
 * row's dimension value before convertRowTypesToOutputTypes). A string dimension: DG_ERR_ARG.
 * dg_result_dim_dictionary of a long dimension gives each value's decimal text (Long.toString). */
int dg_result_dim_longs(const dg_result* res, int32_t dim, int64_t* out);

typedef struct {
  int32_t grouper;          /* what actually ran */
  int32_t reserved;
  int64_t table_slots;      /* HBM table capacity (0 for the sort) */
  int64_t max_groups;       /* the limit in force (0: none) */
  int64_t flushed_entries;  /* LDS entries upserted into the HBM table */
  int64_t direct_elements;  /* elements that bypassed a full LDS table */
} dg_grouper_info;
/* What grouped a dg_groupby_run result (a dg_merge result: the sort). */
int dg_result_grouper_info(const dg_result* res, dg_grouper_info* out);
/* ---- groupBy limit push-down ----
 * GroupByQuery.isApplyLimitPushDown (query/groupby/GroupByQuery.java:377-416: a limited DefaultLimitSpec
 * whose ORDER BY columns are all grouping dimensions, no having spec, no subtotals) orders rows by
 * getRowOrderingForPushDown (:423-528): the bucket time first (last with the sortByDimsFirst context
 * flag on a non-ALL granularity), then the ORDER BY dimensions in their order, each under its
 * StringComparator and direction (compareDimsForLimitPushDown :600-633), then the other dimensions
 * ascending; the grouper keeps the first `limit` rows (LimitedBufferHashGrouper.java). dg_result_limit
 * applies that to a dg_groupby_run / dg_merge result on the device: afterwards the result holds
 * min(limit, groups) groups in that order (comparator-equal groups keep the result's natural order),
 * fetched as before; dg_result_export refuses a limited result. */
typedef struct {
  int32_t dim;         /* index into dg_groupby.dimensions */
  int32_t descending;  /* OrderByColumnSpec.Direction.DESCENDING */
  const int32_t* rank; /* rank of every id of the result's dictionary of `dim` under the column's
                          StringComparator (0 <= rank < cardinality, nulls first, comparator-equal
                          values share a rank); NULL = LEXICOGRAPHIC, the id order itself */
} dg_order_column;

typedef struct {
  const dg_order_column* columns;
  int32_t n_columns;
  int32_t limit;              /* > 0 */
  int32_t sort_by_dims_first; /* query context sortByDimsFirst */
} dg_limit;

int dg_result_limit(dg_result* res, const dg_limit* spec);
/* ---- groupBy post-processing on the device ----
 * GroupByQuery.postProcess over a resident dg_groupby_run* / dg_merge / dg_groupby_merge_devices result that
 * has not been limited: the having spec (the HavingSpec classes of query/groupby/having), then DefaultLimitSpec.build
 * (query/groupby/orderby/DefaultLimitSpec.java:122-290: makeComparator, metricOrdering, LimitingFn,
 * TopNFunction; TopNSequence.java). One call applies, in this order:
 *   1. having  keep the groups the postfix program accepts (n_having = 0: all of them)
 *   2. order   sort = 1: the survivors by the comparator chain: bucket time first (last with
 *              sort_by_dims_first on a non-ALL granularity, absent for ALL), the columns in their order.
 *              Comparator-equal groups keep the result's key order (a stable sort; the reference's
 *              MinMaxPriorityQueue leaves ties unspecified), or dimensions-then-time order with
 *              sort_by_dims_first on a non-ALL granularity. sort = 0 (LimitingFn): the natural order.
 *   3. limit   keep the first `limit` (0 = all)
 * Afterwards the result holds exactly the surviving groups in that order, fetched as before, and counts as
 * limited (dg_result_export refuses it, as does a second dg_result_post_process / dg_result_limit).
 *
 * The having program is postfix over a stack of booleans (at most DG_HAVING_MAX_OPS ops, at most 32
 * operands alive). The device never parses numbers: every greaterThan / lessThan / equalTo leaf arrives as
 * one closed interval of the aggregator's ORDER KEY, its own comparator as an unsigned 64-bit number
 * (HavingSpecMetricComparator.java:36-80 is monotone in the metric for a fixed value):
 *   long outputs    (Long.compare)     v ^ 2^63
 *   double outputs  (Doubles.compare)  NaN -> ~0; else bits < 0 ? ~bits : bits | 2^63  (NaN greatest, -0.0 < 0.0)
 *   float outputs                      the double key of the exactly widened float32
 * An aggregator order column compares the same keys (AggregatorFactory.getComparator); a dimension column
 * compares ranks (as dg_order_column) or ids when rank is NULL; a descending column is complemented.
 *
 * Refused before any launch, the result unchanged: an already limited result, a program that is too long
 * or whose stack under- or overflows or does not end with one value, aggregator / dimension indices out of
 * range, ranks outside [0, cardinality), a negative limit (DG_ERR_ARG); a result of 2^32 groups or more
 * (DG_ERR_UNSUPPORTED: group references are 32-bit). On any later error the result is unchanged too. */
#define DG_HAVING_MAX_OPS 128
#define DG_HAVING_ALWAYS 0    /* push true */
#define DG_HAVING_NEVER 1     /* push false */
#define DG_HAVING_AND 2       /* pop `arg` operands, push their conjunction (arg = 0: true) */
#define DG_HAVING_OR 3        /* pop `arg` operands, push their disjunction (arg = 0: false) */
#define DG_HAVING_NOT 4       /* negate the top */
#define DG_HAVING_AGG_RANGE 5 /* push lo <= order key of aggregator `arg` <= hi (lo > hi: never) */
#define DG_HAVING_DIM_EQ 6    /* push (merged dictionary id of dimension `arg` == lo) */
typedef struct {
  int32_t op;  /* DG_HAVING_* */
  int32_t arg;
  uint64_t lo, hi;
} dg_having_op;
#define DG_ORDER_DIM 0
#define DG_ORDER_AGG 1
typedef struct {
  int32_t kind;        /* DG_ORDER_DIM | DG_ORDER_AGG */
  int32_t index;       /* into dg_groupby.dimensions / the call's aggregators */
  int32_t descending;
  int32_t reserved;
  const int32_t* rank; /* DG_ORDER_DIM: as dg_order_column.rank; NULL = the id order */
} dg_post_column;
typedef struct {
  const dg_having_op* having;
  int32_t n_having;           /* 0 = no having spec */
  int32_t n_columns;
  const dg_post_column* columns;
  int32_t sort;               /* 0 = LimitingFn: natural order, columns ignored after validation */
  int32_t sort_by_dims_first; /* query context sortByDimsFirst */
  int32_t limit;              /* 0 = none */
  int32_t reserved;
} dg_post_process;
typedef struct {
  int64_t groups_in;
  int64_t groups_after_having;
  int64_t groups_kept;
  double having_ms; /* device time of the having pass and the survivor compaction (0 without phase timing) */
  double sort_ms;   /* device time of the word loads, the sorts and the gather */
} dg_post_info;
int dg_result_post_process(dg_result* res, const dg_post_process* spec, dg_post_info* info /* may be NULL */);
/* ---- post-aggregators the device decides on ----
 * The VALUES of post-aggregators stay the caller's (the Java toolchests compute them per row:
 * GroupByStrategyV2.mergeResults, GroupByStrategyV2.java:286-300). Two DECISIONS of GroupByQuery.postProcess depend
 * on them: a having spec over a post-aggregator (GroupByQueryRunnerTest.testPostAggHavingSpec) and a limit spec
 * ordered by one (DefaultLimitSpec.makeComparator takes postAgg.getComparator(), DefaultLimitSpec.java:190-260).
 * dg_result_post_aggregate evaluates the post-aggregators those decisions need for every group of a resident
 * result, and dg_result_post_process then reads them like aggregators.
 *
 * A post-aggregator is a postfix program over one group's aggregator slots, compiled and type-checked by the
 * caller (the device never sees JSON or names). Operand types are static; the stack holds raw 64-bit words, at
 * most DG_POST_MAX_STACK of them; a program has at most DG_POST_MAX_OPS ops and leaves exactly one value.
 *   DG_POST_AGG arg         push aggregator `arg` of the group: long outputs push the int64, double outputs the
 *                           double, float outputs the exactly widened float32 (FieldAccessPostAggregator.java +
 *                           Number.doubleValue); a DG_AGG_PAIR_TIME entry cannot be read
 *   DG_POST_CONST_D/_L imm  push a double (its bits) / a long constant (ConstantPostAggregator.java)
 *   DG_POST_L2D             (double) long          DG_POST_D2L  Java's (long) double: NaN -> 0, saturating
 *   DG_POST_ADD/SUB/MUL     IEEE fp64, each op rounded on its own (ArithmeticPostAggregator.java:206-228)
 *   DG_POST_DIV             rhs == 0.0 ? 0.0 : lhs / rhs (:229-235)       DG_POST_QUOT  lhs / rhs (:236-242)
 *   DG_POST_DMAX/DMIN       Double.compare(b, a) > 0 ? b : a / < 0 (DoubleGreatestPostAggregator.java:77-92,
 *                           DoubleLeastPostAggregator.java); the caller folds from -inf / +inf constants
 *   DG_POST_LMAX/LMIN       Long.compare (LongGreatestPostAggregator.java:76-93, LongLeastPostAggregator.java);
 *                           folded from Long.MIN_VALUE / MAX_VALUE
 * A NaN value is the canonical NaN (Double.doubleToLongBits). `order` is the comparator of the top-level
 * post-aggregator: DG_POST_ORDER_DOUBLE (Double.compareTo: arithmetic by default, doubleGreatest / doubleLeast),
 * DG_POST_ORDER_LONG (longGreatest / longLeast), DG_POST_ORDER_NUMERIC_FIRST (ArithmeticPostAggregator.Ordering.
 * numericFirst, :277-299: -inf < +inf < NaN < every finite value), DG_POST_ORDER_NONE (ConstantPostAggregator's
 * always-equal comparator: an order column of it decides nothing).
 *
 * dg_result_post_aggregate: a dg_groupby_run* / dg_merge / dg_groupby_merge_devices result (either grouper) gets
 * n_cols (1..DG_POST_MAX_COLS) columns [n_cols][groups] beside its slots, one launch (k_post_eval). Refused before
 * any launch with DG_ERR_ARG, the result unchanged: a limited or post-processed result, a second call, a program
 * that is too long, under- or overflows the stack, mixes operand types, does not end with exactly one value or
 * whose order kind does not fit its value's type, a slot index out of range, DG_POST_AGG of a DG_AGG_PAIR_TIME
 * slot. *out_ms = the kernel's device time (0 without phase timing).
 * dg_result_post_process afterwards: a DG_HAVING_AGG_RANGE.arg or DG_ORDER_AGG index n_aggs + j means post column
 * j, its interval / order under the column's order kind (keys: LONG v ^ 2^63; DOUBLE as a double aggregator;
 * NUMERIC_FIRST -inf -> 0, +inf -> 1, NaN -> 2, finite -> the double key; NONE: the key 0). Without post columns
 * such an index is refused as before. The columns are dropped by dg_result_post_process: they exist to decide.
 * dg_result_post_values: the raw words of post column `col` for groups [start, start + count), before
 * dg_result_post_process (a shim that would rather not recompute the values reads them here). */
#define DG_POST_MAX_OPS 64
#define DG_POST_MAX_STACK 16
#define DG_POST_MAX_COLS 16
#define DG_POST_AGG 0
#define DG_POST_CONST_D 1
#define DG_POST_CONST_L 2
#define DG_POST_L2D 3
#define DG_POST_D2L 4
#define DG_POST_ADD 5
#define DG_POST_SUB 6
#define DG_POST_MUL 7
#define DG_POST_DIV 8
#define DG_POST_QUOT 9
#define DG_POST_DMAX 10
#define DG_POST_DMIN 11
#define DG_POST_LMAX 12
#define DG_POST_LMIN 13
#define DG_POST_ORDER_NONE 0
#define DG_POST_ORDER_DOUBLE 1
#define DG_POST_ORDER_LONG 2
#define DG_POST_ORDER_NUMERIC_FIRST 3
typedef struct {
  int32_t op;   /* DG_POST_* */
  int32_t arg;  /* DG_POST_AGG: index into the call's aggregators */
  uint64_t imm; /* DG_POST_CONST_D: the double's bits; DG_POST_CONST_L: the long */
} dg_post_agg_op;
typedef struct {
  const dg_post_agg_op* ops;
  int32_t n_ops;
  int32_t order; /* DG_POST_ORDER_* */
} dg_post_agg;
int dg_result_post_aggregate(dg_result* res, const dg_post_agg* cols, int32_t n_cols, double* out_ms /* may be NULL */);
int dg_result_post_values(const dg_result* res, int32_t col, int64_t start, int64_t count, uint64_t* out);
/* topN ranked by a post-aggregator: NumericTopNMetricSpec may name one (query/topn/NumericTopNMetricSpec.java);
 * TopNNumericResultBuilder.addEntry (TopNNumericResultBuilder.java:112-183) computes the pruned post-aggregators per
 * dimension value, per segment, before its priority queue, and TopNBinaryFn (TopNBinaryFn.java:65-71,97-110)
 * recomputes them after every combine. dg_topn_run_post / dg_topn_merge_post are the _opts forms with one
 * trailing program (metric == NULL: the _opts form itself). With a program topn->metric_agg is ignored: every
 * touched value's ranking key is the program over the value's aggregator slots under the program's order kind
 * (`inverted` flips it); the selection, the candidate ordering, out_cut_ties, the per-bucket lists and the merge's
 * re-ranking after each combine are otherwise unchanged, the host steps running the same evaluator as the device.
 * Outputs stay n_aggs slots per entry: the caller computes the values it shows (TopNQueryQueryToolChest.java:
 * 196-206). DG_ERR_ARG before any launch: a program dg_result_post_aggregate would refuse, DG_POST_ORDER_NONE (a
 * comparator that ranks nothing), a dimension-ordered spec (topn->dim_order >= 0) with a program. */
int dg_topn_run_post(dg_segment* const* segs, int32_t n_segs, const dg_scan* scan, const dg_topn* topn,
                     const dg_topn_opts* opts, const dg_post_agg* metric, int32_t* out_n, int32_t* out_ids,
                     uint64_t* out_values, dg_metrics* metrics);
int dg_topn_merge_post(dg_segment* const* segs, const dg_scan* scan, const dg_topn* topn, const dg_topn_lists* in,
                       const dg_topn_opts* opts, const dg_post_agg* metric, int32_t* out_n, int32_t* out_list,
                       int64_t* out_keys, uint64_t* out_values);
/* ---- derived columns: numeric expressions ----
 * ExpressionVirtualColumn, the `expression` of the simple aggregator factories and ExpressionDimFilter
 * (segment/virtual/ExpressionVirtualColumn.java, SimpleDoubleAggregatorFactory.java:59, ExpressionFilter.java:
 * 54-66) all evaluate one numeric expression per row. dg_segment_derive_column evaluates it ONCE per segment on
 * the device (k_expr_eval) into a flat LONG, DOUBLE or FLOAT column in HBM and registers it under `name`; from
 * then on every call that names the column reads it like a stored one (aggregator inputs, numeric filter leaves,
 * numeric dimensions, dg_rows_run). It costs 8 bytes per row (FLOAT: 4) of HBM, counted in
 * dg_segment_device_bytes, until dg_segment_drop_derived or dg_segment_release.
 *
 * The expression is a postfix program over up to DG_EXPR_MAX_INPUTS stored numeric columns ("__time" allowed),
 * compiled and type-checked by the caller. Types are static, long or double; a LONG input pushes the long, a
 * DOUBLE the double, a FLOAT its exactly widened float32; every NaN is the canonical one.
 *   DG_EXPR_INPUT arg / CONST_L imm / CONST_D imm (the double's bits)
 *   DG_EXPR_L2D, DG_EXPR_D2L (Java's saturating cast, NaN -> 0), DG_EXPR_D2F ((float), only as the last op of a
 *   DG_COL_FLOAT output)
 *   DG_EXPR_ADD SUB MUL DIV MOD: both operands long (wrapping; MIN / -1 = MIN, MIN % -1 = 0) or both double (IEEE,
 *   % = fmod), each op rounded on its own           DG_EXPR_NEG, DG_EXPR_NOT (!(x > 0) in the operand's type)
 *   DG_EXPR_LT LE GT GE (doubles by Double.compare), DG_EXPR_EQ NE (doubles by ==): 1 / 0 in the operands' type
 *   DG_EXPR_AND / OR: (l > 0 ? r : l) / (l > 0 ? l : r)      DG_EXPR_SELECT: pops c, a, b -> c > 0 ? a : b
 *   DG_EXPR_ABS, CEIL, FLOOR (doubles), MIN, MAX (Math.min / max), IDIV (long / long, or (long)(x / y))
 * A long division by zero (the reference throws ArithmeticException for the rows its cursor visits) poisons
 * the value; a select keeps the poison of its condition and of the branch it chose only. A build that finds
 * a poisoned row registers nothing and returns DG_ERR_UNSUPPORTED ("division by zero in N rows").
 *
 * dg_segment_derive_column is a call on the segment's context like a query (cancel / timeout_ms as in dg_scan).
 * An identical column (name, program, inputs, type) already there: DG_OK, out->built = 0, nothing runs. Refused
 * before any launch: DG_ERR_ARG — a program the checker rejects (length, stack, operand types, result type), a
 * name that is a stored column or a derived column of another program; DG_ERR_UNSUPPORTED — an input the
 * segment lacks, or a string, multi-value or unsupported one (the reference types those per row). A failed,
 * cancelled or timed-out build leaves nothing behind.
 * dg_segment_drop_derived: frees the column and whatever was cached on it (numeric-dimension encoding).
 * DG_ERR_NOT_FOUND: no such column; DG_ERR_ARG: a stored column. No call may be using the column. */
#define DG_EXPR_MAX_OPS 64
#define DG_EXPR_MAX_STACK 16
#define DG_EXPR_MAX_INPUTS 8
#define DG_EXPR_INPUT 0
#define DG_EXPR_CONST_L 1
#define DG_EXPR_CONST_D 2
#define DG_EXPR_L2D 3
#define DG_EXPR_D2L 4
#define DG_EXPR_D2F 5
#define DG_EXPR_ADD 6
#define DG_EXPR_SUB 7
#define DG_EXPR_MUL 8
#define DG_EXPR_DIV 9
#define DG_EXPR_MOD 10
#define DG_EXPR_NEG 11
#define DG_EXPR_NOT 12
#define DG_EXPR_LT 13
#define DG_EXPR_LE 14
#define DG_EXPR_GT 15
#define DG_EXPR_GE 16
#define DG_EXPR_EQ 17
#define DG_EXPR_NE 18
#define DG_EXPR_AND 19
#define DG_EXPR_OR 20
#define DG_EXPR_SELECT 21
#define DG_EXPR_ABS 22
#define DG_EXPR_CEIL 23
#define DG_EXPR_FLOOR 24
#define DG_EXPR_MIN 25
#define DG_EXPR_MAX 26
#define DG_EXPR_IDIV 27
typedef struct {
  int32_t op;   /* DG_EXPR_* */
  int32_t arg;  /* DG_EXPR_INPUT: index into `inputs` */
  uint64_t imm; /* DG_EXPR_CONST_L: the long; DG_EXPR_CONST_D: the double's bits */
} dg_expr_op;
typedef struct {
  const char* const* inputs; /* stored columns of the segment, "__time" allowed */
  int32_t n_inputs;
  const dg_expr_op* ops;
  int32_t n_ops;
  int32_t out_type; /* DG_COL_LONG / DG_COL_DOUBLE / DG_COL_FLOAT */
} dg_expr;
typedef struct {
  int32_t built; /* 0: an identical column was already there */
  int32_t type;
  int64_t rows, device_bytes, poisoned_rows;
  double build_ms;
} dg_derived_info;
int dg_segment_derive_column(dg_segment* seg, const char* name, const dg_expr* expr, const volatile int32_t* cancel,
                             int64_t timeout_ms, dg_derived_info* out /* may be NULL */);
int dg_segment_drop_derived(dg_segment* seg, const char* name);
/* number of merged groups */
int64_t dg_result_groups(const dg_result* res);
/* groups [start, start + count), in result order (bucket time, then dimension values in Java
 * String order, nulls first): bucket_time[count] (ALL granularity: the universal timestamp = the
 * query interval's start, GroupByStrategyV2.getUniversalTimestamp :125-138), ids[count * n_dims]
 * = indices into the result's merged dictionary of each dimension, values[count * n_aggs] in the
 * slot encoding of dg_timeseries_run. Any output pointer may be NULL (under ALL granularity the
 * caller knows every bucket time and passes NULL). Destinations in pinned host memory (dg_host_alloc,
 * or memory the caller registered with HIP) receive the columns by DMA straight from the device;
 * others through the library's pinned staging. */
int dg_result_fetch_groups(dg_result* res, int64_t start, int64_t count, int64_t* bucket_time, int32_t* ids,
                           uint64_t* values);
/* Pinned host memory for result delivery (since ABI 14): the shim allocates its result buffers once
 * and wraps them as direct ByteBuffers (JNI NewDirectByteBuffer), the way the processing pool's
 * buffers are allocated once at startup (OffheapBufferGenerator.java:53 allocateDirect). */
int dg_host_alloc(int64_t bytes, void** out);
void dg_host_free(void* p);
/* Phase timing (since ABI 15, process-wide, on by default): the dg_metrics *_ms phase times come from
 * GPU timestamps the calls record between their launch groups. A small query pays ~25 us for them
 * (configs[0]), so a caller timing queries end to end turns them off and samples phases in separate
 * calls (the phase fields then read 0). No reference counterpart: the reference's per-query metrics
 * (QueryMetrics reportSegmentTime etc.) are host wall times. */
int dg_set_phase_timing(int32_t on);
/* rows aggregated into each group of [start, start + count) */
int dg_result_fetch_rows(dg_result* res, int64_t start, int64_t count, int64_t* rows);
/* merged dictionary of dimension `dim` (the union of the segments' dictionaries, Java String
 * order, null first when present): cardinality, and a bulk export like dg_segment_dim_dictionary
 * (a null value has length 0) */
int32_t dg_result_dim_cardinality(const dg_result* res, int32_t dim);
int dg_result_dim_dictionary(const dg_result* res, int32_t dim, int64_t* offsets, char* bytes, int64_t* total_bytes);
void dg_result_release(dg_result* res);

/* ---- cross-device groupBy merge (QueryRunnerFactory.mergeRunners over devices, processing/.../query/
 * QueryRunnerFactory.java:62; GroupByMergingQueryRunnerV2.java:170-290 semantics) ----
 * Every device runs dg_groupby_run over its segments; the devices' groups are then re-keyed into one
 * cluster-wide key space (dg_result_export), cut into key ranges (dg_keys_partition), exchanged
 * (RCCL all-to-all over xGMI — the transport is the caller's: torch.distributed in
 * incubator-druid_amd/distributed.py, or the JNI shim's own communicator) and merged on the receiving
 * device (dg_merge), which combines equal keys with the combining aggregators in partial order. */
typedef struct {
  int32_t n_dims;
  const int32_t* card;      /* [n_dims] cardinality of the cluster-wide dictionary of each dimension
                               (the union of every device's merged dictionary, Java String order,
                               nulls first) */
  int64_t period_ms;        /* 0 = ALL granularity */
  int64_t bucket0;          /* non-ALL: epoch ms of bucket index 0 (on the query's period grid) */
  int64_t n_buckets;        /* non-ALL: bucket indices [0, n_buckets) */
  int64_t universal_time;   /* ALL: the result timestamp (GroupByStrategyV2.getUniversalTimestamp) */
  int32_t n_aggs;
  const int32_t* agg_kinds; /* [n_aggs] DG_AGG_* (combine semantics of each aggregator) */
} dg_keyspace;

/* total bits of a key of the key space; DG_ERR_UNSUPPORTED above 64 */
int dg_keyspace_bits(const dg_keyspace* ks, int32_t* bits);
/* Re-key res into the key space: maps[d][merged id of res] = cluster-wide id, strictly increasing
 * (so the ascending order is kept). Writes dg_result_groups(res) records into caller-allocated
 * DEVICE buffers of res's device: d_keys[n], d_slots[n * (1 + n_aggs)] (rows aggregated, then the
 * values in the slot encoding of dg_timeseries_run). Completes before returning. */
int dg_result_export(dg_result* res, const dg_keyspace* ks, const int32_t* const* maps, uint64_t* d_keys,
                     uint64_t* d_slots);
/* Key ranges of ascending device keys d_keys[n]: out_pos[i] = first index with key >= splits[i]
 * (splits ascending, host array), i.e. range i = [out_pos[i - 1], out_pos[i]). */
int dg_keys_partition(dg_context* ctx, const uint64_t* d_keys, int64_t n, const uint64_t* splits, int32_t n_splits,
                      int64_t* out_pos);
/* Merge n records (device buffers of ctx's device: keys, slots as written by dg_result_export),
 * the concatenation of partials that are each ascending, into a dg_result in the key space. Equal
 * keys combine in input order. The result's dimension ids are cluster-wide ids: its
 * dg_result_dim_cardinality is ks->card[d], and the dictionary is the caller's. */
int dg_merge(dg_context* ctx, const dg_keyspace* ks, const uint64_t* d_keys, const uint64_t* d_slots, int64_t n,
             dg_result** out, dg_metrics* metrics);

/* ---- in-process cross-device merge (QueryRunnerFactory.mergeRunners over the devices of ONE process,
 * query/QueryRunnerFactory.java:62: a historical is one JVM whose processing pool drives every
 * segment, ChainedExecutionQueryRunner.java:89-180; GroupByMergingQueryRunnerV2.java:170-290
 * semantics) ----
 * parts: n_parts dg_groupby_run results of one query, each on its own context (device), in merge
 * order. The library builds the union of their merged dictionaries, re-keys every part into that key
 * space on its own device (as dg_result_export), cuts the keys into n_targets ranges at splitters
 * sampled from all parts (dg_keys_partition), moves every range to its target's device with peer
 * copies over xGMI (hipMemcpyPeerAsync; a device copy when part and target share a device) and
 * merges it there (dg_merge: equal keys combine in part order with the combining aggregators).
 * outs[t] = key range t of the merged result, resident on targets[t]; concatenated in t order they
 * are the whole merged, ordered result. The outputs fetch like dg_groupby_run results: their
 * dg_result_dim_dictionary is the union dictionary. n_targets == 1: the whole merge on one device.
 * Parts stay valid (the caller releases them). No transport from the caller is needed.
 * A part that groups by a long dimension (dg_groupby_run_dims) is DG_ERR_UNSUPPORTED: the dictionary union
 * compares strings. dg_result_export / dg_merge with the caller's own maps take such results as any other. */
int dg_groupby_merge_devices(dg_result* const* parts, int32_t n_parts, dg_context* const* targets, int32_t n_targets,
                             dg_result** outs, dg_metrics* metrics);

/* TimeseriesBinaryFn fold (query/timeseries/TimeseriesBinaryFn.java:67-70) as the toolchest's
 * mergeResults applies it over runners' results (ResultMergeQueryRunner: by time, then runner
 * order): n_lists lists in dg_timeseries_run's output layout (list i holds n[i] buckets: times[i * cap
 * + k], rows[...], values[(i * cap + k) * n_aggs ...]) — the segments of one call, or the lists of
 * several devices' calls concatenated. Results of one granularity bucket combine with
 * AggregatorFactory.combine (long wrap, float adds in float, Math.min/max with NaN and -0.0); ALL
 * granularity keeps the earliest result's timestamp. skip_empty: skipEmptyBuckets drops buckets with
 * zero rows before merging. Output: out_n merged buckets, ascending (descending when scan->descending),
 * out_rows = rows aggregated per bucket. Host memory only. */
int dg_timeseries_merge(const dg_scan* scan, int32_t n_lists, const int32_t* n, int32_t cap, const int64_t* times,
                        const int64_t* rows, const uint64_t* values, int32_t skip_empty, int32_t out_cap, int32_t* out_n,
                        int64_t* out_time, int64_t* out_rows, uint64_t* out_values);

/* ---- BufferAggregator record layout (query/aggregation/BufferAggregator.java:35-199) ----
 * Writes n records of aggregate slots (n_aggs per record, the dg_*_run slot encoding) into Druid's
 * buffer layout so a JNI shim can fill a processing-pool direct ByteBuffer in place
 * (GetDirectBufferAddress): aggregator a at byte offsets[a] of each record_size-byte record, the
 * value as its BufferAggregator stores it — count / long* as an 8-byte long (LongSumBufferAggregator
 * buf.putLong), double* as an 8-byte double, float* as a 4-byte float (FloatSumBufferAggregator
 * buf.putFloat) — big-endian (java.nio.ByteBuffer's default order, big_endian != 0) or little-endian.
 * Host memory only; no device work. */
typedef struct {
  int32_t n_aggs;
  const int32_t* kinds;   /* DG_AGG_* */
  const int32_t* offsets; /* byte offset of each aggregator inside a record */
  int32_t record_size;
  int32_t big_endian;
} dg_record_layout;

int dg_records_pack(const uint64_t* slots, int64_t n, const dg_record_layout* layout, void* out);

/* ---- diagnostics (test harness; no reference counterpart) ----
 * Decode n raw LZ4 blocks (host buffers, <= 64 KiB decoded each) through the same attach-time
 * checkpoint index and HIP decoder the segment path uses. out: n * 65536 bytes, block i at
 * i * 65536; out_lens[i] = decoded length, or -1 when the block fails validation (not decoded).
 * *ms = device time of the decode kernel; prof (optional, NULL = off): 12 words per decoded block,
 * s_memtime stamps of the decoder's phases + counters (tools/lz4_profile.py prints them). */
int dg_debug_lz4_decode(dg_context* ctx, const uint8_t* const* blocks, const int32_t* lens, int32_t n, uint8_t* out,
                        int32_t* out_lens, double* ms, uint64_t* prof);

/* Which HIP decoder the attach-time classification routes one raw LZ4 block to (host only, no
 * device work): *kind = -1 malformed (fails validation), 0 general (k_lz4_decode), 1 general with
 * wide checkpoints, 2 light (k_lz4_light). Since ABI 11. */
int dg_debug_lz4_classify(const uint8_t* block, int32_t len, int32_t* kind);

/* Measurement probes (since ABI 16): what the device and its host link deliver to plain kernels and
 * copies, timed with HIP events over `iters` repetitions after one warm-up; *ms = average per
 * repetition. Buffers are allocated and freed inside the call.
 *   DG_PROBE_COPY      n bytes read and n bytes written by a grid-stride 16-byte copy kernel (HBM)
 *   DG_PROBE_D2H       n bytes device -> pinned host memory (hipMemcpyAsync, DMA)
 *   DG_PROBE_H2D       n bytes pinned host memory -> device
 *   DG_PROBE_GATHER    n elements: an 8-byte word read in order, a 16-byte record gathered at a pseudo-random
 *                      row (a permutation), four 8-byte stores in order (the groupBy reduce's memory floor)
 *   DG_PROBE_ZC_WRITE  n bytes written by a kernel straight into pinned host memory (zero-copy over the link,
 *                      the dg_result_fetch_groups path)
 *   DG_PROBE_SORT      the groupBy sort alone: n packed [key | element index] words with the headline's key
 *                      shape (two uniform 17-bit dictionary ids below 100000), sorted by the engine's radix
 *                      passes (timed alone; the input is rewritten before each repetition) and checked
 *                      ascending afterwards (DG_ERR_DEVICE when not). DG_PROBE_SORT_DEFER=d in the environment:
 *                      only key bits [d, 34) are sorted and the check is on that prefix.
 *   DG_PROBE_CHAIN     n dependent one-workgroup kernels in a row on one stream (each reads the word its
 *                      predecessor wrote): the per-launch cost of a chain of small kernels
 *   DG_PROBE_CHAIN_GRAPH  the same chain captured once into a hipGraph and replayed with hipGraphLaunch
 *                      (capture and instantiation outside the timing)
 *   DG_PROBE_HOST_LAUNCH  host time per kernel launch call (n launches of the chain's kernel, timed on the
 *                      host without waiting for them)
 *   DG_PROBE_HOST_H2D  host time per hipMemcpyAsync of n bytes pinned host -> device (the staged upload)
 *   DG_PROBE_HOST_JOIN host time per cross-stream join (hipEventRecord on one stream + hipStreamWaitEvent
 *                      on another) */
#define DG_PROBE_COPY 0
#define DG_PROBE_D2H 1
#define DG_PROBE_H2D 2
#define DG_PROBE_GATHER 3
#define DG_PROBE_ZC_WRITE 4
#define DG_PROBE_SORT 5
#define DG_PROBE_CHAIN 6
#define DG_PROBE_CHAIN_GRAPH 7
#define DG_PROBE_HOST_LAUNCH 8
#define DG_PROBE_HOST_H2D 9
#define DG_PROBE_HOST_JOIN 10
int dg_debug_probe(int32_t device, int32_t kind, int64_t n, int32_t iters, double* ms);

/* Where the first radix pass's digit totals of the context's last groupBy call came from: *source = 0
 * the histogram kernel over the call's elements (or no sort ran), 1 the segments' cached per-value row
 * counts (built by an earlier eligible groupBy over the same segments and last dimension). */
int dg_debug_groupby_totals_source(dg_context* ctx, int32_t* source);

/* The sort plan of the context's last groupBy call: out[0] = global radix passes of the plan (0: no sort
 * ran), out[1] = low key bits left to the reduce (0: the classic sort over every key bit), out[2] = 1 when a
 * run of equal sorted prefix was longer than the reduce orders and the call sorted classically after all
 * (its result is the classic one). DG_GB_DEFER_BITS=k forces out[1] = k (0: classic), DG_GB_DEFER_PASSES=P the
 * pass count, where the query allows a deferral at all. */
int dg_debug_groupby_sort_plan(dg_context* ctx, int32_t out[3]);

/* The cached long-dimension encoding of a LONG column (built by the first dg_groupby_run* that groups by
 * it or the first dg_topn_run_opts over it; no reference counterpart, the reference reads the long per row): *built = 0 / 1, *cardinality = its
 * distinct values, *device_bytes = HBM held by the ids (4 B per row) and the value list (8 B per value),
 * part of dg_segment_device_bytes, *build_ms = device time of the build. Any output may be NULL.
 * DG_ERR_NOT_FOUND: no such column; DG_ERR_ARG: not a LONG column. */
int dg_debug_long_dim_info(dg_segment* seg, const char* column, int32_t* built, int64_t* cardinality,
                           int64_t* device_bytes, double* build_ms);

#ifdef __cplusplus
}
#endif
#endif /* DRUIDGPU_H */
