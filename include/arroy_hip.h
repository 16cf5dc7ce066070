/*
 * arroy_hip.h — C ABI of libarroy_hip.so: the MI355X (gfx950) implementation of arroy's
 * distance-kernel hot path.  Plain pointers and sizes only; no C++/torch types.
 *
 * arroy (Rust, /root/reference) has no FFI of its own: the boundary of the hot path is
 * the crate-internal `Distance` trait (src/distance/mod.rs:40-124) driven by three
 * batched loops.  Per-pair FFI is useless for a GPU, so every entry point below replaces
 * one *loop* (or one storage-to-memory staging step) of the reference; the citation after
 * each declaration names the reference code it stands in for.  INTEGRATION.md shows the
 * `extern "C"` block and the call-site patches a maintainer would add to arroy.
 *
 * Conventions
 *   - every function returns an `ah_status` (0 = ok); no C++ exception crosses the ABI
 *     (the reference catches worker panics at src/writer.rs:799-827);
 *   - `ah_last_error()` returns the thread's last error text (-> Error::Panic(String),
 *     src/error.rs:84-85);
 *   - the library never keeps a host pointer past the call that received it (LMDB pages
 *     move after writes, src/writer.rs:512-513); output buffers are caller-allocated;
 *   - a finalized dataset changes only through ah_dataset_update_* (exclusive calls); between
 *     updates it is immutable and may be used by any number of host threads concurrently
 *     (Reader is Sync); `ah_build_forest` is single-caller per dataset;
 *   - results never depend on thread / stream / workgroup scheduling.
 *
 * Numerics contract: every f32 result is bit-identical to arroy's x86-64 AVX+FMA tier
 * (src/spaces/simple_avx.rs) for dims >= 32, its SSE tier for 16 <= dims < 32
 * (src/spaces/simple_sse.rs) and its scalar tier below (src/spaces/simple.rs:49-51,81-83).
 */
#ifndef ARROY_HIP_H
#define ARROY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AH_ABI_VERSION 7   /* v2: ah_node.tree is 32 bits, ah_build_options.margin_mode, ah_build_stats.margin_mode_launches,
                                  ah_last_error_detail, ah_dataset_replicate, ah_dataset_upload_flush
                              v3: AH_MARGIN_DENSE_MFMA, ah_build_stats.dense_launches / dense_columns (appended)
                              v4: ah_forest_digest, ah_tuning_set / _get / _reset, ah_debug_launch_coverage,
                                  ah_build_stats.rows_* / screen8_* / screen_unavailable (appended)
                              v5: ah_search_stats / ah_index_search_stats, ah_build_options.max_host_threads (appended),
                                  ah_host_cache_trim, ah_device_cache_trim, ah_dataset_reserve_build, ah_synth_rows_host, ah_build_forest_stream (the node sink during the
                                  build), ah_build_stats.seconds_setup / seconds_after_device / host_blob_recycled
                              v6: ah_debug_dense_tiles, ah_device_cache_stats, ah_forest_digest_keyed, ah_search_stats.descent_block
                              v7: ah_build_stats.seconds_reserve / seconds_reserve_wait (appended), ah_rerank_stats /
                                  ah_dataset_rerank_stats, ah_search_stats.rerank_screened8 / screen8_retried_chunks / descent_multi, AH_SYNTH_CLUSTERED / AH_SYNTH_LOW_RANK (arroy_hip_policy.h),
                                  ah_dataset_replicate falls back to a copy through pinned host memory when the two devices
                                  have no peer access;
                                  device groups (ah_group_*, ah_build_forest_group_stream): additions only, the number stays 7 —
                                  a caller that needs them looks the symbols up; so are ah_dataset_packed_info,
                                  ah_dataset_packed_rows and the test aid ah_debug_query_screen_verify;
                                  v7 additions: updates of a finalized dataset (ah_dataset_update_vectors / _records,
                                  ah_group_update_vectors / _records, the test aid ah_debug_update_paths);
                                  ah_index_footprint_get / ah_index_compact; ah_index_audit / ah_forest_view_audit;
                                  ah_index_drop_trees; ah_index_create_from_encoded; ah_index_encode_nodes;
                                  ah_index_create_from_legacy */

/* every entry point is exported from the shared object (it is built with -fvisibility=hidden) */
#if defined(__GNUC__)
#define AH_API __attribute__((visibility("default")))
#else
#define AH_API
#endif

/* arroy::distances (src/lib.rs:145-150).  The value is also the tag used in files/tests. */
typedef enum ah_metric {
    AH_EUCLIDEAN = 0,              /* src/distance/euclidean.rs                 header {bias:f32}           */
    AH_MANHATTAN = 1,              /* src/distance/manhattan.rs                 header {bias:f32}           */
    AH_COSINE = 2,                 /* src/distance/cosine.rs                    header {norm:f32}           */
    AH_DOT_PRODUCT = 3,            /* src/distance/dot_product.rs               header {extra_dim,norm:f32} */
    AH_BQ_EUCLIDEAN = 4,           /* src/distance/binary_quantized_euclidean.rs header {bias:f32}          */
    AH_BQ_MANHATTAN = 5,           /* src/distance/binary_quantized_manhattan.rs header {bias:f32}          */
    AH_BQ_COSINE = 6               /* src/distance/binary_quantized_cosine.rs    header {norm:f32}          */
} ah_metric;

/* Mapping onto arroy::Error (src/error.rs:6-85). */
typedef enum ah_status {
    AH_OK = 0,
    AH_ERR_INVALID_DIMENSION = 1,  /* Error::InvalidVecDimension  (error.rs:17-23)              */
    AH_ERR_CANCELLED = 2,          /* Error::BuildCancelled       (error.rs:54-55)              */
    AH_ERR_DEVICE = 3,             /* HIP runtime failure      -> Error::Panic(ah_last_error()) */
    AH_ERR_OUT_OF_MEMORY = 4,      /* host or HBM allocation   -> Error::Panic                  */
    AH_ERR_INVALID_ARGUMENT = 5,   /* contract violation       -> Error::Panic                  */
    AH_ERR_MISSING_ITEM = 6,       /* Error::MissingKey           (error.rs:38-46)              */
    AH_ERR_NOT_FINALIZED = 7,      /* dataset used before ah_dataset_finalize -> Error::Panic   */
    AH_ERR_NEED_PREPROCESS = 8     /* DotProduct dataset searched/built before ah_preprocess_dot */
} ah_status;

typedef struct ah_dataset ah_dataset;   /* opaque: the HBM-resident image of ImmutableLeafs */
typedef struct ah_forest ah_forest;     /* opaque: host-side result of one forest build     */

/* Size in bytes of D::Header for the metric (4, or 8 for DotProduct). src/distance/<metric>.rs `Header`. */
AH_API size_t ah_header_size(int metric);
/* Size in bytes of one stored vector: 4*dims for f32 codecs (src/unaligned_vector/f32.rs),
 * ceil(dims/64)*8 for the 1-bit codec (src/unaligned_vector/binary_quantized.rs:80-91). */
AH_API size_t ah_vector_size(int metric, uint32_t dimensions);

AH_API int ah_abi_version(void);
AH_API int ah_device_count(int *out_count);
/* Text of the calling thread's last failure ("" if none).  Never NULL. */
AH_API const char *ah_last_error(void);
/* Structured part of the calling thread's last failure, so that the Rust side can rebuild the typed variants of
 * arroy::Error instead of a string: AH_ERR_INVALID_DIMENSION -> Error::InvalidVecDimension { expected, received }
 * (src/error.rs:17-23), AH_ERR_MISSING_ITEM -> Error::MissingKey { mode: "Item", item } (src/error.rs:58-67). */
typedef struct ah_error_detail {
    int status;          /* the ah_status the failing call returned (AH_OK if the thread has not failed yet) */
    uint32_t item;       /* AH_ERR_MISSING_ITEM: the item id that does not exist                             */
    uint64_t expected;   /* AH_ERR_INVALID_DIMENSION: dimensions (or record bytes) of the dataset            */
    uint64_t received;   /* AH_ERR_INVALID_DIMENSION: what the caller passed                                 */
} ah_error_detail;
AH_API int ah_last_error_detail(ah_error_detail *out);

/* ------------------------------------------------------------------------------------------
 * Dataset = what `ImmutableLeafs::new` builds (src/parallel.rs:271-293): instead of a map
 * id -> pointer into an LMDB page, the records are split into three arrays in HBM (ids,
 * headers, 128-byte-aligned vector rows) in ascending item-id order.
 * ---------------------------------------------------------------------------------------- */

/* `capacity` = number of items that will be uploaded (exact or an upper bound). */
AH_API int ah_dataset_create(int metric, uint32_t dimensions, uint64_t capacity, int device, ah_dataset **out);

/* Stage `n` stored item records `[0u8][header][vector]` (src/node.rs:224-228,252-258) straight
 * from LMDB pages.  record_ptrs[i] may be arbitrarily (mis)aligned; every record is
 * `record_len` bytes (ImmutableLeafs asserts a constant length, src/parallel.rs:286).
 * Ids must be strictly ascending within and across calls (RoaringBitmap iteration order,
 * src/parallel.rs:283).  Records are copied into pinned staging buffers and sent with
 * hipMemcpyAsync, double-buffered; the pointers are not used after return. */
AH_API int ah_dataset_upload_records(ah_dataset *ds, const uint32_t *item_ids, const uint8_t *const *record_ptrs,
                              size_t record_len, size_t n);

/* `Writer::add_item` for a batch (src/writer.rs:380-394): f32 vectors, row-major n x dims; the
 * library applies the codec (`UnalignedVector::from_slice`) and `D::new_header` on device. */
AH_API int ah_dataset_upload_vectors(ah_dataset *ds, const uint32_t *item_ids, const float *vectors, size_t n);

/* Benchmark harness only: materialise `n_items` synthetic items (ids 0..n-1) directly in HBM with
 * the generator of arroy_hip_policy.h, then codec + new_header as in ah_dataset_upload_vectors. */
AH_API int ah_dataset_fill_synthetic(ah_dataset *ds, uint64_t seed, int distribution, uint64_t n_items);

/* Uploads are asynchronous: a call returns once the records are copied out of the caller's pages into the pinned
 * staging ring, the last DMA transfers may still be in flight.  ah_dataset_finalize (and every call that reads the
 * dataset) waits for them; ah_dataset_upload_flush does only that and reports a failed transfer. */
AH_API int ah_dataset_upload_flush(ah_dataset *ds);
/* DotProduct only: records staged with ah_dataset_upload_records carry whatever header the database holds.  Items
 * written by `Writer::add_item` have {extra_dim: 0, norm: 0} until `DotProduct::preprocess` ran
 * (src/distance/dot_product.rs:119-165), so such a dataset still needs ah_preprocess_dot; a caller that staged an
 * already built (preprocessed) database says so here (src/writer.rs:964-976 runs preprocess inside every build). */
AH_API int ah_dataset_set_preprocessed(ah_dataset *ds, int preprocessed);
/* Freeze the dataset (build the id -> row index).  Required before any query/build call. */
AH_API int ah_dataset_finalize(ah_dataset *ds);
/* A replica of `src` on another GPU of the node, copied device to device (xGMI) instead of staged again over PCIe:
 * what the one-tree-batch-per-GPU build needs (`Writer::build` shares ONE ImmutableLeafs between all its tasks,
 * src/writer.rs:530,556-591).  The replica has its own handle and lifetime; destroy it with ah_dataset_destroy. */
AH_API int ah_dataset_replicate(ah_dataset *src, int device, ah_dataset **out);
/* Optional, right after ah_dataset_create: obtain — on a helper thread, while the records are staged over PCIe — the device
 * memory the first `n_trees`-tree build of this dataset will ask for (the binary16 / int8 copies of the rows, the build's
 * scratch) and park it in the library's device cache.  Fresh HBM can cost the driver 20+ ms per GB (a box whose memory was
 * just released by another process scrubs it); `Writer::build` knows its tree count before it collects the items
 * (src/writer.rs:518-519).  split_after 0 = dimensions.  Never fails for lack of memory: the build then allocates itself. */
AH_API int ah_dataset_reserve_build(ah_dataset *ds, uint32_t n_trees, uint32_t split_after);
AH_API int ah_dataset_len(const ah_dataset *ds, uint64_t *out_n_items);
/* `Reader::item_vector` (src/reader.rs:266-276): decoded f32 vector (dims floats; +-1.0 for BQ). */
AH_API int ah_dataset_item_vector(ah_dataset *ds, uint32_t item_id, float *out_vector);
/* Copy stored headers of rows [first_row, first_row+n) to the host (header_size bytes each): what the
 * host needs to rewrite LMDB after `ah_preprocess_dot`. */
AH_API int ah_dataset_read_headers(ah_dataset *ds, uint64_t first_row, uint64_t n, void *out_headers);
AH_API int ah_dataset_destroy(ah_dataset *ds);

/* `DotProduct::preprocess` (src/distance/dot_product.rs:119-165): max norm over all items, then
 * header.norm = max^2, header.extra_dim = sqrt(max^2 - |v|^2) for every item, on device. */
AH_API int ah_preprocess_dot(ah_dataset *ds, float *out_max_norm);

/* Updates of a finalized dataset (v7 additions): `Writer::build`'s item changes (src/writer.rs:497-505: to_delete = updated,
 * to_insert = items & updated) applied to the dataset on its device, so that an incremental build re-sends only the
 * changed rows instead of staging every item again.  First every id of remove_ids leaves (ids that are not present are
 * ignored, as `descendants -= to_delete` ignores them), then every id of upsert_ids is written, replacing its row or adding
 * a new one.  Both lists strictly ascending; an id may be in both.  Only the upserted rows cross PCIe, through the staging
 * ring, codec and header kernels of ah_dataset_upload_vectors / _records.
 *   - Afterwards the dataset behaves bit for bit like one freshly staged and finalized with the resulting items: rows in
 *     ascending-id order, the same id -> row table, the same results of every call that reads it.  The copies the library
 *     derives from the rows (binary16 / int8 screens, the packed scan copy) and its decisions about them are dropped and
 *     rebuilt on demand; ah_dataset_rerank_stats restarts.
 *   - DotProduct: the dataset needs ah_preprocess_dot again after every update (AH_ERR_NEED_PREPROCESS until then).
 *   - All or nothing: bad arguments (unsorted or duplicate ids, a wrong record_len -> AH_ERR_INVALID_DIMENSION, a NULL
 *     pointer with a non-zero count, a group member -> AH_ERR_INVALID_ARGUMENT, an unfinalized dataset ->
 *     AH_ERR_NOT_FINALIZED) and failed allocations leave the dataset exactly as it was.
 *   - Exclusive: refused (AH_ERR_INVALID_ARGUMENT) while any ah_index built on the dataset is alive — an index holds row
 *     positions.  Any other call on the dataset concurrent with an update is the caller's to prevent, as for staging.
 *   - The dataset may grow past the capacity given to ah_dataset_create, shrink to no items, and an empty dataset may be
 *     updated.  A finalized dataset is therefore immutable between updates only. */
AH_API int ah_dataset_update_vectors(ah_dataset *ds, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                                     const float *vectors, size_t n_upsert);
AH_API int ah_dataset_update_records(ah_dataset *ds, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                                     const uint8_t *const *record_ptrs, size_t record_len, size_t n_upsert);
/* Test aid (v7 addition): how the updates of this dataset were applied so far — rows written in place (the id set did not
 * change), appended after the last row (every new id above the last one, room in the allocation), or merged into new arrays. */
AH_API int ah_debug_update_paths(ah_dataset *ds, uint64_t *out_in_place, uint64_t *out_appended, uint64_t *out_merged);

/* ------------------------------------------------------------------------------------------
 * Search side (src/reader.rs:376-400, 607-640)
 * ---------------------------------------------------------------------------------------- */

/* Raw batched `D::built_distance(query, item)` (non-normalized), `QueryBuilder::by_vector`
 * semantics for the query (src/reader.rs:64-75: codec + `D::new_header`).  `item_ids == NULL`
 * scans rows 0..n-1 of the dataset in id order; otherwise one distance per listed id. */
AH_API int ah_distances_by_vector(ah_dataset *ds, const float *query, const uint32_t *item_ids, size_t n, float *out);
/* Same with the query taken from a stored item (`by_item`, src/reader.rs:46-51). */
AH_API int ah_distances_by_item(ah_dataset *ds, uint32_t query_item, const uint32_t *item_ids, size_t n, float *out);

/* The re-rank loop + `median_based_top_k` + `D::normalized_distance` (src/reader.rs:381-399):
 * `sorted_ids` ascending and unique (src/reader.rs:378-379) or NULL for "all items".  Writes
 * min(k, n) pairs ordered by (OrderedFloat(distance), id) ascending. */
AH_API int ah_rerank_by_vector(ah_dataset *ds, const float *query, const uint32_t *sorted_ids, size_t n, size_t k,
                        uint32_t *out_ids, float *out_distances, size_t *out_n);
AH_API int ah_rerank_by_item(ah_dataset *ds, uint32_t query_item, const uint32_t *sorted_ids, size_t n, size_t k,
                      uint32_t *out_ids, float *out_distances, size_t *out_n);
/* Many queries in one submission (candidate lists concatenated; list q is
 * ids[offsets[q] .. offsets[q+1])).  Outputs are n_queries x k, short lists padded with id
 * 0xFFFFFFFF / distance NaN; out_counts[q] = min(k, len_q) says how many are real (0xFFFFFFFF is
 * also a legal item id, src/tests/writer.rs:161-179).  Results are identical to n_queries single
 * calls; a submission with >= 2 candidates per stored row is evaluated row-major on the device
 * (every row leaves HBM once per submission). */
AH_API int ah_rerank_batch(ah_dataset *ds, const float *queries, size_t n_queries, const uint32_t *ids,
                    const uint64_t *offsets, size_t k, uint32_t *out_ids, float *out_distances,
                    uint32_t *out_counts);

/* ABI v7.  Where the wall time of ah_rerank_batch went, summed over the calls of every thread since the last reset — kept
 * only while the tunable AH_RERANK_TIMING is 1 (ah_tuning_set; two extra events and a few clock reads per submission).  A
 * submission that is slow on one box and not on another shows here whether the host (prep / ids / enqueue) or the device
 * (sync_wait) paid: bench.py prints it next to the re-rank figures. */
typedef struct ah_rerank_stats {
    uint64_t calls;               /* ah_rerank_batch calls (their sub-batches summed)                                     */
    uint64_t queries, candidates;
    double seconds_wall;          /* entry -> return                                                                      */
    double seconds_prep;          /* entry -> first enqueue: argument checks, segment / tile tables, scratch, query copy  */
    double seconds_ids;           /* host copies of the candidate ids into pinned memory (they overlap the device's work) */
    double seconds_enqueue;       /* launching copies and kernels (the calls themselves, not their execution)             */
    double seconds_sync_wait;     /* blocked in hipStreamSynchronize: the device still had work when the host was done    */
    double seconds_device_span;   /* HIP events: first enqueue of the submission -> its stream idle                       */
    /* how the certified top-k screen went (kept whatever AH_RERANK_TIMING says) */
    uint64_t queries_screened;    /* queries answered through the screen (int8 or binary16 rows first, f32 for the survivors) */
    uint64_t survivors;           /* ... candidates of theirs evaluated in f32                                            */
    uint64_t chunks_int8;         /* sub-batches whose screen started on the int8 copy of the rows and stayed there       */
    uint64_t chunks_int8_retried; /* ... that left more survivors than the selection holds and ran again on binary16 rows
                                     (eight of them within one window of 64 sub-batches the int8 stage served switch that
                                     stage off for the dataset) */
} ah_rerank_stats;
AH_API int ah_dataset_rerank_stats(ah_dataset *ds, ah_rerank_stats *out, int reset);
/* The packed copy of the rows that the ungathered f32 scan reads (tunable AH_SCAN_PACKED): *out_present = 1 when it exists,
 * *out_raw_rows = its rows kept in f32 (an inf / NaN, or an exponent spread of 15 binades or more).  Either pointer may be
 * NULL.  Made by the first ah_distances_by_* / ah_bench_scan call over all rows, never by a build or a search. */
AH_API int ah_dataset_packed_info(ah_dataset *ds, int *out_present, uint64_t *out_raw_rows);
/* The same, plus *out_grid_rows = the rows of the copy stored in the 24-bit fixed-point form (tunable AH_SCAN_GRID, read when
 * the copy is made: rows whose elements are all integer multiples of one power of two, magnitudes below 2^23); they are not
 * among the raw rows.  Any pointer may be NULL.  An addition to v7: a caller that needs it looks the symbol up. */
AH_API int ah_dataset_packed_rows(ah_dataset *ds, int *out_present, uint64_t *out_raw_rows, uint64_t *out_grid_rows);
/* Test aid: the counters of the tunable AH_SCREEN_VERIFY=1 for the query-side screens (the certified top-k screen of
 * ah_search_batch and ah_rerank_batch on this dataset).  Under it every candidate with a finite screen value is also evaluated
 * in the reference's f32 arithmetic: *out_checked counts those candidates, *out_violations the ones whose reference distance
 * fell outside the interval [L, U] the screen derived for them (must be 0).  Both stay 0 while the tunable is 0.  Either
 * pointer may be NULL; reset != 0 zeroes the counters after reading them. */
AH_API int ah_debug_query_screen_verify(ah_dataset *ds, uint64_t *out_checked, uint64_t *out_violations, int reset);

/* ------------------------------------------------------------------------------------------
 * Build side (src/writer.rs:1193-1233, 1398-1531; src/distance/mod.rs:126-223)
 * ---------------------------------------------------------------------------------------- */

#define AH_SPLIT_SAMPLES 12   /* choose_two + 10 x choose (src/distance/mod.rs:139,149-152) */

/* The margin loop (src/writer.rs:1201-1207,1424-1431,1494-1501): `D::side(normal, item)` for every
 * listed item.  `normal_vector` is in the metric's codec (ah_vector_size bytes), `normal_header`
 * is D::Header.  Bit i (LSB first) of side_bits = 1 when item i goes Right
 * (`margin.is_sign_positive()`, src/distance/mod.rs:103-110); (n+7)/8 bytes. Optionally also
 * returns the margins themselves (out_margins may be NULL). */
AH_API int ah_split_sides(ah_dataset *ds, const void *normal_vector, const void *normal_header,
                   const uint32_t *sorted_ids, size_t n, uint8_t *side_bits, uint64_t *out_n_left,
                   float *out_margins);

/* The margins of the tree descent (src/reader.rs:366-369): `D::margin(&normal_i, query_leaf)` for many split-plane
 * normals at once.  `normals` is a dataset whose ITEMS are normals (stage them with ah_dataset_upload_records:
 * header = the normal's header); `leaf_vector` / `leaf_header` is the query leaf in the metric's codec
 * (by_vector: codec + D::new_header; by_item: the stored item).  item_ids NULL = every normal in row order. */
AH_API int ah_margins(ah_dataset *normals, const void *leaf_vector, const void *leaf_header, const uint32_t *item_ids,
                      size_t n, float *out_margins);

/* `D::create_split` (src/distance/{euclidean.rs:55-77,cosine.rs:73-85,dot_product.rs:98-113,...}) with the
 * randomness supplied by the host: sample_ids[0..1] = choose_two, [2..11] = the ten `choose` draws
 * (the RNG policy stays in the caller, as with `R: Rng`). */
AH_API int ah_create_split(ah_dataset *ds, const uint32_t sample_ids[AH_SPLIT_SAMPLES], void *out_normal_vector,
                    void *out_normal_header);

typedef void (*ah_progress_fn)(void *user, uint32_t level, uint64_t nodes_done, uint64_t items_routed);

/* How the margin pass of a level (src/writer.rs:1201-1207 for every pending node of every tree) is laid out on the
 * device.  Every mode produces the same forest bit for bit; AUTO picks per level with a cost model.  The other values
 * pin one kernel family for every level where it is legal (f32 metrics, dimensions >= 32, full-dataset trees, >= 2
 * trees; LDS modes additionally need the group's normals of the level to fit in LDS) and use the node-major kernel
 * elsewhere: they exist so that tests can compare EVERY kernel instantiation with the oracle, and for A/B timing. */
typedef enum ah_margin_mode {
    AH_MARGIN_AUTO = 0,
    AH_MARGIN_NODE_MAJOR = 1,      /* one tree at a time, tiles of one node, its normal in LDS                       */
    AH_MARGIN_ROWS_2 = 2,          /* row-major: one pass over the rows serves 2 / 4 / 8 / 16 trees, normals via L2   */
    AH_MARGIN_ROWS_4 = 4,
    AH_MARGIN_ROWS_8 = 8,
    AH_MARGIN_ROWS_16 = 16,
    AH_MARGIN_ROWS_LDS_8 = 0x108,  /* row-major, all normals of a group of 8 / 16 trees resident in LDS               */
    AH_MARGIN_ROWS_LDS_16 = 0x110,
    /* Dense screen on the matrix units (ABI v3): the binary16 screen values of ALL (row, node) pairs of a level as one
     * matrix product rows x normals^T (v_mfma_f32_32x32x16_f16), of which every row uses one entry per tree; pairs the
     * screen cannot decide are recomputed in the reference's f32 arithmetic, so the forest is the same bit for bit.
     * Cheaper than the row-major passes while a tree has few nodes (top ~6 levels); needs the screen, i.e. it is
     * ignored (node-major instead) together with AH_MARGIN_EXACT_ONLY and beyond AH_DENSE_MAX_COLS nodes per level. */
    AH_MARGIN_DENSE_MFMA = 0x200,
    /* Flag, OR-ed into any of the above: evaluate every margin in the reference's f32 arithmetic only.  Without it the
     * f32 metrics first evaluate a *certified screen*: the same dot product on a binary16 shadow copy of the rows and
     * of the level's normals (half the bytes), with a rigorous bound E on |screen - reference f32 margin| derived
     * from the measured quantisation errors ("certified screening"); only the SIGN of a margin is ever
     * used (`D::side`, src/distance/mod.rs:103-110), so |screen| > E decides the side and every other pair (about 1 %)
     * is recomputed with the reference arithmetic in the same kernel.  Sides — hence forests — are identical. */
    AH_MARGIN_EXACT_ONLY = 0x1000
} ah_margin_mode;

typedef struct ah_build_options {
    uint32_t n_trees;              /* trees built by THIS call (the caller shards trees over GPUs)   */
    uint32_t split_after;          /* 0 = dimensions (src/writer.rs:474-477)                         */
    const uint64_t *tree_seeds;    /* n_trees seeds (src/writer.rs:575: one RNG per root task)       */
    const volatile int *cancel;    /* polled while a level runs (the reference polls per node and per item,
                                      src/writer.rs:1178,1196): non-zero -> launches that have not started yet drain
                                      without work, the call returns AH_ERR_CANCELLED when the level's stream is idle
                                      (at most one level: <= 0.25 s at 10M x 768 x 100 trees) */
    ah_progress_fn progress;       /* may be NULL (src/writer.rs:53-69 SubStep).  Called once per digested level with
                                      `level` = depth + 1: ascending, except at the bottom of a build whose last levels
                                      run group of trees by group of trees (AH_BUILD_TAIL_GROUPS), where every group
                                      reports its own last levels; nodes_done / items_routed never decrease */
    void *progress_user;
    uint32_t max_trees_in_flight;  /* 0 = as many as HBM allows                                      */
    uint32_t margin_mode;          /* ah_margin_mode; 0 = AH_MARGIN_AUTO                             */
    uint32_t max_host_threads;     /* ABI v5: host threads this build may keep busy for its output path (page commits,
                                      bounce copies, node list); 0 = 8.  The reference gives a build its rayon pool
                                      (src/writer.rs:538-548); eight concurrent builds of an 8-GPU node share the host */
    uint32_t reserved0;            /* 0 */
} ah_build_options;

/* Whole-forest build: `make_tree_in_file` for every tree (src/writer.rs:556-591,1167-1261) with the
 * randomness policy of arroy_hip_policy.h.  Level-synchronous on device; nothing is visible to the
 * caller until the whole forest exists (src/writer.rs:597-607). */
AH_API int ah_build_forest(ah_dataset *ds, const ah_build_options *options, ah_forest **out);

/* The same build over caller-given item subsets: `incremental_index_large_descendant` (src/writer.rs:660-739), i.e.
 * `make_tree_in_file` for every Descendants node that grew beyond split_after during an incremental insert.  Tree t
 * of the result covers the ascending id list item_ids[offsets[t] .. offsets[t+1]) and uses options->tree_seeds[t];
 * options->n_trees = number of subsets.  A subset that fits in one Descendants node yields a one-node tree. */
AH_API int ah_build_subtrees(ah_dataset *ds, const ah_build_options *options, const uint32_t *item_ids,
                             const uint64_t *offsets, ah_forest **out);

enum { AH_NODE_DESCENDANTS = 1, AH_NODE_SPLIT = 2 };   /* node tags, src/node.rs:216-241 */

typedef struct ah_node {
    uint8_t kind;           /* AH_NODE_DESCENDANTS | AH_NODE_SPLIT                                   */
    uint8_t has_normal;     /* 0 = `normal: None` (random split fallback, src/writer.rs:1220-1227)   */
    uint16_t reserved;      /* 0                                                                    */
    uint32_t tree;          /* tree index inside this forest (arroy's target_n_trees, src/writer.rs:1371-1380,
                               can exceed 65 535, hence 32 bits since ABI v2)                         */
    uint32_t left, right;   /* forest-local node indices (SPLIT)                                    */
    uint64_t offset;        /* SPLIT: byte offset into the normals blob; DESCENDANTS: first id index */
    uint32_t count;         /* DESCENDANTS: number of item ids; SPLIT: items under the node         */
    uint32_t depth;
} ah_node;

typedef struct ah_forest_view {
    uint32_t n_trees;
    uint64_t n_nodes;
    const uint32_t *roots;        /* n_trees forest-local node indices                               */
    const ah_node *nodes;         /* n_nodes, children before parents (post-order) inside each tree  */
    /* Normals: one fixed-size record per split node at byte `ah_node.offset` of `normals`.  Inside a record
     * the vector (metric codec, ah_vector_size bytes) sits at `normal_vector_offset` and D::Header
     * (ah_header_size bytes) at `normal_header_offset`; `normal_stride` may exceed their sum (the f32 metrics pad a
     * record to whole 128-byte lines, the padding is zero).  (The records are the device layout copied back
     * verbatim, so nothing is repacked on the host; the Rust side copies both parts into the LMDB value
     * `[2u8][left][right][header][vector]` anyway, src/node.rs:229-237.) */
    const uint8_t *normals;
    uint64_t normals_len;
    uint64_t normal_stride;
    uint64_t normal_vector_offset;
    uint64_t normal_header_offset;
    const uint32_t *descendants;  /* item ids, ascending inside each Descendants node                */
    uint64_t descendants_len;
} ah_forest_view;

typedef struct ah_build_stats {
    double seconds_total;         /* wall time of ah_build_forest                                    */
    double seconds_device;        /* HIP-event time of all kernels                                   */
    double seconds_margin;        /* HIP-event time of the margin/side kernel only                   */
    uint64_t margin_evaluations;  /* number of (item, node-visit) units incl. retries                */
    uint64_t margin_launches;
    uint64_t margin_row_passes;   /* row-major passes (each streams all rows once and serves several trees)  */
    uint64_t split_nodes, descendant_nodes, dummy_normals, retries;
    uint32_t levels;
    /* margin launches per kernel family: [0] node-major f32, [1] rows x2, [2] rows x4, [3] rows x8, [4] rows x16,
     * [5] LDS x8, [6] LDS x16, [7] node-major 1-bit */
    uint64_t margin_mode_launches[8];
    uint64_t screened_launches;   /* margin launches that ran the certified binary16 screen                  */
    uint64_t screen_fallbacks;    /* (item, node) pairs the screen could not decide (recomputed in f32)       */
    uint64_t screen_violations;   /* AH_SCREEN_VERIFY=1 only: decided pairs whose f32 side differs (must be 0) */
    uint64_t dense_launches;      /* ABI v3: levels whose first attempt ran as one MFMA product (AH_MARGIN_DENSE_MFMA)  */
    uint64_t dense_columns;       /* ABI v3: normals (columns) those products covered, summed over the levels          */
    /* ABI v4: which schedule variants of the row-major pass ran (kernel launches, not passes) */
    uint64_t rows_xcd_launches;   /* launches that pinned every (chunk, tree group) to one XCD                          */
    uint64_t rows_nt_launches;    /* ... of which streamed the rows with non-temporal loads                             */
    uint64_t rows_split_launches; /* extra launches of passes cut at the work-item limit of one dispatch                */
    uint64_t screen8_pairs;       /* (item, node) pairs that met the int8 first stage of the node-major screen          */
    uint64_t screen8_decided;     /* ... of which its first digit decided (768 bytes of a 768-d row)                    */
    uint64_t screen8b_decided;    /* ... and of the rest, decided by the rows' second int8 digit (768 more bytes); what is
                                     left goes on to the binary16 stage                                                  */
    uint32_t screen_unavailable;  /* the build wanted the screen but its copies could not be allocated: f32 arithmetic  */
    uint32_t tail_groups;         /* (was reserved) groups of trees the last big level and what followed it ran in, summed
                                     over the batches: their ids and normals left the device under the next group's
                                     kernels (AH_BUILD_TAIL_GROUPS); 0 = every level for all trees                      */
    /* ABI v5: where the wall time outside the kernels went (summed over the batches of the build) */
    double seconds_setup;         /* entry of a batch -> its first launch (device buffers, pinned memory, host blobs)    */
    double seconds_after_device;  /* last launch of a batch -> its return (ids' read-back, node list, teardown)          */
    uint64_t host_blob_recycled;  /* output blobs (normals, ids) taken committed from the pool of destroyed forests     */
    /* ABI v7: ah_dataset_reserve_build, as the first build after it saw it */
    double seconds_reserve;       /* run time of the helper thread that obtained the build's device memory under the staging */
    double seconds_reserve_wait;  /* ... and how long this build waited for it before it started (NOT in seconds_total)      */
} ah_build_stats;

AH_API int ah_forest_view_get(const ah_forest *forest, ah_forest_view *out);
/* 64-bit digest of the CONTENT of a forest, independent of how it was laid out in memory (batching, record padding):
 * per tree, in the node order of ah_forest_view (post-order), kind / has_normal / children / count / depth of every
 * node, header + vector bytes of every split plane, item ids of every Descendants node.  Two builds of the same
 * dataset with the same seeds must agree whatever the margin mode or tuning: bench.py and the GPU tests compare the
 * screened and the f32-only build of the 10M x 100-tree forest this way.  out_per_tree: n_trees values or NULL.
 * The recipe (tests/test_gpu_forest_witnesses.py restates it in Python and checks that every field below moves the value),
 * with mix = ah_mix64 of arroy_hip_policy.h and H(bytes, seed) = the four-lane byte hash `hash_bytes` of forest.hip:
 *   tree t, whose first node in the view is node b:  h = mix(0x61727279 + t); then for every node i of the tree, ascending,
 *     h = mix(h ^ H(four u64 {kind | has_normal << 8 | depth << 32, count, left - b, right - b}, i - b))   (Descendants: 0, 0)
 *     a split with a normal:  h = mix(h ^ H(record[normal_vector_offset, normal_header_offset), 1)), the vector and its zero
 *                             padding, then h = mix(h ^ H(record[normal_header_offset, + 8), 2)), D::Header zero-padded
 *     a Descendants node:     h = mix(h ^ H(its `count` u32 ids, 3))
 *   per_tree[t] = h;  total = mix(n_trees), then total = mix(total ^ per_tree[t]) for t ascending. */
AH_API int ah_forest_digest(const ah_forest *forest, uint64_t *out_per_tree, uint64_t *out_total);
/* ABI v6: the per-tree digests with the caller's key in place of the tree's index inside THIS forest — e.g. the tree's
 * index in the whole index when the forest is one GPU's share of it (trees t = device mod G, src/writer.rs:556-591): the
 * digest of tree t is then the same whichever share, batch or device built it, and the union of the shares' digests can be
 * compared with the digests of a one-GPU build (bench.py does, `build_10m.union`).  tree_keys / out_per_tree: n_trees values. */
AH_API int ah_forest_digest_keyed(const ah_forest *forest, const uint64_t *tree_keys, uint64_t *out_per_tree);
AH_API int ah_forest_stats(const ah_forest *forest, ah_build_stats *out);
/* Node sink in the shape `TmpNodes::put` expects (src/parallel.rs:130-147): children first, parent
 * last (post-order), per tree. `payload`: SPLIT -> the normal record of ah_forest_view (vector at
 * normal_vector_offset, header at normal_header_offset) or NULL for `normal: None`; DESCENDANTS -> u32 ids. */
typedef int (*ah_node_sink_fn)(void *user, uint32_t tree, uint32_t node, uint8_t kind, uint32_t left,
                               uint32_t right, const void *payload, size_t payload_len);
AH_API int ah_forest_visit(const ah_forest *forest, ah_node_sink_fn sink, void *user);
AH_API int ah_forest_destroy(ah_forest *forest);

/* ------------------------------------------------------------------------------------------
 * Streaming build (ABI v5): the node sink DURING the build.  `Writer::build` hands every finished tree node to
 * `TmpNodes::put` (src/parallel.rs:130-147) and drains the tmp files into LMDB at the end (src/writer.rs:597-607);
 * nothing in the reference ever needs the whole forest in one piece.  ah_build_forest_stream therefore never
 * materialises it: the split planes of a level (as soon as the level is final) and the item-id lists (after the last
 * level) travel device -> pinned ring -> `sink`, batch by batch, while the next levels are computed.  The host keeps
 * 64 MiB of pinned memory and the node table instead of the 9.4 GB a 10M x 768 x 100-tree forest occupies.
 *
 * Order: breadth-first — a split node arrives BEFORE its children (its record names their ids; the reference's ids are
 * arbitrary too, src/parallel.rs:239-254, and TmpNodes is an append-only log keyed by id).  The Descendants nodes of a
 * tree arrive after all of its split nodes, in ascending (tree, position) order over the whole call: after the last
 * level, or — when the last big level and what follows it run in groups of trees (AH_BUILD_TAIL_GROUPS, the default
 * for builds whose id lists are worth it) — a group's Descendants as soon as that group is complete, i.e. between the
 * split planes of the groups after it.  `id`s are unique over the whole call, dense from 0, assigned in creation
 * order (a node's children are id-consecutive: left, left + 1).  `sink` is called from ONE library thread, one batch at
 * a time; `nodes` and `payload` are valid only during the call (the payload is the pinned DMA buffer itself: copy or
 * encode out of it).  A non-zero return stops the build: AH_ERR_CANCELLED.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_stream_node {
    uint32_t id;             /* this node                                                                      */
    uint32_t tree;           /* tree index inside this build                                                   */
    uint8_t kind;            /* AH_NODE_SPLIT | AH_NODE_DESCENDANTS                                            */
    uint8_t has_normal;      /* SPLIT: 0 = `normal: None` (src/writer.rs:1220-1227): no payload                 */
    uint16_t reserved;
    uint32_t left, right;    /* SPLIT: ids of the children                                                     */
    uint32_t count;          /* DESCENDANTS: item ids in the payload; SPLIT: items under the node              */
    uint32_t depth;
    uint64_t payload_offset; /* into ah_node_batch.payload.  SPLIT: the normal record (vector at normal_vector_offset,
                                D::Header at normal_header_offset, as in ah_forest_view); DESCENDANTS: `count` u32 item
                                ids, ascending                                                                  */
} ah_stream_node;

typedef struct ah_node_batch {
    uint32_t kind;           /* all nodes of a batch are of one kind                                           */
    uint32_t level;          /* SPLIT: depth of the nodes; DESCENDANTS: 0                                      */
    uint64_t n_nodes;
    const ah_stream_node *nodes;
    const uint8_t *payload;
    uint64_t payload_len;
    uint64_t normal_stride, normal_vector_offset, normal_header_offset;
} ah_node_batch;

typedef int (*ah_node_batch_fn)(void *user, const ah_node_batch *batch);

/* `options` as for ah_build_forest.  out_roots: options->n_trees node ids (the roots, in tree order); out_stats may be
 * NULL.  The forest is the one ah_build_forest builds for the same seeds, node for node (only the numbering differs:
 * ah_forest_view numbers children before parents). */
AH_API int ah_build_forest_stream(ah_dataset *ds, const ah_build_options *options, ah_node_batch_fn sink, void *user,
                                  uint32_t *out_roots, ah_build_stats *out_stats);

/* ------------------------------------------------------------------------------------------
 * Encoded node stream (v7 additions; callers look the symbols up): the same streaming build, but every node arrives as
 * the bytes `NodeCodec::bytes_encode` would produce (src/node.rs:229-241), encoded on the device, so a Writer only has to
 * `put(key, slice)`:
 *   split        [2][left u32 BE][right u32 BE], then [D::Header][vector] (ah_header_size + ah_vector_size bytes) unless
 *                `normal: None`
 *   Descendants  [1] + RoaringBitmap::serialize_into of the item ids (portable format, no run containers)
 * Same forest, same batch order and same ah_stream_node metadata as ah_build_forest_stream for the same seeds, except:
 *   - id, left, right, out_roots and the child ids inside the values have `node_id_base` added (reserve the range with one
 *     bump of the id generator); a build whose ids would pass 2^32 - 1 is refused with AH_ERR_INVALID_ARGUMENT;
 *   - a batch has normal_stride = normal_vector_offset = normal_header_offset = 0 (the mark of an encoded batch), and node
 *     i's value is payload[nodes[i].payload_offset, nodes[i + 1].payload_offset); the last one ends at payload_len.
 * The values are encoded piece by piece on the read-back worker's stream into a device buffer as large as the pinned
 * double buffer; if that buffer cannot be had the call returns AH_ERR_OUT_OF_MEMORY (there is no unencoded fall-back).
 * ah_build_forest_group_stream has no encoded twin.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_encode_options {
    uint32_t node_id_base;   /* added to every node id of the call */
    uint32_t flags;          /* 0 */
} ah_encode_options;
AH_API int ah_build_forest_stream_encoded(ah_dataset *ds, const ah_build_options *options, const ah_encode_options *enc,
                                          ah_node_batch_fn sink, void *user, uint32_t *out_roots, ah_build_stats *out_stats);
/* Descendants values of `n_lists` ascending id lists, ids[offsets[i] .. offsets[i + 1]), encoded on ds's device (the tag byte
 * included).  out_value_offsets[0 .. n_lists]: value i is out_values[out_value_offsets[i], out_value_offsets[i + 1]).
 * out_values == NULL: only the offsets (the sizes).  A list that does not ascend strictly, or an out_cap smaller than
 * out_value_offsets[n_lists], is AH_ERR_INVALID_ARGUMENT; nothing is written past out_cap. */
AH_API int ah_encode_descendants(ah_dataset *ds, const uint32_t *ids, const uint64_t *offsets, size_t n_lists,
                                 uint8_t *out_values, uint64_t out_cap, uint64_t *out_value_offsets);

/* ------------------------------------------------------------------------------------------
 * Device groups: one replica of the dataset per listed device, staged from ONE host pass, and one forest built on all of
 * them.  Trees are independent given the read-only dataset (`Writer::build` runs one task per root over ONE shared
 * ImmutableLeafs, src/writer.rs:530,556-591), so a group shards TREES: tree t of a build is built on member t mod G, and
 * the forest is the one a single dataset builds with the same seeds, node for node.
 *
 * Staging: every chunk of an upload is gathered from the caller's pages into the group's pinned ring ONCE and sent to
 * every member by one hipMemcpyAsync per member from that same slot, on the member's own stream (no peer copy, no second
 * host pass); each member then runs the codec / header kernels on its own device.  A slot is reused once every member's
 * transfer out of it has completed; the gather of chunk k+1 overlaps the transfers of chunk k.  Group calls are
 * single-caller, like the staging calls of a dataset.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_group ah_group;   /* opaque: one replica dataset per listed device */

/* `devices[0 .. n_devices)`: a device may be listed more than once (several replicas on one GPU).  n_devices == 0, a NULL
 * pointer or a device index >= ah_device_count is AH_ERR_INVALID_ARGUMENT, reported before any device is touched. */
AH_API int ah_group_create(int metric, uint32_t dimensions, uint64_t capacity, const int *devices, uint32_t n_devices,
                           ah_group **out);
/* The contracts of ah_dataset_upload_records / ah_dataset_upload_vectors, for every member at once. */
AH_API int ah_group_upload_records(ah_group *group, const uint32_t *item_ids, const uint8_t *const *record_ptrs,
                                   size_t record_len, size_t n);
AH_API int ah_group_upload_vectors(ah_group *group, const uint32_t *item_ids, const float *vectors, size_t n);
AH_API int ah_group_upload_flush(ah_group *group);
AH_API int ah_group_set_preprocessed(ah_group *group, int preprocessed);
AH_API int ah_group_finalize(ah_group *group);
/* ah_preprocess_dot on every member; the members' max norms must agree bit for bit (AH_ERR_DEVICE otherwise). */
AH_API int ah_group_preprocess_dot(ah_group *group, float *out_max_norm);
/* ah_dataset_reserve_build for every member, with its share of `n_trees` (trees t = member mod G). */
AH_API int ah_group_reserve_build(ah_group *group, uint32_t n_trees, uint32_t split_after);
AH_API int ah_group_size(const ah_group *group, uint32_t *out_n_members);
/* Member i as a BORROWED dataset handle: every call that reads a dataset takes it (distances, re-rank, ah_index_create*,
 * search, the builds ...).  Every call that would change one replica without the others refuses it with
 * AH_ERR_INVALID_ARGUMENT — ah_dataset_upload_records / _vectors, ah_dataset_fill_synthetic, ah_dataset_set_preprocessed,
 * ah_dataset_finalize, ah_preprocess_dot — and so does ah_dataset_destroy: use the ah_group_* call.  It lives as long as
 * the group. */
AH_API int ah_group_member(ah_group *group, uint32_t i, ah_dataset **out);
AH_API int ah_group_destroy(ah_group *group);   /* the members, the pinned ring, everything */
/* ah_dataset_update_vectors / _records for every member at once (v7 additions): the upserted rows go through the group's
 * pinned ring once, one transfer per member, and each member merges on its own device.  Two phases: every member's
 * buffers are obtained and filled first, then all members commit; a failure on any member leaves every member unchanged. */
AH_API int ah_group_update_vectors(ah_group *group, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                                   const float *vectors, size_t n_upsert);
AH_API int ah_group_update_records(ah_group *group, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                                   const uint8_t *const *record_ptrs, size_t record_len, size_t n_upsert);

/* One forest on every member: `options->n_trees` / `tree_seeds` describe the WHOLE forest; tree t is built on member
 * t mod G by one host thread per member (each holds its own device; options->max_host_threads is split between them; the
 * caller's current device is restored).  `sink` sees the contract of ah_build_forest_stream: called from one library
 * thread at a time, a split node before its children, ids unique and dense from 0 over the whole call, children
 * id-consecutive, `tree` = the global tree index; out_roots in global tree order.  One difference: the members' batches
 * interleave in the order they reach the sink, so the Descendants nodes arrive in ascending (tree, position) order per
 * member, not over the whole call (a sink keyed by id, as TmpNodes is, does not notice).  `options->cancel` stops every member;
 * `progress` is called from the calling thread only, with nodes_done / items_routed summed over the members (they never
 * decrease).  A non-zero sink return, a cancel or a member's error stops all members; no sink call follows the decision,
 * every thread is joined and the FIRST error's status and text are returned; the group stays usable.  out_stats (may be
 * NULL): the members' counters summed, levels = the deepest member's, seconds_total = wall time of this call;
 * out_member_stats (may be NULL): one entry per member. */
AH_API int ah_build_forest_group_stream(ah_group *group, const ah_build_options *options, ah_node_batch_fn sink, void *user,
                                        uint32_t *out_roots, ah_build_stats *out_stats, ah_build_stats *out_member_stats);

/* ------------------------------------------------------------------------------------------
 * Whole search on device (src/reader.rs:317-401): the forest mirrored in HBM next to its dataset, best-first
 * descent + candidate collection + sort/dedup + re-rank + top-k for a batch of queries in one call.
 * Node identity (the tie-break of the reference's BinaryHeap<(OrderedFloat<f32>, NodeId)>) is the forest-local
 * node index; a host that hands out global node ids in that same order (children before parents, as
 * INTEGRATION.md does) preserves every tie-break.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_index ah_index;

/* Upload the forest (nodes, split-plane normals, descendants) to the dataset's device.  The ah_forest may be
 * destroyed afterwards; the dataset must outlive the index. */
AH_API int ah_index_create(ah_dataset *ds, const ah_forest *forest, ah_index **out);
/* Same from caller-owned arrays in the ah_forest_view shape (e.g. tree nodes decoded from LMDB by `Reader::open`):
 * validated, copied to the device, not retained. */
AH_API int ah_index_create_from_view(ah_dataset *ds, const ah_forest_view *view, ah_index **out);
AH_API int ah_index_destroy(ah_index *index);

/* `QueryBuilder::by_vector` (queries = nq x dims f32, query_items = NULL) or `by_item` (queries = NULL,
 * query_items = nq ids) with `search_k` (0 = count * n_trees, src/reader.rs:330), `oversampling`
 * (0 = D::DEFAULT_OVERSAMPLING) and optional `candidates` (have_filter != 0: ascending ids).
 * Any count (`Reader::nns(count)`); counts above 2048 leave the batched top-k for the single-query kernels, query by
 * query.  Outputs nq x count, padded with id 0xFFFFFFFF / NaN; out_counts[q] = results of query q. */
AH_API int ah_search_batch(ah_index *index, const float *queries, const uint32_t *query_items, size_t nq, size_t count,
                           size_t search_k, size_t oversampling, const uint32_t *filter_sorted, size_t n_filter,
                           int have_filter, uint32_t *out_ids, float *out_distances, uint32_t *out_counts);

/* Which device path served the searches of an index (ABI v5).  ah_search_batch has several tiers — four descents, three
 * dedup paths, two re-rank paths — that return the same bits; these counters are how a caller (and the parity tests)
 * can tell that the intended one ran instead of a silent fall-back.  All values count since the index was created or
 * since the last call with reset != 0. */
typedef struct ah_search_stats {
    uint64_t calls;                 /* ah_search_batch calls that reached the device                                   */
    uint64_t chunks;                /* sub-batches they were cut into                                                  */
    uint64_t queries;
    /* the descent that produced a query's candidates (src/reader.rs:341-374); these four and `descent_block` below sum to
     * `queries` */
    uint64_t descent_wave_small;    /* one wave per query, 256 queue entries / 64 leaves per octet                     */
    uint64_t descent_wave_big;      /* ... its second pass, 1024 / 128                                                 */
    uint64_t descent_octet_lds;     /* one octet per query, the sequential queue in LDS                                */
    uint64_t descent_octet_global;  /* ... the queue in global memory (capacity = number of nodes)                     */
    /* nns.sort_unstable(); nns.dedup() (src/reader.rs:378-379), in queries */
    uint64_t dedup_flag_bitmap;     /* leaf tiles: duplicates flagged through one bit per id in LDS                    */
    uint64_t dedup_flag_hash;       /* leaf tiles: ... through a hash set of the candidates in LDS (big id spaces)     */
    uint64_t dedup_sorted_bitmap;   /* sorted path: the LDS bitmap walked in order                                     */
    uint64_t dedup_sort_lds;        /* sorted path: bitonic sort in LDS                                                */
    uint64_t dedup_sort_global;     /* sorted path: bitonic sort in global memory                                      */
    /* the re-rank (src/reader.rs:381-399), in queries */
    uint64_t rerank_tiles;          /* rows of a leaf x the queries that reached it                                    */
    uint64_t rerank_sorted;         /* from the sorted candidate lists (the kernels of ah_rerank_batch)                */
    uint64_t tile_visits;           /* (query, leaf) pairs the leaf tiles served                                       */
    uint64_t tile_units_16;         /* work units of 9..16 visits of one leaf (operands through the LDS ring)          */
    uint64_t tile_units_8;          /* ... of 5..8 visits (LDS ring)                                                   */
    uint64_t tile_units_4;          /* ... of 1..4 visits (registers)                                                  */
    /* sub-batches the leaf tiles handed to the sorted path, and why (one chunk may count under several reasons) */
    uint64_t fallback_chunks;
    uint64_t fallback_non_finite;   /* a non-finite distance: src/reader.rs:611-621 looks at positions                 */
    uint64_t fallback_select;       /* the selection / the hash set did not fit its LDS buffers                        */
    uint64_t fallback_queue;        /* a queue outgrew LDS (the sorted path has the global-memory queue)               */
    uint64_t fallback_visits;       /* more leaf visits than the visit buffer holds                                    */
    uint64_t fallback_launch;       /* the runtime rejected a launch of the tile path                                  */
    uint64_t filtered_queries;      /* queries under a candidate filter                                                */
    uint64_t leaf_kept_passes;      /* passes over every Descendants id for |leaf & candidates| (once per filtered call) */
    /* certified top-k screen of the tile re-rank (Cosine / DotProduct): candidates evaluated on the binary16 copy of the
     * rows first, only those whose proven distance interval reaches the top `count` in f32 */
    uint64_t rerank_screened;       /* queries whose top-k went through the screen                                      */
    uint64_t screen_survivors;      /* candidates of those queries evaluated in f32 (the rest: 2 x dims bytes each)     */
    uint64_t descent_block;         /* ABI v6: one block (32 octets, one tree each) per query: submissions of few queries;
                                       a fifth tier of the descent — the five sum to `queries` */
    /* ABI v7: the int8 copy of the rows as the first stage of that screen (big submissions; 1 byte per dimension) */
    uint64_t rerank_screened8;      /* queries (of rerank_screened) whose candidates were evaluated on the int8 rows first */
    uint64_t screen8_retried_chunks; /* sub-batches whose int8 stage left more survivors than the selection holds: done again
                                       with the binary16 rows first (eight of them within one window of 64 sub-batches the
                                       int8 stage served switch that stage of the index off) */
    uint64_t descent_multi;         /* queries (of descent_block) whose trees were dealt over several blocks, one wave of
                                       eight octets each: one query on more than one compute unit (submissions of <= 32 queries) */
} ah_search_stats;
AH_API int ah_index_search_stats(ah_index *index, ah_search_stats *out, int reset);

/* ------------------------------------------------------------------------------------------
 * Resident candidate filters (ABI v7 addition: look the symbols up).  `QueryBuilder::candidates` (src/reader.rs:110-123)
 * as an object that lives on the device next to its index: the bitmap over [0, largest stored id] and
 * |descendants & candidates| of every node, which ah_search_batch makes anew for every call that carries an id list,
 * are made once.  A host keeps one filter per tenant or facet bitmap and names it in any number of searches.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_filter ah_filter;
/* sorted_ids: strictly ascending; ids that are not stored are legal and match nothing (a RoaringBitmap may hold anything).
 * The filter is immutable and may serve concurrent searches of any number of threads.  It must be destroyed before its
 * index (ah_index_destroy refuses while one is alive). */
AH_API int ah_filter_create(ah_index *index, const uint32_t *sorted_ids, size_t n, ah_filter **out);
/* out_listed: ids given; out_stored: those of them that are rows of the dataset (exact); out_device_bytes: HBM the filter
 * holds.  Any pointer may be NULL. */
AH_API int ah_filter_info(const ah_filter *f, uint64_t *out_listed, uint64_t *out_stored, uint64_t *out_device_bytes);
AH_API int ah_filter_destroy(ah_filter *f);

/* Filter expressions on the device (ABI v7 addition: look the symbols up).  The filters of an index are plain bitmaps of one
 * length, so tenant AND facet, facet A OR facet B, everything NOT deleted are one streaming pass over (largest id + 1) / 8
 * bytes instead of an id list evaluated, walked and uploaded by the host.
 *   AH_FILTER_AND / _OR   1 <= n <= AH_FILTER_COMBINE_MAX operands
 *   AH_FILTER_ANDNOT      operands[0] minus the union of the others, n >= 1
 *   AH_FILTER_NOT         n == 1: every id of [0, largest stored id] the operand does not hold (ids that are not stored match
 *                         nothing, as in every filter)
 * An operand may be named more than once; with n == 1 AND, OR and ANDNOT give a copy.  The result is a new, independent,
 * immutable filter of the operands' index (they may be destroyed before it), counted like a created one, and bit for bit the
 * filter ah_filter_create makes from the ascending id list of the expression's result: the same bitmap, the same per-node
 * counts, the same `stored`, hence the same path choices in every search.  Its `listed` (ah_filter_info) is the number of set
 * bits; a list-made filter also counts the listed ids above the largest stored id, which no bitmap holds.  All or nothing
 * (AH_ERR_OUT_OF_MEMORY leaves nothing held and no counter moved); may run concurrently with searches under its operands.
 * Refused (AH_ERR_INVALID_ARGUMENT, the offending position named): out NULL, n out of range, an unknown op, a NULL operand,
 * an operand of another index, a suspended index. */
typedef enum ah_filter_op { AH_FILTER_AND = 0, AH_FILTER_OR = 1, AH_FILTER_ANDNOT = 2, AH_FILTER_NOT = 3 } ah_filter_op;
#define AH_FILTER_COMBINE_MAX 64
typedef struct ah_filter_combine_stats {
    uint64_t words;          /* 32-bit bitmap words written                                                             */
    uint64_t leaves;         /* Descendants nodes in use with at least one id                                           */
    uint64_t leaves_walked;  /* ... whose ids were tested against the new bitmap (the rest: derived from the operands' counts) */
    uint64_t ids_walked;     /* ids of those leaves                                                                     */
} ah_filter_combine_stats;
AH_API int ah_filter_combine(int op, ah_filter *const *operands, size_t n, ah_filter **out, ah_filter_combine_stats *out_stats);
/* A filter from a bitmap as the host holds it: bit i (bit i & 63 of words[i >> 6]) set = id i is a candidate.  n_bits is
 * arbitrary: bits of the last word at or above n_bits are ignored, and so are bits above the largest stored id — those are
 * still counted in `listed`, the set bits among the first n_bits.  Only the bits up to the largest stored id travel to the
 * device.  The result equals ah_filter_create of the list of set bits.  n_bits == 0 gives an empty filter; `words` is not
 * used after return. */
AH_API int ah_filter_create_bitmap(ah_index *index, const uint64_t *words, uint64_t n_bits, ah_filter **out);
/* Test aid: the filter as it is on the device — out_len_bits: largest stored id + 1; out_bits: its ceil(len_bits / 32) bitmap
 * words; out_leaf_kept: the n_nodes (ah_index_export_info) per-node counts.  Any pointer may be NULL. */
AH_API int ah_filter_export(const ah_filter *f, uint64_t *out_len_bits, uint32_t *out_bits, uint32_t *out_leaf_kept);

#define AH_NO_FILTER 0xFFFFFFFFu
/* ah_search_batch in which every query names its filter: filter_of_query[q] is an index into `filters` or AH_NO_FILTER;
 * NULL = every query under filters[0] (n_filters == 1) or unfiltered (n_filters == 0).  Query q returns exactly what
 * ah_search_batch returns for it alone under the id list of its filter — the same ids and distance bits, whatever else is
 * in the call.  Runs of at least AH_SEARCH_FILTER_GROUP_MIN queries with one filter are served like a single-filter call
 * (uniform sub-batches); the rest share mixed sub-batches whose descents look up every query's own filter. */
AH_API int ah_search_batch_filters(ah_index *index, const float *queries, const uint32_t *query_items, size_t nq, size_t count,
                                   size_t search_k, size_t oversampling, ah_filter *const *filters, size_t n_filters,
                                   const uint32_t *filter_of_query, uint32_t *out_ids, float *out_distances,
                                   uint32_t *out_counts);
/* How ah_search_batch_filters cut its calls, and the filters of the index.  Counts since the index was created or since the
 * last call with reset != 0 (filters_alive is a level, never reset). */
typedef struct ah_filter_stats {
    uint64_t calls;                 /* ah_search_batch_filters calls that reached the device                           */
    uint64_t uniform_batches;       /* sub-batches of one filter (or of unfiltered queries): the paths of ah_search_batch */
    uint64_t mixed_batches;         /* sub-batches whose queries are under different filters: sorted re-rank           */
    uint64_t uniform_queries;
    uint64_t mixed_queries;
    uint64_t filters_created;
    uint64_t filters_alive;
    uint64_t leaf_kept_passes;      /* passes over every Descendants id at filter creation (one per filter)            */
} ah_filter_stats;
AH_API int ah_index_filter_stats(ah_index *index, ah_filter_stats *out, int reset);

/* Per-query search parameters (ABI v7 addition: look the symbols up).  ah_search_batch_filters in which every query also names
 * its own count, search_k and oversampling: the three knobs of `QueryBuilder` a host's coalesced requests differ in. */
typedef struct ah_query_params {      /* 16 bytes; one per query */
    uint64_t search_k;                /* 0 = count * n_trees (src/reader.rs:330) */
    uint32_t count;                   /* Reader::nns(count); > 0 */
    uint32_t oversampling;            /* 0 = D::DEFAULT_OVERSAMPLING */
} ah_query_params;
/* Query q returns exactly what ah_search_batch returns for it alone with params[q] under the id list of its filter — the same
 * ids, the same distance bits and the same out_counts[q] — whatever else is in the call and however the call is cut (counts
 * above the batched top-k's 2048 and the positional rule for non-finite distances included).  The outputs are nq x out_stride,
 * out_stride >= the largest count; row q holds out_counts[q] = min(count_q, candidates_q) results, the rest of it is padded
 * with 0xFFFFFFFF / NaN.  filters, n_filters and filter_of_query are those of ah_search_batch_filters.  The call is cut into
 * sub-batches by filter as there; inside a filter's run the queries are ordered by the size of their candidate buffer
 * (AH_SEARCH_PARAMS_SORT), a sub-batch's scratch is sized by its own largest search_k and count, and counts beyond the batched
 * top-k share no sub-batch with the others.  Refused (AH_ERR_INVALID_ARGUMENT, the position named): params NULL, a count of 0
 * or >= 2^31, out_stride below the largest count, then what ah_search_batch_filters refuses, then a search_k whose candidate
 * buffer does not fit.  nq == 0 is AH_OK. */
AH_API int ah_search_batch_params(ah_index *index, const float *queries, const uint32_t *query_items, size_t nq,
                                  const ah_query_params *params, size_t out_stride, ah_filter *const *filters, size_t n_filters,
                                  const uint32_t *filter_of_query, uint32_t *out_ids, float *out_distances, uint32_t *out_counts);
/* How ah_search_batch_params cut its calls.  Counts since the index was created or since the last call with reset != 0.  (The
 * sub-batches also count in ah_search_stats and ah_filter_stats, like those of ah_search_batch_filters.) */
typedef struct ah_params_stats {
    uint64_t calls;                 /* ah_search_batch_params calls that reached the device                             */
    uint64_t batches;               /* their sub-batches                                                                */
    uint64_t varied_batches;        /* sub-batches whose queries do not all share one (count, effective search_k)       */
    uint64_t queries;
    uint64_t varied_queries;        /* queries of the varied sub-batches                                                */
    uint64_t big_count_queries;     /* queries of sub-batches whose counts leave the batched top-k (single-query kernels) */
} ah_params_stats;
AH_API int ah_index_params_stats(ah_index *index, ah_params_stats *out, int reset);

/* Exhausted filters (ABI v7 addition: look the symbols up).  The reference's loop counts only kept ids towards search_k
 * (src/reader.rs:341-374): under a filter whose kept ids over ALL leaves, duplicates across trees included, number at most
 * the effective search_k, it cannot stop before its queue is empty, and the candidates are exactly K(f), the distinct ids the
 * filter keeps and some leaf holds, whatever the query.  With the tunable AH_SEARCH_EXHAUSTED=1 (default 0: nothing changes)
 * ah_search_batch_filters and ah_search_batch_params answer such a query from K(f) without the descent: the same ids, distance
 * bits and counts.  K(f) is made on the device on first use, once per filter and residence (ah_filter_suspend frees it), and
 * counts in ah_filter_info's device_bytes from then on.  Both filter calls refuse a suspended filter by name. */
/* sum over the nodes of |descendants & candidates|: what a drained descent collects, duplicates across trees included */
AH_API int ah_filter_kept_total(ah_filter *f, uint64_t *out);
/* test aid: K(f), ascending; out_ids may be NULL (count only); makes the list if it does not exist */
AH_API int ah_filter_kept_ids(ah_filter *f, uint32_t *out_ids, uint64_t cap, uint64_t *out_n);
/* Counts since the index was created or since the last call with reset != 0.  Exhausted queries count in none of ah_search_stats
 * (`calls` apart), uniform_* / mixed_* of ah_filter_stats, or batches / varied_* / big_count_queries of ah_params_stats. */
typedef struct ah_exhausted_stats {
    uint64_t queries;        /* answered from their filter's list */
    uint64_t batches;        /* their sub-batches */
    uint64_t empty_queries;  /* ... of `queries`, answered without a launch (empty list) */
    uint64_t lists_made, list_ids;   /* kept lists made, ids in them */
    uint64_t leaves_walked;  /* leaves whose ids k_kept_mark tested */
} ah_exhausted_stats;
AH_API int ah_index_exhausted_stats(ah_index *index, ah_exhausted_stats *out, int reset);

/* Filters across index maintenance (ABI v7 addition: look the symbols up).  A live filter blocks ah_index_delete_items /
 * _insert_items / _graft / _drop_trees / _compact and ah_index_suspend, because its per-node counts would go stale.  What
 * does not go stale is its bitmap, apart from the ids the host's update touched.  ah_filter_suspend keeps the filter and
 * takes it out of filters_alive: it no longer blocks anything, and every call that would read it (ah_search_batch_filters,
 * ah_filter_combine, ah_filter_export, a second ah_filter_suspend) refuses it by name (AH_ERR_INVALID_ARGUMENT, "suspended").
 * It waits until no queued search reads the filter.  ah_filter_info (the old listed / stored; device_bytes: the block it
 * still holds) and ah_filter_destroy stay legal; ah_index_destroy refuses while a suspended filter exists.  Legal on a live
 * index only.
 *
 * ah_filter_resume_batch brings n suspended filters of ONE index back on that index as it is now (not suspended).  Filter i
 * becomes, bit for bit, the filter ah_filter_create makes now from the ascending list of
 *     ((old set \ edits[i].remove) | edits[i].add) & [0, largest stored id now]
 * — the same length, bitmap words (zero up to the 64-word multiple), per-node counts for every node slot of the current node
 * array, and `stored`; `listed` is the number of set bits, as for a combined filter.  An id in both lists ends up set; ids
 * that are not stored, or above the largest stored id, are legal in both lists.  The per-node counts of up to
 * AH_FILTER_RESUME_GROUP filters are made in ONE pass over the Descendants ids (ah_filter_create: one pass per filter); for
 * its duration the call holds a copy of one group's bitmaps laid side by side (64 bytes per 32 ids of the id range).  Where
 * that copy would pass 256 MiB (ids beyond 2^27) the counts are made a filter a pass, and `groups` is `filters`.
 * All or nothing: on any failure every filter is still suspended with its old bitmap, no counter has moved, nothing is held.
 * filters_created does not move, filters_alive rises by n, leaf_kept_passes by `groups` (an index with nodes).  May run next
 * to searches under other filters; not concurrent with maintenance of the same index.  n == 0 is AH_OK.  Refused
 * (AH_ERR_INVALID_ARGUMENT, the offending position named): filters NULL, an edit list that is NULL with a length or not
 * strictly ascending, a NULL filter, a filter of another index than filters[0]'s, a suspended index, a filter that is not
 * suspended, a filter named twice. */
#define AH_FILTER_RESUME_GROUP 16   /* filters whose per-node counts one pass over the Descendants ids serves */
typedef struct ah_filter_edit {      /* the host's delta of one filter; either list may be NULL with n == 0 */
    const uint32_t *remove_sorted; size_t n_remove;   /* strictly ascending */
    const uint32_t *add_sorted;    size_t n_add;      /* strictly ascending */
} ah_filter_edit;
typedef struct ah_filter_resume_stats {
    uint64_t filters, groups;        /* groups = ceil(filters / AH_FILTER_RESUME_GROUP) = passes over the Descendants ids */
                                     /* (`filters` where the id range is too long for grouped passes: above)             */
    uint64_t words;                  /* 32-bit bitmap words written, all filters                                        */
    uint64_t ids_removed, ids_added; /* bits the clears cleared, then bits the sets set (an id in both lists that was set: both) */
    uint64_t leaves, ids_walked;     /* Descendants nodes with >= 1 id; their ids, counted once per group                */
} ah_filter_resume_stats;
AH_API int ah_filter_suspend(ah_filter *f);
AH_API int ah_filter_resume_batch(ah_filter *const *filters, const ah_filter_edit *edits /* NULL = no edits */, size_t n,
                                  ah_filter_resume_stats *out_stats /* may be NULL */);
/* Suspended filters of the index: a level, like filters_alive. */
AH_API int ah_index_filters_suspended(ah_index *index, uint64_t *out);

/* Filters from serialized RoaringBitmaps (ABI v7 addition: look the symbols up).  `QueryBuilder::candidates` takes a
 * `&RoaringBitmap`; what `RoaringBitmap::serialize_into` writes becomes a resident filter without the host walking the ids or
 * expanding a dense bitmap: the headers are parsed on the host (O(containers)), the container payloads travel in one copy
 * and are expanded on the device, and the per-node counts of up to AH_FILTER_RESUME_GROUP filters are made in ONE pass over
 * the Descendants ids, as in ah_filter_resume_batch (a pass per filter where the id range is too long for that: there).
 * Accepted: the portable Roaring serialisation, little-endian, at any byte address —
 *   u32 cookie    12346 (no run containers; what roaring 0.10 writes), then u32 nc; or low 16 bits 12347, nc = (cookie >> 16) + 1,
 *                 then ceil(nc / 8) bytes of run flags (bit i & 7 of byte i >> 3: container i is a run container)
 *   nc x (u16 key, u16 cardinality - 1), keys strictly ascending
 *   nc x u32 byte offset from the start of the blob: always with 12346, with 12347 only when nc >= 4
 *   the containers in key order, back to back: run (u16 n_runs, n_runs x (u16 start, u16 length - 1)), array (cardinality
 *   <= 4096: ascending u16) or bitmap (8192 bytes, bit v & 63 of 64-bit word v >> 6)
 * Filter i is, bit for bit, the filter ah_filter_create makes from the ascending list of the ids blob i holds: the same
 * length, bitmap, per-node counts and `stored`; `listed` is the bitmap's cardinality, ids above the largest stored id
 * included.  Ids that are not stored are legal and match nothing; containers wholly above the largest stored id never
 * travel.  The filters are immutable and independent of each other and of the blobs, which are not used after return.
 * All or nothing: on any failure no filter exists, no counter has moved, nothing is held and every out[i] is NULL.  On
 * success filters_created and filters_alive rise by n, leaf_kept_passes by `groups` (an index with nodes).  n == 0 is AH_OK.
 * May run next to searches; not concurrent with maintenance of the same index.  Refused (AH_ERR_INVALID_ARGUMENT, the blob and,
 * where there is one, the container named), from the headers alone and in this order: out NULL, blobs / lens NULL, a NULL
 * blob, a blob shorter than its headers, an unknown cookie, keys that do not ascend strictly, a container past `len`, an
 * offset entry that disagrees with the sizes, `len` that is not the end of the last container; then what ah_filter_create
 * refuses about the index; then, found on the device in the containers that travelled (the lowest (blob, container) is the
 * one named): an array that does not ascend strictly, a bitmap container whose popcount is not its cardinality, runs that
 * overlap, are out of order or reach past 65535, runs whose total length is not the cardinality. */
typedef struct ah_filter_roaring_stats {
    uint64_t filters, groups;        /* groups = passes over the Descendants ids: ceil(filters / AH_FILTER_RESUME_GROUP), or */
                                     /* `filters` where the id range is too long for grouped passes (ah_filter_resume_batch) */
    uint64_t array_containers, bitmap_containers, run_containers;   /* expanded on the device                              */
    uint64_t skipped_containers;     /* key wholly above the largest stored id: never uploaded                             */
    uint64_t bytes_uploaded;         /* container payload bytes that travelled                                             */
    uint64_t leaves, ids_walked;     /* as ah_filter_resume_stats                                                          */
} ah_filter_roaring_stats;
AH_API int ah_filter_create_roaring(ah_index *index, const uint8_t *bytes, size_t len, ah_filter **out);
AH_API int ah_filter_create_roaring_batch(ah_index *index, const uint8_t *const *blobs, const size_t *lens, size_t n,
                                          ah_filter **out /* n handles */, ah_filter_roaring_stats *out_stats /* may be NULL */);

/* Incremental insert routing, `insert_items_in_descendants_from_frozen_reader` (src/writer.rs:1398-1459), for
 * every tree of the index at once: each of the `n` items (they must already be rows of the index's dataset — the
 * reference also re-creates `ImmutableLeafs` over all current items for every build, src/writer.rs:530) walks from
 * each root to the Descendants node it lands in, by `D::side` at split planes and by the coin of
 * arroy_hip_policy.h (`ah_route_side_is_left`, keyed by tree_seeds[t]) at `normal: None` nodes.
 * out_leaf[t * n + i] = forest-local node index reached by item i in tree t.  The host merges the items into those
 * Descendants nodes and re-splits the ones that grew beyond split_after (src/writer.rs:1411-1414, 546-561). */
AH_API int ah_route_items(ah_index *index, const uint32_t *item_ids, size_t n, const uint64_t *tree_seeds,
                          uint32_t *out_leaf);

/* ------------------------------------------------------------------------------------------
 * Deletes on a resident index (ABI v7 addition: look the symbols up).  `delete_items_from_trees` (src/writer.rs:978-1114),
 * the first tree step of an incremental `Writer::build`, applied to the index where it lives, so that the index of the last
 * build serves this build's ah_route_items instead of being uploaded again.
 *
 * `sorted_ids` strictly ascending; ids that are in no tree are legal (a RoaringBitmap may hold anything), 0xFFFFFFFF is a
 * legal id, n == 0 is legal.  `split_after` is the bound of `fit_in_descendant` (n <= split_after, src/writer.rs:474-477).
 * Bottom-up, as `delete_items_in_file` does, every node yields (replacement node, Some(ids) | None):
 *   - a Descendants node keeps descendants - sorted_ids, ascending; it is put only if its length changed; Some(kept);
 *   - a split node whose new children are (L, l) and (R, r), first case that matches:
 *       l is Some and empty      L and the node are removed, (R, r) takes its place (with both empty the right child stays,
 *                                as an empty Descendants node);
 *       r is Some and empty      R and the node are removed, (L, l) takes its place;
 *       both Some and |l| + |r| <= split_after
 *                                L and R are removed, the node becomes Descendants of l U r (always put), and may merge
 *                                again with its sibling one level up;
 *       otherwise                it stays a split node, put only if a child changed; None.
 *   A root that is a Descendants node stays, even empty.  Afterwards the roots are in ascending node order
 *   (`roots.sort_unstable()`, src/writer.rs:1001).  An id is expected at most once per tree, as in every forest the
 *   reference writes.  With n == 0 the delta is empty unless the forest holds siblings that fit together.  A merged node
 *   of more than 4096 ids (a split_after that large) is sorted by one block in device memory, as are more than 4096 roots:
 *   correct, and slow only there.
 *
 * The index afterwards: node indices are stable, removed nodes (and nodes no root reaches) are free slots, the roots are
 * in the new order, the descendants are rewritten into new memory, the normals are not touched.  ah_search_batch* and
 * ah_route_items return what an ah_index_create_from_view of the forest after the delete returns on the same dataset: the
 * same ids, distance bits and counts, the same landing nodes (a hole never changes the relative order of the surviving
 * node indices, so every (distance, node) tie-break holds).
 *
 * The delta is what the host writes to its store (the final state of `TmpNodes`): `removed` node indices ascending; `put`,
 * the nodes that stay and whose content changed, ascending by `put_index`, each an ah_node with kind and has_normal and
 * either left / right or (offset, count) into `desc` (ascending ids); `roots` in the index's new tree order.  A node put
 * and later removed by its parent's merge is in `removed` only.  ah_node.tree and .depth are 0.
 *
 * All or nothing: a bad argument or a failed allocation leaves the index as it was, searchable.  Refused
 * (AH_ERR_INVALID_ARGUMENT) while the index has live filters (their per-node counts would be stale) or is suspended.
 * Not concurrent with any other call on the same index: searches of other threads must have returned.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_index_delta ah_index_delta;
typedef struct ah_index_delta_view {
    uint64_t n_removed;
    const uint32_t *removed;
    uint64_t n_put;
    const uint32_t *put_index;
    const ah_node *put;
    const uint32_t *desc;
    uint64_t desc_len;
    uint32_t n_trees;
    const uint32_t *roots;
} ah_index_delta_view;
AH_API int ah_index_delete_items(ah_index *index, const uint32_t *sorted_ids, size_t n, uint32_t split_after,
                                 ah_index_delta **out_delta);
/* Pointers into the delta, valid until ah_index_delta_destroy. */
AH_API int ah_index_delta_get(const ah_index_delta *d, ah_index_delta_view *out);
AH_API int ah_index_delta_destroy(ah_index_delta *d);

/* ------------------------------------------------------------------------------------------
 * Dropped trees on a resident index (ABI v7 addition: look the symbol up).  `delete_extra_trees` (src/writer.rs:631-655,
 * called at :522), the tree step of an incremental `Writer::build` that runs BEFORE the delete, applied to the index where
 * it lives: a build that shrinks the forest (a lower n_trees, or `target_n_trees` following the item count) keeps its index
 * resident instead of uploading every node, id and normal again.
 *
 * The call does min(n_drop, n_trees) times what the reference does: `root = roots.swap_remove(0); delete_tree(root)`.
 * n_drop >= n_trees leaves an index of zero trees, which is legal: the searches and ah_route_items answer it with nothing.
 * n_drop == 0 does nothing: the delta is empty and carries the current roots, nothing is allocated beyond the delta and the
 * index's arrays are not replaced.
 *   Roots        the surviving roots are left in the order the repeated swap_remove(0) leaves them: from [r0 .. r5] with
 *                n_drop = 4 that is [r2, r1].  With AH_DROP_SORT_ROOTS they are left ascending by node index instead, what
 *                `roots.sort_unstable()` (src/writer.rs:1001) makes of them: for a host that calls no ah_index_delete_items
 *                (which sorts them itself) in the same build.
 *   Nodes        every node reachable from a dropped root becomes a free slot (kind 0, all zeros, as a delete leaves them);
 *                node indices are stable; the nodes of the surviving trees are bit-unchanged, except that the offset of a
 *                Descendants node moves.
 *   Descendants  rewritten into new memory: the lists of the surviving Descendants nodes in ascending node order with their
 *                exact lengths (what ah_index_compact relies on).
 *   Ranks        rebuilt, as ah_index_delete_items leaves them: per node the number of in-use nodes below it, which the coins
 *                of ah_route_items at `normal: None` nodes are keyed by.
 *   Normals      not touched: the rows of the dropped split nodes are orphaned, ah_index_footprint_get reports them and the
 *                free slots, ah_index_compact reclaims both.
 * Afterwards ah_search_batch*, ah_route_items, ah_index_insert_items, ah_index_delete_items, ah_index_graft,
 * ah_index_compact and ah_index_audit return what they return on an ah_index_create_from_view of the store after the drop, on
 * the same dataset with the roots in the same order: ids, distance bits, counts, landing nodes and coins.
 *
 * The delta (ah_index_delta_get): `removed` holds every node of the dropped trees, ascending — what the host deletes from
 * its store; n_put = 0 and desc_len = 0; `roots` is the new order.
 *
 * The rules of ah_index_delete_items hold: all or nothing (every buffer is obtained before the kernel that fills it, the
 * kernels write new memory only, the pointers are swapped after the last read-back; a bad argument — unknown bits in `flags`
 * among them — or a failed allocation leaves the index as it was, searchable, holding nothing extra); refused
 * (AH_ERR_INVALID_ARGUMENT) while the index has live filters or is suspended; not concurrent with any other call on the
 * same index.  For the duration of the call the index holds its nodes, ranks and the surviving ids a second time, plus
 * scratch of four words per node slot.
 * ---------------------------------------------------------------------------------------- */
#define AH_DROP_SORT_ROOTS 1u
AH_API int ah_index_drop_trees(ah_index *index, uint32_t n_drop, uint32_t flags, ah_index_delta **out_delta);

/* ------------------------------------------------------------------------------------------
 * Inserts and grafts on a resident index (ABI v7 additions: look the symbols up).  The other tree steps of an incremental
 * `Writer::build`, applied to the index where it lives: with ah_index_delete_items they make the index of build N serve
 * build N + 1 and the searches after it, and only the normals of the new split nodes ever travel to the device.
 *
 * The rules of ah_index_delete_items hold for both calls: all or nothing (a bad argument or a failed allocation leaves the
 * index as it was, searchable); refused (AH_ERR_INVALID_ARGUMENT) while the index has live filters or is suspended; not
 * concurrent with any other call on the same index.
 *
 * ah_index_insert_items — `insert_items_in_descendants_from_frozen_reader` (src/writer.rs:1398-1459) for every tree at once.
 * Every id is routed exactly as ah_route_items routes it (the same landing nodes, the same coin at `normal: None` nodes,
 * keyed by tree_seeds[t]), and every Descendants node an id landed in becomes `descendants | to_insert`
 * (src/writer.rs:1412): ascending, an id the list already holds is not added twice.  `sorted_ids` strictly ascending; every
 * id must be a row of the index's dataset (the first that is not is named, AH_ERR_INVALID_ARGUMENT); 0xFFFFFFFF is a legal
 * id; n == 0 is legal and gives an empty delta.  The descendants are rewritten into new memory; node indices, free slots,
 * roots and normals do not change.  The delta (ah_index_delta_get): n_removed = 0; `put` / `put_index` are the Descendants
 * nodes an id landed in, ascending, with their new lists in `desc` — a node is put even when it held every id it received,
 * as the reference inserts it into `descendants_to_update` regardless; `roots` is the current order.  Which nodes outgrew
 * `split_after` the host reads from the counts.  A node that receives more than 4096 ids in one call is sorted by one block
 * in device memory: correct, and slow only there.
 *
 * ah_index_graft — adds the trees of `view` (typically what ah_forest_view_get returns for the forest of
 * ah_build_subtrees or ah_build_forest) to the index: `incremental_index_large_descendant` (src/writer.rs:660-739, the
 * sub-tree's root keeping the descendant's id, :693-702) and the added trees (:556-561) in one operation.  targets[t] is
 * the index of an in-use Descendants node that the root of tree t replaces, or AH_NEW_ROOT: new roots are appended
 * to the index's roots in view order.  Node identity is the tie-break of every descent and the host hands node ids out
 * through `ConcurrentNodeIds`, which reuses freed ids first (src/parallel.rs:222-254), so new nodes interleave with old
 * ones: the graft renumbers.  new_index[k] is the final index of view node k; the final indices run over [0, N'),
 * N' = nodes in use before the call + view nodes that are not replacing roots; a replacing root takes its target's place
 * and its new_index entry must be 0xFFFFFFFF; the existing in-use nodes fill the positions not named, in their current
 * relative order.  new_index == NULL: the new nodes follow all existing ones, in view order.  Afterwards the index has no
 * free slots and is what ah_index_create_from_view makes of the host's store listed in ascending id order: the same nodes,
 * roots and descendants (the normals are the same rows under other row numbers: the new ones are appended behind the old
 * ones, and rows orphaned by earlier deletes or grafts stay until ah_index_compact reclaims them).  out_new_of_old (may be
 * NULL): one word per node slot before the call, the node's new index, 0xFFFFFFFF for a free slot and for nothing else (a
 * replaced target maps to the place its sub-tree's root took).
 * Checked before anything is touched: the view (as ah_index_create_from_view checks it); targets distinct, in use and
 * Descendants nodes; new_index values distinct and < N'.  NOT checked: that the ids of a replaced node are the ids of its
 * sub-tree — that is the host's contract, as in the reference.
 * ---------------------------------------------------------------------------------------- */
AH_API int ah_index_insert_items(ah_index *index, const uint32_t *sorted_ids, size_t n, const uint64_t *tree_seeds,
                                 ah_index_delta **out_delta);
#define AH_NEW_ROOT 0xFFFFFFFFu
AH_API int ah_index_graft(ah_index *index, const ah_forest_view *view, const uint32_t *targets, const uint32_t *new_index,
                          uint32_t *out_new_of_old);

/* The index as it is on the device, for tests that compare structure and for a host that audits a long-lived index.  Reads
 * only; refused while the index is suspended.  ah_index_export_info gives the sizes of the caller's buffers;
 * ah_index_export fills those that are not NULL: nodes[n_nodes] (kind 0 = a free slot; a split node's `offset` is its
 * normal ROW, not a byte offset; a Descendants node's `offset` / `count` index `descendants`; tree and depth are 0),
 * roots[n_trees], descendants[desc_len], normal_rows[n_normals x normal_row_bytes] (the device's padded rows) and
 * normal_headers[n_normals x normal_header_floats]. */
typedef struct ah_index_info {
    uint64_t n_nodes;
    uint64_t desc_len;
    uint32_t n_trees;
    uint32_t n_normals;
    uint64_t normal_row_bytes;
    uint32_t normal_header_floats;
    uint32_t reserved;
} ah_index_info;
AH_API int ah_index_export_info(const ah_index *index, ah_index_info *out);
AH_API int ah_index_export(ah_index *index, ah_node *nodes, uint32_t *roots, uint32_t *descendants, void *normal_rows,
                           float *normal_headers);

/* ------------------------------------------------------------------------------------------
 * Compaction of a resident index (ABI v7 additions: look the symbols up).  An index that deletes, inserts and grafts keep
 * resident across builds collects waste no upload clears any more: every split node a delete removes leaves its normal row
 * behind (3 KB at 768 dimensions), a replaced sub-tree likewise; a delete that no graft follows leaves free node slots, which
 * every coin of ah_route_items pays for through the ranks and ah_index_export shows as kind 0; and a graft grows the rows
 * geometrically and never shrinks them.
 *
 * ah_index_footprint_get — what the index holds and how much of it is waste.  Reads only: one counting pass over the node
 * array on the device (a scratch of a few words per node slot for its duration).  Legal with live filters; refused while
 * the index is suspended.  `device_bytes` is the sum of the arrays as the index asks for them (nodes, roots, the ranks a
 * delete left, descendants, normal rows and headers at capacity), not what an allocator rounds them to.
 *
 * ah_index_compact — removes the waste on the device.  Afterwards the index is what ah_index_create_from_view makes of the
 * forest as it is now, listed in ascending node order:
 *   - no free slots; the in-use nodes keep their relative order, a node's new index is the number of in-use nodes below it
 *     (its rank); children and roots are remapped, the order of the roots stays; the ranks are freed;
 *   - normal rows are 1:1 with the split nodes that have a normal, in node order: the row of such a node moves to "number
 *     of in-use split nodes with a normal and a smaller index", the row a fresh index gives it (also when no row is dead
 *     but a graft appended rows of nodes that interleave with older ones); row and header bytes are copied unchanged;
 *     n_normals = live rows, and the arrays have room for max(1, n_normals) rows;
 *   - the descendants are not touched: delete, insert and graft write them in node order with the exact length, and
 *     removing holes does not change that order;
 *   - n_leaves, max_desc, desc_len, the search statistics and the int8-stage window stay as they are.
 * ah_search_batch*, ah_route_items, ah_index_insert_items, ah_index_delete_items and ah_index_graft afterwards return what
 * they return on that fresh index: ids, distance bits, counts, landing nodes and the coins at `normal: None` nodes (keyed
 * by the rank, which is now the index).  out_new_of_old (may be NULL): one word per node slot before the call, the node's
 * new index, 0xFFFFFFFF for a free slot and for nothing else — the convention of ah_index_graft.  out_stats (may be NULL).
 *
 * Nothing to do — no free slot, no dead or misplaced row, no spare row, no ranks: AH_OK, moved = 0, out_new_of_old is the
 * identity.  On a fresh index and directly after a compaction the host knows that, and nothing is allocated or launched;
 * otherwise the counting pass finds it and gives its scratch back.
 *
 * The compaction is NOT in place: rows move towards the front, and a wave would write over a row another wave has yet to
 * read.  For the duration of the call the index therefore holds, next to its own arrays, the new ones: the live rows and
 * headers, the in-use nodes and the roots a second time, plus scratch of three words per node slot and one per live row.
 *
 * The rules of ah_index_delete_items hold: all or nothing (every buffer is obtained before the first kernel that fills it,
 * the kernels write new memory only, the pointers are swapped after the last copy has landed; a bad argument or a failed
 * allocation leaves the index as it was, searchable, holding no extra memory); refused (AH_ERR_INVALID_ARGUMENT) while the
 * index has live filters or is suspended; not concurrent with any other call on the same index.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_index_footprint {
    uint64_t n_nodes;        /* node slots */
    uint64_t free_slots;     /* of them kind == 0 */
    uint64_t n_normals;      /* normal rows in use by the arrays (what ah_index_export_info reports) */
    uint64_t live_normals;   /* rows named by an in-use split node with a normal */
    uint64_t normals_cap;    /* rows the arrays have room for */
    uint64_t desc_len;
    uint64_t device_bytes;   /* HBM the index holds: nodes, roots, ranks, descendants, normal rows and headers at capacity */
} ah_index_footprint;
AH_API int ah_index_footprint_get(ah_index *index, ah_index_footprint *out);
typedef struct ah_index_compact_stats {
    uint64_t nodes_before, nodes_after;
    uint64_t normals_before, normals_after;     /* n_normals */
    uint64_t normals_cap_before, normals_cap_after;
    uint64_t device_bytes_before, device_bytes_after;
    uint32_t moved;          /* 0: there was nothing to do and nothing was written */
    uint32_t reserved;
} ah_index_compact_stats;
AH_API int ah_index_compact(ah_index *index, uint32_t *out_new_of_old, ah_index_compact_stats *out_stats);

/* ------------------------------------------------------------------------------------------
 * Resident forests (ABI v7 additions: look the symbols up).  A build ends with every normal and every item id in HBM;
 * ah_index_create and ah_index_graft then upload both blobs of the forest's view again.  A RESIDENT forest keeps, next to
 * its usual host content, a device copy of what an index holds of it — the normal rows at the dataset's row pitch, their
 * headers and the descendants ids, exactly the arrays ah_index_create_from_view makes of the forest's own view (row r is the
 * r-th split node with a normal in view order, the ids lie at the view's offsets) — and two calls make an index from it, or
 * graft it into one, without uploading either.
 *
 * ah_build_forest_resident / ah_build_subtrees_resident — the arguments, the checks, the errors and the forest of
 * ah_build_forest / ah_build_subtrees: ah_forest_view_get, ah_forest_digest, ah_forest_stats and ah_forest_visit give the same
 * content bit for bit (seconds_device also counts the extra stage).  At the end of every batch one more stage reads the
 * levels' records where they lie and writes rows and headers in view order, and copies the batch's ids device to device.
 * Failing to obtain the device copy is NOT an error: the call returns AH_OK with an ordinary forest (the rule of the
 * screen's copies).  The plain entry points enqueue what they always did.  The streaming builds have no resident form.
 * ah_forest_resident_info — *out_resident = 1 while the forest holds its device copy, *out_device_bytes what it asked the
 * device for (0 otherwise); either may be NULL.  ah_forest_release_device frees the copy and leaves an ordinary forest (legal
 * on any forest); ah_forest_destroy frees it too.
 *
 * ah_index_create_from_forest — new_index == NULL: the index of ah_index_create(ds, forest); ah_index_export gives the same
 * bytes.  new_index given: a permutation of [0, n_nodes), new_index[k] the final index of view node k — the numbering of the
 * host's store (roots first, `ConcurrentNodeIds`), in the convention of ah_index_graft: the result is what
 * ah_index_create_from_view makes of that renumbered store in nodes, roots and every node's ids, every split node resolves to
 * the same row bytes and header; row numbers and blob offsets may differ as after a graft, and after ah_index_compact the
 * export is byte-identical.  (It IS a graft of every tree as AH_NEW_ROOT onto an index of nothing; new_index is checked as
 * there.)
 * ah_index_graft_forest — ah_index_graft with the forest's view: the same arguments are checked before anything is touched,
 * all or nothing, refused with live filters or on a suspended index.
 *
 * Both calls read rows, headers and ids from the forest's device arrays (device-to-device row copies and the graft's list
 * gather); only the node records, the roots and the index tables come from the host, the nodes of a library-built forest are
 * not walked again, and no second copy of the normals exists at any time.  A successful call CONSUMES the device copy — the
 * forest is an ordinary forest afterwards; where no renumbering moves them the index adopts the blocks as its own —
 * and sets *out_from_device = 1 (may be NULL).  When the forest is not resident (never was, released, consumed), lives on
 * another device than the dataset, or was built for another metric or dimension count, the call silently takes the host
 * view — ah_index_create / ah_index_graft, the same result — and sets *out_from_device = 0.  A failed call leaves the forest
 * resident.  The forest may be destroyed as soon as the call returns.
 * ---------------------------------------------------------------------------------------- */
AH_API int ah_build_forest_resident(ah_dataset *ds, const ah_build_options *options, ah_forest **out);
AH_API int ah_build_subtrees_resident(ah_dataset *ds, const ah_build_options *options, const uint32_t *item_ids,
                                      const uint64_t *offsets, ah_forest **out);
AH_API int ah_forest_resident_info(const ah_forest *forest, int *out_resident, uint64_t *out_device_bytes);
AH_API int ah_forest_release_device(ah_forest *forest);
AH_API int ah_index_create_from_forest(ah_dataset *ds, ah_forest *forest, const uint32_t *new_index, int *out_from_device,
                                       ah_index **out);
AH_API int ah_index_graft_forest(ah_index *index, ah_forest *forest, const uint32_t *targets, const uint32_t *new_index,
                                 uint32_t *out_new_of_old, int *out_from_device);

/* ------------------------------------------------------------------------------------------
 * Audit of a resident index (ABI v7 additions: look the symbols up): `Reader::assert_validity` (src/reader.rs:509-589) and
 * `Reader::stats` (src/reader.rs:210-252) where the forest lives.  After its first upload the host never sees an index
 * again — deletes, inserts, grafts and compactions rewrite it in HBM, suspend / resume carry it across an update of the
 * dataset — and three contracts of this header are stated, not checked: ids an update removed must leave the index before
 * it is searched (ah_index_resume), the ids of a grafted sub-tree must be those of the node it replaces (ah_index_graft),
 * and a view's lists must hold ascending ids that are rows of the dataset, every item once per tree
 * (ah_index_create_from_view checks ranges and reachability only).  The audit answers "is this still a forest that
 * reaches every item once per tree" without exporting anything: one level walk over the nodes and one read of the
 * descendants, on the device.
 *
 * A node is IN USE when its kind is AH_NODE_SPLIT or AH_NODE_DESCENDANTS (0 is a free slot a delete left; anything else
 * is an unknown kind: neither in use nor a legal target of a link).  A node is REACHED when a chain of valid links leads
 * to it from a valid entry of roots[]; it is accounted once, under the tree (position in roots[]) that claimed it first.
 * The classes, each a property of the arrays and not of the order the kernels ran in:
 *   BAD_ROOT      entries of roots[] that are out of range or name a node that is not in use.  first_node: the smallest
 *                 such POSITION in roots[].
 *   BAD_LINK      child links of reached split nodes that are out of range or name a node that is not in use.
 *                 first_node: the smallest split node holding one.
 *   LINKED_TWICE  per node, links = valid root entries + valid child links of reached split nodes that name it; the class
 *                 is the sum of (links - 1) over nodes with more than one, = links followed - nodes reached: a shared
 *                 sub-tree, a cycle, a root that is also a child, a root named twice.  first_node: the smallest node with
 *                 more than one link.
 *   FLOATING      nodes in use that are not reached ("tree nodes floating around").
 *   BAD_NORMAL    reached split nodes with a normal whose row is >= n_normals; for a view: whose record is out of the
 *                 blob or misaligned.
 *   BAD_LIST      reached Descendants nodes with offset + count > the length of the descendants.  Their ids are not read.
 *   UNSORTED      reached Descendants nodes whose ids are not strictly ascending (equal neighbours count).
 *   FOREIGN       id occurrences in reached lists that are no row of the dataset (0xFFFFFFFF is a legal id: foreign only
 *                 when it is not stored).  first_node: the smallest node holding one.
 *   DUPLICATE     per tree, occurrences of a stored id beyond its first.
 *   MISSING       (tree, stored item) pairs where the tree holds no occurrence of the item.
 * first_node of DUPLICATE / MISSING is the root of first_duplicate_tree / first_missing_tree.
 *
 * With the six structure counts (BAD_ROOT .. BAD_LIST) at 0, the list and coverage counts, the first_* fields and
 * out_trees are exact.  With a structure violation only valid == 0, n_trees, nodes_in_use, nodes_reached, the structure
 * counts, their first_node and out_trees[t].root are promised (a shared leaf is read under one of its trees).  With
 * n_trees == 0 only FLOATING can be non-zero, as in the reference.
 *
 * ah_index_audit reads only, like ah_index_footprint_get: legal with live filters and concurrently with searches, not
 * concurrent with a mutating call on the same index, refused while the index is suspended.  All or nothing about
 * memory: every scratch block (three words per node slot, a few per tree, and the coverage words: one bit per row and
 * tree of a group of trees, at most AH_AUDIT_COVER_MB MiB, default 64, or one tree's) is obtained before the first
 * launch; a failed allocation returns AH_ERR_OUT_OF_MEMORY and holds nothing.  *out and out_trees are untouched on any
 * error.  AH_OK whatever the findings: the report is the result, not a status.  out_trees: n_trees entries or NULL.
 *
 * ah_forest_view_audit audits arrays the host holds (nodes decoded from LMDB before ah_index_create_from_view, the view
 * of a build) without making an index of them: it uploads nodes, roots and ids into scratch (not the normals: their
 * offsets are judged on the host), runs the same kernels and frees the scratch.  It refuses only NULL pointers, sizes
 * beyond 32 bits, a normal vector / header that does not fit the record stride and an unfinalized dataset; everything
 * else ah_index_create_from_view refuses it COUNTS, so no ah_index with a broken structure ever exists.
 * ---------------------------------------------------------------------------------------- */
typedef struct ah_tree_stats {     /* `TreeStats`, src/reader.rs:216-240 */
    uint32_t root;                 /* node index of the tree's root */
    uint32_t depth;                /* a root that is a Descendants node: 1 */
    uint32_t split_nodes;
    uint32_t dummy_normals;        /* split nodes with `normal: None` */
    uint32_t descendants;          /* Descendants NODES, as in the reference */
    uint32_t reserved;
    uint64_t items;                /* ids in those nodes, with multiplicity */
} ah_tree_stats;

enum { AH_AUDIT_BAD_ROOT, AH_AUDIT_BAD_LINK, AH_AUDIT_LINKED_TWICE, AH_AUDIT_FLOATING, AH_AUDIT_BAD_NORMAL,
       AH_AUDIT_BAD_LIST, AH_AUDIT_UNSORTED, AH_AUDIT_FOREIGN, AH_AUDIT_DUPLICATE, AH_AUDIT_MISSING, AH_AUDIT_CLASSES };

/* (the report cannot carry the name of the call that fills it: in C a typedef and a function share one name space) */
typedef struct ah_index_audit_report {
    uint64_t n_items;              /* rows of the dataset */
    uint64_t n_trees, nodes_in_use, nodes_reached;
    uint64_t count[AH_AUDIT_CLASSES];
    uint32_t first_node[AH_AUDIT_CLASSES]; /* smallest offending node index (BAD_ROOT: smallest position in roots[]); 0xFFFFFFFF: none */
    uint32_t first_missing_tree, first_missing_id;   /* smallest (tree position, id) pair counted under MISSING */
    uint32_t first_duplicate_tree, first_duplicate_id;
    uint32_t valid;                /* 1 iff every count is 0 */
    uint32_t reserved;
} ah_index_audit_report;

AH_API int ah_index_audit(ah_index *index, ah_index_audit_report *out, ah_tree_stats *out_trees);
AH_API int ah_forest_view_audit(ah_dataset *ds, const ah_forest_view *view, ah_index_audit_report *out, ah_tree_stats *out_trees);

/* A resident index from the bytes LMDB stores for the tree nodes (ABI v7 addition: look the symbol up).  A process that opens
 * an existing database (`Reader::open`) passes the `(key, value)` pairs of its cursor over the tree keys straight through:
 * node_ids[i] is the node id of the key, values[i] / lens[i] the `NodeCodec` value (src/node.rs:229-241) as it lies in the
 * map, at any byte address.  The host copies the values into pinned memory in chunks and reads none of their bytes; they
 * are measured, linked, unpacked and expanded on the device.
 *   split node    9 bytes (`normal: None`) or 9 + ah_header_size + ah_vector_size: [2][left u32 BE][right u32 BE][header][vector]
 *   Descendants   [1] + what `RoaringBitmap::deserialize_from` accepts: the serialisation ah_filter_create_roaring documents,
 *                 cookie 12346 or 12347 (run containers, the offset header from 4 containers on)
 * Only these v0.7 layouts are read; tag 0 (an item) and unknown tags are refused.
 * node_ids ascend strictly (the order the cursor yields); node i of the index is the value of the i-th id, and every left,
 * right and root id is replaced by its rank among node_ids.  The index is, array for array under ah_index_export /
 * ah_index_export_info / ah_index_footprint_get, the index ah_index_create_from_view makes of the decoded view: children
 * and roots as ranks, the descendants concatenated in node order, the normal rows in node order.  Nodes no root reaches are
 * legal, as in a view.  Values and arrays are not retained.  n_nodes == 0 with n_trees == 0 gives a legal empty index.
 * All or nothing: on any error nothing stays allocated and *out is NULL.  May run while other indexes of the dataset
 * serve searches.
 * Refused (AH_ERR_INVALID_ARGUMENT; the node id and the reason in ah_last_error, the smallest node position when several
 * values are bad): a NULL argument, node_ids that do not ascend strictly, a value that is empty or whose tag is neither 1 nor
 * 2, a split value of any other length, a Descendants value shorter than its headers, an unknown cookie, keys that do not
 * ascend strictly, a container past the end, an offset entry that disagrees with the sizes, bytes behind the last
 * container; a child or root id that is not among node_ids; an array container that does not ascend strictly, a bitmap
 * container whose popcount is not its cardinality, runs that overlap, are out of order or reach past 65535, runs whose
 * total length is not the cardinality; a node reachable twice, 2^32 - 1 or more nodes or ids.  A dataset that is not
 * finalized: AH_ERR_NOT_FINALIZED.
 * AH_DECODE_CHUNK_BYTES (tunable, default 64 MiB): the bytes of values one staged chunk holds, never below the largest value. */
typedef struct ah_index_decode_stats {
    uint64_t values, split_values, normals, descendants_values, ids;
    uint64_t containers_array, containers_bitmap, containers_run;
    uint64_t wave_values, block_containers;   /* which expansion path served what: Descendants values a wavefront expanded, */
                                              /* containers of the values a block expanded (bitmap / run containers among them) */
    uint64_t bytes_staged, chunks;            /* descriptors and values in whole 16-byte units; uploads                      */
    double seconds_total, seconds_host_copy;
} ah_index_decode_stats;
AH_API int ah_index_create_from_encoded(ah_dataset *ds, const uint32_t *node_ids, const uint8_t *const *values, const size_t *lens,
                                        size_t n_nodes, const uint32_t *root_ids, uint32_t n_trees, ah_index **out,
                                        ah_index_decode_stats *out_stats /* may be NULL */);

/* A resident index from the tree node bytes of an OLDER database, upgraded (ABI v7 addition: look the symbol up): what
 * `Reader::open` decodes through `GenericReadNodeCodecFromV0_4_0` (src/node.rs:284-319) and `upgrade::from_0_6_to_current`
 * (src/upgrade.rs:183-270) rewrites.  Arguments, guarantees, chunking (AH_DECODE_CHUNK_BYTES, AH_LAUNCH_MAX_ITEMS) and refusals
 * are those of ah_index_create_from_encoded, and with AH_NODE_LAYOUT_V0_7 the call IS ah_index_create_from_encoded, through the
 * same code.  Under the two legacy layouts Descendants values are unchanged and a split value is
 *   [2][left NodeId][right NodeId][vector]     1 + 5 + 5 + ah_vector_size bytes, no header; NodeId = [mode u8][item u32 BE]
 * A child's mode is Tree or Item — Tree = 2, Item = 3 under AH_NODE_LAYOUT_V0_5 (v0.5 and v0.6), Item = 0, Tree = 1 under
 * AH_NODE_LAYOUT_V0_4 — and an Item child points straight at a stored item.  A normal is never absent: `normal: None` was stored
 * as a vector `is_zero` accepts (f32: every element == 0.0, so -0.0 is zero and a NaN is not; binary-quantized: every byte 0).
 * A normal that is not zero gets `D::new_header(vector)`, made by the code that makes the headers of ah_dataset_upload_vectors:
 * the norm for Cosine and BinaryQuantizedCosine, all zeros for the other metrics (a Euclidean or Manhattan bias is 0, as in the
 * reference on such files).
 * The index is the UPGRADED one — array for array under ah_index_export / ah_index_export_info / ah_index_footprint_get what
 * ah_index_create_from_encoded makes of the values `from_0_6_to_current` writes: node i < n_nodes is value i; every Item child,
 * taken in node order and left before right, becomes a Descendants node of that one id at slot n_nodes + j (j = 0, 1, ...), its
 * list appended to the descendants in that order; normal rows exist only for normals that are not zero.  Everything is done on
 * the device: the host copies the bytes and reads none.
 * Writing the upgraded database back needs no further entry point: ah_index_encode_nodes(index, NULL, ..., node_id_of) with
 * node_id_of = node_ids followed by last node id + 1 + j for the new slots yields the v0.7 values, of which the split slots and
 * the new slots are what `from_0_6_to_current` puts.
 * Refused in addition (AH_ERR_INVALID_ARGUMENT, as above): an unknown layout; a split value that is not 11 + ah_vector_size
 * bytes long; a child mode byte that is neither Tree nor Item under the layout; a Tree child or a root that is not among
 * node_ids; n_nodes + new nodes, or the ids with those of the new nodes, reaching 2^32 - 1.
 * *out_stats describes the values as given; *out_legacy (zeroed under AH_NODE_LAYOUT_V0_7) what the legacy layout added. */
typedef enum ah_node_layout {
    AH_NODE_LAYOUT_V0_7 = 0,  /* what ah_index_create_from_encoded reads */
    AH_NODE_LAYOUT_V0_5 = 1,  /* v0.5 and v0.6 */
    AH_NODE_LAYOUT_V0_4 = 2
} ah_node_layout;
typedef struct ah_index_legacy_stats {
    uint64_t split_values, zero_normals, headers_made, item_children, new_nodes;
} ah_index_legacy_stats;
AH_API int ah_index_create_from_legacy(ah_dataset *ds, int layout, const uint32_t *node_ids, const uint8_t *const *values,
                                       const size_t *lens, size_t n_nodes, const uint32_t *root_ids, uint32_t n_trees,
                                       ah_index **out, ah_index_decode_stats *out_stats /* may be NULL */,
                                       ah_index_legacy_stats *out_legacy /* may be NULL */);

/* The nodes of a resident index as the bytes LMDB stores for them (ABI v7 addition: look the symbol up) — the inverse of
 * ah_index_create_from_encoded, for the host's store after ah_index_delete_items / ah_index_insert_items / ah_index_graft /
 * ah_index_compact (the delta's put_index, the grafted indices) and for writing a whole resident index back.
 * Value i is the `NodeCodec` v0.7 value (src/node.rs:229-241) of node slot node_indices[i]:
 *   split node    [2][left u32 BE][right u32 BE] and, when the node has a normal, [D::Header][vector]
 *                 (ah_header_size + ah_vector_size bytes, the words ah_index_export returns for its row, unchanged)
 *   Descendants   [1] + the portable Roaring serialisation without run containers (cookie 12346)
 * byte for byte what ah_build_forest_stream_encoded and ah_encode_descendants produce for the same node.  The children are
 * written as the STORE's ids: node_id_of[child] (one word per node slot of the index; entries of free slots are not read)
 * or, with node_id_of == NULL, node_id_base + child.
 * The values lie back to back in out_values in the order listed, value i at out_value_offsets[i] ..
 * out_value_offsets[i + 1] (n + 1 offsets, the last one the total).  The list may be in any order and may repeat an index.
 * node_indices == NULL: every node slot 0 .. n_nodes - 1 (n is ignored, n_nodes + 1 offsets); a free slot (kind 0) gets a
 * zero-length value.  out_values == NULL: the offsets only, as in ah_encode_descendants.
 * Refused with AH_ERR_INVALID_ARGUMENT, all of it before the first byte is written to out_values: a listed index >= n_nodes
 * or a listed free slot (the first offender by list position is named in ah_last_error); a split node with a child that is a
 * free slot; a listed node or a child whose id node_id_base + index would pass 2^32 - 1; out_cap smaller than the total; a
 * suspended index; a node whose list or normal row lies outside the index's arrays or a list that does not ascend (an index
 * ah_index_audit does not find valid).
 * The call reads only, like ah_index_audit: legal with live filters and concurrently with searches, not concurrent with a
 * mutating call on the same index.  Memory: 28 bytes of device scratch per listed node (+ 4 per listed index, + 4 per node
 * slot with node_id_of), and the values piece by piece — whole values that fit half of AH_READBACK_MB MiB, a longer value in
 * a piece of its own — through two device halves and the calling thread's pinned buffer: never the total.  A failed
 * allocation returns its status and holds nothing; out_value_offsets may then have been written, *out_stats not. */
typedef struct ah_index_encode_stats {
    uint64_t n_values, n_split, n_descendants, n_free;  /* listed values, and what they were                              */
    uint64_t value_bytes, pieces;                       /* the total; device -> host pieces (0 with out_values == NULL)   */
    double seconds;
} ah_index_encode_stats;
AH_API int ah_index_encode_nodes(ah_index *index, const uint32_t *node_indices, size_t n, const uint32_t *node_id_of,
                                 uint32_t node_id_base, uint8_t *out_values, uint64_t out_cap,
                                 uint64_t *out_value_offsets /* n + 1 */, ah_index_encode_stats *out_stats /* may be NULL */);

/* An index outlives an update of its dataset.  An ah_index stores ITEM IDS, never row positions — its descendants are a
 * copy of the view's ids and every kernel goes from an id to its row through the dataset as it is at the time of the
 * call — so nothing in it goes stale when ah_dataset_update_* moves rows.  ah_index_suspend gives up the index's hold on
 * the dataset (the update's "no live index" rule then lets the update through); until ah_index_resume every search, route,
 * filter or delete call on the index is refused (AH_ERR_INVALID_ARGUMENT), ah_index_destroy is not.  Refused while the index
 * has live filters.  ah_index_resume takes the hold again on the SAME dataset handle, which must be finalized (and has by
 * construction the metric, dimensions and device of the index; each is checked and named when it differs).  Ids of the
 * index that the update removed from the dataset must leave the index (ah_index_delete_items) before it is searched: a
 * search expects every id of its index to be a row of the dataset.  Host code only. */
AH_API int ah_index_suspend(ah_index *index);
AH_API int ah_index_resume(ah_index *index, ah_dataset *ds);

/* ------------------------------------------------------------------------------------------
 * Measurement helpers (bench.py).  They time with hipEvents recorded on the same stream the
 * kernels run on and never touch the host data path.
 * ---------------------------------------------------------------------------------------- */

/* Launch the Q=1 distance scan `iterations` times back to back over the first `n` rows and report
 * the total kernel time in milliseconds (HIP events on the launch stream).  The query is
 * item `query_item`.  Distances of the last iteration are left in an internal device buffer; if
 * `out` is non-NULL they are copied to it (n floats) after the timed region. */
AH_API int ah_bench_scan(ah_dataset *ds, uint32_t query_item, uint64_t n, uint32_t iterations, float *out,
                  double *out_ms_total);
/* Device-to-device copy of `bytes` bytes, `iterations` times: the measured streaming ceiling. */
AH_API int ah_bench_memcpy(int device, uint64_t bytes, uint32_t iterations, double *out_ms_total);
/* Read-only stream over `bytes` bytes (16-byte loads, integer checksum, nothing written), `iterations` times: the
 * measured read ceiling of the device, the practical bound of the scan kernels next to the 8 TB/s spec peak. */
AH_API int ah_bench_read(int device, uint64_t bytes, uint32_t iterations, double *out_ms_total);
/* Name of the device (hipDeviceProp_t.name / gcnArchName) into buf. */
AH_API int ah_device_name(int device, char *buf, size_t buf_len);

/* The blobs (normals, item ids) of destroyed forests are kept committed in a process-wide pool and handed to the next
 * build, which then takes no page faults for its 9.4 GB of output (AH_HOST_CACHE_MB bounds the pool, default 16 GiB;
 * 0 = keep nothing).  This returns the pool's memory to the system; *out_bytes (may be NULL) = committed bytes released. */
AH_API int ah_host_cache_trim(uint64_t *out_bytes);
/* Device memory is cached the same way: HBM the library has obtained (datasets, their binary16 / int8 copies, the ~28 GB of
 * scratch of a 10M x 100-tree build) goes back to the driver only under memory pressure or here — a hipMalloc that lands on
 * memory the driver is still scrubbing after a hipFree was measured to stall a build's first launch by a second
 * (AH_DEVICE_CACHE_MB bounds the idle bytes, default 96 GiB; 0 = plain hipMalloc / hipFree).  device < 0: every device. */
AH_API int ah_device_cache_trim(int device, uint64_t *out_bytes);
/* ABI v6: what the library holds on `device` (< 0: every device) right now — bytes handed out to its datasets, indexes,
 * builds and per-thread scratch (`live`), and bytes parked in the cache (`idle`).  Either pointer may be NULL.  The caches
 * live as long as a dataset does: when the last dataset of a device is destroyed its idle blocks go back to the driver, and
 * with the last dataset of the process the host blob pool goes back to the system (AH_CACHE_KEEP_IDLE=1 keeps them). */
AH_API int ah_device_cache_stats(int device, uint64_t *out_live_bytes, uint64_t *out_idle_bytes);
/* Benchmark harness only: n x dims synthetic rows of the generator of arroy_hip_policy.h (the rows
 * ah_dataset_fill_synthetic makes in HBM) in HOST memory, items first_item .. first_item + n - 1, on all host cores. */
AH_API int ah_synth_rows_host(uint64_t seed, int distribution, uint64_t first_item, uint64_t n, uint32_t dims, float *out);

/* Tunables: measurement / test aids that steer the SCHEDULE of the kernels (which family a level takes, grids, cache
 * policy), never a result.  `name` is the environment variable that initialises the tunable when the library is loaded
 * ("AH_ROWS_XCD", "AH_DENSE", "AH_SCREEN8", ...: DESIGN.md lists them).  Set them while no call is running. */
AH_API int ah_tuning_set(const char *name, int64_t value);
AH_API int ah_tuning_get(const char *name, int64_t *out_value, int64_t *out_default);
AH_API int ah_tuning_reset(void);   /* every tunable back to its built-in default (not to the environment's value) */

/* Test aid: run the block -> work-item maps of the build's launches on the device — the same device functions the
 * margin kernels call and the same host-side launch plans the build uses, under the current tunables — over a shape,
 * and count how often every work item is served (every count must be 1).
 *   kind 0: screened row-major pass, a = trees per group (2 / 4 / 8 / 16), b = groups; out_counts[b][n_rows]
 *   kind 1: dense MFMA screen, a = columns (normals of the level);               out_counts[row tiles][column tiles] (ah_debug_dense_tiles)
 *   kind 2: exact-pairs pass after the dense screen, a = trees;                   out_counts[a][ceil(n_rows / 1024)]
 * `dims` sizes the rows as the build would.  out_len = number of counters the caller allocated (checked). */
AH_API int ah_debug_launch_coverage(int device, int kind, uint64_t n_rows, uint32_t dims, uint32_t a, uint32_t b,
                                    uint32_t *out_counts, uint64_t out_len);
/* Test aid (ABI v6): the tile shape the dense MFMA screen takes for a level of `n_cols` normals under the current tunables
 * (the narrow kernel: 160 rows x 64 / 128 columns; the wide one: 256 x 128 / 256) — kind 1 of ah_debug_launch_coverage
 * counts [ceil(n_rows / tile_rows)][ceil(n_cols / tile_cols)] tiles. */
AH_API int ah_debug_dense_tiles(uint64_t n_rows, uint32_t n_cols, uint32_t *out_tile_rows, uint32_t *out_tile_cols);

#ifdef __cplusplus
}
#endif

#endif /* ARROY_HIP_H */
