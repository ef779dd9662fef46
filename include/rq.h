/* rq.h -- C ABI of the MI355X dense-retrieval backend (librq_hip.so).
 *
 * This is the drop-in boundary for the reference's dense path.  The reference has no native code;
 * the calls below replace the two third-party services its DenseIndex talks to:
 *
 *   reference rag_uq/streaming_index.py          replaced by
 *   ------------------------------------------   ---------------------------------------------
 *   :252-263  chromadb client + collection       rq_index_create / rq_load
 *   :306      collection.get()['ids'] (dedup)    host-side id table (Python), rq_index_size
 *   :326-331  collection.add(embeddings=...)     rq_index_add_f32 / rq_index_add_f16
 *   :355-359  collection.query(n_results=top_k)  rq_search (host buffers) / rq_search_device
 *   :363-368  score = 1 - distance, best first   scores returned as cosine similarity, best first
 *   :373      collection.count()                 rq_index_size
 *   (Chroma persistence directory)               rq_save / rq_load
 *
 * Conventions: plain pointers and sizes, no torch types.  Host buffers are C-contiguous and owned by
 * the caller; device memory is owned by the library.  Every int-returning call returns 0 on success
 * or a negative RQ_E* code; the message is in rq_last_error() (thread local).  Calls block unless
 * the name ends in _device.  One rq_index may be used from one thread at a time (the reference is
 * single-threaded, streaming_index.py has no locks).  There is no CPU fallback: without a gfx950
 * device every call that touches data fails with RQ_ENODEVICE.
 *
 * Caller buffers (every pointer argument of every *_device call: queries, thresholds, candidate lists, pools, masks, CSR query
 * arrays, and all outputs; pinned by tests/test_gpu_memory_contract.py):
 *   alignment: the natural alignment of the element type -- 4 bytes for float / int32_t / uint32_t, 8 bytes for double / int64_t /
 *            uint64_t, 2 bytes for fp16 rows -- and no more.  A view into a larger array is as good as an allocation of its own.
 *            Every load and store of a caller's array is one element wide; the wider accesses of the kernels touch only the
 *            library's own padded buffers.
 *   extents: a call reads and writes exactly the extents its arguments state -- [B][dim], [B][k], [B][k][s], [B][cap], [B],
 *            [B + 1], [n_q_tokens], [n_masks][W] -- whatever the number of query slots of the passes that serve it: no byte in
 *            front of an array, none behind it, no row of a pad slot.  Every slot of every output array is written: a result, or
 *            the padding the call defines (-1, 0.0, key 0, RQ_GROUP_NONE, count 0), d_status included.  An optional output
 *            that is NULL is skipped.  A fixup form writes the rows of the flagged queries only.
 *   inputs:  are never written.
 *   refusal: a call that returns RQ_EINVAL has written none of its outputs.
 *   deferred outputs: under "pipeline" 1 and 2, with announced batches and in bundles (see the flush call below) the outputs of a
 *            call belong to the library from the call until the call that completes them, or the stream's flush, or the release
 *            of the stream: they are written by later launches, each call's own [B][k] and d_status and nothing else, and must
 *            stay valid and untouched until then.
 *
 * Score definition (pinned by oracle/dense_oracle.py, "parity unpinned" upstream -- Chroma's own
 * arithmetic is not in the reference tree):
 *   cosine:  s = fp32( dot64(q, x) / (||q||_64 * ||x||_64 + 1e-30) )   on the STORED fp16 row x
 *   ip:      s = fp32( dot64(q, x) )
 *   order:   s descending, then row ascending;  k_eff = min(k, N);  missing entries row = -1.
 * Non-finite and extreme inputs, both metrics, every route (rq_search, the *_device forms, trains, multi-device indexes, filtered
 * searches, rq_search_mmr's candidates, rq_score_rows, rq_search_range, the grouped calls rq_search_grouped* and rq_group_collapse_device,
 * the group-member calls rq_search_group_members* and rq_group_fill_device; tests/nonfinite_oracle.py restates it):
 *   zero-norm query: a query whose fp64 norm is 0 scores every row 0.0, whatever the row holds (a NaN or infinite row included):
 *            its answer is rows 0 .. k_eff-1 (filtered: the first k_eff allowed rows) at 0.0.
 *   NaN:     any other score that comes out NaN (a NaN element on either side, inf - inf, 0 x inf, inf / inf -- under cosine every
 *            row or query with an infinite element, its norm being infinite) counts as -inf.
 *   +-inf:   legitimate scores (inner product with an infinite element) that order like any other: +inf first, -inf last, equal
 *            scores by row ascending.  A -inf row is still a row: k_eff = min(k, N) does not shrink, and once the better rows
 *            are used up the answer goes on with the -inf rows in row order.
 *   -0.0:    ranks with and is returned as +0.0.
 *   A query below RQ_TINY_QUERY_NORM (csrc/rq_final_body.h; fp32-subnormal elements) follows the definition with its 1e-30 as it
 *   stands.  Non-finite queries, and rows among the candidates that score -inf, are answered by the repair ladder (exact, slower);
 *   non-finite stored rows cost finite queries nothing.  The grouped and group-member calls leave such queries
 *   uncertified like any other search; they are answered by those calls' own fixups (rq_search_grouped_fixup_device: rung 2 and the
 *   exclusion loop over all -inf and all +inf tie runs; rq_search_group_members_fixup_device: the same, then the fill again).
 */
#ifndef RQ_H
#define RQ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rq_index rq_index;

enum { RQ_OK = 0, RQ_EINVAL = -1, RQ_ENODEVICE = -2, RQ_EHIP = -3, RQ_ENOMEM = -4, RQ_EIO = -5, RQ_EUNSUPPORTED = -6 };
enum { RQ_METRIC_COSINE = 0, RQ_METRIC_IP = 1 };
#define RQ_MAX_DIM 768
#define RQ_MAX_K 1024

/* Number of visible HIP devices (0 if none / no driver). */
int rq_device_count(void);

/* Create an empty index of `dim`-element rows (1 <= dim <= RQ_MAX_DIM).  NULL on error.
 * Stored row length: rows are kept zero padded to 384 fp16 elements (768 B per row) when dim <= 384 and to 768 elements
 *   (1 536 B) otherwise; option "row_pad" reads it and, on an empty index, changes it.  Results do not depend on it (scores are
 *   bit-identical); memory and the bytes every scan streams do.
 * n_devices == 1: one row shard on device_ids[0] (the form every *_device call works on; shards in other processes
 *   are merged with rq_merge_keys_device).
 * n_devices  > 1: the rows are sharded across device_ids[0..n_devices) inside the library: every appended block is cut
 *   into n_devices contiguous pieces, piece j is stored on device_ids[j]; rq_search enqueues the search on every device
 *   before it waits for any, copies each device's k best (score, row) pairs back and merges them on the host in the
 *   canonical order.  Same rq_index_add_f16 / _f32, rq_search, rq_index_get_rows_f16, rq_save / rq_load, rq_set_option
 *   calls; the device-pointer entry points (*_device) return RQ_EUNSUPPORTED on such an index.  A device may be named
 *   more than once (several shards on one GPU). */
rq_index* rq_index_create(int dim, int n_devices, const int* device_ids);
void rq_index_destroy(rq_index* idx);

int rq_index_dim(const rq_index* idx);
int64_t rq_index_size(const rq_index* idx);
/* Global id of this shard's row 0 (default 0); out_rows / keys carry row_offset + local row. */
int rq_index_set_row_offset(rq_index* idx, int64_t row_offset);
int rq_index_reserve(rq_index* idx, int64_t n_rows);

/* Append n rows (row-major [n][dim]).  _f16: IEEE binary16 bit patterns, stored as given.
 * _f32: rounded to fp16 (round-to-nearest-even); with normalize != 0 each row is first divided by
 * its fp64 L2 norm (cosine is invariant to it and fp16 range is never exceeded).
 * The fp64 norm of the STORED row is computed on device and kept for exact scoring. */
int rq_index_add_f16(rq_index* idx, const uint16_t* rows, int64_t n_rows);
int rq_index_add_f32(rq_index* idx, const float* rows, int64_t n_rows, int normalize);
/* Same, rows already in device memory of the index's GPU.  The call first waits for ALL prior work on
 * the device (the rows may come from any stream of the caller), then appends synchronously. */
int rq_index_add_f16_device(rq_index* idx, const void* d_rows, int64_t n_rows);
int rq_index_add_f32_device(rq_index* idx, const float* d_rows, int64_t n_rows, int normalize);
/* Copy stored rows [row_begin, row_begin+n) back to the host as fp16 bit patterns [n][dim]. */
int rq_index_get_rows_f16(const rq_index* idx, int64_t row_begin, int64_t n_rows, uint16_t* out);

/* Exact top-k of B queries ([B][dim] fp32, host).  out_scores [B][k], out_rows [B][k] (-1 padded).
 * Results are exact (see score definition): an on-device certificate proves it per query, and the
 * queries it cannot prove are re-run with a wider candidate set, finally with a full fp64 scan. */
int rq_search(rq_index* idx, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows);

/* Asynchronous form: all pointers are device pointers, work is enqueued on `stream` (a hipStream_t,
 * NULL = default stream).  d_keys ([B][k] uint64, may be NULL) receives sortable (score, global row)
 * keys for cross-shard merging.  d_status[B]: 0 = certified exact, 1 = not certified -- call
 * rq_search_fixup_device after the stream has the results you need repaired.
 * Calls on different streams may overlap; each stream has its own workspace. */
int rq_search_device(rq_index* idx, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                     uint64_t* d_keys, int* d_status, void* stream);
/* Deferred tails (option "pipeline"): the tail of a search (threshold, fp64 re-score, final top-k) is taken off
 * the critical path of `stream` so that the next corpus scan starts at once.
 *   1: the tail runs on an internal stream (two cross-stream events per call);
 *   2: the tail of call i is executed by extra workgroups of the scan launch of call i+1 on the same stream (no
 *      events, scans never overlap each other; calls of <= 64 queries, k <= 128).
 * In both modes the outputs of rq_search_device calls are complete on `stream` only after this call
 * (rq_search_fixup_device implies it); output buffers must stay valid until then.  Mode 1 also reads d_queries
 * until then, mode 2 keeps its own copy.
 * Mode 2 with announced batches (rq_search_hint_next_device, options "scan_ahead" / "scan_bundle") defers more than the tail:
 * a call may be held back WHOLE -- scan and tail -- until up to three calls after it have been made, so that one corpus pass
 * serves them all.  Nothing is enqueued for such a call beyond the copy of its queries; its outputs are written only by work
 * of a later call of the stream or of this flush.  The contract above holds as written: complete after this call, output
 * buffers valid until then.  Every other route on the stream and every change of the index (appends, a reserve that
 * reallocates, options, rq_save, rq_stream_release, rq_index_destroy) completes what is held back first: a held-back call
 * returns the rows the index held when it was made. */
int rq_search_flush_device(rq_index* idx, void* stream);
/* "pipeline" = 2 loops that know their next batch: announce the queries of the NEXT rq_search_device call on `stream`
 * before making the current one.  The current call's launch then prepares them (norms, unit-norm fp16 fragments) with 64
 * extra workgroups, and the next call -- when it is given exactly d_next_queries and B -- needs no preparation launch of its
 * own (measured: one 5 us kernel + a launch boundary per batch).  d_next_queries must hold its final contents when the
 * current call is made and stay unchanged until the call that searches it.  Advisory: a hint that cannot be used (more than
 * 64 queries, another pipeline mode, a different pointer / B at the next call, a flush in between) is dropped and the
 * next call prepares its queries itself; results never depend on it.  B = 0 or NULL withdraws a pending hint.
 * Option "scan_ahead" (default 1): on shards the Infinity Cache cannot hold (rows x 1536 B > 208 MiB), a call over the fp16
 * rows that has an announced successor scans BOTH batches in one 128-query pass; the next call, when it brings exactly
 * d_next_queries, B and the same metric (any k), enqueues no scan of its own and runs the two batches' tails.  Anything else
 * (another call, a flush, rq_stream_release) completes the first batch as usual and discards the half scanned ahead.
 * Option "scan_bundle" (default 4; 2 = pairs only): once a stream has completed three such pairs back to back -- since its
 * workspace was created, or since its last flush, unmatched call, release or call of another kind --, up to FOUR consecutive
 * announced 64-query calls are scanned by ONE 256-query pass: the first two only copy their queries, the third launches the
 * pass (over itself, the two before it and the batch it announces), the fourth runs all four tails in one launch, each with
 * its own k and outputs.  Only the last call of such a bundle may have fewer than 64 queries.  A call that does not bring
 * the announced batch, or announces nothing, ends the bundle: the calls held back are scanned then by the narrowest pass
 * (64, 128 or 256 queries) and nothing is lost; a batch scanned ahead that never comes is discarded.  Results are later by
 * up to three calls, never different.  Read-only option "bundles4" counts the 256-query passes made this way. */
int rq_search_hint_next_device(rq_index* idx, const float* d_next_queries, int B, void* stream);
/* A TRAIN of searches enqueued by one call (serving loops, the multi-GPU bench: a 125 k-row shard answers a 64-query batch in
 * ~25 us, which a host loop that crosses the language boundary twice per batch cannot feed): batch i = B queries at
 * d_queries[i], searched exactly as rq_search_device(idx, d_queries[i], B, k, metric, d_scores[i], d_rows[i],
 * d_keys ? d_keys[i] : NULL, d_status[i], streams[i % n_streams]) would, after announcing d_queries[i + n_streams] -- the
 * batch the same stream searches next -- with rq_search_hint_next_device.  The pointer tables are HOST arrays of device
 * pointers; d_queries holds n_batches + n_streams entries, the last n_streams of which are only announced (the first
 * batches of the NEXT train; NULL = nothing to announce).  Results are complete per stream after rq_search_flush_device,
 * as for single calls.  Replaces, n_batches times over, the collection.query of reference rag_uq/streaming_index.py:355-359. */
int rq_search_train_device(rq_index* idx, int n_batches, const float* const* d_queries, int B, int k, int metric,
                           float* const* d_scores, int64_t* const* d_rows, uint64_t* const* d_keys, int* const* d_status,
                           void* const* streams, int n_streams);
/* The library keeps one search workspace per caller stream: about 11 MB at 1M rows per 64 query slots, two of them for
 * alternating calls.  A stream that scans announced batches ahead holds one workspace of 256 slots ("scan_bundle" = 4: about
 * 44 MB at 1M rows; 128 slots, 22 MB, with "scan_bundle" = 2), sized once by its first such call, beside one of 64 slots and
 * 3 MB of prepared queries (8 slots of 64).  Call this before a
 * stream that has been used for searches is destroyed, or when it will not be used again: waits for the device, scans
 * the calls an open bundle still holds back, runs any deferred tail, frees the stream's workspace.  (Beyond 8 streams the library drops idle workspaces by itself.) */
int rq_stream_release(rq_index* idx, void* stream);
/* Synchronises `stream`, re-runs the queries whose d_status is non-zero with wider candidate sets /
 * the exact scan, patches d_scores/d_rows/d_keys/d_status in place.  Returns the number repaired. */
int rq_search_fixup_device(rq_index* idx, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                           uint64_t* d_keys, int* d_status, void* stream);

/* Merge per-shard key lists: d_keys_in [B][n_per_query] (any order, 0 = empty) -> best k per query.
 * d_rows receives the global row ids carried by the keys.  d_keys_out may be NULL. */
int rq_merge_keys_device(const uint64_t* d_keys_in, int n_per_query, int B, int k, float* d_scores, int64_t* d_rows,
                         uint64_t* d_keys_out, void* stream);

/* ---- filtered searches: the top-k over an allowed set of rows (the `where` of the collection.query this backend replaces,
 * reference rag_uq/streaming_index.py:355-359) --------------------------------------------------------------------------
 * A filter is a bitmap over the LOCAL rows of one single-device index: bit r % 32 of word r / 32 set = row r is allowed (local:
 * without row_offset; outputs still carry row_offset + row).  n_rows must equal rq_index_size (bits beyond it are ignored).  A
 * filter belongs to its index and to that size: after an append every call that takes it returns RQ_EINVAL ("stale filter"), as
 * does a filter of another index.  Creation blocks; the bookkeeping is done on the host from the bitmap (the device form copies
 * its n_rows / 8 bytes back once): the allowed count, the first RQ_MAX_K allowed rows, which bins hold an allowed row.  NULL on
 * error (rq_last_error); RQ_EUNSUPPORTED on a multi-device index, as the *_device calls (a striped filter is not built).
 * Memory: n_rows / 8 bytes of HBM, + 4 n_rows bytes per metric once a search has scanned with it (the masked row scales), + 4 bytes
 * per allowed row once a search has taken the gather route; n_rows / 8 + n_rows / 16 bytes on the host.
 * rq_index_destroy frees the filters it still owns: a filter must not be used, or destroyed, after its index. */
typedef struct rq_filter rq_filter;
rq_filter* rq_filter_create(rq_index* idx, const uint32_t* bits, int64_t n_rows);                        /* host bitmap */
rq_filter* rq_filter_create_device(rq_index* idx, const uint32_t* d_bits, int64_t n_rows, void* stream);  /* device bitmap, complete on `stream` */
int64_t rq_filter_count(const rq_filter* f);                                                             /* allowed rows */
void rq_filter_destroy(rq_filter* f);
/* rq_search / rq_search_device / rq_search_fixup_device over the allowed rows only.  Score definition as above with the top-k
 * taken over the allowed rows in the canonical order (score descending, then row ascending); k_eff = min(k, allowed rows), missing
 * entries (0.0, -1); a zero-norm query returns the first k_eff allowed rows with score 0.  Results are exact and never depend on
 * the route taken.
 * A filtered call behaves like a "pipeline" = 0 call: its results are complete in stream order, and it first completes whatever
 * `stream` still defers (a fused tail, a scanned-ahead pair, a hint), as rq_search_fixup_device does.  Not extended:
 * rq_search_train_device, hints, "scan_ahead", "pipeline" 1 and 2.  Filtered calls never touch the int8 image ("scan8_used" and
 * its ladder stay as they are), and their scans keep to the selection forms that honour a NaN row scale: "epi" = 0 and
 * "wide_batch" = 2 are ignored by a filtered call (it runs "epi" = 1 and the default 128-query pass).
 * Outputs of rq_search_filtered_device are repaired with rq_search_fixup_filtered_device and the SAME filter only: the unfiltered
 * rq_search_fixup_device would replace every uncertified query of theirs with unfiltered results.
 * Routes (csrc/rq_filter_plan.h), tried in this order: no row allowed -> padding; GATHER: exactly the allowed rows are re-scored
 * in fp64 (cost grows with B x allowed rows, not with the shard) -- taken when B x allowed <= rows and 4 x allowed <= rows (measured), or when the allowed rows
 * sit in fewer than two bins per wanted bin; SCAN: the usual scan passes over row scales in which excluded rows are NaN, a tail
 * that drops excluded rows, the same certificate -- only when enough of the tail's partitions hold an allowed row for its
 * threshold to narrow; else gather when at most a quarter of the rows is allowed, else EXACT: the fp64 scan of the shard.
 * Options: "filter_route" (-1 = that rule (default), 1 = gather, 2 = scan, 3 = exact: forces a route, for tests and A/B);
 * read-only "filter_route_last" (the route the last filtered call took: 0 = no row allowed, 1..3, -1 = none yet) and
 * "filter_repaired" (queries of filtered calls that came back uncertified and were repaired). */
int rq_search_filtered(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows);
int rq_search_filtered_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores,
                              int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_fixup_filtered_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores,
                                    int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream);

/* ---- per-query filters: one allowed set per query in one call (a batch of questions from different tenants, sources or users) ----
 * `filters` is a HOST array of B pointers, read during the call only and never kept: filters[q] restricts query q, a NULL entry
 * leaves that query unrestricted, entries may repeat in any arrangement.
 * Answer: query q's answer is, by definition, that of rq_search_filtered(idx, filters[q], ...) for that query alone (of rq_search for
 *   a NULL entry): the same score definition, canonical order, NaN, -0.0 and +-inf rules; k_eff = min(k, allowed rows of THAT query's
 *   filter), missing entries (0.0, -1) with key 0; a zero-norm query returns the first k_eff allowed rows of its own filter at 0.0;
 *   row_offset is added; keys as elsewhere (rq_merge_keys_device).  Results are exact and never depend on the plan.
 * Stream: the call behaves like a "pipeline" = 0 call.  It first completes whatever `stream` still defers (a fused tail, a
 *   scanned-ahead pair, a hint), its results are complete in stream order, and it defers nothing.  It never touches the int8 image.
 *   Not extended: rq_search_train_device, hints, "scan_ahead", "pipeline" 1 and 2; the MMR, range, grouped and member calls keep
 *   their one filter per call.
 * Refusals: every non-null entry gets the checks of rq_search_filtered: a filter of another index, or a stale filter, ANYWHERE in the
 *   array refuses the whole call before anything is enqueued (RQ_EINVAL).  RQ_EUNSUPPORTED on a multi-device index.  RQ_EINVAL for
 *   filters == NULL, B outside 1 .. 65535, k outside 1 .. RQ_MAX_K, an unknown metric, a null pointer; d_status is required in
 *   the device forms.
 * Status and repair: d_status[q] is 0 when query q is certified and 1 otherwise.  rq_search_fixup_filtered_each_device (the SAME
 *   arguments) waits for the stream, reads the statuses, repairs every flagged query with the repair ladder of
 *   rq_search_fixup_filtered_device under that query's OWN filter, patches the outputs in place and returns the number repaired.
 *   rq_search_filtered_each: blocking, host buffers, staged on the index's own stream like rq_search_filtered, repair included.
 * Plan (csrc/rq_filter_each_plan.h): the queries are grouped by filter pointer and every group is routed by the rule of
 *   rq_search_filtered with its own number of queries.  The groups of the GATHER route together are the ragged set: the batch is
 *   prepared once, one ragged gather launch re-scores each query's own allowed rows (the bits of the gather route) and one final
 *   launch ranks them -- three launches whatever the number of filters; beyond 1 GiB of candidate keys the set is cut into rounds.
 *   Groups of the SCAN and EXACT routes and the NULL entries run the existing call of their route, through pointer offsets when
 *   their queries are one contiguous run of the batch and through a staging copy otherwise (arrange a batch by filter to avoid the
 *   copy).  When more than 12 such filtered groups share 64 queries, ONE exact fp64 scan of the shard answers all of them, each query's keys
 *   masked by its own bitmap (the shared exact route).  A batch whose entries are all the same filter is exactly the
 *   rq_search_filtered_device call; a batch of NULL entries is the unfiltered search.
 * Timing: rq_timing counts one search and B queries per call, not one per group.
 * Memory: per stream, the staging of the largest scattered group (B_g x (4 dim + 20 k + 4) bytes) and the call's tables (about 64 bytes per
 *   query) beside the workspace every search keeps.
 * Options: "filter_route" forces the route of every group (1: every group with a row to return joins the ragged set; 2: one pass per
 *   group; 3: all of them take the shared exact route); "filter_route_last" reports the last group's route (-1: it was a NULL entry);
 *   "filter_repaired" counts the repairs of rq_search_fixup_filtered_each_device too.  Read-only: "filter_each_calls" (calls so
 *   far), "filter_each_groups_last" (distinct filters of the last call, NULL counting as one), "filter_each_ragged_last" (queries the
 *   ragged launches answered), "filter_each_rounds_last" (ragged rounds), "filter_each_shared_exact_last" (queries the shared exact
 *   route answered), "filter_each_routes_last" (bit r set = some group took route r: 0 no row allowed, 1 gather, 2 scan, 3 exact,
 *   4 a NULL entry).  Test hook "filter_each_key_cap": candidate keys per ragged round (0 = the default, 1 GiB / 8). */
int rq_search_filtered_each_device(rq_index* idx, const rq_filter* const* filters, const float* d_queries, int B, int k, int metric,
                                   float* d_scores, int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_fixup_filtered_each_device(rq_index* idx, const rq_filter* const* filters, const float* d_queries, int B, int k, int metric,
                                         float* d_scores, int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_filtered_each(rq_index* idx, const rq_filter* const* filters, const float* queries, int B, int k, int metric,
                            float* out_scores, int64_t* out_rows);

/* ---- diversified search: MMR selection over candidate rows (what a max_marginal_relevance_search(query, k, fetch_k, lambda_mult)
 * does on the host with the fetch_k embeddings of the collection.query of reference rag_uq/streaming_index.py:355-359) ----------
 * Greedy maximal marginal relevance: k of m candidates per query, each step taking the candidate that is most relevant and least
 * similar to the rows already taken.  Per query: candidate positions 0..m-1, each a global row c_i and a relevance rel_i (fp32).
 *   absent candidate: c_i = -1 or any row outside [row_offset, row_offset + rq_index_size), or a NaN rel_i.  It is never selected
 *     and its row is never read.  Duplicates are not checked: the candidate rows must be distinct.
 *   pair similarity: the score definition above with STORED rows on both sides: d = sum_e (double)x_i[e] * (double)x_j[e];
 *     cosine: sim(i, j) = fp32( d / (n_i * n_j + 1e-30) ), n = the stored fp64 row norm; ip: sim(i, j) = fp32(d); a NaN sim
 *     counts as -inf, as for every score.  The zero-norm-query rule of the score definition does NOT apply to sim, which has no
 *     query: a zero row against a row with an infinite element is 0 x inf = NaN, hence -inf, under both metrics.
 *   penalty: pen_i (fp32) = 0 before the first pick, afterwards the maximum of sim(i, j) over the selected j.
 *   value: v_i = lambda * (double)rel_i - (1.0 - lambda) * (double)pen_i in fp64: two products and one subtraction, each
 *     rounded, no fused multiply-add.  A term whose weight (lambda, 1.0 - lambda) is exactly 0 is 0 whatever its other factor, an
 *     infinite one included; a NaN v (inf - inf) counts as -inf.
 *   step: among the present, unselected candidates the greatest v wins, the lowest position on equal v;
 *     k_eff = min(k, present candidates) steps.
 *   outputs, in selection order: d_rows / out_rows the global rows; d_scores / out_scores the candidate's relevance, passed through
 *     unchanged (for a search: its cosine, so everything downstream keeps working); d_mmr / out_mmr (may be NULL) fp32(v) at the
 *     moment of selection; entries beyond k_eff are (0.0, -1, 0.0).
 *   Hence lambda = 1 returns the candidates in relevance order (on a search's own candidates: that search's top k, also where rows
 *     are non-finite and penalties infinite), and at lambda = 0 the first pick is position 0 and every later d_mmr is -pen of the
 *     row picked.
 * rq_mmr_select_device: asynchronous, pure selection over a caller's candidates [B][m] in device memory, any order, any relevance (a
 *   fused hybrid score as well as a cosine).  It runs in stream order after whatever produced the candidates and defers nothing.
 *   RQ_EINVAL unless 1 <= k <= m <= RQ_MAX_K, 1 <= B <= 65535, lambda finite and within [0, 1] (NaN included), a known metric and
 *   non-null pointers (d_mmr aside); RQ_EUNSUPPORTED on a multi-device index; RQ_ENODEVICE as everywhere.
 * rq_search_mmr: blocking, host buffers ([B][dim] queries; out_scores, out_rows, out_mmr [B][k]).  The exact top
 *   min(fetch_k, rows) -- with a filter f (may be NULL): min(fetch_k, allowed rows), over the allowed rows only -- staged as
 *   rq_search_filtered stages its call, then the selection, then the copies back.  It behaves like a "pipeline" = 0 call: whatever the
 *   index's own stream still defers is completed first; uncertified queries are repaired with the usual ladder, so the candidates
 *   are exact.  RQ_EINVAL unless 1 <= k <= fetch_k <= RQ_MAX_K and lambda within [0, 1]; the filter checks are those of
 *   rq_search_filtered (another index's filter, a stale filter: RQ_EINVAL); RQ_EUNSUPPORTED on a multi-device index.
 * The selection reads the stored rows: one rq_index from one thread at a time, as for a search, and no append while a selection is
 *   in flight.  Memory: none kept; rq_search_mmr stages B x (fetch_k x 12 + k x 16) bytes for the call.
 * Not extended: rq_search_train_device, hints, "pipeline" 1 and 2 (a deferred search's candidates are complete only after
 *   rq_search_flush_device: flush, then select), multi-device indexes.
 * Read-only option "mmr_calls": selections launched so far (both entry points). */
int rq_mmr_select_device(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_rel, int B, int m, int k, double lambda, int metric,
                         float* d_scores, int64_t* d_rows, float* d_mmr, void* stream);
int rq_search_mmr(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int fetch_k, double lambda, int metric,
                  float* out_scores, int64_t* out_rows, float* out_mmr);

/* ---- scoring given rows: the exact score of named (query, row) pairs (what hybrid fusion needs for a passage that only the OTHER
 * retriever returned: reference rag_uq/streaming_index.py:485-523 writes 0.0 there, :498-499, because collection.query scores only
 * what it returns; also re-scoring a re-ranker's candidates, checking a cached answer against the index) ---------------------------
 * One list of m rows per query, no ranking: scores[q][j] is the score of query q and row rows[q][j], position for position.
 *   lists: rows / d_rows [B][m] int64 GLOBAL rows (row_offset + local row), scores / d_scores [B][m] fp32.  Duplicates are allowed, a
 *     list need not be sorted.
 *   absent entry: a value outside [row_offset, row_offset + rq_index_size), -1 included.  Its score is 0.0 -- the reference's own
 *     value for "not scored" -- and no row is read for it.  On an empty index every entry is absent.
 *   score: the score definition above on the STORED fp16 row; a NaN score counts as -inf, as for every score; -0.0 is returned as
 *     0.0, as every search returns it; a zero-norm query scores every present row 0.0 under both metrics.
 *   same bits as every other route: the value is the one rq_search and the gather route of a filtered search return for that pair
 *     (the queries are prepared by the same kernel, every dot product is summed in the same order: csrc/rq_rowdot.h).
 * rq_score_rows_device: asynchronous, device pointers; its results are complete in stream order.  It behaves like a "pipeline" = 0
 *   call, as rq_search_filtered_device does: it first completes whatever `stream` still defers (a fused tail, a scanned-ahead pair, a
 *   hint), because it uses the stream's prepared-query slots, and it defers nothing itself.  Afterwards the stream's "last search"
 *   has no bin records (rq_debug_bin_records: RQ_EINVAL), as after a gather-route call.  Queries are taken in groups of 1 024.
 * rq_score_rows: blocking, host buffers, staged on the index's own stream like rq_search_filtered: B x dim x 4 + B x m x 12 bytes of
 *   HBM for the call (RQ_ENOMEM with a message when that fails).
 * RQ_EINVAL unless 1 <= B <= 65535, 1 <= m <= RQ_MAX_SCORE_ROWS, a known metric and non-null pointers; RQ_EUNSUPPORTED on a
 *   multi-device index, for both forms; RQ_ENODEVICE as everywhere.  The call reads the stored rows: one rq_index from one thread at
 *   a time, and no append while a call is in flight.
 * Not extended: rq_search_train_device, hints, "pipeline" 1 and 2, multi-device indexes.
 * Read-only options "score_calls" (calls so far, both entry points) and "score_pairs" (B x m per call: present pairs are not
 *   counted separately).  rq_timing is untouched: a scoring call is not a search. */
#define RQ_MAX_SCORE_ROWS 65536
int rq_score_rows_device(rq_index* idx, const float* d_queries, int B, const int64_t* d_rows, int m, int metric,
                         float* d_scores, void* stream);
int rq_score_rows(rq_index* idx, const float* queries, int B, const int64_t* rows, int m, int metric, float* out_scores);

/* ---- range searches: every row that scores at least a threshold (what a caller of the collection.query of reference
 * rag_uq/streaming_index.py:355-359 gets today by fetching k rows and cutting the list on the host -- abstaining when no passage is
 * relevant enough, near-duplicate checks on ingest, "how many passages clear the bar") ------------------------------------------
 * For query q with threshold thr[q] (fp32):
 *   score: the score definition above on the STORED fp16 row; a NaN score counts as -inf, -0.0 is +0.0, a zero-norm query scores
 *     every row 0.0 -- the rules of every search.
 *   a row qualifies iff its returned fp32 score s satisfies s >= thr[q]: the comparison is on the fp32 values, after the NaN and
 *     -0.0 rules.  With a filter f (may be NULL) only allowed rows can qualify.
 *   count[q] (int64) = the number of qualifying rows.  It is exact, also when it exceeds cap.
 *   outputs [B][cap]: the min(count[q], cap) best qualifying rows in the canonical order (score descending, then row ascending),
 *     global rows = row_offset + local row; entries beyond that are (0.0, -1), with key 0 where keys are asked for.
 *   thr[q] must be finite.  Where the host can see the thresholds (rq_search_range) a NaN or infinite threshold is RQ_EINVAL; in the
 *     device forms a non-finite d_thr[q] makes that query return nothing, with count 0 and status 0.
 *   Hence a zero-norm query returns rows 0 .. min(N, cap) - 1 at 0.0 with count N when thr <= 0 and nothing when thr > 0; filtered,
 *     the first allowed rows and the allowed count.  An empty index returns count 0 and padding.
 *   same bits as every other route: a row's score is the value rq_score_rows and rq_search return for that pair (csrc/rq_rowdot.h), so
 *     thr = that value includes the row and nextafter(thr, +inf) excludes it.
 * RQ_EINVAL unless 1 <= cap <= RQ_MAX_K, 1 <= B <= 65535, a known metric and non-null pointers (d_keys and f aside); the filter checks
 *   are those of rq_search_filtered (another index's filter, a stale filter: RQ_EINVAL); RQ_EUNSUPPORTED on a multi-device index;
 *   RQ_ENODEVICE as everywhere.
 * rq_search_range_device: asynchronous, device pointers, no host synchronisation.  It behaves like a "pipeline" = 0 call, as
 *   rq_search_filtered_device does: it first completes whatever `stream` still defers (a fused tail, a scanned-ahead pair, a hint) and
 *   its results are complete in stream order.  It never touches the int8 image, and with a filter its scans keep to the forms that
 *   honour a NaN row scale.  d_status[B]: 0 = complete, 1 = this query's outputs are not (its qualifying rows overflowed the candidate
 *   list -- d_count[q] is exact already -- or the query is NaN / infinite): call rq_search_range_fixup_device with the SAME arguments.
 * rq_search_range_fixup_device: synchronises `stream`, re-runs the queries whose d_status is non-zero on the exact route, patches
 *   d_scores / d_rows / d_keys / d_count / d_status in place.  Returns the number repaired.
 * rq_search_range: blocking, host buffers, staged on the index's own stream like rq_search_filtered (repair included):
 *   B x (dim x 4 + cap x 12 + 16) bytes of HBM for the call (RQ_ENOMEM with a message when that fails).
 * Routes (csrc/rq_range_plan.h); results never depend on the route.  No row to return (an empty index, a filter that allows none)
 *   -> padding.  SCAN (1), the hot path: the call's usual fp16 scan passes, then a range tail that walks the query's bin records
 *   (csrc/rq_device.h): a 64-row bin is skipped iff the certificate's last step, with thr in the place of the k-th score, proves
 *   that none of its rows reaches thr; every other bin's rows are re-scored exactly.  The cost is one scan plus the bins that clear
 *   the bar: a threshold that most bins clear re-scores most of the shard.  GATHER (2), filtered calls only: exactly the allowed
 *   rows are re-scored, when B x allowed <= rows and 4 x allowed <= rows (the measured rule of rq_search_filtered).  EXACT (3): the
 *   fp64 scan of the shard, keys below thr emptied -- when the scan's scores say nothing (the "eps" rule of rq_search), and for the
 *   queries the fixup repairs.
 * Not extended: rq_search_train_device, hints, "scan_ahead", "pipeline" 1 and 2, multi-device indexes, the int8 image.  More than
 *   RQ_MAX_K rows per query are not returned; the count is still exact.
 * rq_timing counts a range call as a search (searches, queries; repaired queries as exact_scans).
 * Options: "range_route" (-1 = the rule (default), 1 = scan, 2 = gather (filtered calls), 3 = exact: forces a route, for tests and
 *   A/B); "range_cand_cap" (test hook: qualifying rows a query of the scan route may hold before it overflows; 0 = default 4096, never
 *   below cap); read-only "range_route_last" (the route the last range call took: 0 = no row to return, 1..3, -1 = none yet),
 *   "range_calls" (calls so far, both entry points), "range_repaired" (queries repaired by the fixup), "range_bins_last" (bins the
 *   last call's range tail re-scored, summed over its queries; -1 = it did not take the scan route; waits for the device). */
int rq_search_range_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, const float* d_thr, int cap, int metric,
                           float* d_scores, int64_t* d_rows, uint64_t* d_keys, int64_t* d_count, int* d_status, void* stream);
int rq_search_range_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, const float* d_thr, int cap, int metric,
                                 float* d_scores, int64_t* d_rows, uint64_t* d_keys, int64_t* d_count, int* d_status, void* stream);
int rq_search_range(rq_index* idx, const rq_filter* f, const float* queries, int B, const float* thr, int cap, int metric,
                    float* out_scores, int64_t* out_rows, int64_t* out_count);

/* ---- grouped searches: the best row of each of the k best groups (what a caller of the collection.query of reference
 * rag_uq/streaming_index.py:355-359 does on the host for a chunked corpus -- over-fetch, keep the best passage per article, hope the
 * over-fetch was enough; "field collapsing", "search_groups", "grouping search" elsewhere) ------------------------------------------
 * groups: every stored row has a group id (int32).  RQ_GROUP_NONE (-1), the default, means the row is a group of its own; any value
 *     >= 0 puts the row in the same group as every other row carrying that value.  Ids need not be dense.
 *   ranking: the score definition and canonical order above: score descending, then row ascending; NaN counts as -inf; -0.0 is +0.0;
 *     a zero-norm query scores every row 0.0.  With a filter f (may be NULL) only allowed rows take part: the rows in play.
 *   winner: a group's winner is its best row in that order; groups rank by their winners.
 *   result for k: the winners of the k best groups, best first, with their scores and group ids;
 *     k_eff = min(k, distinct groups among the rows in play); entries beyond that are (0.0, -1, RQ_GROUP_NONE), with key 0 where keys
 *     are asked for.
 *   Hence: with no group set the result is rq_search's, bit for bit; with every row in one group k_eff = 1; a zero-norm query returns
 *     the lowest row of each of the first k_eff groups in row order; a row's score has the same bits as rq_score_rows gives that pair.
 * rq_index_set_groups: host array, LOCAL rows [row_begin, row_begin + n_rows), blocking; it waits for prior work on the device, as an
 *   append does.  RQ_EINVAL for a range outside the stored rows or an id below RQ_GROUP_NONE.  rq_index_get_groups is the read-back
 *   (of the device copy).  Storage: 4 B per row of HBM, allocated by the first rq_index_set_groups, which follows rq_index_reserve and
 *   append growth, + a host copy of 4 B per row for the repair below; rows appended later are RQ_GROUP_NONE.  Groups are NOT written by
 *   rq_save: the files stay as they are, and an index that rq_load creates has no group set.
 * rq_group_collapse_device: asynchronous, pure selection over a caller's candidates [B][m] in device memory, any order, with
 *   1 <= k <= m <= RQ_MAX_K.  absent candidate: as for rq_mmr_select_device -- c_i = -1 or any row outside [row_offset, row_offset +
 *   rq_index_size), or a NaN score; it is never a winner and its group is never read.  The candidate rows must be distinct.
 *   d_cand_groups [B][m] may be NULL: the group is looked up by row in the index (4 bytes per candidate; no stored row is read).  Given
 *   explicitly (any negative id = RQ_GROUP_NONE) it serves fused hybrid pools and lists merged from several shards: merging per-shard
 *   grouped top-k lists and collapsing again is exact.  d_status[q] = 0 when the present candidates hold at least k
 *   distinct groups, else 1.  It runs in stream order after whatever produced the candidates and defers nothing.
 * rq_search_grouped_device: asynchronous, device pointers.  It behaves like a "pipeline" = 0 call: it first completes what `stream`
 *   defers (a fused tail, a scanned-ahead pair, a hint), as rq_search_filtered_device does.  One rung: the exact search for m1 rows
 *   (the filtered search when f is given), then the collapse; the candidates stay in the stream's workspace (B x m1 x 12 bytes).
 *   d_status[q]: 0 = the result is proven, 1 = not -- call rq_search_grouped_fixup_device with the SAME arguments.  Proven: the search
 *   certified the query, and its list either holds at least k groups or already holds every row in play.
 * rq_search_grouped_fixup_device: synchronises `stream`, repairs the flagged queries in place and returns how many it repaired.
 *   Rung 2: m = min(rows in play, RQ_MAX_K), repaired by the usual ladder, then collapsed.  Rung 3, for queries still short of k
 *   groups, the exclusion loop: the d winners found are the exact top d groups, because the list was the exact top m rows; the rows in
 *   play that belong to none of them become a temporary rq_filter (built on the host from the group copy); that query is searched
 *   filtered for up to RQ_MAX_K rows, collapsed, and the new winners are appended; until k winners are found or no row is left.  Every
 *   round adds at least one group; no other scan kernel is involved.
 * rq_search_grouped: blocking, host buffers ([B][dim] queries; out_scores, out_rows, out_groups [B][k], all required), staged on the
 *   index's own stream like rq_search_mmr, repair included: B x (dim x 4 + k x 16 + 4) bytes of HBM for the call.
 * RQ_EINVAL unless 1 <= k <= RQ_MAX_K, 1 <= B <= 65535, a known metric and non-null pointers (d_keys, d_cand_groups and f aside); the
 *   filter checks are those of rq_search_filtered (another index's filter, a stale filter: RQ_EINVAL); RQ_EUNSUPPORTED on a multi-device
 *   index, for every call of this section; RQ_ENODEVICE as everywhere.  One rq_index from one thread at a time, and no
 *   rq_index_set_groups while a grouped call is in flight.
 * Not extended: these calls return one row per group only -- group_size > 1 needs per-group member counts and a row list per group, and
 *   is served by rq_search_group_members* ("group members", below); rq_search_train_device, hints, "pipeline" 1 and 2, "scan_ahead",
 *   multi-device indexes.
 * rq_timing counts a grouped call as a search (searches, queries; its repairs as the ladder counts them).
 * Options: "group_fetch" (1 .. RQ_MAX_K, default 8: the first rung asks for m1 = this multiple of k, clamped to [k, min(rows in play,
 *   RQ_MAX_K)]; the default is the measured choice of DESIGN.md 4.16); "group_fetch_cap" (test hook, like "range_cand_cap": the largest m
 *   any rung may ask for, never below a call's k; 0 = RQ_MAX_K; it lets small shapes reach rung 3); read-only "group_calls" (collapses
 *   launched, every entry point and rung), "group_repaired" (queries the grouped fixup repaired), "group_rounds_last" (exclusion rounds
 *   of the last fixup that repaired anything, summed over its queries). */
#define RQ_GROUP_NONE (-1)
int rq_index_set_groups(rq_index* idx, int64_t row_begin, int64_t n_rows, const int32_t* groups);
int rq_index_get_groups(const rq_index* idx, int64_t row_begin, int64_t n_rows, int32_t* out);
int rq_group_collapse_device(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_scores, const int32_t* d_cand_groups, int B, int m, int k,
                             float* d_scores, int64_t* d_rows, int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_grouped_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                             int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_grouped_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                                   int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream);
int rq_search_grouped(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows,
                      int32_t* out_groups);

/* ---- group members: the best s rows of each of the k best groups ("the top k articles, each with its two or three best passages":
 * inner_hits / group_size elsewhere) -------------------------------------------------------------------------------------------------
 * For a query, a group size s >= 1 and k >= 1 with k x s <= RQ_MAX_K:
 *   groups and their rank: exactly as rq_search_grouped defines them -- rows in play, winner, groups rank by their winners,
 *     k_eff = min(k, distinct groups among the rows in play).
 *   members of a group: its rows in play, in the canonical order (score descending, then row ascending).  NaN counts as -inf; -0.0 is
 *     +0.0; a zero-norm query scores every row 0.0; a -inf row is still a row; a row with RQ_GROUP_NONE is a group of one.
 *   result: for group slot j < k_eff, count[q][j] = min(s, rows in play of that group); rows[q][j][0 .. count) and scores[q][j][0 .. count)
 *     are the best members, best first; entries beyond count are (0.0, -1); slots beyond k_eff are (0.0, -1, RQ_GROUP_NONE, count 0).
 *   Hence: s = 1 is rq_search_grouped's answer bit for bit; member 0 of every slot is that slot's winner, same row and same score bits;
 *     every member's score has the bits rq_score_rows returns for that pair (the dot product of csrc/rq_rowdot.h over queries prepared
 *     as rq_score_rows_device prepares them); with no group set every slot has count 1 and the result is rq_search's; a zero-norm query
 *     returns the lowest s rows in play of each of the first k_eff groups.
 * The members are fetched through the group, not through the ranking (a group's third-best row may rank anywhere): the library keeps a
 *   group member table -- the rows with id >= 0 sorted by (id, row), the sorted distinct ids and their offsets; ids need not be dense,
 *   the kernel finds a group's range by binary search.  It is built from the host copy of the ids by the FIRST call of this section that
 *   needs it (blocking: a host sort and three uploads; rq_search_grouped users pay nothing) and dropped by rq_index_set_groups; an
 *   append does not invalidate it (appended rows are RQ_GROUP_NONE and belong to no list), growth and rq_index_reserve leave it alone,
 *   rq_index_destroy frees it, rq_save stays as it is.  Storage: 4 B per grouped row + 8 B per distinct group of HBM, and as much host
 *   memory while it is built (the host copy of the ids, 4 B per row, is rq_index_set_groups's).
 * The fill kernel (csrc/rq_group_members.hip): one workgroup per (query, group slot) scores every row of the slot's group that is in
 *   play and sorts the keys in LDS; at most RQ_GROUP_FILL_MAX = 4096 rows (32 KiB of keys: a structural limit).  A group with more rows
 *   in the table than option "group_fill_cap" is not filled: its slot gets count = -1 and (0.0, -1) entries, and the query's status
 *   becomes 1.
 * rq_group_fill_device: asynchronous, pure fill over a caller's groups (the articles of a fused hybrid pool, a grouped call's own
 *   outputs): d_win_rows, d_win_groups [B][k] name the slots.  An absent slot (row -1 or outside [row_offset, row_offset +
 *   rq_index_size)) gets count 0; a slot whose id is negative is its row alone (count 1 when the row is in play); otherwise the members
 *   are the rows in play carrying the id (none: count 0); the same group may stand in two slots.  d_scores, d_rows [B][k][s], d_count
 *   [B][k] (int32), d_status [B] (0, or 1 when a slot overflowed).  It behaves like rq_score_rows_device towards the stream: it completes
 *   what `stream` defers, runs in stream order, defers nothing, and leaves no bin records.
 * rq_search_group_members_device: asynchronous; the grouped search (rq_search_grouped_device's one rung, winners in the stream's
 *   workspace: B x k x 12 bytes) then the fill.  d_groups [B][k].  d_status[q] = 0 iff the grouped stage proved the query and every
 *   slot was filled; else call rq_search_group_members_fixup_device with the SAME arguments.
 * rq_search_group_members_fixup_device: synchronises `stream`, repairs the flagged queries in place and returns how many it repaired:
 *   their winners are searched again and repaired (Rung 2 and Rung 3 of rq_search_grouped_fixup_device), the fill runs again, and a slot
 *   that still overflows takes the exact route -- the group's rows in play become a temporary rq_filter (built on the host from the
 *   group copy and the caller's filter), the query is searched filtered for s rows and repaired by the usual ladder.
 * rq_search_group_members: blocking, host buffers (out_scores, out_rows [B][k][s]; out_groups, out_count [B][k]; all required), staged
 *   on the index's own stream like rq_search_grouped, repair included: B x (dim x 4 + k x s x 12 + k x 8 + 4) bytes of HBM for the call.
 * RQ_EINVAL unless k >= 1, s >= 1, k x s <= RQ_MAX_K, 1 <= B <= 65535, a known metric and non-null pointers (f aside); the filter checks
 *   are those of rq_search_filtered (another index's filter, a stale filter: RQ_EINVAL); RQ_EUNSUPPORTED on a multi-device index;
 *   RQ_ENODEVICE as everywhere.  One rq_index from one thread at a time, and no rq_index_set_groups while such a call is in flight.
 * Not extended: keys (d_keys) and merging members across shards -- a group's members in a shard where the group is not among that
 *   shard's top k are not in that shard's lists, so the merge argument of DESIGN.md 4.16 does not carry over; rq_search_train_device;
 *   hints; "pipeline" 1 and 2; "scan_ahead".
 * rq_timing counts the call as a search, as a grouped call does.
 * Options: "group_fill_cap" (test hook: rows of a group the fill kernel takes; it can only lower the maximum, 0 = default =
 *   RQ_GROUP_FILL_MAX); read-only "group_table_builds" (member tables built), "group_fill_calls" (fills launched, every entry point and
 *   the repair's), "group_fill_repaired" (queries the fixup filled by the exact route: those that held an overflowed slot; a query that
 *   only its grouped stage flagged is counted by "group_repaired"), "group_fill_rows_last" (members scored by the last fill, summed over
 *   its slots; -1 = none yet; waits for the device). */
#define RQ_GROUP_FILL_MAX 4096
int rq_group_fill_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, const int64_t* d_win_rows,
                         const int32_t* d_win_groups, float* d_scores, int64_t* d_rows, int32_t* d_count, int* d_status, void* stream);
int rq_search_group_members_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, float* d_scores,
                                   int64_t* d_rows, int32_t* d_groups, int32_t* d_count, int* d_status, void* stream);
int rq_search_group_members_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, float* d_scores,
                                         int64_t* d_rows, int32_t* d_groups, int32_t* d_count, int* d_status, void* stream);
int rq_search_group_members(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int s, int metric, float* out_scores, int64_t* out_rows,
                            int32_t* out_groups, int32_t* out_count);

/* ---- sparse search: exact BM25 top-k over a posting index that lives on the device (the sparse half of the hybrid retriever,
 * reference rag_uq/streaming_index.py:168-177, which include/rq_bm25.h answers on the host cores) ------------------
 * An rq_sparse is an object of its own, beside rq_index: an inverted index in CSR form -- token t owns postings
 * [indptr[t], indptr[t+1]): rows[] = document rows, contrib[] = that posting's float64 score contribution -- copied to one device.
 * Definition: that of rq_bm25_topk, restated.
 *   score(q, d) = the float64 sum of contrib[p] over the query's tokens, with repetition, added IN QUERY ORDER starting from 0.0.
 *   Only documents with score > 0 are returned: a NaN or negative total and an exact cancellation are left out; a +inf total is a
 *     score like any other and ranks first.
 *   Results are best first, equal scores by DESCENDING row, at most k per query; out_rows is padded with -1, out_scores with 0.0.
 *   Every returned score has the bits rq_bm25_topk returns, every row list is identical to its list (the kernel performs the same
 *     additions in the same order; csrc/rq_sparse.hip).
 * rq_sparse_create: host CSR arrays, COPIED to the device (unlike rq_bm25_create, which borrows them): 12 B per posting + 8 B per
 *   token of HBM.  It refuses what rq_bm25_create refuses (indptr[0] != 0, a decreasing indptr, a row outside [0, n_docs)), and
 *   also rows of a token that are not STRICTLY ascending (the kernel binary-searches them; BM25Index produces them so) and
 *   n_docs >= 2^31: NULL with the message in rq_last_error(); NULL + the "no HIP device" message without a gfx950 device.
 * Queries: query q owns q_tokens[q_indptr[q] .. q_indptr[q+1]), token ids in query order with repetition.
 * rq_sparse_topk: blocking, host buffers (out_rows [B][k] int32, out_scores [B][k] float64), staged on a stream the handle owns.
 *   RQ_EINVAL unless 1 <= B <= 65535, 1 <= k <= RQ_SPARSE_MAX_K, q_indptr[0] >= 0 and never decreasing, every token id in
 *   [0, n_tokens), non-null pointers.
 * rq_sparse_topk_device: asynchronous, device pointers, no host synchronisation in steady state; results are complete in stream
 *   order.  n_q_tokens = the length of d_q_tokens.  The host cannot see the queries: a token id outside [0, n_tokens) is an EMPTY
 *   posting list, and an entry of d_q_indptr outside [0, n_q_tokens] or below its predecessor is clamped (no read outside the arrays).
 * rq_sparse_topk_masked / rq_sparse_topk_masked_device: the same calls with one ALLOWED SET per query: the batch
 *   form of BM25Index.search(..., allowed_ids=), behind the `allowed_ids` / `allowed_ids_each` keywords of the batch calls.
 *   Definition: scores are added exactly as above; a document outside the query's allowed set then scores 0.0 BEFORE the score > 0
 *     selection.  Query q's answer is therefore rq_sparse_topk's answer over its allowed documents alone -- every row, order, count
 *     and score bit -- and that of rq_bm25_topk_masked (include/rq_bm25.h).  An empty set returns nothing.
 *   Masks: `masks` is [n_masks][W] uint32, W = ceil(n_docs / 32); bit r % 32 of word r / 32 set = document row r is allowed (the
 *     bitmap layout of rq_filter_create).  Bits at or beyond n_docs are ignored, whatever they hold.  mask_of[q] is the mask of query
 *     q of the CALL, -1 = unrestricted; the same mask may serve any number of queries, in any arrangement.
 *   Checks: those of rq_sparse_topk / rq_sparse_topk_device, and RQ_EINVAL for mask_of == NULL, n_masks < 0 and masks == NULL with
 *     n_masks > 0 (n_masks == 0 without a table is legal when every entry is -1).  The blocking form sees mask_of and refuses an
 *     entry outside [-1, n_masks) with RQ_EINVAL; the device form cannot, and treats such an entry as "allows nothing" (padding, no
 *     read outside the arrays: the manner of the token clamping).  The device form reads d_masks and d_mask_of in stream order and
 *     keeps neither.
 *   Kernel: the tile kernel of rq_sparse_topk, instantiated with the mask in two places.  Before any posting is looked up a
 *     workgroup ORs the mask words of its tile (at most 256 words, one load per thread, the ragged last tile cut at n_docs) and
 *     leaves at once when no document is allowed; after the accumulation and before anything is counted or selected, the
 *     accumulators of the disallowed documents are set to 0.0.  The accumulation itself, the final kernel, the workspace, the rounds,
 *     "tile_docs", "cand_cap" and "profile" are those of the unmasked call, which keeps its code, counters and launch count.
 *   Cost: that of the unmasked call, minus the tiles that leave early.  Out of scope: a gather route for selective masks (score only
 *     the allowed rows with rq_sparse_score_rows_device, then select); whether it pays is a later measurement.
 * Workspace and threading: one workspace per handle, tiles x min(k, tile_docs) x 12 B + 4 B per tile for every query of a round.  A
 *   handle is used from one thread and its calls are ordered by the caller: one stream, or events between streams.  A call that
 *   needs a larger workspace than the handle has waits for the device once (hipDeviceSynchronize) and allocates; a call that fits
 *   does not wait.
 * Options (rq_sparse_set_option / rq_sparse_get_option; results never depend on them): "tile_docs" (documents per workgroup, a power
 *   of two in 64 .. 8192, default 4096: one float64 accumulator per document in LDS; settable any time), "cand_cap" (test hook:
 *   candidate bytes -- tiles x min(k, tile_docs) x 12 per query -- one round of queries may hold, 0 = default = 1 GiB; a call beyond it
 *   runs in rounds, a query beyond it alone in a round of its own); read-only "calls" (masked calls included), "masked_calls", "rounds_last", "tiles_last"
 *   (tiles x B of the last call), "masked_tiles_last" (tiles of the last call whose mask allowed no document: exact, waits for the
 *   device, 0 after an unmasked call), "skipped_tiles_last" (of the tiles that passed the mask, those in which no token of the query
 *   had a posting: they leave before any work; waits for the device); "profile" (measurement hook, default 0: 1 = every call records HIP events around its launches;
 *   read-only "tile_ms_last" / "final_ms_last" then give the last call's time in the tile and in the final kernels, summed over its
 *   rounds; they wait for the device, -1 when the last call recorded none).  rq_sparse_get_option returns -1 with a message for
 *   an unknown name.
 * rq_sparse_score_rows_device: the BM25 score of named (query, row) pairs, the device form of BM25Index.score_rows_batch (what hybrid
 *   fusion needs for a passage that only the dense retriever returned).  d_rows [B][m] int32, d_scores [B][m] float64,
 *   position for position: the float64 sum of the contributions of the query's tokens whose posting list holds the row, with
 *   repetition, added IN QUERY ORDER starting from 0.0 -- the bits of the corresponding entry of a full score vector.  A row outside
 *   [0, n_docs), -1 included, scores 0.0 and reads nothing; rows may repeat.  Token ids and offsets get the clamping rules of
 *   rq_sparse_topk_device.  One thread per pair, a binary search per token over that token's strictly ascending rows: no atomics, no
 *   workspace, no synchronisation; complete in stream order.  RQ_EINVAL unless 1 <= B <= 65535, 1 <= m <= RQ_MAX_SCORE_ROWS and
 *   non-null pointers.  rq_sparse_score_rows: blocking, host buffers, staged on the handle's stream like rq_sparse_topk, with its
 *   checks of the queries.  Read-only option "score_calls" (both entry points).
 * rq_sparse_set_groups / rq_sparse_topk_grouped / rq_sparse_topk_grouped_device: one document per GROUP, the batch
 *   form of BM25Index.search(..., distinct_by=): behind the `distinct_by` keyword of the batch calls.
 *   Table: rq_sparse_set_groups copies one int32 per document to the device (4 B per document of HBM).  -1 = a group of its own;
 *     any other non-negative int32 is a group id, ids need not be dense or small.  RQ_EINVAL for a negative value other than -1 and
 *     for an n_docs that is not the handle's.  A second call replaces the table (it waits for the device once).  Read-only option
 *     "grouped": 1 when a table is set.
 *   Definition (BM25Index._search_distinct): scores are added exactly as above, a document outside the query's allowed set scores
 *     0.0, the documents with score > 0 are ordered by score descending and equal scores by DESCENDING row, that order is walked
 *     keeping the first document of every group -- a -1 document is never collapsed -- and the first k kept documents are returned:
 *     out_rows / out_scores as above, out_count [B] the number of results, which may be below k although more than k documents
 *     score > 0.  Every row, score bit and count is the host definition's.
 *   Arguments: those of the masked calls and out_count; mask_of == NULL with n_masks == 0 = every query unrestricted.  RQ_EINVAL
 *     without a group table and for a null out_count; limits, clamping rules (tokens, offsets, a mask_of entry outside
 *     [-1, n_masks)), workspace rule and stream rule are those of rq_sparse_topk_masked*.
 *   Tile kernel: the kernel above instantiated with an in-tile collapse after the accumulation and the mask zeroing and before the
 *     positives are counted: of every group only the tile's best document -- the larger (score bits, row) -- keeps its score, the
 *     others are set to 0.0 (an LDS open-addressing table keyed by group id, 2 x tile slots of 8 B; a slot is claimed by atomicCAS and
 *     raised to the best document by a CAS loop that compares keys: a maximum, whatever the order of arrival).  This is exact: a
 *     query's winner is the best document of its group everywhere, so it survives its own tile's collapse, and if k other
 *     group-bests of that tile ranked above it, k distinct groups would beat it globally -- a tile's min(k, tile) best group-bests
 *     hold every winner of that tile.  A grouped call runs in tiles of min("tile_docs", 4096): accumulators + table = 96 KiB of
 *     LDS at the most; results never depend on it.
 *   Final kernel: a kernel of its own.  The tiles' candidates hold a group at most once per tile; they are walked in ranked chunks
 *     of at most RQ_SPARSE_MAX_K (the selection body with a key bound strictly below the previous chunk's threshold, then the
 *     bitonic sort), a candidate is emitted when its group is -1 or has not been walked before (an LDS set of group ids with the
 *     order index of each group's first candidate, lowered by atomicMin), until k are emitted or the candidates run out.
 *   The ungrouped calls keep their code, counters and launch count.  Read-only options: "grouped_calls" (counted in "calls" too, and
 *     in "masked_calls" when mask_of is given), "final_chunks_last" (the largest number of chunks one query's walk took in the last
 *     grouped call; waits for the device; 0 after any other call).
 *   The per-query BM25Index.search with distinct_by (it stays on the host) remains the definition these calls are tested against.
 * Not extended: per_group > 1, a host-core rq_bm25_topk_grouped (the host route is the loop of BM25Index._search_distinct),
 *   multi-device handles. */
typedef struct rq_sparse rq_sparse;
#define RQ_SPARSE_MAX_K 1024
rq_sparse* rq_sparse_create(int device_id, const int64_t* indptr, const int32_t* rows, const double* contrib, int64_t n_tokens, int64_t n_docs);
void rq_sparse_destroy(rq_sparse* h);
int64_t rq_sparse_postings(const rq_sparse* h);
int rq_sparse_topk(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, int32_t* out_rows, double* out_scores);
int rq_sparse_topk_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                          int32_t* d_rows, double* d_scores, void* stream);
int rq_sparse_topk_masked(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, const uint32_t* masks, int n_masks,
                          const int32_t* mask_of, int32_t* out_rows, double* out_scores);
int rq_sparse_topk_masked_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                                 const uint32_t* d_masks, int n_masks, const int32_t* d_mask_of, int32_t* d_rows, double* d_scores, void* stream);
int rq_sparse_set_groups(rq_sparse* h, const int32_t* groups, int64_t n_docs);
int rq_sparse_topk_grouped(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, const uint32_t* masks, int n_masks,
                           const int32_t* mask_of, int32_t* out_rows, double* out_scores, int32_t* out_count);
int rq_sparse_topk_grouped_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                                  const uint32_t* d_masks, int n_masks, const int32_t* d_mask_of, int32_t* d_rows, double* d_scores, int32_t* d_count,
                                  void* stream);
int rq_sparse_score_rows_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, const int32_t* d_rows,
                                int m, double* d_scores, void* stream);
int rq_sparse_score_rows(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, const int32_t* rows, int m, double* out_scores);
int rq_sparse_set_option(rq_sparse* h, const char* name, double value);
double rq_sparse_get_option(const rq_sparse* h, const char* name);

/* ---- hybrid fusion: both pools of a batch fused on the device (the fusion of reference rag_uq/streaming_index.py:485-523 as
 * HybridRetriever._fuse_batch_rows computes it for a whole batch, with its `complete_scores` rule) -----------------
 * An rq_hybrid is an object of its own, beside rq_index and rq_sparse: the KEY SPACE that joins a sparse and a dense index.
 *   keys 0 .. nb-1 are the sparse rows; dense row j has key dense_key[j]: a sparse row when BM25 holds the same document, else a
 *     value >= nb.  Every key lies in [0, n_keys), nb <= n_keys < 2^31, and dense_key is INJECTIVE: rq_hybrid_create checks both on
 *     the host and refuses otherwise.  known[key] (one byte per key, non-zero = the document store knows the key).  dense_row[key],
 *     the inverse map (-1: no dense row), is derived by the library.  The three tables are COPIED to the device: 4 B per dense row +
 *     5 B per key.
 * Per query the inputs are a sparse pool [K1] (int32 rows, float64 scores, -1 padded: the output layout of rq_sparse_topk_device) and
 *   a dense pool [K2] (int64 rows, fp32 scores, -1 padded: the output layout of rq_search_device, for an index with row offset 0).
 *   0 <= K1 <= RQ_SPARSE_MAX_K, 0 <= K2 <= RQ_MAX_K, K1 + K2 >= 1 (a pool of width 0 needs no arrays).  A dense row outside
 *   [0, n_dense) or a sparse row outside [0, nb) is absent.  Rows within one pool are distinct; this is not checked, as for
 *   rq_mmr_select_device: a repeated row leaves that query's result unspecified, but it causes no read or write outside the arrays.
 * Definition.  Candidates are the positions 0 .. K1+K2-1, sparse pool first; each has a key, b and d, both float64: the fp32 dense
 *   score is widened, the missing side is 0.0.
 *   valid = present and known[key].
 *   a key in both pools: the sparse position takes the dense position's d, and the dense position becomes invalid.
 *   missing rows (the `complete_scores` rule): for a valid sparse position without a dense score, miss_dense = dense_row[key] (it may
 *     be -1); for a valid dense-only position with key < nb, miss_sparse = key; everything else is -1.  Where a miss entry is >= 0
 *     and an extra score is supplied, the extra replaces the 0.0.
 *   max_b and max_d are taken over the valid candidates; a NaN among them makes the maximum NaN.  The maximum is then replaced by 1.0
 *     when it is 0, NaN or infinite (and when no candidate is valid).
 *   h = (b / max_b + d / max_d) / 2 in float64: two divisions, one addition and one division by 2, each rounded, no fused
 *     multiply-add.
 *   order: h descending with -0.0 as +0.0; equal h by ascending candidate position.  A NaN h ranks as -inf, as every score in this
 *     header, and is returned as it is.
 *   output [B][top_k]: key (int32), b, d, h (float64), optionally the candidate position (int32: < K1 = the sparse pool);
 *     count[B] = min(valid candidates, top_k); entries beyond count are (-1, 0.0, 0.0, 0.0), position -1.  1 <= top_k <= RQ_MAX_K.
 *   Every key, position, count and score has the bits of tests/hybrid_oracle.py, which is the host path's arithmetic.
 * rq_hybrid_missing_device: d_miss_dense [B][K1] int64 (feeds rq_score_rows_device, where -1 is "absent, 0.0"), d_miss_sparse
 *   [B][K2] int32 (feeds rq_sparse_score_rows_device); either may be NULL when its K is 0.
 * rq_hybrid_fuse_device: d_miss_dense / d_extra_dense [B][K1] fp32 / d_miss_sparse / d_extra_sparse [B][K2] float64 may all be NULL
 *   (missing scores stay 0.0); an extra array without its miss array is RQ_EINVAL.  d_pos may be NULL.  One workgroup per query,
 *   everything in LDS (at most 2 048 candidates, under 64 KiB), the kernel instantiated for the candidate count padded to a power of
 *   two (64 .. 2 048).  Both device forms: no workspace, no synchronisation, complete in stream order.
 * rq_hybrid_missing / rq_hybrid_fuse: blocking, host buffers, staged on a stream the handle owns.
 * RQ_EINVAL for sizes outside the limits above, B outside 1 .. 65535 and null pointers; RQ_ENODEVICE as everywhere;
 *   rq_hybrid_create: NULL with the message in rq_last_error(), NULL + the "no HIP device" message without a gfx950 device.  A handle
 *   is used from one thread.  Read-only options (rq_hybrid_get_option, -1 with a message for an unknown name): "calls", "fuse_calls",
 *   "missing_calls" (both entry points each), "nb", "n_dense", "n_keys".
 *   Filtered pools (rq_sparse_topk_masked_device, rq_search_filtered_each_device) fuse as they are: the fusion needs no filter of its own.
 * rq_hybrid_set_groups / rq_hybrid_fuse_grouped_device / rq_hybrid_fuse_grouped: the fusion with one candidate per GROUP (DESIGN.md
 *   4.23), HybridRetriever._fuse(..., distinct_by=) for a batch.  rq_hybrid_set_groups copies key_group [n_keys] int32 to the device
 *   (4 B per key; the conventions of rq_sparse_set_groups: -1 = a group of its own, any other value >= 0, RQ_EINVAL otherwise and for
 *   an n_keys that is not the handle's; a second call replaces the table).  The fuse calls take the pool arguments of rq_hybrid_fuse*
 *   without the miss and extra arrays and give its outputs in its layout, so rq_router_rerank_device consumes them as they are.
 *   Definition: validity, the merge of a key held by both pools, max_b, max_d and h are those above, taken over ALL valid
 *   candidates -- the maxima before the collapse; the full ranking of the K1 + K2 candidates is computed (h descending, equal h by
 *   ascending position, NaN as -inf), the first candidate of every group is kept, a -1 candidate always, and the first top_k kept
 *   candidates are returned: count = min(kept, top_k).  One workgroup per query, the same instantiations; after the ranking the
 *   (group, rank) pairs are sorted in the spent sort array, a pair whose predecessor has another group is its group's first rank, and
 *   a prefix sum over the ranks' keep flags gives the output positions: no LDS beyond rq_hybrid_fuse_device's.  RQ_EINVAL without
 *   a group table.  Read-only options "grouped" and "grouped_calls" (counted in "calls" and "fuse_calls" too).
 *   The per-query HybridRetriever.hybrid_search with distinct_by (it stays on the host) remains the definition they are tested against.
 * Not extended: MMR over the fused pool, grouping with the `complete_scores` rule, per_group > 1, multi-device handles. */
typedef struct rq_hybrid rq_hybrid;
#define RQ_HYBRID_MAX_CAND 2048
rq_hybrid* rq_hybrid_create(int device_id, int64_t nb, int64_t n_dense, const int64_t* dense_key, const uint8_t* known, int64_t n_keys);
void rq_hybrid_destroy(rq_hybrid* h);
double rq_hybrid_get_option(const rq_hybrid* h, const char* name);
int rq_hybrid_missing_device(rq_hybrid* h, const int32_t* d_sp_rows, const int64_t* d_de_rows, int B, int K1, int K2, int64_t* d_miss_dense,
                             int32_t* d_miss_sparse, void* stream);
int rq_hybrid_missing(rq_hybrid* h, const int32_t* sp_rows, const int64_t* de_rows, int B, int K1, int K2, int64_t* miss_dense, int32_t* miss_sparse);
int rq_hybrid_fuse_device(rq_hybrid* h, const int32_t* d_sp_rows, const double* d_sp_scores, const int64_t* d_de_rows, const float* d_de_scores, int B,
                          int K1, int K2, const int64_t* d_miss_dense, const float* d_extra_dense, const int32_t* d_miss_sparse,
                          const double* d_extra_sparse, int top_k, int32_t* d_keys, double* d_b, double* d_d, double* d_h, int32_t* d_pos,
                          int32_t* d_count, void* stream);
int rq_hybrid_fuse(rq_hybrid* h, const int32_t* sp_rows, const double* sp_scores, const int64_t* de_rows, const float* de_scores, int B, int K1, int K2,
                   const int64_t* miss_dense, const float* extra_dense, const int32_t* miss_sparse, const double* extra_sparse, int top_k,
                   int32_t* out_keys, double* out_b, double* out_d, double* out_h, int32_t* out_pos, int32_t* out_count);
int rq_hybrid_set_groups(rq_hybrid* h, const int32_t* key_group, int64_t n_keys);
int rq_hybrid_fuse_grouped_device(rq_hybrid* h, const int32_t* d_sp_rows, const double* d_sp_scores, const int64_t* d_de_rows, const float* d_de_scores,
                                  int B, int K1, int K2, int top_k, int32_t* d_keys, double* d_b, double* d_d, double* d_h, int32_t* d_pos, int32_t* d_count,
                                  void* stream);
int rq_hybrid_fuse_grouped(rq_hybrid* h, const int32_t* sp_rows, const double* sp_scores, const int64_t* de_rows, const float* de_scores, int B, int K1,
                           int K2, int top_k, int32_t* out_keys, double* out_b, double* out_d, double* out_h, int32_t* out_pos, int32_t* out_count);

/* ---- router gate: the learned gate and the rerank of the fused pool on the device (reference rag_uq/router.py:74-177 as the
 * evaluation loop applies it, experiments/run_evaluation.py:165-184) ------------------------------------------------
 * An rq_router holds the weights of a RetrievalRouter with num_layers 1 or 2, COPIED to one device and read-only after creation.
 *   num_layers 2: W0 [H][3], b0 [H], w1 [H], b1 (Linear(3, H) -> ReLU -> Linear(H, 1) -> Sigmoid), 1 <= H <= RQ_ROUTER_MAX_HIDDEN;
 *   num_layers 1: w1 [3], b1: a logistic unit on the three features (hidden, w0 and b0 are ignored).
 *   Weights are given as fp32, as they are in a state dict, and widened exactly.  use_batch_norm != 0 and num_layers > 2 are
 *   refused with the reason in rq_last_error(): the reference never builds them.
 * Input per query: columns key [P] (int32), b [P], d [P] (float64) and count -- the output layout of rq_hybrid_fuse_device,
 *   1 <= P <= RQ_MAX_K.  ALL P slots, padding included, take part in the normalisation and get a weight (the reference pads the
 *   columns to num_passages with 0.0 before the router sees them).
 * Definition.  All arithmetic is float64, every operation rounded on its own, no fused multiply-add.
 *   normalisation, mode RQ_ROUTER_NORM_STATS: stats = (bm25_mean, bm25_std, dense_mean, dense_std), four doubles in HOST memory
 *     read at call time: nb = (b - bm25_mean) / (bm25_std + 1e-6), nd likewise.
 *   mode RQ_ROUTER_NORM_QUERY (stats may be NULL): per query and per column x, mean = S(x) / P,
 *     var = S((x - mean) * (x - mean)) / (P - 1), scale = sqrt(var) + 1e-6, nx = (x - mean) / scale.  P = 1 gives 0/0 = NaN.
 *     S is a fixed pairwise tree: the column is padded with +0.0 to the next power of two n, then a[i] = a[i] + a[i + n/2] for
 *     i < n/2, n halved each time; the sum does not depend on the thread count.
 *     The reference's batch-wise form over the whole [B][P] tensor is deliberately not offered: a question's answer would depend
 *     on its neighbours in the batch.
 *   gate: df = nd - nb; z = 0.0; for j = 0 .. H-1 in order: a_j = ((W0[j][0]*nb + W0[j][1]*nd) + W0[j][2]*df) + b0[j],
 *     r_j = a_j > 0 ? a_j : 0, z = z + w1[j]*r_j; then z = z + b1 and w = 1.0 / (1.0 + exp(-z)).
 *     num_layers 1: z = ((w1[0]*nb + w1[1]*nd) + w1[2]*df) + b1.
 *   rerank: h = w*d + (1.0 - w)*b: a product, a subtraction, a product and an addition.  Candidates are the positions i < count
 *     with key[i] >= 0 (a count outside 0 .. P is clamped).  order: h descending with -0.0 as +0.0; a NaN h ranks as -inf, as every
 *     score in this header, and is returned as it is; equal h by ascending position.
 *   output [B][top_r], 1 <= top_r <= P: key (int32), b, d, w, h (float64), pos (int32: the position in the input);
 *     count_out[B] = min(candidates, top_r); entries beyond it are (-1, 0.0, 0.0, 0.0, 0.0, -1).
 *   Everything but exp has the bits of tests/router_gate_oracle.py; w is within 2^-49 relative of it (3 ulp of the device
 *     library's exp), and exactly 0, 1 or NaN where the definition gives that.
 * rq_router_gate_device: d_w [B][P] in input order (RetrievalRouter.forward).  rq_router_rerank_device: as above; its w is the
 *   bits of rq_router_gate_device's w at that position (one device function serves both).  One workgroup per query, everything in
 *   LDS (about 47 KiB at P = 1 024, under 64 KiB), the kernel instantiated for P padded to a power of two (64 .. 1 024).  Both
 *   device forms: no workspace, no synchronisation, complete in stream order.
 * rq_router_gate / rq_router_rerank: blocking, host buffers, staged on a stream the handle owns.
 * RQ_EINVAL for sizes outside the limits above, B outside 1 .. 65535, null pointers or an unknown mode; RQ_ENODEVICE as
 *   everywhere; rq_router_create: NULL with the message in rq_last_error(), NULL + the "no HIP device" message without a gfx950
 *   device.  A handle is used from one thread.  Read-only options (rq_router_get_option, -1 with a message for an unknown name):
 *   "calls", "gate_calls", "rerank_calls" (both entry points each), "hidden", "layers".
 * Not extended: router training, batch norm and deeper nets, multi-device handles, MMR or grouping over the routed pool. */
typedef struct rq_router rq_router;
#define RQ_ROUTER_MAX_HIDDEN 256
#define RQ_ROUTER_NORM_STATS 0
#define RQ_ROUTER_NORM_QUERY 1
rq_router* rq_router_create(int device_id, int num_layers, int hidden, int use_batch_norm, const float* w0, const float* b0, const float* w1, float b1);
void rq_router_destroy(rq_router* r);
double rq_router_get_option(const rq_router* r, const char* name);
int rq_router_gate_device(rq_router* r, const double* d_b, const double* d_d, int B, int P, int mode, const double* stats, double* d_w, void* stream);
int rq_router_gate(rq_router* r, const double* b, const double* d, int B, int P, int mode, const double* stats, double* out_w);
int rq_router_rerank_device(rq_router* r, const int32_t* d_keys, const double* d_b, const double* d_d, const int32_t* d_count, int B, int P, int mode,
                            const double* stats, int top_r, int32_t* d_out_keys, double* d_out_b, double* d_out_d, double* d_out_w, double* d_out_h,
                            int32_t* d_out_pos, int32_t* d_out_count, void* stream);
int rq_router_rerank(rq_router* r, const int32_t* keys, const double* b, const double* d, const int32_t* count, int B, int P, int mode, const double* stats,
                     int top_r, int32_t* out_keys, double* out_b, double* out_d, double* out_w, double* out_h, int32_t* out_pos, int32_t* out_count);

/* Tuning / test hooks: "kstage" (1: an LDS stage holds whole rows, 2: half rows), "ring" (LDS stages 2..6; the
 * (kstage, ring, prefetch) triples built are listed in csrc/rq_scan.hip, others fail with RQ_EHIP at search time),
 * "wg_per_cu", "nt" (non-temporal corpus loads: 0, 1, -1 = auto), "slack_bins" (extra bins beyond k, -1 = auto),
 * "eps" (certificate bound, <0 = derived default), "profile" (HIP events on every scan launch, attached to the dispatch; "profile_stride" n: on every n-th; "profile_legacy" 1: hipEventRecord around it),
 * "prefetch" (LDS fragments read ahead of their MFMAs: 1, 4, 6, 12), "fast_tail" (0 = generic sorted tail),
 * "pipeline" (see rq_search_flush_device), "wide_batch" (calls of more than 64 queries: 0 = passes of 64 only, 1 = passes of
 * 256 / 128 / 64, 3 = 128 / 64, 2 = round 1's 8-wave 128-query pass), "wide128" / "wide256" (variant of csrc/rq_scan_wide.hip),
 * "epi" (selection form of the 64-query scan: 1 = row positions inside the scores, 0 = compare / select),
 * "use_hint" (0: rq_search_hint_next_device is ignored), "scan_ahead" (1 = default: an announced batch is scanned together with
 *   the call before it on shards beyond 208 MiB of fp16 rows, see rq_search_hint_next_device; 0 = never), "scan_bundle" (4 =
 *   default: in a steady announced loop four calls share one 256-query pass; 2 = pairs only; read-only "bundles4" counts those passes),
 * "scan8" (searches may scan an int8 image of the shard instead of its fp16 rows -- half the bytes per pass;
 *   candidates are still re-scored from the fp16 rows in fp64, so results do not change: 0 = never, 1 = for k <= 128 on shards of
 *   200 000 rows and more (default), 2 = always.  The image (+768 B per row) is built by the first search that wants it (no room for it: the fp16 rows stay the operand); a shard whose
 *   worst row quantises with more than 3 % relative error keeps the fp16 scan),
 * "scan8_split" (-1 = default: the queries reach the int8 scan as one int8 image for k <= 32 and as two -- value and residual,
 *   twice the matrix-core work, a third of the candidate rows -- for larger k; 0 / 1: one / two images for every k),
 * "wide8" (default 1: calls of more than 64 queries whose k class runs with one int8 image use 128-query passes over the image;
 *   0: the fp16 passes of "wide_batch"),
 * "thr_mult8" (1.05 .. 2.25, default 1.25: candidate threshold of the int8 scan, T = P - bound - (thr_mult8 - 1) * max(bound,
 *   typical one-image bound); 2.25 certifies by construction, smaller values re-score fewer rows and leave the rare query
 *   whose errors add up to the repair path of rq_search_fixup_device.  When more than 1 in 16 checked queries of a class of
 *   k (<= 32 / larger) needed repair, that class moves one step along one image -> two images -> fp16 scan, until "scan8" or
 *   "scan8_split" is set again),
 * "wide256_8" (default 31: calls of more than 128 queries on the one-image class use 256-query passes over the image, a variant of
 *   csrc/rq_scan_wide.hip; 0 = passes of 128 as in round 2), "bin_bound" (A/B hook, default 1: the tail tests every bin with its own rows'
 *   worst quantisation error instead of the shard's), "stripe_rows" (multi-device index, before the first append: rows per stripe),
 * "tail_local" (A/B hook, default 1: a tail workgroup with more than k re-scored rows publishes only its own k best keys),
 * "poison_cand" (test hook: candidate lists are filled with 0xff..ff keys before every tail),
 * "poison_bins" (test hook: before a search's scan, the bin records of every query slot its passes cover are filled with 0xff bytes).
 * "row_pad" (elements per stored row: 384 or 768.  Always readable.  Default: 384 for dim <= 384, else 768 -- also for an index
 *   that rq_load creates, whatever layout the saved index had: the files are the same.  Settable to 384 or 768 only while the
 *   index holds no rows (a reservation made before is made again with the new row length); RQ_EINVAL for any other value, for
 *   384 when dim > 384, and once rows are stored.  On a multi-device index it is passed to every device's shard.
 *   768 on an index of dim <= 384 keeps the wide layout and every kernel and option of it: the A/B hook.
 *   An index with "row_pad" = 384 (the NARROW layout, csrc/rq_scan_narrow.hip) stores and streams 768 B per row and has ONE built
 *   scan form per pass size: "ring" / "kstage" / "prefetch" / "epi" are accepted and ignored.  Deliberately not built for it: the
 *   int8 image ("scan8" is treated as 0: "scan8_used" stays 0, "scan8_row_err" stays -1 -- an image of a 768-byte row would save
 *   nothing); the 256-query pass (calls of more than 64 queries are cut into passes of 128, then 64; "wide_batch" 0 = 64 only;
 *   "wide128" / "wide256" / "wide8" / "wide256_8" do not apply); the "scan_ahead" pairing (an announced batch still gets its
 *   queries prepared by the fused launch).  The certificate's "eps" stays the bound derived for 768 elements, which holds for
 *   shorter rows too.)
 * "scan8" = 1 measures where the ladder STARTS when the image is built (64 stored rows searched as queries through every rung, the
 *   fastest rung that certifies wins; "scan8_calibrated_rows", "scan8_calib_ms_<class><rung>", "scan8_calib_unc_<class><rung>" report it).
 * Read-only: "repaired_queries" (queries that came back uncertified and were repaired, all rungs of the ladder), "scan8_used" (searches that scanned the int8 image), "scan8_row_err" (worst row's relative int8 error, -1 = image
 * not built), "scan8_level" (ladder position: class k <= 32 + 10 * class of larger k; 0 one image, 1 two images, 2 fp16 scan),
 * "scan8_wide_one_image" (same encoding: 1 = calls of more than 64 queries of that class scan ONE int8 image per query -- also in a class whose 64-query calls
 *   run on two images, when the image-build measurement found one image eligible; given up for the wide calls alone after too many repairs),
 * "scan8_suspended" (bit 0 / 1: that class is back at the fp16 scan), "hints_used" (searches whose announced queries a launch before them prepared or scanned, see rq_search_hint_next_device), "max_row_norm", "max_sub_rel" / "max_sub_abs" (largest share of a stored row that sits in fp16-subnormal elements,
 * which the matrix cores flush), "eps_cosine" / "eps_ip" (the certificate's bound including that term). */
int rq_set_option(rq_index* idx, const char* name, double value);
double rq_get_option(const rq_index* idx, const char* name);

typedef struct rq_timing {
    double scan_ms;          /* sum of HIP-event durations of the scan kernel launches recorded */
    int64_t scan_launches;   /* launches recorded (profile on) */
    int64_t scan_bytes;      /* algorithmic corpus bytes of those launches: rows * 2 * "row_pad" each over the fp16 rows (rows * 768 over the int8 image) */
    int64_t searches;        /* rq_search* calls */
    int64_t queries;         /* queries searched */
    int64_t widened;         /* queries re-run with a wider candidate set */
    int64_t exact_scans;     /* queries that needed the full fp64 scan */
} rq_timing;
int rq_get_timing(rq_index* idx, rq_timing* out);   /* synchronises the device */
int rq_reset_timing(rq_index* idx);

/* Flat-file persistence: <path>.meta (text), <path>.f16 (rows [N][dim] fp16). */
int rq_save(const rq_index* idx, const char* path);
rq_index* rq_load(const char* path, int n_devices, const int* device_ids);

/* Test hook: copy the scan's approximate per-bin maxima of query `query` of the LAST search enqueued on `stream`
 * (bin b = rows 64 b .. 64 b + 63) to the host.  Returns the number of bins copied. */
int64_t rq_debug_pooled(rq_index* idx, void* stream, int query, float* out, int64_t max_bins);
/* Test hook: the raw 8-byte bin records (x, y: csrc/rq_device.h) of query slots q0 .. q0 + nq - 1 of the LAST search enqueued on
 * `stream`, as out[nq][bins][2] uint32 words; synchronises the device.  A search's slots are its queries followed by the pad slots of its
 * passes (a scanned-ahead pair: the call's own 64-slot half).  RQ_EINVAL on a multi-device index, when that search ran no approximate
 * scan (exact route, empty shard) or when q0 + nq exceeds the slots its passes covered.  Returns the number of bins per slot copied. */
int64_t rq_debug_bin_records(rq_index* idx, void* stream, int q0, int nq, uint32_t* out, int64_t max_bins);
/* Test hook: the int8 image's worst relative row error of every bin (fp32, rounded up), i.e. what the tail may lift its candidate
 * threshold by per bin (option "bin_bound").  Fails unless the image is built and up to date.  Returns the number of bins copied. */
int64_t rq_debug_bin_err(rq_index* idx, float* out, int64_t max_bins);

/* Measurement hook: GB/s of a plain streaming read (16-byte loads, nothing else) of the stored shard, averaged over
 * `iters` back-to-back passes -- what THIS GPU delivers right now, the yardstick for the scan kernel's rate.
 * nt: non-temporal loads 0 / 1 / -1 = the scan's own rule.  Negative on error. */
double rq_debug_read_bandwidth(rq_index* idx, int iters, int nt, int wg_per_cu);

/* Development hook: enable != 0 makes every workgroup of the fused scan + tail launches (option "pipeline" = 2) record
 * {start, end} wall-clock ticks (100 MHz), HW_ID and XCC_ID; out (may be NULL) receives [max_wgs][4] words of the last
 * such launch.  enable == 0 switches it off again.  Used by tools/gpu_stamps.py. */
int rq_debug_stamps(rq_index* idx, int enable, unsigned long long* out, int max_wgs);

const char* rq_last_error(void);
const char* rq_version(void);

/* ---- encoder pieces (the embedding the reference asks Ollama for, rag_uq/streaming_index.py:267-288) ----
 * The memory-bound parts of the NomicBert (nomic-embed-text) forward pass as fused gfx950 kernels; the GEMMs between them stay
 * with the framework's library (hipBLASLt).  All pointers are device pointers, fp16 unless noted; `stream` is a hipStream_t.
 * Used by embedders.NomicBertEmbedder (efficient-rag-..._amd/embedders.py), csrc/rq_encoder.hip. */
/* d_rope[pos][0..31] = cos(pos * rope_theta^(-d / 32)), d_rope[pos][32..63] = the sines (fp32 [seq][64]): the rotary table. */
int rq_nb_rope_table_f32(float* d_rope, int seq, float rope_theta, void* stream);
/* ctx[b][t][:] = softmax(rot(q) rot(k)^T / 8 + prefix mask) v per head.  d_qkv [batch * seq][3 * heads * 64] (q | k | v of the
 * fused projection), d_len[batch] = valid tokens of each sequence (the first d_len[b] positions; padded rows come out zero),
 * rotary = rotate-half over the 64 dims with d_rope (at least seq rows).  1 <= seq <= 512 (RQ_EUNSUPPORTED beyond: use the
 * framework's attention; RQ_EINVAL below).  The lengths live in device memory, so no host check sees them: d_len[b] > seq counts as seq, and a
 * negative d_len[b] is an empty sequence -- its seq rows of ctx come out zero and nothing else is written. */
int rq_nb_attention_f16(const void* d_qkv, const int* d_len, const float* d_rope, void* d_ctx, int batch, int seq, int heads, void* stream);
/* The same for a PACKED batch -- no padding rows: the tokens of sequence b are rows [d_offsets[b], d_offsets[b + 1]) of d_qkv and d_ctx
 * (d_offsets: batch + 1 ascending ints, d_offsets[0] = 0), every sequence at most max_seq <= 512 tokens long.  The GEMMs around the
 * attention then run on sum(lengths) rows instead of batch * longest. */
int rq_nb_attention_packed_f16(const void* d_qkv, const int* d_offsets, const float* d_rope, void* d_ctx, int batch, int max_seq, int heads, void* stream);
/* out = LayerNorm(x + res) * gamma + beta over rows of `width` (8..1536, multiple of 8) elements, fp32 statistics; res may be
 * NULL; out may alias x or res. */
int rq_nb_add_layernorm_f16(const void* d_x, const void* d_res, const void* d_gamma, const void* d_beta, void* d_out, int64_t rows, int width,
                            float eps, void* stream);
/* out[t][j] = silu(gate_up[t][j]) * gate_up[t][inter + j]: d_gate_up [rows][2 * inter] (gate | up), d_out [rows][inter]. */
int rq_nb_swiglu_f16(const void* d_gate_up, void* d_out, int64_t rows, int inter, void* stream);
/* d_out[b][:] (fp32) = mean of d_h[b][t][:] over the first d_len[b] tokens (0 for an empty sequence).  d_len[b] > seq counts
 * as seq, and a negative d_len[b] is an empty sequence: its row of d_out is 0. */
int rq_nb_mean_pool_f16(const void* d_h, const int* d_len, float* d_out, int batch, int seq, int width, void* stream);
/* ... of a packed batch: d_out[b][:] = mean of the rows [d_offsets[b], d_offsets[b + 1]) of d_h. */
int rq_nb_mean_pool_packed_f16(const void* d_h, const int* d_offsets, float* d_out, int batch, int max_seq, int width, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RQ_H */
