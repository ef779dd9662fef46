// rq_kernels.h -- host-visible launchers of the HIP kernels (internal; the public C ABI is include/rq.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RqScanArgs {
    const void* x;            // fp16 corpus shard [rows_padded][768] (rq_scan_narrow_launch: [rows_padded][384]), rows_padded % 64 == 0, pad rows zero
    const float* row_scale;   // [rows_padded] 2^-12 / ||row|| (cosine) or 2^-12 (inner product); pad entries NaN
    const _Float16* qh;       // [QB][768] fp16(q / ||q|| * 2^12) of this block (QB = 64, 128 or 256), unused slots zero
    uint2* bins;              // [QB][bins_stride] per (query, quad) record, see rq_device.h
    int64_t bins_stride;      // records per query row, >= nquads
    int64_t n_rows;           // valid rows of the shard
    int nquads;               // ceil(n_rows / 64)
    int nq_valid;             // queries of this block that are real (<= QB)
    float* wgmax;             // [QB][wgmax_stride] largest approximate score per (query, scan workgroup)
    int wgmax_stride;         // >= grid
    // int8 scan (i8 = 1): x = the int8 image of the shard [rows_padded][768], row_scale = s_row / ||row|| (pad entries NaN),
    // qh = int8 queries [QB][768], qscale[QB] = s_query / ||query||; approximate score = int32 sum * row_scale * qscale
    // i8 = 2: the queries come as TWO int8 images (q = s (254 q_hi + q_lo), rq_prep_body): qh = q_hi, qlo = q_lo, approximate
    // score = (254 * sum_hi + sum_lo) * row_scale * qscale / 254 -- the query's quantisation error all but disappears from the bound
    int i8;
    const float* qscale;
    const void* qlo;
    // fp16 128-query passes of rq_scan_wide.hip only: queries 64..127 of the block come from here instead of qh + 64 rows
    // (the two ring slots of a scanned-ahead pair, which need not be neighbours in memory: rq_search.hip "scan_ahead"); null = qh
    // holds the whole block, as it does for the 256-query pass of a bundle (an aligned quarter of the ring, rq_bundle_plan.h)
    const _Float16* qh_hi;
};
#define RQ_WGMAX_STRIDE 1024   // scan grids never exceed this many workgroups

// e0 / e1 (all scan launchers): optional events attached to the dispatch itself (hipExtLaunchKernel): the kernel's own start / end
// time stamps, no extra barrier packets on the stream
hipError_t rq_scan_launch(const RqScanArgs& a, int S, int pf, int ks, int qw, bool nt, int grid, int epi, hipStream_t stream,
                          hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Passes of 128 / 256 queries (rq_scan_wide.hip): one 512-thread workgroup per CU, LDS reads running ahead of the MFMAs
// across stage boundaries, v_med3 selection.  Returns hipErrorInvalidValue for a variant that is not built or does not
// score `queries` queries per pass.
hipError_t rq_scan_wide_launch(const RqScanArgs& a, int variant, int queries, bool nt, int grid, hipStream_t stream,
                               hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Rows of 384 elements (rq_scan_narrow.hip; rq_index.h dpad = 384): a.x = fp16 rows of 768 bytes, a.qh = prepared queries in their
// usual 768-element slots, a.i8 = 0.  queries = 64 (one 16-query group per wave) or 128 (two: records of 128 queries parked in LDS,
// two workgroups per CU); 256-thread workgroups, ring of 3 x 12 KiB stages, prefetch 1, med3 selection.  One built form each.
hipError_t rq_scan_narrow_launch(const RqScanArgs& a, int queries, bool nt, int grid, hipStream_t stream,
                                 hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// dpad (here and below): stored row length in elements, 768 or 384 (rq_index.h); rows are dpad * 2 bytes apart.
// Row statistics at add time: row_norm64[i] = sqrt(sum x^2) in fp64; stats[3] (device, running maxima as double bits):
// largest norm, largest relative and absolute mass of fp16-subnormal elements in a row (see rq_select.hip).
hipError_t rq_rownorm_launch(const void* x, int dpad, int64_t row_begin, int64_t row_end, double* norm64, unsigned long long* stats, hipStream_t stream);

// fp32 rows (device) -> fp16 rows, optionally L2-normalised first (see include/rq.h rq_index_add_f32).
hipError_t rq_convert_f32_launch(const float* src, int dim, int64_t n, int normalize, void* dst_rows_f16, int dpad, hipStream_t stream);
hipError_t rq_pad_f16_launch(const void* src, int dim, int64_t n, void* dst_rows_f16, int dpad, hipStream_t stream);

// Query preparation: qnorm64[q] = ||q|| (fp64); qh = fp16(q / ||q|| * 2^12) padded to 768, slots >= B zero.
// One 256-thread workgroup per query slot (rq_device.h rq_prep_body); run by rq_prep_queries_kernel or, for the NEXT batch
// of a throughput loop, by extra workgroups of the fused scan + tail launch (include/rq.h rq_search_hint_next_device).
struct RqPrepArgs {
    const float* q; int dim; int B;      // raw fp32 queries [B][dim]
    _Float16* qh; float* q32pad; double* qnorm64;
    int nslots;                          // workgroups = query slots written (padded batch size), 0 = none
    // int8 image for the int8 scan (all three NULL = not wanted): q8[slot][768] = round(q / s), s = max|q_i| / 127;
    // qscale8[slot] = s / ||q|| (1 for a zero / unused / non-finite query); qeps8[slot] = ||q - s q8|| / ||q||, the
    // query's share of the certificate's error bound (+inf for a non-finite query)
    signed char* q8; float* qscale8; float* qeps8;
    // second int8 image of the residual: r = q - s q8, q8lo = round(r / (s / 254)); qeps8s[slot] = ||q - s (q8 + q8lo / 254)|| / ||q||
    signed char* q8lo; float* qeps8s;
};
hipError_t rq_prep_queries_launch(const RqPrepArgs& a, hipStream_t stream);   // a.nslots workgroups

// int8 image of rows [row_begin, row_end) for the int8 scan: x8[row][768] = round(x / s_row), s_row = max|x_i| / 127;
// scale_cos[row] = s_row / ||row|| (0 for a zero row), scale_ip[row] = s_row; stat[0] (device, double bits, running
// maximum) = largest ||x - s x8|| / ||x|| of a row (+inf for a row with non-finite elements)
// binerr[row / 64] (device, fp32 bits, running maximum, zero before the first call) = the same figure for the worst row of every bin
hipError_t rq_quant_rows_launch(const void* x, const double* norm64, int64_t row_begin, int64_t row_end, signed char* x8,
                                float* scale_cos, float* scale_ip, unsigned long long* stat, float* binerr, hipStream_t stream);

// Pass 2: per query, the m best bins of bins[q][0..nbins) as sorted keys (score desc, bin asc); 0-padded.
hipError_t rq_select_bins_launch(const uint2* bins, int64_t bins_stride, int64_t nbins, int B, int m,
                                 uint64_t* binkeys, hipStream_t stream);

// Pass 3: exact fp64 re-score of every row of the first nb bins of each query -> candidate keys (score, local row).
struct RqRescoreArgs {
    const void* x;
    int dpad;                  // stored row length of x in elements (768 or 384)
    const float* q32;          // [B][768] raw fp32 queries, zero padded
    const double* qnorm64;     // [B]
    const double* rownorm64;   // [rows_padded]
    const uint64_t* binkeys;   // [B][binkeys_stride]
    int binkeys_stride;
    int nb;                    // bins re-scored per query
    int metric;                // 0 cosine, 1 inner product
    int64_t n_rows;
    uint64_t* cand;            // [B][nb*64]
};
hipError_t rq_rescore_launch(const RqRescoreArgs& a, int B, hipStream_t stream);
// Exact mode only (a.binkeys == nullptr, every bin of the shard): the same keys from a dense fp64 contraction on the matrix cores
// (v_mfma_f64_16x16x4_f64, rq_exact.hip): a 16-row tile is read once for 64 queries instead of once per query.
hipError_t rq_exact_scan_launch(const RqRescoreArgs& a, int B, int cu_count, hipStream_t stream);

// One query of a launch whose queries each bring their own filter (rq_filter_each.hip, include/rq.h rq_search_filtered_each): where
// its candidate keys are and how many, its filter's arrays, which prepared query it is and where its outputs go.
struct RqEachDesc {
    const uint32_t* list;      // ragged gather: the filter's listed rows [na], ascending
    const uint32_t* first;     // the filter's first allowed rows (RqFilterArgs::first)
    const uint32_t* bits;      // per-query key mask: the filter's bitmap
    int64_t key_off;           // the query's candidate keys start at cand + key_off
    int64_t ncand;             // ... and are this many (<= INT32_MAX)
    int64_t na;                // allowed rows: the rows that can be returned
    int q;                     // slot among the prepared queries (q32, qnorm64)
    int out;                   // query of the call: row of the outputs
};

// Pass 4: top-k of the candidates, certificate, outputs.
struct RqFinalArgs {
    const uint64_t* cand;      // [B][ncand]
    int ncand;
    const uint64_t* binkeys;   // [B][binkeys_stride]; entry nb is the best bin that was NOT re-scored
    int binkeys_stride;
    int nb;
    int64_t nbins;             // bins of the shard
    const double* qnorm64;
    int metric;
    float eps;                 // bound on |approximate - exact| in unit-query units
    float max_row_norm;        // for the inner-product bound
    int k;
    int64_t row_offset;        // global id of the shard's row 0
    int64_t n_rows;            // rows that can be returned (a filtered call: the allowed rows)
    const uint32_t* first = nullptr;   // a filtered call: RqFilterArgs::first (the answer of a zero-norm query); null = rows 0, 1, ..
    float* out_scores;         // [B][k]
    int64_t* out_rows;         // [B][k], -1 padded
    uint64_t* out_keys;        // [B][k] optional (global-row keys for cross-shard merging), may be null
    int* out_status;           // [B] 0 = certified exact, 1 = not certified
    // Per-query bookkeeping (null = the uniform layout above).  With it workgroup b serves each[b]: keys cand + key_off, ncand of
    // them, n_rows = na, first = that filter's, qnorm64[q], outputs of query `out`; ncand, n_rows and first above are not read.
    const RqEachDesc* each = nullptr;
};
hipError_t rq_final_launch(const RqFinalArgs& a, int B, hipStream_t stream);

// ---- fast tail (the common case: m <= 128 bins wanted, k <= 128) ----
#define RQ_FAST_MAX_M 320
#define RQ_FAST_MAX_K 320       // beyond that the 512 partition maxima give too loose a threshold (k = 512: every query overflows)
#define RQ_CAND_CAP 4096       // candidate keys per query (compact list written by the tail kernel)

// Fused tail: threshold + bin collection + exact re-score + final top-k + certificate in one launch.
struct RqTailArgs {
    const float* q; int dim;                       // raw fp32 queries [B][dim]
    const void* x; const double* rownorm64; int64_t n_rows;
    int dpad;                                      // stored row length of x in elements (768 or 384): selects the tail kernel's instantiation
    const uint2* bins; int64_t bins_stride; int64_t nbins;
    const float* wgmax; int wgmax_stride; int nwg;
    int nwg_split, nwg2;                           // queries >= nwg_split were scanned by a grid of nwg2 workgroups (a call's narrow passes follow its wide ones)
    int m, metric, k;
    float eps, max_row_norm;
    int64_t row_offset;
    uint64_t* cand;                                // [B][RQ_CAND_CAP] compact candidate keys
    int* rowcount; int* done; int* ovf;            // [B] each, zero before the launch, reset by the kernel
    float* out_scores; int64_t* out_rows; uint64_t* out_keys; int* out_status;
    const float* qeps;                             // per query error share e_q (int8 scan): bound = e_q (1 + eps) + eps; null = eps alone
    const float* binerr;                           // int8 scan: worst row error of every bin (rq_quant_rows_kernel), or null.  A bin is tested against
    float eps_rows_max;                            //   T + (1 + e_q) (eps_rows_max - binerr[bin]): its own rows' bound instead of the shard's worst row
    int local_topk;                                // 1: a workgroup with more than k row jobs publishes only its own k best keys (rq_tail_body.h)
    float thr_mult;                                // threshold T = P - bound - (thr_mult - 1) * max(bound, thr_slack): 2.25 always
    float thr_slack;                               //   certifies; less = fewer candidates, the rare query is repaired (rq_tail_body.h)
    unsigned long long* dbg;                       // development: per-workgroup (start, end) wall-clock stamps of the fused launch, or null
    int stop_after;                                // development: 0 = full kernel, 1..4 = return after phase A..D
    int fused_nv;                                  // development: 0 = the launcher's rule, 1 / 4 / 8 = 512 / 2048 / 4096 bins per riding tail workgroup
};
// workgroups [0, scan_grid) run the scan `sa`, the next ones the tail `ta` of an EARLIER batch, the last pa.nslots the query
// preparation `pa` of a LATER batch
hipError_t rq_scan_tail_launch(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, bool nt, int scan_grid, int epi, hipStream_t stream,
                               hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the same launch over rows of 384 elements (rq_scan_narrow.hip): scan workgroups of rq_scan_narrow_launch's 64-query form, tail
// workgroups that read rows of 768 bytes, the same preparation workgroups
hipError_t rq_scan_narrow_tail_launch(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, bool nt, int scan_grid, hipStream_t stream,
                                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t rq_tail_launch(const RqTailArgs& a, int B, hipStream_t stream);
// Tails of the n = 1..4 batches of a bundle (one 128- or 256-query pass, rq_bundle_plan.h) in ONE launch, each with its own k and
// outputs, plus pa.nslots workgroups that prepare the queries of the batch announced after them: grid = chunks x (B[0] + .. +
// B[n - 1]) tail workgroups, then pa.  No two of the tails may share cand / rowcount / done / ovf.
#define RQ_BUNDLE_TAILS 4
hipError_t rq_bundle_tail_launch(const RqTailArgs* t, const int* B, int n, const RqPrepArgs& pa, hipStream_t stream);
// Two query preparations in ONE launch (a.nslots + b.nslots workgroups): a bundle member's own batch and the one it announces.
hipError_t rq_prep2_queries_launch(const RqPrepArgs& a, const RqPrepArgs& b, hipStream_t stream);
// chunk size rule shared by both launchers: 512-bin chunks while that keeps the grid around a thousand workgroups
// (enough to spread the hits, few enough to be one dispatch round), else 2048-bin chunks
static inline bool rq_tail_small_chunks(int64_t nbins, int B) { return ((nbins + 511) / 512) * B <= 1536; }

// ---- filtered searches (rq_filter.hip, include/rq.h rq_filter): only the rows whose bit is set take part ----
// What the filtered tail kernel gets beside its RqTailArgs (a SECOND kernel argument: RqTailArgs and every kernel that takes
// it alone stay as they are).
struct RqFilterArgs {
    const uint32_t* bits;     // [ceil(n_rows / 32)] bit r % 32 of word r / 32: local row r is allowed; bits >= n_rows are clear
    const uint32_t* first;    // [min(na, RQ_MAX_K)] the first allowed rows, ascending: the answer of a zero-norm query
    int64_t na;               // allowed rows
};
// rq_tail_launch with the filter: rq_tail_kernel<NV, DP, true>.  a.m must be min(k, na).
hipError_t rq_tail_filtered_launch(const RqTailArgs& a, const RqFilterArgs& f, int B, hipStream_t stream);
// out[i] = src[i] for an allowed row i < n_rows, NaN for every other i < cap: the scan's row scales under a filter.
hipError_t rq_mask_scale_launch(const float* src, const uint32_t* bits, int64_t n_rows, int64_t cap, float* out, hipStream_t stream);
// cand[i] = 0 for every candidate key (score, LOCAL row) whose row is not allowed; n keys in all.
hipError_t rq_mask_keys_launch(uint64_t* cand, int64_t n, const uint32_t* bits, hipStream_t stream);
// Exact fp64 re-score of the listed rows for B queries: cand[q * cand_stride + j] = key(score(q, list[j]), list[j]), j < nlist.
// The per-row arithmetic is rq_tail_body.h's (16 lanes per row, the same summation order).
struct RqGatherArgs {
    const void* x; int dpad;  // stored rows and their length in elements (768 or 384)
    const double* rownorm64;
    const float* q32;         // [B][768] raw fp32 queries, zero padded (rq_prep_body)
    const double* qnorm64;    // [B]
    const uint32_t* list;     // [nlist] local rows, each < the shard's rows
    int64_t nlist;
    int metric;
    uint64_t* cand; int64_t cand_stride;
};
#define RQ_GATHER_MAX_CHUNKS 65535   // chunks of 256 listed rows per launch (grid y); rq_gather_score_launch loops beyond
hipError_t rq_gather_score_launch(const RqGatherArgs& a, int B, hipStream_t stream);

// ---- one filter per query (rq_filter_each.hip, include/rq.h rq_search_filtered_each) ----
// The ragged gather: rq_gather_score_kernel with a list per query.  The queries of a launch come as runs that share a list
// (RqEachRun: the queries of one filter); a work item is (run, 256-row chunk of its list, query of the run), the query running
// fastest, so that the workgroups in flight together re-score the SAME 256 rows for the queries that share them -- the reason
// rq_gather_score_kernel puts the query on blockIdx.x.  Item i of the launch belongs to the run with item_base <= i < the next
// run's (found by bisection, uniform over the workgroup).  Keys: cand[each[j].key_off + position in the list], 64-bit offsets.
struct RqEachRun {
    int64_t item_base;         // work items of the runs before this one
    int64_t na;                // rows of the run's list, >= 1
    int first, count;          // the run's queries: each[first .. first + count)
};
struct RqRaggedArgs {
    const void* x; int dpad;   // stored rows and their length in elements (768 or 384)
    const double* rownorm64;
    const float* q32;          // [prepared queries][768] raw fp32 queries, zero padded (rq_prep_body); addressed by each[j].q
    const double* qnorm64;
    const RqEachDesc* each;    // the launch's queries
    const RqEachRun* runs; int nruns;   // nruns >= 1; runs[nruns] is a sentinel whose item_base is the number of items
    int metric;
    uint64_t* cand;
};
#define RQ_RAGGED_MAX_ITEMS 2147483647LL   // work items per launch (grid x); rq_gather_ragged_launch loops beyond
hipError_t rq_gather_ragged_launch(const RqRaggedArgs& a, int64_t items, hipStream_t stream);
// rq_mask_keys_launch with a bitmap per query: key j of query i (cand[each[i].key_off + j], j < each[i].ncand) becomes 0 unless
// its row's bit is set in each[i].bits.  nq <= 65535.
hipError_t rq_mask_keys_each_launch(uint64_t* cand, const RqEachDesc* each, int nq, int64_t max_ncand, hipStream_t stream);
// Rows of [n][dim] floats gathered (dst[i] = src[pos[i]]) and a sub-batch's results scattered back to the queries pos[i] of the call
// (scores / rows / keys [n][k], status [n]; keys may be null on both sides together); src null: the queries pos[i] get padding
// (0.0, -1, key 0) and status 0.
hipError_t rq_each_gather_rows_launch(const float* src, const int* pos, int n, int dim, float* dst, hipStream_t stream);
struct RqEachScatterArgs {
    const int* pos; int n, k;
    const float* src_scores; const int64_t* src_rows; const uint64_t* src_keys; const int* src_status;   // src_scores null: padding
    float* scores; int64_t* rows; uint64_t* keys; int* status;
};
hipError_t rq_each_scatter_launch(const RqEachScatterArgs& a, hipStream_t stream);

// ---- MMR selection (rq_mmr.hip, include/rq.h rq_mmr_select_device): k of m candidate rows per query, greedily by
// v = lambda rel - (1 - lambda) max similarity to the rows already picked; one workgroup per query ----
struct RqMmrArgs {
    const void* x; int dpad;      // stored rows and their length in elements (768 or 384)
    const double* rownorm64;
    int64_t n_rows, row_offset;   // candidates carry GLOBAL rows: row_offset + local row; anything outside the shard is absent
    const int64_t* cand_rows;     // [B][m], -1 = absent
    const float* cand_rel;        // [B][m] relevance, NaN = absent
    int m, k, metric;             // 1 <= k <= m <= RQ_MAX_K
    double lambda;
    float* out_scores;            // [B][k] the picked candidates' relevance, unchanged
    int64_t* out_rows;            // [B][k] global rows in selection order, -1 padded
    float* out_mmr;               // [B][k] fp32(v) at the moment of selection, or null
};
hipError_t rq_mmr_launch(const RqMmrArgs& a, int B, hipStream_t stream);

// ---- scoring given rows (rq_score.hip, include/rq.h rq_score_rows_device): scores[q][j] = score(query q, rows[q][j]), one list of
// m global rows per query; grid (queries, tiles of RQ_SCORE_TILE positions) ----
struct RqScoreArgs {
    const void* x; int dpad;      // stored rows and their length in elements (768 or 384)
    const double* rownorm64;
    int64_t n_rows, row_offset;   // the lists carry GLOBAL rows: row_offset + local row; anything outside the shard is absent; n_rows >= 1
    const float* q32;             // [queries][768] raw fp32 queries, zero padded (rq_prep_body)
    const double* qnorm64;        // [queries]
    const int64_t* rows;          // [queries][m]
    int m, metric;
    float* scores;                // [queries][m]: the score of a present entry, 0.0 for an absent one
};
hipError_t rq_score_rows_launch(const RqScoreArgs& a, int queries, hipStream_t stream);

// Merge G sorted key lists per query (cross-shard): in [B][G*k] -> top-k scores/rows/keys.
hipError_t rq_merge_keys_launch(const uint64_t* keys, int n_per_query, int B, int k, float* out_scores, int64_t* out_rows,
                                uint64_t* out_keys, hipStream_t stream);
hipError_t rq_read_probe_launch(const void* x, int64_t bytes, bool nt, int grid, uint32_t* sink, hipStream_t stream);
