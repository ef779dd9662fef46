// rq_index.h -- internal definitions shared by the host translation units: rq_api.hip (storage, options, the C ABI),
// rq_search.hip (search orchestration), rq_filter.hip (filtered searches), rq_filter_each.hip (one filter per query), rq_mmr.hip (MMR selection), rq_score.hip (scoring given rows), rq_range.hip (range searches), rq_group.hip (grouped searches), rq_group_members.hip (the members of the top groups), rq_scan8.hip (the int8 image and its ladder) and
// rq_multi.hip (the multi-device parent): error channel, the index object, the per-stream workspaces, the device guard, the pieces
// of a call that the routes share.  The staging of the blocking host-buffer forms is rq_stage.h's.
// Not part of the public boundary (that is include/rq.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/rq.h"
#include "rq_bundle_plan.h"
#include "rq_device.h"
#include "rq_kernels.h"

#define RQ_INTERNAL __attribute__((visibility("hidden")))

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
RQ_INTERNAL int set_err(int code, const char* fmt, ...);   // stores the message of rq_last_error() (thread local), returns code
RQ_INTERNAL const char* rq_err_text();
#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return set_err(RQ_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// hipFree every pointer of the list that is set, and null it
template <class... T>
static inline void free_dev(T*&... p) { ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...); }

// ---------------------------------------------------------------------------------------------
// index object
// ---------------------------------------------------------------------------------------------
// One set of prepared queries (rq_kernels.h RqPrepArgs): RQ_DPAD-wide slots in both row layouts.
struct QuerySet {
    _Float16* qh = nullptr;       // unit-norm fp16 query fragments for the scan
    float* q32 = nullptr;         // padded fp32 queries / fp64 norms for the tails
    double* qn = nullptr;
    signed char* q8 = nullptr;    // int8 scan: the queries' int8 image, their scales and quantisation errors
    float* qscale8 = nullptr;
    float* qeps8 = nullptr;
    signed char* q8lo = nullptr;  // second int8 image (the residual) and the error left after both
    float* qeps8s = nullptr;
};

struct Workspace {
    int bcap = 0;                 // query slots (multiple of 64)
    int64_t bins_stride = 0;      // bin records per query
    int64_t binkeys_cap = 0;      // entries per query
    size_t cand_elems = 0;        // candidate keys allocated in total (queries of a call x keys per query)
    QuerySet qs;                  // [bcap] the call's prepared queries
    uint2* bins = nullptr;        // [bcap][bins_stride] scan output: one record per (query, quad), see rq_device.h
    uint64_t* binkeys = nullptr;
    uint64_t* cand = nullptr;
    float* wgmax = nullptr;       // [bcap][RQ_WGMAX_STRIDE]
    int* rowcount = nullptr;      // [bcap] fast tail: candidate rows appended so far
    float* thr = nullptr;         // [bcap]
    int* done = nullptr;          // [bcap] fast tail: workgroups of the query that have finished
    int* ovf = nullptr;           // [bcap] fast tail: a workgroup found more bins / rows than it could hold
    bool counters_zero = false;   // rowcount/done/ovf known to be all zero (the tail kernel leaves them so)
    // staging for rq_search_fixup_device
    int fix_bcap = 0, fix_k = 0;
    float* fix_q = nullptr;
    float* fix_scores = nullptr;
    int64_t* fix_rows = nullptr;
    uint64_t* fix_keys = nullptr;
    int* fix_status = nullptr;
    // range searches (rq_range.hip): per query slot the candidate keys appended so far, the status rq_final_kernel writes (unused: the
    // range kernels write the caller's), a norm of 1.0 for rq_final_kernel (the keys of a zero-norm query are already its answer)
    int rg_bcap = 0;
    unsigned* rg_slot = nullptr;
    int* rg_status = nullptr;
    double* rg_one = nullptr;
};

// Per caller stream: two workspaces (alternating calls), an internal tail stream and the events that
// order scan -> tail and tail -> reuse of the same workspace two calls later ("pipeline" option).
struct StreamCtx {
    Workspace w[2];
    hipStream_t tail = nullptr;
    hipEvent_t ev_scan[2] = {nullptr, nullptr};
    hipEvent_t ev_tail[2] = {nullptr, nullptr};
    bool tail_pending[2] = {false, false};
    uint64_t calls = 0;
    // "pipeline" = 2: the tail of the last search waits here and rides along with the next scan launch of the stream
    bool fused_pending = false;
    RqTailArgs fused_tail;
    int fused_B = 0;
    // "pipeline" = 2 keeps the prepared queries of consecutive calls apart in a ring of RQ_RING_SLOTS slots of 64 queries, ONE
    // allocation (rq_search.hip ring_slot): a lone call scans its slot while the tail that rides with it reads the slot before
    // and the extra workgroups of the same launch prepare the hinted queries of the next call into the slot after
    // (rq_search_hint_next_device); the members of a bundle take consecutive slots.  Which slot: rq_bundle_plan.h.
    QuerySet ring;                      // RQ_RING_SLOTS x 64 slots
    const float* hint_q = nullptr;      // queries announced for the next fused call, not yet prepared
    int hint_B = 0;
    const float* prepped_q = nullptr;   // queries a launch has already prepared ...
    int prepped_B = 0, prepped_slot = -1;   // ... and the slot they are in
    // options "scan_ahead" / "scan_bundle": up to four consecutive calls of the stream are scanned by ONE pass into the quarters
    // of workspace w[b_par] (rq_bundle_plan.h: state, roles, slots).  b_tail[j] / b_B[j]: member j's tail -- while members are
    // only gathered, its k, m and outputs alone; once the pass is enqueued, complete.  The batch scanned ahead (member bs.n of an
    // AHEAD bundle, b_tail without k / m / outputs) belongs to the next call if it brings await_q, await_B and await_metric;
    // anything else (another call, a flush) completes the members that came and discards that quarter.
    BundleState bs;
    RqTailArgs b_tail[RQ_BUNDLE_MAX];
    int b_B[RQ_BUNDLE_MAX] = {0, 0, 0, 0};
    int b_par = 0, b_metric = -1;
    const float* await_q = nullptr;
    int await_B = 0, await_metric = -1;
    // where the stream's last call left its bin records (test hooks rq_debug_bin_records / rq_debug_pooled): query slot j of
    // that call is rec_bins + j * rec_stride; its passes covered rec_slots slots (rec_B of them valid, the rest pad).
    // rec_bins == nullptr: the last call ran no approximate scan (exact route, empty shard).
    const uint2* rec_bins = nullptr;
    int64_t rec_stride = 0;
    int rec_B = 0, rec_slots = 0;
    // grouped searches (rq_group.hip): the candidate rows of the stream's last rq_search_grouped_device call ([B][m1] scores and
    // rows, grp_elems allocated of each) and its search's status ([grp_bcap])
    float* grp_scores = nullptr;
    int64_t* grp_rows = nullptr;
    int* grp_status = nullptr;
    size_t grp_elems = 0;
    int grp_bcap = 0;
    // group members (rq_group_members.hip): the winners of the stream's last rq_search_group_members_device call ([B][k] scores and
    // rows, gm_elems allocated of each); the fill reads the rows
    float* gm_scores = nullptr;
    int64_t* gm_rows = nullptr;
    size_t gm_elems = 0;
    // one filter per query (rq_filter_each.hip).  The tables of a call (per-query descriptors, runs, batch positions) are written into
    // pinned host memory and copied to each_tab on the stream; each_ev marks the end of that copy (the next call waits for it before
    // it writes the pinned block again).  each_q .. each_status: the staging sub-batch of a group whose queries are not one
    // contiguous run, [each_bcap] queries and [each_bcap][each_k] results.
    char* each_pin = nullptr;
    char* each_tab = nullptr;
    size_t each_tab_bytes = 0;
    hipEvent_t each_ev = nullptr;
    bool each_ev_pending = false;
    float* each_q = nullptr;
    float* each_scores = nullptr;
    int64_t* each_rows = nullptr;
    uint64_t* each_keys = nullptr;
    int* each_status = nullptr;
    int each_bcap = 0, each_k = 0;
};

// A row filter (include/rq.h rq_filter): the set of local rows a filtered search may return.  It belongs to one index at one size
// (n): an append makes it stale.  The bookkeeping is done once, on the host, from the bitmap; device arrays beyond the bitmap are
// built by the first search that needs them.
struct rq_filter {
    rq_index* idx = nullptr;
    int64_t n = 0, na = 0;               // rows of the index at creation, allowed rows
    std::vector<uint32_t> bits;          // host copy of the bitmap, bits >= n clear
    std::vector<int32_t> occ_prefix;     // [bins + 1] bins before bin b that hold an allowed row (rq_filter_plan.h)
    uint32_t* d_bits = nullptr;          // [ceil(n / 32)]
    uint32_t* d_first = nullptr;         // [min(na, RQ_MAX_K)] first allowed rows
    uint32_t* d_list = nullptr;          // [na] every allowed row, ascending (gather route; lazy)
    float* scale[2] = {nullptr, nullptr};   // [scale_cap] masked row scales per metric (scan route; lazy)
    int64_t scale_cap[2] = {0, 0};
};

// Default scan variant: half-row stages (kstage 2), ring of 3, one LDS fragment ahead (prefetch 1, <= 168 VGPRs),
// 2 workgroups per CU.  All variants stream at the same rate; this one leaves room on every CU (registers:
// 2 x 168 + 168 <= 512 VGPRs; LDS: 3 x 53 760 B <= 160 KB) for a tail workgroup to be resident beside the scan.
struct rq_index {
    int dim = 0, device = 0, cu_count = 256;
    // Stored row length in elements (option "row_pad"): 384 for dim <= 384, else 768 (RQ_DPAD); fixed before the first row is stored.
    // Everything that addresses corpus rows takes its stride from here (rowb()).  384 = the narrow layout (rq_scan_narrow.hip): rows of
    // 768 bytes, no int8 image, passes of 64 / 128 queries.  The query-side buffers (qh, q32, rings) are 768 elements wide in both.
    int dpad = RQ_DPAD;
    bool narrow() const { return dpad != RQ_DPAD; }
    size_t rowb() const { return (size_t)dpad * 2; }   // bytes per stored fp16 row
    int64_t n = 0, cap = 0, row_offset = 0;
    char* x = nullptr;
    double* rownorm64 = nullptr;
    float* inv_norm = nullptr;
    float* ones = nullptr;
    int64_t ones_valid = 0;
    // int8 image of the shard for the int8 scan (option "scan8"), built lazily for rows [0, x8_valid)
    signed char* x8 = nullptr;
    float* scale8_cos = nullptr;   // [cap] s_row / ||row||, pad rows NaN
    float* scale8_ip = nullptr;    // [cap] s_row
    float* binerr8 = nullptr;      // [cap / 64] worst row's relative quantisation error of every bin (fp32, rounded up)
    unsigned long long* d_stat8 = nullptr;   // device: bits of the largest relative quantisation error of a row
    int64_t x8_valid = 0;
    double max_e8 = 0.0;           // host copy of that maximum over rows [0, x8_valid)
    double* d_maxnorm = nullptr;   // device: bits of the running maxima {row norm, relative, absolute fp16-subnormal mass of a row}
    double max_row_norm = 0.0, max_sub_rel = 0.0, max_sub_abs = 0.0;
    unsigned long long* dbg_stamps = nullptr;   // development (rq_debug_stamps)
    // rq_search_fixup_device saw too many repairs behind the int8 scan; kept apart for k <= 32 ([0]) and larger k ([1])
    // per class: 0 = one int8 image per query, 1 = two images, 2 = suspended (fp16 scan); escalated by rq_search_fixup_device
    int scan8_level[2] = {0, 1};
    int64_t scan8_checked[2] = {0, 0}, scan8_repaired[2] = {0, 0};
    int64_t scan8_used = 0;        // searches that scanned the int8 image
    bool calibrating = false;      // scan8_calibrate is running its sample searches
    int64_t calib_rows = 0;        // rows of the shard when the ladder's start levels were last measured (0 = not yet)
    float calib_ms[2][3] = {{0, 0, 0}, {0, 0, 0}};   // per class, per rung (one image / two images / fp16): ms of the 64-query sample search
    int calib_unc[2][3] = {{0, 0, 0}, {0, 0, 0}};    // ... and its uncertified queries
    bool wg_auto = true;           // scan workgroups per CU by the library's rule (option "wg_per_cu" pins it)
    bool last_use8 = false;        // the caller's last search scanned the int8 image (what rq_search_fixup_device's repairs are counted against)
    // Calls of more than 64 queries in a class whose own rung is "two images" (k > 32 by default): the 256- / 128-query passes exist for ONE image only,
    // and one image there beats the fp16 wide passes (1M rows, 500 queries, k = 100: 740 against 944 us).  Allowed when the image-build measurement found the
    // one-image rung eligible for the class (or the image is forced, scan8 = 2); given up -- for wide calls only -- when more than 1 in 16 of their queries needed repair.
    bool wide1_ok[2] = {false, false}, wide1_off[2] = {false, false}, last_wide1 = false;
    int64_t wide1_checked[2] = {0, 0}, wide1_repaired[2] = {0, 0};
    int64_t repaired_total = 0;    // queries that came back uncertified and were repaired (any rung of the repair ladder)
    int64_t hints_used = 0;        // rq_search_hint_next_device: searches whose queries a launch before them prepared or scanned ahead
    int64_t bundles4 = 0;          // 256-query passes of bundles of three or four calls ("scan_bundle")
    uint64_t scan_seq = 0;         // scan launches seen while profile = 1 (every profile_stride-th one is timed)
    // options
    int ring = 3, prefetch = 1, kstage = 2, wide_batch = 1, wg_per_cu = 2, nt = -1, slack_bins = -1, profile = 0, profile_stride = 1, scan_nostore = 0, fast_tail = 1, pipeline = 0, tail_stop = 0, poison_cand = 0, poison_bins = 0, wide128 = 0, wide256 = 2, epi = 1, use_hint = 1, scan_ahead = 1, scan_bundle = 4, profile_legacy = 0, scan8 = 1, tail_local = 1, scan8_split = -1, wide8 = 1, wide256_8 = 31, bin_bound = 1, exact_mfma = 1, fused_nv = 0;
    double thr_mult8 = 1.25;       // int8 scan: threshold = P - thr_mult8 * bound (rq_tail_body.h)
    double eps = -1.0;
    std::map<hipStream_t, StreamCtx> ctx;
    hipStream_t own_stream = nullptr;
    // host-call staging
    float* h_dq = nullptr; float* h_dscores = nullptr; int64_t* h_drows = nullptr; int* h_dstatus = nullptr;
    int h_bcap = 0, h_kcap = 0;
    // small blocking searches (the reference's one-query-per-call pattern): results leave in ONE copy into pinned memory
    char* hs_dev = nullptr; char* hs_pin = nullptr; float* hs_pin_q = nullptr; size_t hs_bytes = 0, hs_qfloats = 0;
    void* add_stage = nullptr; size_t add_stage_bytes = 0;   // device staging of host-row appends
    bool hs_small = false;         // which staging path the search in flight uses (search_begin / search_end)
    // Multi-device parent (rq_index_create with n_devices > 1): no device memory of its own, one single-device child per
    // entry of device_ids.  Global rows are dealt to the children in stripes of `stripe` rows, round robin (rq_multi.hip):
    // global row g -> stripe s = g / stripe, child s % G, local row (s / G) * stripe + g % stripe.
    std::vector<rq_index*> shards;
    int64_t stripe = 65536;
    bool poisoned = false;         // an append failed part-way inside a child: the global <-> local mapping no longer holds
    std::vector<size_t> m_live;    // search staging of the parent, kept between calls: children that hold rows,
    std::vector<float> m_scores;   // their k best scores [live child][B][k]
    std::vector<int64_t> m_rows;   // and local rows
    int m_B = 0;
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t ev_used = 0;
    int64_t ev_bytes = 0;          // algorithmic corpus bytes of the launches those events time (fp16 rows or their int8 image)
    rq_timing t = {};
    // filtered searches (rq_filter.hip)
    std::vector<rq_filter*> filters;   // the filters this index still owns
    int filter_route = -1;             // option "filter_route": -1 = the rule (rq_filter_plan.h), 1 gather, 2 scan, 3 exact
    int filter_route_last = -1;        // the route the last filtered call took (0 = empty filter)
    int64_t filter_repaired = 0;       // queries of filtered calls that came back uncertified and were repaired
    // one filter per query (rq_filter_each.hip, rq_filter_each_plan.h): read-only options "filter_each_calls", "filter_each_groups_last",
    // "filter_each_ragged_last", "filter_each_rounds_last", "filter_each_shared_exact_last", "filter_each_routes_last"
    int64_t each_calls = 0, each_groups_last = 0, each_ragged_last = 0, each_rounds_last = 0, each_shared_last = 0, each_routes_last = 0;
    int64_t each_key_cap = 0;          // option "filter_each_key_cap": keys per ragged round (test hook; 0 = 1 GiB / 8)
    int64_t mmr_calls = 0;             // option "mmr_calls": MMR selections launched (rq_mmr.hip)
    int64_t score_calls = 0, score_pairs = 0;   // options "score_calls" / "score_pairs": scoring calls and their B x m pairs (rq_score.hip)
    // range searches (rq_range.hip)
    int range_route = -1;              // option "range_route": -1 = the rule (rq_range_plan.h), 1 scan, 2 gather, 3 exact
    int range_route_last = -1;         // the route the last range call took (0 = no row to return, -1 = none yet)
    int range_cand_cap = 0;            // option "range_cand_cap": qualifying rows a query may hold before it overflows (0 = the plan's default)
    int64_t range_calls = 0, range_repaired = 0;   // calls so far; queries the range fixup repaired
    unsigned long long* range_bins = nullptr;      // device: bins the last scan-route call re-scored, all queries ("range_bins_last")
    bool range_bins_valid = false;
    // grouped searches (rq_group.hip): one int32 group id per stored row, RQ_GROUP_NONE (-1) = a group of its own
    int32_t* d_groups = nullptr;       // [cap], allocated by the first rq_index_set_groups; null = every row is RQ_GROUP_NONE
    std::vector<int32_t> h_groups;     // [n] host copy once d_groups exists (the exclusion loop of the fixup builds its filters from it)
    int group_fetch = 8;               // option "group_fetch": the first rung fetches this multiple of k (rq_group_plan.h)
    int group_fetch_cap = 0;           // option "group_fetch_cap": the largest m any rung asks for (test hook; 0 = RQ_MAX_K)
    int64_t group_calls = 0, group_repaired = 0, group_rounds_last = 0;   // collapses launched; queries the fixup repaired; exclusion rounds of the last fixup
    // group members (rq_group_members.hip): the member table (rq_group_members_plan.h GroupTable) on the device, built from h_groups by
    // the first fill that needs it and dropped by rq_index_set_groups; appended rows are RQ_GROUP_NONE and belong to no list
    int32_t* gt_ids = nullptr;         // [gt_groups] distinct ids, ascending
    uint32_t* gt_off = nullptr;        // [gt_groups + 1]
    uint32_t* gt_rows = nullptr;       // [grouped rows] local rows by (id, row)
    int64_t gt_groups = 0, gt_largest = 0;
    bool gt_valid = false;
    int group_fill_cap = 0;            // option "group_fill_cap": rows of a group the fill kernel takes (test hook; 0 = RQ_GROUP_FILL_MAX, can only lower it)
    int64_t group_table_builds = 0, group_fill_calls = 0, group_fill_repaired = 0;   // table builds; fill launches; queries the member fixup filled by the exact route
    int* gm_scored = nullptr;          // device: members scored by the last fill, one word per (query, slot) ("group_fill_rows_last")
    int64_t gm_scored_slots = 0, gm_scored_cap = 0;
};

// Derived bound on |approximate scan score - exact score| for unit queries and cosine scaling:
//   fp16 rounding of the unit query (2^-11 relative, 2^-25 absolute in the subnormal range),
//   fp32 accumulation inside the MFMA chain (<= 4 * 768 * 2^-24 of sum|q_i x_i| <= 1, conservative),
//   two fp32 roundings for the row scale,
//   2^-17 relative for the row position that rq_scan_wide.hip writes into the 6 low mantissa bits of a score
//   (4.88e-4 + 8e-7 + 1.83e-4 + 1.2e-7 + 7.6e-6 = 6.8e-4).  See DESIGN.md "certificate".
static const float RQ_EPS_DEFAULT = 7.0e-4f;

// Beyond this bound the approximate pass cannot narrow anything down (cosine scores live in [-1, 1]): scan exactly.
static const float RQ_EPS_USELESS = 0.05f;

static const int RQ_NB_MAX = 3071;

// Every entry point works on the index's device and puts the caller's current device back on return (a caller that
// holds tensors on another GPU, e.g. torch with several devices, must not find its device switched under it).
struct DeviceGuard {
    int prev = -1, dev = -1;
    bool ok = true;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define RQ_ON_DEVICE(idx)                                                                                  \
    DeviceGuard dg_((idx)->device);                                                                        \
    if (!dg_.ok) return set_err(RQ_EHIP, "cannot select device %d", (idx)->device)


// ---- entry points shared between the translation units -----------------------------------------------------
// How run_pipeline is called.
enum CallFlags : unsigned {
    CALL_MAY_DEFER = 1,       // the caller accepts results that are complete only after rq_search_flush_device ("pipeline" option)
    CALL_FORCE_GENERIC = 2,   // the generic sorted tail, whatever "fast_tail" says
    CALL_ALLOW8 = 4,          // the int8 image may be the scan operand
    CALL_FETCH = 8,           // the fetch of a route built on the search (MMR, grouped): like the caller's own search, what it scanned is what the ladder repairs (last_use8)
};
// A call that ends after its scan passes (rq_range.hip: the range tail reads the bin records itself).  In: the candidate keys the
// workspace must hold.  Out: where the call's records, prepared queries and candidate keys are.
struct ScanOnly {
    size_t cand_elems = 0;
    Workspace* w = nullptr;
};
struct SearchOut {   // a call's device outputs (keys may be null); from: those of its queries from `off` on, k results each
    float* scores; int64_t* rows; uint64_t* keys; int* status;
    SearchOut from(int off, int k) const { return {scores + (size_t)off * k, rows + (size_t)off * k, keys ? keys + (size_t)off * k : nullptr, status + off}; }
};
RQ_INTERNAL int err_no_device();   // rq_api.hip: RQ_ENODEVICE and its message
// rq_search.hip
// filt (optional): the call ranks the filter's rows only (the caller has checked that it belongs to idx and is not stale)
RQ_INTERNAL int run_pipeline(rq_index* idx, const float* d_q, int B, int k, int metric, int nb, const SearchOut& out, hipStream_t s, unsigned flags,
                             const rq_filter* filt = nullptr, ScanOnly* scan_only = nullptr);
// the repair ladder of rq_search_fixup_device; filt: of rq_search_fixup_filtered_device (no int8 rung, no int8 accounting)
RQ_INTERNAL int fixup_ladder(rq_index* idx, const rq_filter* filt, const float* d_queries, int B, int k, int metric, float* d_scores,
                             int64_t* d_rows, uint64_t* d_keys, int* d_status, hipStream_t s);
RQ_INTERNAL int check_search_args(const rq_index* idx, const void* q, int B, int k, int metric, const void* sc, const void* rows);
RQ_INTERNAL int flush_tails(rq_index* idx, hipStream_t s);
RQ_INTERNAL int ensure_ones(rq_index* idx, hipStream_t s);
RQ_INTERNAL int fill_empty(int B, int k, const SearchOut& out, hipStream_t s);   // the outputs of a call that has no row to return: padding, status 0
// with_int8 = false: the int8 pointers stay null and the prepare kernel skips the int8 image (the routes that only re-score rows)
RQ_INTERNAL RqPrepArgs prep_args(const QuerySet& qs, const float* q, int dim, int B, int nslots, bool with_int8);
// The stream's workspace for a call that runs no scan (gather route, rq_score.hip): bpad prepared-query slots, cand_elems candidate
// keys (either may be unwanted: null); the stream's last call then has no bin records.  mark_no_scan: only that record.
RQ_INTERNAL int scanless_workspace(rq_index* idx, hipStream_t s, int bpad, size_t cand_elems, const QuerySet** qs, uint64_t** cand);
RQ_INTERNAL int mark_no_scan(rq_index* idx, hipStream_t s);
RQ_INTERNAL int ensure_range_ws(Workspace& w, int bpad);   // the rg_* arrays for bpad query slots (rq_range.hip)
// rq_filter.hip
RQ_INTERNAL void free_filters(rq_index* idx);   // rq_index_destroy: the filters the index still owns
RQ_INTERNAL int ensure_filter_scale(rq_index* idx, const rq_filter* f, int metric, hipStream_t s);
RQ_INTERNAL int check_filter(const rq_index* idx, const rq_filter* f);   // null, another index's, stale, multi-device
RQ_INTERNAL int ensure_filter_list(rq_filter* f);   // f->d_list: every allowed row, ascending (the gather routes)
RQ_INTERNAL int search_filtered_device(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s);
// one filter's queries down `route` (rq_filter_plan.h FilterRoute): what search_filtered_device does after its plan
RQ_INTERNAL int run_filter_route(rq_index* idx, rq_filter* f, int route, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s);
RQ_INTERNAL int flush_all(rq_index* idx);   // completes every open bundle and launches every tail still waiting for a scan ("pipeline" = 2)
RQ_INTERNAL bool bundles_open(const rq_index* idx);   // a stream holds calls whose scan is still to be enqueued (rq_bundle_plan.h GATHER)
// rq_group.hip
struct GroupOut {   // a grouped call's device outputs (keys may be null)
    float* scores; int64_t* rows; int32_t* groups; uint64_t* keys; int* status;
};
RQ_INTERNAL int search_grouped_device(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int metric, const GroupOut& out, hipStream_t s);   // rung 1, nothing waits
RQ_INTERNAL int grouped_fixup(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int metric, const GroupOut& out, hipStream_t s);   // rungs 2 and 3; queries repaired
// rq_group_members.hip
RQ_INTERNAL void drop_group_table(rq_index* idx);   // rq_index_set_groups, rq_index_destroy (the device is idle)
RQ_INTERNAL void free_ctx(StreamCtx& c);
// rq_scan8.hip
RQ_INTERNAL void drop_x8(rq_index* idx);
RQ_INTERNAL void scan8_reset_levels(rq_index* idx);
RQ_INTERNAL int ensure_x8(rq_index* idx, hipStream_t s);
RQ_INTERNAL void scan8_account(rq_index* idx, int k, int checked, int repaired);
RQ_INTERNAL int rq_add_host_common(rq_index* idx, const void* rows, int64_t n_rows, bool is_f32, int normalize);
RQ_INTERNAL int rq_search_begin(rq_index* idx, const float* queries, int B, int k, int metric);      // stage + enqueue, no wait
RQ_INTERNAL int rq_search_end(rq_index* idx, int B, int k, int metric, float* out_scores, int64_t* out_rows);   // wait, repair, hand over
RQ_INTERNAL rq_index* rq_multi_create(int dim, int n_devices, const int* device_ids);
RQ_INTERNAL int rq_multi_reserve(rq_index* idx, int64_t n_rows);
RQ_INTERNAL int rq_multi_add(rq_index* idx, const void* rows, int64_t n_rows, bool is_f32, int normalize);
RQ_INTERNAL int rq_multi_get_rows(const rq_index* idx, int64_t row_begin, int64_t n_rows, uint16_t* out);
RQ_INTERNAL int rq_multi_search(rq_index* idx, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows);
