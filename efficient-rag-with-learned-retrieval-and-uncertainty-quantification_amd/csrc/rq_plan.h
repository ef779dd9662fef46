// rq_plan.h -- what a search call will do, decided before anything is allocated or launched: the route (int8 image, exact,
// fast or generic tail), the cut into passes of 256 / 128 / 64 queries, the wide scan grid and where the second grid starts,
// the non-temporal-load rule.  Plain arithmetic on the index's fields and the call's arguments: no HIP runtime call, nothing
// is written to the index (tests/native/plan_check.cpp runs it on the host).  What depends on a remembered stream or on a
// device result -- fused / piped / pair, the workgroups per CU of the second grid, building the int8 image -- stays with
// run_pipeline (rq_search.hip).
#pragma once
#include "rq_index.h"

// Bound on |scan score - exact score| handed to the tail kernels, which use it as is for cosine and multiplied by the
// largest row norm for the inner product: the derived bound (or option "eps") plus what the matrix cores drop by flushing
// the fp16-subnormal elements of a stored row (rq_select.hip rq_rownorm_kernel).
static inline float scan_eps(const rq_index* idx, int metric) {
    const double base = idx->eps < 0 ? (double)RQ_EPS_DEFAULT : idx->eps;
    if (metric == RQ_METRIC_COSINE) return (float)(base + idx->max_sub_rel * (1.0 + 1e-6));
    return (float)(base + (idx->max_row_norm > 0.0 ? idx->max_sub_abs / idx->max_row_norm * (1.0 + 1e-6) : 0.0));
}
// the shard's share of the int8 scan's bound (unit-query units; the query's own share is added per query by the tail):
// worst row + the fp32 steps between the exact int32 sum and the bin record (two scale products, two 6-bit truncations)
static inline float scan8_eps(const rq_index* idx) { return (float)(idx->max_e8 * 1.000001 + 2e-5); }

static inline int nb_default(const rq_index* idx, int k) {
    const int slack = idx->slack_bins >= 0 ? idx->slack_bins : std::max(8, k / 8);
    return k + slack;
}

// What the scoring and MMR calls (`what`) refuse alike: B outside 1..65535, an unknown metric and, last, a multi-device index.
static inline int check_batch_metric(const rq_index* idx, int B, int metric, const char* what) {
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (metric != RQ_METRIC_COSINE && metric != RQ_METRIC_IP) return set_err(RQ_EINVAL, "unknown metric %d", metric);
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "RQ_EUNSUPPORTED: %s on a multi-device index: use one index per device", what);
    return RQ_OK;
}

// Queries per group of a call that holds keys_per_query candidate keys for each: as many as keep the keys within 1 GiB, at
// least one, at most B.  The exact scans hold ceil(n / 64) * 64 keys per query, the filter's gather route its allowed rows.
static inline int queries_per_gib(int B, int64_t keys_per_query) {
    const int64_t per_q = std::max<int64_t>(keys_per_query * (int64_t)sizeof(uint64_t), 1);
    return (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 30) / per_q));
}

// Device bytes a blocking search of B queries for k results stages (rq_filter.hip; 64-bit throughout).
struct SearchStaging { size_t q = 0, scores = 0, rows = 0, status = 0; };
static inline SearchStaging search_staging(int dim, int B, int k) {
    const size_t b = (size_t)B, bk = b * (size_t)k;
    return {b * (size_t)dim * sizeof(float), bk * sizeof(float), bk * sizeof(int64_t), b * sizeof(int)};
}

#define RQ_SCAN8_MIN_ROWS 100000
// ... and k <= 128 (beyond that the candidate sets of the looser bound outweigh the bytes saved)
#define RQ_SCAN8_AUTO_MAX_K 128
#define RQ_SCAN8_SMALL_K 32     // up to here one int8 image per query, beyond two (plan_call)
#define RQ_SCAN8_MAX_ROW_ERR 0.03   // beyond that the candidate sets stop being small: such a shard keeps the fp16 scan
static inline int scan8_kclass(int k) { return k <= RQ_SCAN8_SMALL_K ? 0 : 1; }

// Shards that cannot stay in the 256 MiB Infinity Cache between two scans
static inline bool beyond_cache(int64_t rows, int64_t row_bytes) { return rows * row_bytes > ((int64_t)208 << 20); }

// Workgroups of a scan pass that runs wg_cu workgroups per CU (the grids: below, at CallPlan).
static inline int scan_grid(const rq_index* idx, int nquads, int wg_cu) {
    return (int)std::min<int64_t>(std::min<int64_t>(nquads, RQ_WGMAX_STRIDE), (int64_t)idx->cu_count * wg_cu);
}
// The fast tail's threshold is the m-th largest PARTITION maximum (rq_tail_body.h phase A; m = the rows wanted), and a scan pass leaves
// one maximum per workgroup.  A pass of fewer workgroups than that has no such maximum: the threshold is -inf, every bin becomes a
// candidate, the lists overflow, and the ladder searches every query of the pass again.  The 64-query passes run two workgroups per
// CU, which covers RQ_FAST_MAX_K on any device of 160 CUs and more; the wide passes run ONE per CU -- 256 on an MI355X -- so a call
// with a wide pass over the fp16 rows that wants more rows than that takes the generic tail at once (plan_call).  This is the bound
// that can be proven; how loose the threshold already is just below it is a matter of the corpus, and stays with the ladder.
static inline bool fast_tail_fits(const rq_index* idx, int k, int nwg) { return std::min<int64_t>(k, idx->n) <= (int64_t)nwg; }

// Calls of more than 64 queries: passes of 128 queries over the image (two 16-query groups per wave, rq_scan.hip I8 = 3) while
// the class runs with one image per query and "wide8" is on; otherwise the fp16 passes of rq_scan_wide.hip.
// ... or while it runs with two images for its 64-query calls and one image is known to be good enough for the wide ones (wide1, rq_index.h)
static inline bool scan8_wide_level_ok(const rq_index* idx, int kclass) {
    const int lvl = idx->scan8_level[kclass];
    // (not under an explicit "scan8_split" = 1: the caller asked for two images everywhere, which no wide pass offers)
    return lvl == 0 || (lvl == 1 && idx->scan8_split < 0 && !idx->wide1_off[kclass] && (idx->scan8 == 2 || idx->wide1_ok[kclass] || idx->calib_rows == 0));
}

// int8 scan ("scan8": 0 = never; 1 = k <= RQ_SCAN8_AUTO_MAX_K on shards of RQ_SCAN8_MIN_ROWS rows and more; 2 = always): the scan
// reads the int8 image of the shard when its worst row quantises well enough.  The size rule: on Gaussian rows the image
// pays down to 125k rows (fused two-stream loop, us per batch int8 / fp16: 250k rows 35.0 / 59.8, 125k rows 25.0 / 29.0),
// but a 125k-row document-structured shard takes 64 us against 34 in the same loop (profiles/r02_shard_shapes.txt).  Its bound does not
// involve fp16 subnormals (the image is relative to each row's largest element), so it is decided BEFORE `exact` (plan_call).
// Two phases: scan8_wanted says whether the call brings the image up to date (ensure_x8, which may build it and calibrate the
// ladder: the caller's side effect), scan8_usable whether the call then scans it.
static inline bool scan8_wanted(const rq_index* idx, int B, int k, int nb, unsigned flags) {
    const int kclass = scan8_kclass(k);
    const int64_t nbins = (idx->n + 63) / 64;
    const bool wide_ok = B <= 64 || (idx->wide8 && idx->wide_batch != 0 && scan8_wide_level_ok(idx, kclass));
    return (flags & CALL_ALLOW8) && !idx->narrow() && idx->scan8 && idx->scan8_level[kclass] < 2 && nb >= 0 && 2 * (int64_t)nb < nbins && wide_ok &&
           !(flags & CALL_FORCE_GENERIC) && idx->fast_tail && k <= RQ_FAST_MAX_K &&
           (idx->scan8 == 2 || (idx->n >= RQ_SCAN8_MIN_ROWS && k <= RQ_SCAN8_AUTO_MAX_K));
}
static inline bool scan8_usable(const rq_index* idx, int B, int k) {   // (after ensure_x8: the class's level is read again)
    const int kclass = scan8_kclass(k);
    return idx->x8 && idx->x8_valid == idx->n && idx->max_e8 <= RQ_SCAN8_MAX_ROW_ERR && idx->scan8_level[kclass] < 2 &&
           (B <= 64 || (scan8_wide_level_ok(idx, kclass) && (idx->scan8_level[kclass] == 0 || idx->scan8 == 2 || idx->wide1_ok[kclass])));
}

static const int RQ_MAX_PASSES = 1024;

struct CallPlan {
    int nquads = 0;           // ceil(rows / 64); bin = quad
    int64_t nbins = 0;
    bool narrow = false;      // rows of 384 elements (rq_scan_narrow.hip): no int8 image, passes of 64 / 128 queries, no scanned-ahead pair
    int kclass = 0;           // class of k of the int8 ladder
    bool use8 = false;        // the scan reads the int8 image
    bool split8 = false;      // ... with the queries as two images
    bool exact = false;       // every bin re-scored, no corpus scan
    int nb = 0;               // bins re-scored per query (exact: all of them)
    int m = 0;                // generic tail: bins re-scored + the first one that is not
    bool fast = false;        // the fast tail (rq_tail.hip) instead of select / re-score / final
    int64_t ncand = 0;        // candidate keys per query
    int64_t stride = 0;       // bin records per query
    int pass_q[RQ_MAX_PASSES];   // queries per corpus pass, widest first
    int npass = 0, bpad = 0;  // ... and the query slots they cover
    int64_t scan_rowb = 0;    // bytes a scan reads per row
    bool nt = false;          // non-temporal corpus loads
    int grid_wide = 0;        // workgroups of the passes that run ONE 512-thread workgroup per CU
    int nwg_split = 0;        // first query of the first pass of the second grid (a scanned-ahead pair: the caller's)
};

// Scan grids.  Every fp16 pass of more than 64 queries, and the int8 256-query pass, runs ONE 512-thread workgroup per CU ("wide");
// the 64-query passes and the int8 128-query pass run wg_per_cu 256-thread workgroups per CU.  A call's passes are cut widest first,
// so its wide passes precede its narrow ones: the tail is told where the second grid starts (nwg_split).  Until round 3 the first
// pass's grid served the whole call, and the remainder pass of e.g. 384 int8 queries ran at half its occupancy (232 us instead of 150).
// (rows of 384 elements: both forms are 256-thread workgroups)
static inline bool pass_wide(const CallPlan& p, int qb) { return qb > 64 && !p.narrow && (!p.use8 || qb == 256); }

// Everything about a call of B queries on a shard that holds rows which does not depend on its stream.  nb < 0: exact scan.
static inline int plan_call(const rq_index* idx, int B, int k, int metric, int nb, bool use8, unsigned flags, CallPlan* plan) {
    CallPlan& p = *plan;
    p.nquads = (int)((idx->n + 63) / 64);
    p.nbins = p.nquads;
    p.narrow = idx->narrow();
    p.kclass = scan8_kclass(k);
    p.use8 = use8;
    // Queries as ONE int8 image or as TWO (value + residual: the query's share of the bound vanishes, every corpus fragment
    // feeds two MFMAs).  Measured at 1M rows, fused loop: k = 10  132 us per batch with one image, 143-146 with two (the
    // scan stops being purely HBM-bound); k = 100  189 us with one, 153 with two (a third of the candidate rows).  "scan8_split"
    // -1 (default): one image for k <= 32, two beyond; 0 / 1: one / two for every k.  That is only where a class STARTS: when
    // more than 1 in 16 checked queries of a class needed repair, rq_search_fixup_device moves it one step along
    // one image -> two images -> fp16 scan (clustered corpus + random queries at k = 10: one image 19 of 64 queries repaired,
    // two images none, 245 us per batch against 275 with the fp16 scan).
    p.split8 = use8 && idx->scan8_level[p.kclass] == 1 && B <= 64;      // (wide calls: one image)
    // tiny shards (fewer than two bins per wanted bin): the approximate pass cannot narrow anything down
    // ... and shards whose rows keep so much of their norm in fp16-subnormal elements that the fp16 scan's scores say nothing
    p.exact = nb < 0 || 2 * (int64_t)nb >= p.nbins || (!use8 && idx->eps < 0 && scan_eps(idx, metric) > RQ_EPS_USELESS);
    if (p.exact) nb = (int)std::min<int64_t>(p.nbins, INT32_MAX / 64);
    if (!p.exact && nb > RQ_NB_MAX) return set_err(RQ_EINVAL, "nb %d too large", nb);
    p.nb = nb;
    p.m = nb + 1;
    p.fast = !p.exact && !(flags & CALL_FORCE_GENERIC) && idx->fast_tail && k <= RQ_FAST_MAX_K;
    p.ncand = p.fast ? (int64_t)RQ_CAND_CAP : (int64_t)nb * RQ_BIN_ROWS;
    p.stride = (p.nbins + 63) / 64 * 64;
    // Queries per corpus pass: 64, or -- once a call has more than 64 -- 128 / 256 (every LDS fragment of the corpus feeds
    // two MFMAs per wave; option "wide_batch": 0 = passes of 64 only, 1 = 64/128/256, 2 = round 1's 8-wave 128-query pass,
    // 3 = 64/128 without the 256-query pass).  A call is cut into passes greedily: 256 while more than 128 queries remain,
    // then 128, then 64.
    const int wb = idx->wide_batch;
    const int big = wb == 1 ? 256 : (wb == 2 || wb == 3 ? 128 : 64);
    p.npass = p.bpad = 0;
    for (int left = B; left > 0;) {
        int qb = 64;
        if (p.narrow) qb = (wb != 0 && left > 64) ? 128 : 64;   // rows of 384 elements: 128 then 64 (rq_scan_narrow.hip)
        else if (use8 && B > 64) {                               // int8 image: passes of 256 (rq_scan_wide.hip I8), 128 (rq_scan.hip I8 = 3) and 64 queries
            if (idx->wide256_8 && big >= 256 && left > 128) qb = 256;
            else if (left > 64 || !idx->wide256_8) qb = 128;
        }
        else if (big >= 256 && left > 128) qb = 256;
        else if (big >= 128 && left > 64) qb = 128;
        if (p.npass == RQ_MAX_PASSES) return set_err(RQ_EINVAL, "too many passes");
        p.pass_q[p.npass++] = qb;
        p.bpad += qb;
        left -= qb;
    }
    // non-temporal loads only for shards that cannot stay in the 256 MiB Infinity Cache between two scans
    // (measured: 192 MB shard 36 us with default policy vs 39 us nt; 1.5 GB shard 250 us nt vs 285 us default)
    p.scan_rowb = use8 ? RQ_DPAD : (int64_t)idx->rowb();
    p.nt = idx->nt < 0 ? beyond_cache(idx->n, p.scan_rowb) : idx->nt != 0;
    p.grid_wide = scan_grid(idx, p.nquads, 1);
    p.nwg_split = p.bpad;
    for (int blk = p.npass - 1, q0 = p.bpad; blk >= 0 && !pass_wide(p, p.pass_q[blk]); --blk) p.nwg_split = (q0 -= p.pass_q[blk]);
    // a call with a pass on the wide grid whose workgroups are fewer than the rows wanted: the generic tail (fast_tail_fits)
    // (not over the int8 image, which only the fast tail reads: there the ladder's own count of repairs takes the class off the image)
    if (p.fast && !use8 && p.nwg_split > 0 && !fast_tail_fits(idx, k, p.grid_wide)) {
        p.fast = false;
        p.ncand = (int64_t)nb * RQ_BIN_ROWS;
    }
    return RQ_OK;
}
