// rq_filter_plan.h -- which route a filtered search takes (include/rq.h rq_search_filtered), decided like the call plan of
// rq_plan.h: plain arithmetic on the index's fields, the call's arguments and what the filter recorded at creation.  No HIP
// runtime call, nothing is written to the index or to the filter (tests/native/filter_plan_check.cpp runs it on the host).
// Results never depend on the route: every route returns the exact top-k of the allowed rows.
#pragma once
#include "rq_plan.h"

enum FilterRoute {
    FROUTE_EMPTY = 0,    // no row allowed: the outputs are padding
    FROUTE_GATHER = 1,   // the listed rows re-scored in fp64 (rq_gather_score_kernel): cost grows with B x na, not with N
    FROUTE_SCAN = 2,     // the scan passes with the masked row scale, the filter-aware tail, the certificate
    FROUTE_EXACT = 3,    // the exact fp64 scan of the whole shard, excluded rows' keys emptied
};

// Gather re-scores B x na rows, a scan streams N (once per pass): gather is taken while B x na x RQ_FILTER_GATHER_DIV <= N and the
// list fits (below).  Measured at 1M x 768 (tools/gpu_filter.py, profiles/filter_routes.json): workgroups of different
// queries share the listed rows through the caches, so a gathered (query, row) pair costs 0.15 ns at B = 64 and gather meets the scan
// at B x na = 1.5 N (B = 64), 3.2 N (B = 256) and, one query alone being bound by latency, 0.22 N (B = 1).  1 is inside all three
// once na <= N / 4 holds as well; a first guess of 8 left a factor of ten on the table (B = 64, na = 16 000: gather 218 us, scan
// 285 us, each with its repair step).
#define RQ_FILTER_GATHER_DIV 1
// The list fits while at most a quarter of the rows is allowed.  For a filter the scan cannot serve (below) that is also the choice
// between gathering and the exact scan: measured at B = 64, gather takes 2.35 ms at na = N / 4 (0.94 ms at N / 10) against the exact
// scan's 3.45 ms whatever na; extrapolated they meet near na = 0.37 N.
#define RQ_FILTER_LIST_DIV 4

// What plan_filter needs of a filter.
struct FilterShape {
    int64_t n = 0, na = 0;               // rows of the index the filter was made for, allowed rows
    const int32_t* occ_prefix = nullptr; // [bins + 1]: occ_prefix[b] = bins before b that hold at least one allowed row
};

// Partitions of the tail's threshold (rq_tail_body.h phase A) that hold an allowed row, for a scan grid of G workgroups:
// scan workgroup b owns bins [b * nquads / G, (b + 1) * nquads / G) (rq_scan_body.h), and partition p is the workgroups
// b = p (mod NP), NP = 64 / 256 / 512 by m.
static inline int filter_occupied_partitions(const FilterShape& f, int nquads, int G, int m) {
    const int NP = m <= 8 ? 64 : (m <= 64 ? 256 : 512);
    int count = 0;
    for (int p = 0; p < NP && p < G; ++p) {
        bool any = false;
        for (int b = p; b < G && !any; b += NP) {
            const int lo = (int)((int64_t)b * nquads / G), hi = (int)((int64_t)(b + 1) * nquads / G);
            any = f.occ_prefix[hi] > f.occ_prefix[lo];
        }
        count += any ? 1 : 0;
    }
    return count;
}

// forced: option "filter_route" (-1 = the rule).  *plan (optional) receives the call plan the scan route would run with.
static inline int plan_filter(const rq_index* idx, const FilterShape& f, int B, int k, int metric, int forced, CallPlan* plan = nullptr) {
    if (f.na <= 0) return FROUTE_EMPTY;
    CallPlan local;
    CallPlan& p = plan ? *plan : local;
    const int nb = nb_default(idx, k);
    // the plan of the scan route: never the int8 image, never deferred (flags 0)
    if (plan_call(idx, B, k, metric, nb, false, 0, &p) != RQ_OK) return FROUTE_EXACT;
    if (forced == FROUTE_GATHER || forced == FROUTE_EXACT) return forced;
    if (forced == FROUTE_SCAN) return p.exact ? FROUTE_EXACT : FROUTE_SCAN;
    const bool list_fits = f.na * RQ_FILTER_LIST_DIV <= f.n;
    // gather: cheaper than one scan pass (the measured constants above) ...
    if (list_fits && (int64_t)B * f.na * RQ_FILTER_GATHER_DIV <= f.n) return FROUTE_GATHER;
    // ... or the scan's own "fewer than two bins per wanted bin" rule over the bins that hold an allowed row
    const int64_t occ_bins = f.occ_prefix[p.nbins];
    if (2 * (int64_t)nb >= occ_bins) return FROUTE_GATHER;
    if (p.exact) return list_fits ? FROUTE_GATHER : FROUTE_EXACT;   // (a shard whose scan scores say nothing: rq_plan.h)
    if (p.fast) {
        // P is the m-th largest partition maximum: it bounds the m-th best allowed score only if at least m partitions of
        // every grid the call's passes use hold an allowed row
        const int m = (int)std::min<int64_t>(k, f.na);
        const int grid_narrow = scan_grid(idx, p.nquads, idx->wg_per_cu);
        bool ok = true;
        if (p.nwg_split > 0) ok = ok && filter_occupied_partitions(f, p.nquads, p.grid_wide, m) >= m;
        if (p.nwg_split < p.bpad) ok = ok && filter_occupied_partitions(f, p.nquads, grid_narrow, m) >= m;
        if (!ok) return list_fits ? FROUTE_GATHER : FROUTE_EXACT;
    }
    return FROUTE_SCAN;
}
