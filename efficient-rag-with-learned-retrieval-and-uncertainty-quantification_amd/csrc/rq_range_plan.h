// rq_range_plan.h -- the host side of a range search (include/rq.h rq_search_range*) that needs no device: the argument checks,
// the route, the groups of queries a call is cut into, the candidate capacity of a query and the bytes the blocking call stages.
// Plain arithmetic in the manner of rq_filter_plan.h: no HIP runtime call, nothing is written to the index or to the filter
// (tests/native/range_plan_check.cpp runs it on the host).  Results never depend on the route: every route returns the exact
// count and the best min(count, cap) qualifying rows.
#pragma once
#include "rq_filter_plan.h"

enum RangeRoute {
    RROUTE_EMPTY = 0,    // an empty index, or a filter that allows no row: counts 0, the outputs are padding
    RROUTE_SCAN = 1,     // the fp16 scan passes, then the range tail: only the bins whose record cannot prove "no row reaches thr" are re-scored
    RROUTE_GATHER = 2,   // filtered calls: the listed rows re-scored (rq_gather_score_kernel), cost B x na
    RROUTE_EXACT = 3,    // the exact fp64 scan of the whole shard (rq_exact_scan_kernel), keys below the threshold emptied
};

#define RQ_RANGE_GROUP 1024        // queries per pass of the scan route: records, candidate keys and prepared queries stay bounded
#define RQ_RANGE_CAND_CAP 4096     // default candidate keys per query (as the fast tail's RQ_CAND_CAP): 32 KiB a query
#define RQ_RANGE_CHUNK 2048        // bin records one workgroup of the range tail walks

// What every entry point refuses (RQ_EINVAL unless noted).  thr: the thresholds where the host can see them (the blocking form),
// else null -- a non-finite d_thr[q] then makes that query return nothing (include/rq.h).
static inline int check_range_args(const rq_index* idx, const void* queries, int B, const void* d_or_h_thr, const float* host_thr, int cap, int metric,
                                   const void* scores, const void* rows, const void* count) {
    if (!idx || !queries || !d_or_h_thr || !scores || !rows || !count) return set_err(RQ_EINVAL, "null argument");
    if (cap < 1 || cap > RQ_MAX_K) return set_err(RQ_EINVAL, "cap %d outside 1..%d", cap, RQ_MAX_K);
    if (int r = check_batch_metric(idx, B, metric, "range searches")) return r;
    if (host_thr)
        for (int q = 0; q < B; ++q)
            if (!(host_thr[q] - host_thr[q] == 0.f)) return set_err(RQ_EINVAL, "threshold %d is not finite", q);
    return RQ_OK;
}

// Qualifying rows a query of the scan route may hold before it overflows (status 1: the fixup re-runs it on the exact route).
// forced: option "range_cand_cap" (0 = the default).  Never below cap: a query that does not overflow has every qualifying row
// in its list, and one that holds cap of them must be able to return them.
static inline int range_cand_capacity(int cap, int forced) { return std::max(cap, forced > 0 ? forced : RQ_RANGE_CAND_CAP); }

// forced: option "range_route" (-1 = the rule).  f: the call's filter or null.
static inline int plan_range(const rq_index* idx, const FilterShape* f, int B, int metric, int forced, CallPlan* plan = nullptr) {
    if (idx->n <= 0 || (f && f->na <= 0)) return RROUTE_EMPTY;
    CallPlan local;
    CallPlan& p = plan ? *plan : local;
    // the plan of the scan route: never the int8 image, never deferred (flags 0); nb = 0, k = 1: no bin is wanted for a top-k, so
    // p.exact says only whether the scan's scores say anything (the eps reason of rq_plan.h)
    if (plan_call(idx, std::min(B, RQ_RANGE_GROUP), 1, metric, 0, false, 0, &p) != RQ_OK) return RROUTE_EXACT;
    if (forced == RROUTE_EXACT) return RROUTE_EXACT;
    if (forced == RROUTE_GATHER) return f ? RROUTE_GATHER : (p.exact ? RROUTE_EXACT : RROUTE_SCAN);   // (unfiltered calls have no list)
    if (forced == RROUTE_SCAN) return p.exact ? RROUTE_EXACT : RROUTE_SCAN;
    // gather: the measured rule of plan_filter (rq_filter_plan.h): the list fits and costs less than one scan pass
    if (f && f->na * RQ_FILTER_LIST_DIV <= f->n && (int64_t)B * f->na * RQ_FILTER_GATHER_DIV <= f->n) return RROUTE_GATHER;
    return p.exact ? RROUTE_EXACT : RROUTE_SCAN;
}

// The call's queries in groups: group i = queries [i * group, min(B, (i + 1) * group)).  The scan route takes RQ_RANGE_GROUP
// queries a pass; the routes that hold keys_per_query keys for every query (exact: ceil(n / 64) * 64, gather: na) as many as
// keep them within 1 GiB (queries_per_gib).
struct RangeGroups { int group = 0, count = 0; };
static inline RangeGroups range_groups(int route, int B, int64_t keys_per_query) {
    RangeGroups g;
    g.group = route == RROUTE_SCAN ? std::min(B, RQ_RANGE_GROUP) : std::min(queries_per_gib(B, keys_per_query), RQ_RANGE_GROUP);
    g.count = (B + g.group - 1) / g.group;
    return g;
}

// Workgroups of the range tail: (queries of the group, chunks of RQ_RANGE_CHUNK bins).
static inline unsigned range_chunks(int64_t nbins) { return (unsigned)((nbins + RQ_RANGE_CHUNK - 1) / RQ_RANGE_CHUNK); }

// Device bytes the blocking rq_search_range stages: B x (dim x 4 + 4 + cap x 12 + 8 + 4) (64-bit throughout).
struct RangeStaging {
    size_t q = 0, thr = 0, scores = 0, rows = 0, count = 0, status = 0;
    size_t total() const { return q + thr + scores + rows + count + status; }
};
static inline RangeStaging range_staging(int dim, int B, int cap) {
    const size_t b = (size_t)B, bc = b * (size_t)cap;
    RangeStaging s;
    s.q = b * (size_t)dim * sizeof(float); s.thr = b * sizeof(float);
    s.scores = bc * sizeof(float); s.rows = bc * sizeof(int64_t); s.count = b * sizeof(int64_t); s.status = b * sizeof(int);
    return s;
}
