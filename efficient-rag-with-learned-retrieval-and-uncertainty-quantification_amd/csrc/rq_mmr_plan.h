// rq_mmr_plan.h -- the host side of an MMR selection (include/rq.h rq_mmr_select_device, rq_search_mmr) that needs no device:
// the argument checks, how many candidates rq_search_mmr fetches, the launch geometry of rq_mmr_kernel and the bytes the blocking
// call stages.  Plain arithmetic in the manner of rq_filter_plan.h: no HIP runtime call, nothing is written to the index
// (tests/native/mmr_check.cpp runs it on the host).
#pragma once
#include "rq_plan.h"

#define RQ_MMR_THREADS 512                        // one workgroup per query: 8 waves
#define RQ_MMR_ROWS_PER_ROUND (RQ_MMR_THREADS / 16 * 2)   // 16 lanes per candidate row, two rows in flight per lane group

// What rq_mmr_select_device refuses (RQ_EINVAL unless noted).  The device pointers are only tested for null.
static inline int check_mmr_select_args(const rq_index* idx, const void* cand_rows, const void* cand_rel, int B, int m, int k, double lambda, int metric,
                                        const void* scores, const void* rows) {
    if (!idx || !cand_rows || !cand_rel || !scores || !rows) return set_err(RQ_EINVAL, "null argument");
    if (m < 1 || m > RQ_MAX_K) return set_err(RQ_EINVAL, "m %d outside 1..%d", m, RQ_MAX_K);
    if (k < 1 || k > m) return set_err(RQ_EINVAL, "k %d outside 1..m = %d", k, m);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return set_err(RQ_EINVAL, "lambda %g outside [0, 1]", lambda);   // (NaN fails both comparisons)
    return check_batch_metric(idx, B, metric, "MMR selection");
}

// ... and rq_search_mmr (the filter's own checks are rq_filter.hip's check_filter).
static inline int check_mmr_search_args(const rq_index* idx, const void* queries, int B, int k, int fetch_k, double lambda, int metric, const void* scores,
                                        const void* rows) {
    if (!idx || !queries || !scores || !rows) return set_err(RQ_EINVAL, "null argument");
    if (fetch_k < 1 || fetch_k > RQ_MAX_K) return set_err(RQ_EINVAL, "fetch_k %d outside 1..%d", fetch_k, RQ_MAX_K);
    if (k < 1 || k > fetch_k) return set_err(RQ_EINVAL, "k %d outside 1..fetch_k = %d", k, fetch_k);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return set_err(RQ_EINVAL, "lambda %g outside [0, 1]", lambda);
    return check_batch_metric(idx, B, metric, "MMR searches");
}

// Candidates per query that rq_search_mmr searches for and hands to the selection: min(fetch_k, rows in play), but never fewer
// than k, the width of the outputs (the search pads with (0.0, -1), which the selection takes as absent).  rows_in_play: the rows
// of the index, or the allowed rows of the filter.
static inline int mmr_fetch(int k, int fetch_k, int64_t rows_in_play) {
    return (int)std::max<int64_t>(k, std::min<int64_t>(fetch_k, rows_in_play));
}

struct MmrGeometry {
    unsigned grid = 0, block = RQ_MMR_THREADS;   // one workgroup per query
    int rounds = 0;                              // passes of RQ_MMR_ROWS_PER_ROUND candidate rows per penalty update
    int dp = 0;                                  // instantiation: stored row length in elements
};
static inline MmrGeometry mmr_geometry(const rq_index* idx, int B, int m) {
    MmrGeometry g;
    g.grid = (unsigned)B;
    g.rounds = (m + RQ_MMR_ROWS_PER_ROUND - 1) / RQ_MMR_ROWS_PER_ROUND;
    g.dp = idx->dpad;
    return g;
}

// Device bytes the blocking rq_search_mmr stages (64-bit throughout: B x m x 8 alone reaches 512 MiB at the limits).
struct MmrStaging { size_t q = 0, cand_scores = 0, cand_rows = 0, status = 0, out_scores = 0, out_rows = 0, out_mmr = 0; };
static inline MmrStaging mmr_staging(int dim, int B, int m, int k) {
    const SearchStaging cand = search_staging(dim, B, m), out = search_staging(dim, B, k);   // the search for m candidates, the k selected
    MmrStaging s;
    s.q = cand.q; s.cand_scores = cand.scores; s.cand_rows = cand.rows; s.status = cand.status;
    s.out_scores = out.scores; s.out_rows = out.rows; s.out_mmr = out.scores;
    return s;
}
