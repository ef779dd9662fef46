// rq_group_plan.h -- the host side of a grouped search (include/rq.h rq_index_set_groups, rq_group_collapse_device,
// rq_search_grouped*) that needs no device: the argument checks, how many rows each rung fetches, the launch geometry of
// rq_group_collapse_kernel and the bytes the blocking call stages.  Plain arithmetic in the manner of rq_mmr_plan.h: no HIP runtime
// call, nothing is written to the index (tests/native/group_plan_check.cpp runs it on the host).
#pragma once
#include "rq_plan.h"

#define RQ_GROUP_THREADS 512      // one workgroup per query: 8 waves, two of the RQ_MAX_K candidate slots per thread
#define RQ_GROUP_MIN_SORT 64      // the sort network never runs on fewer slots than one wave

// What rq_index_set_groups / rq_index_get_groups refuse: a range outside the stored rows, a null array, a multi-device index.  The
// values themselves (every id >= RQ_GROUP_NONE) are checked by check_group_ids.
static inline int check_group_range(const rq_index* idx, int64_t row_begin, int64_t n_rows, const void* groups) {
    if (!idx || (!groups && n_rows > 0)) return set_err(RQ_EINVAL, "null argument");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "RQ_EUNSUPPORTED: group ids on a multi-device index: use one index per device");
    if (row_begin < 0 || n_rows < 0 || row_begin > idx->n || n_rows > idx->n - row_begin)
        return set_err(RQ_EINVAL, "rows %lld .. +%lld outside the %lld stored rows", (long long)row_begin, (long long)n_rows, (long long)idx->n);
    return RQ_OK;
}
static inline int check_group_ids(const int32_t* groups, int64_t n_rows) {
    for (int64_t i = 0; i < n_rows; ++i)
        if (groups[i] < RQ_GROUP_NONE) return set_err(RQ_EINVAL, "group id %d of row %lld: ids are >= 0, or RQ_GROUP_NONE (-1)", (int)groups[i], (long long)i);
    return RQ_OK;
}

// What rq_group_collapse_device refuses (RQ_EINVAL unless noted).  The device pointers are only tested for null; cand_groups and
// keys may be null.
static inline int check_group_collapse_args(const rq_index* idx, const void* cand_rows, const void* cand_scores, int B, int m, int k, const void* scores,
                                            const void* rows, const void* groups, const void* status) {
    if (!idx || !cand_rows || !cand_scores || !scores || !rows || !groups || !status) return set_err(RQ_EINVAL, "null argument");
    if (m < 1 || m > RQ_MAX_K) return set_err(RQ_EINVAL, "m %d outside 1..%d", m, RQ_MAX_K);
    if (k < 1 || k > m) return set_err(RQ_EINVAL, "k %d outside 1..m = %d", k, m);
    return check_batch_metric(idx, B, RQ_METRIC_COSINE, "group collapse");   // (a collapse has no metric: the candidates carry their scores)
}

// ... and rq_search_grouped / _device / _fixup_device (the filter's own checks are rq_filter.hip's check_filter).
static inline int check_group_search_args(const rq_index* idx, const void* queries, int B, int k, int metric, const void* scores, const void* rows,
                                          const void* groups) {
    if (!idx || !queries || !scores || !rows || !groups) return set_err(RQ_EINVAL, "null argument");
    if (k < 1 || k > RQ_MAX_K) return set_err(RQ_EINVAL, "k %d outside 1..%d", k, RQ_MAX_K);
    return check_batch_metric(idx, B, metric, "grouped searches");
}

// The largest m a rung may ask for: option "group_fetch_cap" (0 = RQ_MAX_K), the rows in play -- but never fewer than k, the width
// of the outputs (the search pads with (0.0, -1), which the collapse takes as absent).  rows_in_play: the rows of the index, or the
// allowed rows of the filter.
static inline int group_max_fetch(int k, int cap, int64_t rows_in_play) {
    const int64_t hi = std::min<int64_t>(rows_in_play, cap > 0 ? std::min(cap, RQ_MAX_K) : RQ_MAX_K);
    return (int)std::max<int64_t>(k, hi);
}
// Rows per query the FIRST rung searches for: option "group_fetch" x k, clamped to [k, group_max_fetch].
static inline int group_fetch(int k, int mult, int cap, int64_t rows_in_play) {
    const int64_t want = (int64_t)k * (int64_t)std::max(mult, 1);
    return (int)std::max<int64_t>(k, std::min<int64_t>(want, group_max_fetch(k, cap, rows_in_play)));
}

struct GroupGeometry {
    unsigned grid = 0, block = RQ_GROUP_THREADS;   // one workgroup per query
    int sort_n = 0;                                // slots of the sort network: the power of two >= max(m, RQ_GROUP_MIN_SORT)
    size_t lds_bytes = 0;                          // a key and a group id per slot
};
static inline GroupGeometry group_geometry(int B, int m) {
    GroupGeometry g;
    g.grid = (unsigned)B;
    g.sort_n = RQ_GROUP_MIN_SORT;
    while (g.sort_n < m) g.sort_n *= 2;
    g.lds_bytes = (size_t)g.sort_n * (sizeof(uint64_t) + sizeof(int32_t));
    return g;
}

// Device bytes of a grouped call (64-bit throughout): what the blocking rq_search_grouped stages (q, out_*, status) and what the
// device form keeps per stream for its candidates (cand_*: the search for m rows).
struct GroupStaging { size_t q = 0, cand_scores = 0, cand_rows = 0, cand_status = 0, out_scores = 0, out_rows = 0, out_groups = 0, out_keys = 0, status = 0; };
static inline GroupStaging group_staging(int dim, int B, int m, int k) {
    const SearchStaging cand = search_staging(dim, B, m), out = search_staging(dim, B, k);
    GroupStaging s;
    s.q = cand.q; s.cand_scores = cand.scores; s.cand_rows = cand.rows; s.cand_status = cand.status;
    s.out_scores = out.scores; s.out_rows = out.rows; s.out_groups = (size_t)B * (size_t)k * sizeof(int32_t); s.out_keys = out.rows; s.status = out.status;
    return s;
}
