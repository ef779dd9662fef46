// rq_group_members_plan.h -- the host side of a group-members call (include/rq.h rq_group_fill_device, rq_search_group_members*)
// that needs no device: the argument checks, the group member table built from the index's host copy of the group ids, the launch
// geometry of rq_group_members_kernel (grid, sort slots, LDS bytes) and the bytes the blocking call stages.  Plain arithmetic in the
// manner of rq_group_plan.h: no HIP runtime call, nothing is written to the index (tests/native/group_members_plan_check.cpp runs it
// on the host).
#pragma once
#include "rq_group_plan.h"

#define RQ_GROUP_FILL_THREADS 256     // 4 waves; 16 lanes per row, two rows in flight per lane group: 32 members per round
// RQ_GROUP_FILL_MAX (include/rq.h): members one workgroup can sort in LDS, 4096 keys = 32 KiB (structural, not tuned)
#define RQ_GROUP_FILL_MIN_SORT 64     // the sort network never runs on fewer slots than one wave

// What rq_group_fill_device / rq_search_group_members* refuse (RQ_EINVAL unless noted): the pointers are only tested for null (the
// caller passes every required one; f is checked by rq_filter.hip's check_filter).  k x s in 64 bits.
static inline int check_group_members_args(const rq_index* idx, const void* queries, int B, int k, int s, int metric, const void* a0, const void* a1, const void* a2,
                                           const void* a3, const void* a4) {
    if (!idx || !queries || !a0 || !a1 || !a2 || !a3 || !a4) return set_err(RQ_EINVAL, "null argument");
    if (k < 1 || s < 1 || (int64_t)k * (int64_t)s > RQ_MAX_K) return set_err(RQ_EINVAL, "k %d x group size %d outside 1..%d", k, s, RQ_MAX_K);
    return check_batch_metric(idx, B, metric, "group members");
}

// ---- the group member table -----------------------------------------------------------------------------------------------------
// The rows with id >= 0 sorted by (id, row); beside them the sorted distinct ids and where each id's rows begin: the rows of
// ids[i] are rows[off[i] .. off[i + 1]).  Ids need not be dense: the kernel finds a group's range by binary search over ids.
// Bytes, host and HBM alike: 4 per grouped row + 8 per distinct group (+ 4).  largest = rows of the largest group.
struct GroupTable {
    std::vector<int32_t> ids;     // [groups] ascending, distinct
    std::vector<uint32_t> off;    // [groups + 1] (a shard holds fewer than 2^32 - 1 rows)
    std::vector<uint32_t> rows;   // [grouped rows] local rows
    int64_t largest = 0;
};
static inline void group_table_build(const int32_t* groups, int64_t n, GroupTable& t) {
    t.ids.clear(); t.off.clear(); t.rows.clear(); t.largest = 0;
    std::vector<uint64_t> pairs;
    for (int64_t r = 0; r < n; ++r)
        if (groups[r] >= 0) pairs.push_back(((uint64_t)(uint32_t)groups[r] << 32) | (uint64_t)(uint32_t)r);
    std::sort(pairs.begin(), pairs.end());
    t.rows.reserve(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
        const int32_t g = (int32_t)(pairs[i] >> 32);
        if (i == 0 || g != t.ids.back()) { t.ids.push_back(g); t.off.push_back((uint32_t)i); }
        t.rows.push_back((uint32_t)(pairs[i] & 0xffffffffu));
    }
    t.off.push_back((uint32_t)pairs.size());
    for (size_t i = 0; i + 1 < t.off.size(); ++i) t.largest = std::max<int64_t>(t.largest, (int64_t)t.off[i + 1] - (int64_t)t.off[i]);
}
// The lookup the kernel does: index of id g in the sorted ids, -1 = no row carries it.
static inline int64_t group_table_find(const int32_t* ids, int64_t n_ids, int32_t g) {
    int64_t lo = 0, hi = n_ids;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo < n_ids && ids[lo] == g ? lo : -1;
}

// Option "group_fill_cap": rows a group may have in the table and still be filled by the kernel; it can only lower the maximum.
static inline int group_fill_cap(int option) { return option > 0 && option < RQ_GROUP_FILL_MAX ? option : RQ_GROUP_FILL_MAX; }

struct GroupFillGeometry {
    unsigned grid_x = 0, grid_y = 0, block = RQ_GROUP_FILL_THREADS;   // (group slots, queries): one workgroup per (query, slot)
    int sort_n = 0;          // slots of the LDS sort: the power of two >= max(min(largest group, cap), RQ_GROUP_FILL_MIN_SORT)
    size_t lds_bytes = 0;    // dynamic LDS: the query's RQ_DPAD floats, then one key per slot
};
static inline GroupFillGeometry group_fill_geometry(int B, int k, int64_t largest_group, int cap) {
    GroupFillGeometry g;
    g.grid_x = (unsigned)k;
    g.grid_y = (unsigned)B;
    const int64_t hold = std::min<int64_t>(std::max<int64_t>(largest_group, 1), group_fill_cap(cap));
    g.sort_n = RQ_GROUP_FILL_MIN_SORT;
    while (g.sort_n < hold) g.sort_n *= 2;
    g.lds_bytes = RQ_DPAD * sizeof(float) + (size_t)g.sort_n * sizeof(uint64_t);
    return g;
}

// Device bytes of a group-members call (64-bit throughout): what the blocking rq_search_group_members stages, and the winners
// ([B][k] scores and rows) the device form keeps per stream.
struct GroupMembersStaging { size_t q = 0, scores = 0, rows = 0, groups = 0, count = 0, status = 0, win_scores = 0, win_rows = 0; };
static inline GroupMembersStaging group_members_staging(int dim, int B, int k, int s) {
    GroupMembersStaging z;
    const size_t slots = (size_t)B * (size_t)k;
    z.q = (size_t)B * (size_t)dim * sizeof(float);
    z.scores = slots * (size_t)s * sizeof(float);
    z.rows = slots * (size_t)s * sizeof(int64_t);
    z.groups = slots * sizeof(int32_t);
    z.count = slots * sizeof(int32_t);
    z.status = (size_t)B * sizeof(int);
    z.win_scores = slots * sizeof(float);
    z.win_rows = slots * sizeof(int64_t);
    return z;
}
