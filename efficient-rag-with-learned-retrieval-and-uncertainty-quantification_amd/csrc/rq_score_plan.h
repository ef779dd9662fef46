// rq_score_plan.h -- the host side of a scoring call (include/rq.h rq_score_rows_device, rq_score_rows) that needs no device: the
// argument checks, the groups of queries a call is cut into, the launch geometry of rq_score_rows_kernel and the bytes the
// blocking call stages.  Plain arithmetic in the manner of rq_mmr_plan.h: no HIP runtime call, nothing is written to the index
// (tests/native/score_plan_check.cpp runs it on the host).
#pragma once
#include "rq_plan.h"

#define RQ_SCORE_THREADS 256                      // 4 waves; 16 lanes per row, two rows in flight per lane group: 32 positions per round
#ifndef RQ_SCORE_TILE
#define RQ_SCORE_TILE 64                          // list positions per workgroup: two rounds per wave (measured; -D: the A/B of tiles)
#endif
#define RQ_SCORE_GROUP 1024                       // queries per launch: the stream's prepared-query slots stay at 1 024 x 768 x 6 bytes

// What both entry points refuse (RQ_EINVAL unless noted).  The pointers are only tested for null.
static inline int check_score_args(const rq_index* idx, const void* queries, int B, const void* rows, int m, int metric, const void* scores) {
    if (!idx || !queries || !rows || !scores) return set_err(RQ_EINVAL, "null argument");
    if (m < 1 || m > RQ_MAX_SCORE_ROWS) return set_err(RQ_EINVAL, "m %d outside 1..%d", m, RQ_MAX_SCORE_ROWS);
    return check_batch_metric(idx, B, metric, "scoring given rows");
}

// The call's queries in groups of at most RQ_SCORE_GROUP: group i = queries [i * group, min(B, (i + 1) * group)); every group is
// prepared into the same `slots` prepared-query slots (a multiple of 64, as every workspace of the stream).
struct ScoreGroups { int group = 0, count = 0, slots = 0; };
static inline ScoreGroups score_groups(int B) {
    ScoreGroups g;
    g.group = std::min(B, RQ_SCORE_GROUP);
    g.count = (B + g.group - 1) / g.group;
    g.slots = (g.group + 63) / 64 * 64;
    return g;
}

struct ScoreGeometry {
    unsigned grid_x = 0, grid_y = 0, block = RQ_SCORE_THREADS;   // (queries of the group, tiles of the list)
    int dp = 0;                                                  // instantiation: stored row length in elements
};
static inline ScoreGeometry score_geometry(const rq_index* idx, int queries, int m) {
    ScoreGeometry g;
    g.grid_x = (unsigned)queries;
    g.grid_y = (unsigned)((m + RQ_SCORE_TILE - 1) / RQ_SCORE_TILE);
    g.dp = idx->dpad;
    return g;
}

// Device bytes the blocking rq_score_rows stages: B x dim x 4 + B x m x 12 (64-bit throughout: B x m x 8 alone reaches 32 GiB at
// the limits).
struct ScoreStaging {
    size_t q = 0, rows = 0, scores = 0;
    size_t total() const { return q + rows + scores; }
};
static inline ScoreStaging score_staging(int dim, int B, int m) {
    ScoreStaging s;
    s.q = (size_t)B * (size_t)dim * sizeof(float);
    s.rows = (size_t)B * (size_t)m * sizeof(int64_t);
    s.scores = (size_t)B * (size_t)m * sizeof(float);
    return s;
}
