// rq_router_plan.h -- the host side of the router gate (include/rq.h rq_router_*) that needs no device: what rq_router_create
// refuses and the widened weight table it builds, the checks of a call's arguments, the instantiation of the kernel chosen by the
// column length, its threads, the length of the summation tree and the LDS bytes.  Plain arithmetic in the manner of
// rq_hybrid_plan.h: no HIP runtime call, nothing is written outside what the caller hands in
// (tests/native/router_plan_check.cpp runs it on the host).
#pragma once
#include "rq_index.h"

#define RQ_ROUTER_MIN_PAD 64                      // the smallest instantiation: one wave
#define RQ_ROUTER_MAX_THREADS 256
#define RQ_ROUTER_ROW 5                           // doubles per hidden unit: W0[j][0..2], b0[j], w1[j]

// What rq_router_create refuses: batch norm and more than two layers (no such router is ever built), a hidden width outside
// 1 .. RQ_ROUTER_MAX_HIDDEN, null weights.  On success `table` holds the weights widened to float64 in the layout the kernel
// copies to LDS: num_layers 2: [hidden][RQ_ROUTER_ROW]; num_layers 1: w1[0..2].  The bias of the last layer travels by value.
static inline int router_check_create(int num_layers, int hidden, int use_batch_norm, const float* w0, const float* b0, const float* w1, std::vector<double>& table) {
    if (use_batch_norm) return set_err(RQ_EINVAL, "use_batch_norm: a router with batch norm is not supported");
    if (num_layers < 1 || num_layers > 2) return set_err(RQ_EINVAL, "num_layers %d outside 1..2", num_layers);
    if (!w1) return set_err(RQ_EINVAL, "null w1");
    if (num_layers == 1) {
        table.assign(w1, w1 + 3);
        return RQ_OK;
    }
    if (hidden < 1 || hidden > RQ_ROUTER_MAX_HIDDEN) return set_err(RQ_EINVAL, "hidden %d outside 1..%d", hidden, RQ_ROUTER_MAX_HIDDEN);
    if (!w0 || !b0) return set_err(RQ_EINVAL, "null w0 or b0");
    table.resize((size_t)hidden * RQ_ROUTER_ROW);
    for (int j = 0; j < hidden; ++j) {
        double* row = &table[(size_t)j * RQ_ROUTER_ROW];
        row[0] = (double)w0[3 * j]; row[1] = (double)w0[3 * j + 1]; row[2] = (double)w0[3 * j + 2];
        row[3] = (double)b0[j];
        row[4] = (double)w1[j];
    }
    return RQ_OK;
}

// Both calls (pointers are only tested for null; the statistics are four doubles in HOST memory, needed in the STATS mode only).
static inline int router_check_columns(const void* r, const void* b, const void* d, int B, int P, int mode, const void* stats) {
    if (!r) return set_err(RQ_EINVAL, "null handle");
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (P < 1 || P > RQ_MAX_K) return set_err(RQ_EINVAL, "P %d outside 1..%d", P, RQ_MAX_K);
    if (mode != RQ_ROUTER_NORM_STATS && mode != RQ_ROUTER_NORM_QUERY) return set_err(RQ_EINVAL, "unknown normalisation mode %d", mode);
    if (mode == RQ_ROUTER_NORM_STATS && !stats) return set_err(RQ_EINVAL, "RQ_ROUTER_NORM_STATS without statistics");
    if (!b || !d) return set_err(RQ_EINVAL, "null score column");
    return RQ_OK;
}
static inline int router_check_gate(const void* r, const void* b, const void* d, int B, int P, int mode, const void* stats, const void* w) {
    if (int rc = router_check_columns(r, b, d, B, P, mode, stats)) return rc;
    if (!w) return set_err(RQ_EINVAL, "null output");
    return RQ_OK;
}
static inline int router_check_rerank(const void* r, const void* keys, const void* b, const void* d, const void* count, int B, int P, int mode, const void* stats,
                                      int top_r, const void* out_keys, const void* out_b, const void* out_d, const void* out_w, const void* out_h, const void* out_pos,
                                      const void* out_count) {
    if (int rc = router_check_columns(r, b, d, B, P, mode, stats)) return rc;
    if (!keys || !count) return set_err(RQ_EINVAL, "null keys or count");
    if (top_r < 1 || top_r > P) return set_err(RQ_EINVAL, "top_r %d outside 1..P = %d", top_r, P);
    if (!out_keys || !out_b || !out_d || !out_w || !out_h || !out_pos || !out_count) return set_err(RQ_EINVAL, "null output");
    return RQ_OK;
}

// The kernel is instantiated for `pad` slots, P rounded up to a power of two in 64 .. 1 024; threads as in rq_hybrid_plan.h.
static inline int router_pad(int P) {
    int p = RQ_ROUTER_MIN_PAD;
    while (p < P) p <<= 1;
    return p;   // P <= RQ_MAX_K by router_check_columns
}
static inline int router_threads(int pad) { return std::max(64, std::min(RQ_ROUTER_MAX_THREADS, pad / 2)); }
// The summation tree S of the definition runs over P padded with +0.0 to the NEXT power of two -- not to `pad`: a column of 3 is
// summed as (x0 + x2) + (x1 + 0.0) whatever the instantiation, so the bits do not depend on it.
static inline int router_tree(int P) {
    int n = 1;
    while (n < P) n <<= 1;
    return n;
}
// LDS of one workgroup.  Both forms: b, d, and the two arrays of the tree sums (8 B per slot each; the rank form reuses them for
// the sort keys and the weights), the weight table at its largest.  The rank form also: the position that travels with the sort.
static inline size_t router_lds_bytes(int pad, bool rank) {
    return (size_t)pad * (rank ? 32 + 4 : 32) + (size_t)RQ_ROUTER_MAX_HIDDEN * RQ_ROUTER_ROW * 8;
}
