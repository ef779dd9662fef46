// rq_sparse_handle.h -- the rq_sparse object (include/rq.h "sparse search"): the device copy of the posting index and what a handle
// remembers between calls.  Shared by csrc/rq_sparse.hip (create, destroy, top-k, options) and csrc/rq_hybrid.hip (rq_sparse_score_rows*).
#pragma once
#include "rq_sparse_plan.h"

struct rq_sparse {
    int device = 0;
    int64_t n_tokens = 0, n_docs = 0, nnz = 0;
    int64_t* d_indptr = nullptr;
    int32_t* d_rows = nullptr;
    double* d_contrib = nullptr;
    hipStream_t own = nullptr;
    char* ws = nullptr;                   // the one workspace (rq_sparse_plan.h SparsePlan)
    size_t ws_bytes = 0;
    unsigned long long* d_skipped = nullptr;   // [3]: tiles of the last call without a posting, tiles whose mask allows no document,
                                               //      the largest chunk count of a grouped call's final kernel
    int32_t* d_groups = nullptr;          // [n_docs], rq_sparse_set_groups (null: no table)
    bool grouped_lds_set = false;         // the grouped tile kernels may take their 96 KiB of dynamic LDS
    int64_t grouped_calls = 0;            // rq_sparse_topk_grouped* (counted in calls too, and in masked_calls when they carry masks)
    int tile_docs = RQ_SPARSE_TILE_DEFAULT;
    int64_t cand_cap = 0;
    int64_t calls = 0, rounds_last = 0, tiles_last = 0;
    int64_t masked_calls = 0;             // rq_sparse_topk_masked* (counted in calls too)
    int64_t score_calls = 0;              // rq_sparse_score_rows* (csrc/rq_hybrid.hip)
    // option "profile": HIP events before a call's first launch and after every launch; "tile_ms_last" / "final_ms_last" sum them
    int profile = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;           // events the last profiled call recorded: 1 + 2 x rounds (0: none)
};
