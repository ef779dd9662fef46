// rq_gather_body.h -- one workgroup's share of a gather: the exact fp64 re-score of 256 listed rows for one query.  Shared by
// rq_gather_score_kernel (rq_filter.hip: one list for every query of the launch) and rq_gather_ragged_kernel (rq_filter_each.hip:
// a list per query), so that a (query, row) pair gets the same bits from both.  The arithmetic of one row is rq_tail_body.h phase
// C's: 16 lanes per row (sub = lane & 15 owns elements pp * 128 + 8 * sub + e), a wave takes 8 rows per round, fp64 products in
// element order, xor butterfly over the 16 lanes (rq_rowdot.h).
#pragma once
#include "rq_rowdot.h"

// All 256 threads.  q32: the query's padded fp32 row (rq_prep_body); qs: RQ_DPAD floats of LDS, 16-byte aligned; list / nlist: the
// listed local rows (nlist >= 1; every listed row is below the shard's end); base: first list position of the chunk;
// out[j] = key(score(query, list[j]), list[j]) for base <= j < min(base + 256, nlist).  A lane beyond the list reads entry 0;
// every store is predicated.
template <int DP>
__device__ __forceinline__ void rq_gather_chunk(const void* x, const double* rownorm64, const float* q32, const double qn, const uint32_t* list,
                                                const int64_t nlist, const int64_t base, const int metric, uint64_t* out, float* qs) {
    static_assert(DP == 384 || DP == RQ_DPAD, "stored row length");
    constexpr int NP = DP / 128;   // 16-byte loads per lane and row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) qs[pp * 256 + tid] = q32[pp * 256 + tid];
    __syncthreads();
    const int sub = lane & 15, rloc = lane >> 4;
    const char* xb = (const char*)x;
    for (int j0 = wave * 8; j0 < 256; j0 += 32) {
        if (base + j0 >= nlist) break;   // uniform over the wave
        rq_half8 xv[2][NP];
        int64_t rows[2], slot[2];
        double rn[2];
        bool lv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            slot[u] = base + j0 + u * 4 + rloc;
            lv[u] = slot[u] < nlist;
            rows[u] = (int64_t)list[lv[u] ? slot[u] : 0];   // (nlist >= 1; every listed row is below the shard's end)
            rn[u] = rownorm64[rows[u]];
            const char* r = xb + rows[u] * (DP * 2) + sub * 16;
#pragma unroll
            for (int pp = 0; pp < NP; ++pp) xv[u][pp] = *(const rq_half8*)(r + pp * 256);
        }
        double dot[2];
        rq_rowdot16<NP, 2>(xv, qs, sub, dot);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double d = dot[u];
            if (sub == 0 && lv[u]) {
                double sc = d;
                if (metric == 0) sc = d / (qn * rn[u] + 1e-30);
                if (qn == 0.0) sc = 0.0;   // a zero-norm query scores every row 0 (include/rq.h).  For consistency of the keys only:
                                           // rq_final_kernel answers such a query (RqFinalArgs::first) before it reads them
                out[slot[u]] = rq_make_key(rq_sanitize((float)sc), (uint32_t)rows[u]);
            }
        }
    }
}
