// rq_rowdot.h -- the fp64 dot product of stored fp16 rows with an fp32 vector in LDS, 16 lanes per row: the arithmetic shared by
// rq_gather_score_kernel (rq_filter.hip: a query against the listed rows), rq_mmr_kernel (rq_mmr.hip: the row just selected
// against the remaining candidates), rq_score_rows_kernel (rq_score.hip: a query against its own list) and rq_group_members_kernel
// (rq_group_members.hip: a query against the rows of a group).  Lane sub = lane & 15
// of a row's 16 lanes owns elements pp * 128 + 8 * sub + e (one 16-byte load per pp), the products are formed in fp64 and added
// in element order, then an xor butterfly over the 16 lanes.  The tail does NOT call this: rq_tail_body.h phase C keeps its own
// copy of the same summation order (a call changes the tail kernels' registers) -- one order, hence the same bits everywhere.
#pragma once
#include "rq_device.h"

// xv[u][pp]: the lane's 16 bytes of part pp of row u (U rows in flight per lane group); qs: the vector, fp32, 16-byte aligned.
// dot[u] receives the whole dot product of row u in every one of its 16 lanes.  Every lane of the wave must call it.
template <int NP, int U>
__device__ __forceinline__ void rq_rowdot16(const rq_half8 (&xv)[U][NP], const float* qs, int sub, double (&dot)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) dot[u] = 0.0;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        const float4 qlo = *(const float4*)&qs[pp * 128 + 8 * sub], qhi = *(const float4*)&qs[pp * 128 + 8 * sub + 4];
        const float qq[8] = {qlo.x, qlo.y, qlo.z, qlo.w, qhi.x, qhi.y, qhi.z, qhi.w};
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) dot[u] += (double)qq[e] * (double)(float)xv[u][pp][e];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) dot[u] += __shfl_xor(dot[u], off, 64);
}
