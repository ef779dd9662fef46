// rq_sparse_select.h -- the one selection body of the sparse kernels (rq_sparse.hip): the exact cut "the `want` best of these
// candidates" for a workgroup of 256 threads, used by the tile kernel over its LDS accumulator and by the final kernel over the
// tiles' candidates in the workspace.
//
// A candidate is a positive float64 score and a row.  Positive doubles, +inf included, order as their uint64 bit patterns, and a
// row occurs once, so the composite key (score bits, row) -- 96 bits, larger = better: higher score first, equal scores by
// DESCENDING row -- is unique.  The `want`-th largest key is therefore an exact threshold: exactly `want` candidates have a key at
// or above it, also when the cut falls inside a run of equal scores.  It is found by a radix select, most significant byte first:
// a 256-bin histogram in LDS of the candidates that match the prefix found so far, a suffix scan by the first wave, one digit per
// pass, twelve passes at the most.  A pass in which every candidate that matches the new prefix is wanted ends the search early
// (the remaining digits are then zero: the threshold lies at or below all of them and above everything that was cut off).
// No sort of the candidates, no dependence on the order in which threads arrive: the histogram holds counts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SparseSelShared {
    unsigned hist[256];
    unsigned digit, want, cnt;
};

// (hi, lo) >= (thi, tlo)
__device__ __forceinline__ bool sparse_key_ge(uint64_t hi, uint32_t lo, uint64_t thi, uint32_t tlo) { return hi > thi || (hi == thi && lo >= tlo); }

// Src: int64_t size(); bool get(int64_t i, uint64_t& hi, uint32_t& lo) -- false = position i holds no candidate.
// Every thread of the workgroup (256) calls it with the same arguments; at least `want` >= 1 candidates exist.  On return every
// thread holds the threshold.
template <class Src>
__device__ inline void sparse_select_threshold(const Src& src, unsigned want, SparseSelShared& sh, uint64_t& thr_hi, uint32_t& thr_lo) {
    const int tid = (int)threadIdx.x;
    const int64_t n = src.size();
    uint64_t pre_hi = 0;
    uint32_t pre_lo = 0;
    for (int pass = 0; pass < 12; ++pass) {
        sh.hist[tid] = 0;
        __syncthreads();
        // bits above this pass's digit: `above` of hi (passes 0..7), all of hi and `above - 64` of lo (passes 8..11)
        const int above = pass * 8;
        for (int64_t i = tid; i < n; i += 256) {
            uint64_t hi;
            uint32_t lo;
            if (!src.get(i, hi, lo)) continue;
            unsigned d;
            if (pass < 8) {
                if (pass > 0 && (hi >> (64 - above)) != (pre_hi >> (64 - above))) continue;
                d = (unsigned)(hi >> (56 - above)) & 255u;
            } else {
                if (hi != pre_hi) continue;
                const int la = above - 64;
                if (la > 0 && (lo >> (32 - la)) != (pre_lo >> (32 - la))) continue;
                d = (lo >> (24 - la)) & 255u;
            }
            atomicAdd(&sh.hist[d], 1u);
        }
        __syncthreads();
        if (tid < 64) {   // the first wave: lane L owns the digits 255 - 4L .. 252 - 4L, best first
            const int top = 255 - 4 * tid;
            const unsigned c0 = sh.hist[top], c1 = sh.hist[top - 1], c2 = sh.hist[top - 2], c3 = sh.hist[top - 3];
            const unsigned own = c0 + c1 + c2 + c3;
            unsigned inc = own;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(inc, o, 64);
                if (tid >= o) inc += v;
            }
            const unsigned before = inc - own;
            if (before < want && want <= inc) {   // one lane: the digit that holds the want-th best
                unsigned w = want - before, c = c0;
                int d = top;
                if (w > c) { w -= c; --d; c = c1; if (w > c) { w -= c; --d; c = c2; if (w > c) { w -= c; --d; c = c3; } } }
                sh.digit = (unsigned)d;
                sh.want = w;
                sh.cnt = c;
            }
        }
        __syncthreads();
        const unsigned d = sh.digit, cnt = sh.cnt;
        want = sh.want;
        if (pass < 8) pre_hi |= (uint64_t)d << (56 - above);
        else pre_lo |= d << (24 - (above - 64));
        if (cnt == want) break;   // every candidate under the new prefix is wanted
    }
    __syncthreads();              // (sh is free again for the caller)
    thr_hi = pre_hi;
    thr_lo = pre_lo;
}
