// rq_tail.hip -- everything after the corpus scan in ONE launch (k <= 320).
//
// grid (chunks of 512*NV bins, B queries), 256 threads.  Each workgroup
//   A. derives the threshold T = P - 2.25 eps, P = the k-th largest partition maximum (partitions = groups of the
//      scan's per-workgroup maxima; distinct scan workgroups own distinct bins, so at least k rows reach P and the
//      k-th exact score is >= P - eps) with a 20-bit ballot radix select in wave 0,
//   B. finds the bins of its chunk whose largest score reaches T and turns them into ROW JOBS from the bin's 8-byte
//      scan record (rq_device.h): the arg-max row alone when the bound on the second-largest score is below T -- the
//      usual case --, the best two rows when only the bound on the third-largest is, all 64 rows of the bin otherwise,
//   C. re-scores the job rows exactly in fp64 (16 lanes per row, 8 rows of loads in flight per wave) and appends the
//      (score, row) keys to the query's compact candidate list with 8-byte write-through (sc1) stores,
//   D. publishes: every wave drains vmcnt, workgroup barrier, ONE lane draws a ticket (agent-scope atomic add).  The
//      workgroup that draws the last ticket of its query runs ONE agent-scope acquire (buffer_inv sc1 + vmcnt(0), then a
//      workgroup barrier), reads the keys (sc1 loads), ranks them, writes the exact top-k and the certificate, and
//      resets the counters.  No RELEASE fences: a release fence per workgroup serialises on the L2 write-back
//      (measured +60 us per launch); the producer side is write-through stores + drain + barrier + ticket.
// Exactness: a row that is not re-scored has approximate score < T (its bin's largest, second- or third-largest bound
// is below T), so its exact score is < T + eps < s_k; see rq_final_body.h and DESIGN.md 4.2.
// Replaces reference rag_uq/streaming_index.py:355-368 (collection.query + `1 - distance`) after the scan.
#include "rq_device.h"
#include "rq_kernels.h"
#include "rq_tail_body.h"

template <int NV, int DP>
__global__ __launch_bounds__(256) void rq_tail_kernel(RqTailArgs a) {
    __shared__ RqTailLds lds;
    rq_tail_body<NV, DP>(a, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, lds);
}
// The tail of a filtered search (include/rq.h rq_search_filtered): the same workgroups with the filter as a second argument.
template <int NV, int DP, bool FILT>
__global__ __launch_bounds__(256) void rq_tail_kernel(RqTailArgs a, RqFilterArgs f) {
    static_assert(FILT, "the unfiltered tail takes RqTailArgs alone");
    __shared__ RqTailLds lds;
    rq_tail_body<NV, DP, true>(a, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, lds, &f);
}

template <int NV, int DP = RQ_DPAD>
static hipError_t rq_tail_launch_nv(const RqTailArgs& a, int B, hipStream_t stream) {
    const int64_t chunks = (a.nbins + 512 * NV - 1) / (512 * NV);
    if (chunks < 1 || chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((rq_tail_kernel<NV, DP>), dim3((unsigned)chunks, B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t rq_tail_launch(const RqTailArgs& a, int B, hipStream_t stream) {
    if (a.m < 1 || a.m > RQ_FAST_MAX_M || a.k < 1 || a.k > RQ_FAST_MAX_K) return hipErrorInvalidValue;
    if (a.dpad == 384) return rq_tail_small_chunks(a.nbins, B) ? rq_tail_launch_nv<1, 384>(a, B, stream) : rq_tail_launch_nv<4, 384>(a, B, stream);
    if (a.dpad != RQ_DPAD) return hipErrorInvalidValue;
    return rq_tail_small_chunks(a.nbins, B) ? rq_tail_launch_nv<1>(a, B, stream) : rq_tail_launch_nv<4>(a, B, stream);
}

template <int NV, int DP>
static hipError_t rq_tail_filtered_launch_nv(const RqTailArgs& a, const RqFilterArgs& f, int B, hipStream_t stream) {
    const int64_t chunks = (a.nbins + 512 * NV - 1) / (512 * NV);
    if (chunks < 1 || chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((rq_tail_kernel<NV, DP, true>), dim3((unsigned)chunks, B), dim3(256), 0, stream, a, f);
    return hipGetLastError();
}

hipError_t rq_tail_filtered_launch(const RqTailArgs& a, const RqFilterArgs& f, int B, hipStream_t stream) {
    if (a.m < 1 || a.m > RQ_FAST_MAX_M || a.k < 1 || a.k > RQ_FAST_MAX_K || !f.bits || !f.first || f.na < 1 || a.m > f.na) return hipErrorInvalidValue;
    const bool small = rq_tail_small_chunks(a.nbins, B);
    if (a.dpad == 384) return small ? rq_tail_filtered_launch_nv<1, 384>(a, f, B, stream) : rq_tail_filtered_launch_nv<4, 384>(a, f, B, stream);
    if (a.dpad != RQ_DPAD) return hipErrorInvalidValue;
    return small ? rq_tail_filtered_launch_nv<1, RQ_DPAD>(a, f, B, stream) : rq_tail_filtered_launch_nv<4, RQ_DPAD>(a, f, B, stream);
}

// Tails of a bundle (the records of all its batches come from one 128- or 256-query pass) + the preparation of the next batch.
// Block ids: [0, end[0]) tail t0 | [end[0], end[1]) tail t1 | [end[1], end[2]) t2 | [end[2], end[3]) t3 | pa.nslots workgroups of
// rq_prep_body; end[j] = chunks * (B[0] + .. + B[j]), a tail that is not there has end[j] = end[j - 1].  (The name is the pair's,
// which profiles and DESIGN.md know the launch by; a pair is a bundle of two.)
union RqPairLds {
    RqTailLds tail;
    double prep[16];
};
struct RqBundleEnds { int e0, e1, e2, e3; };
template <int NV>
__global__ __launch_bounds__(256) void rq_pair_tail_kernel(RqTailArgs t0, RqTailArgs t1, RqTailArgs t2, RqTailArgs t3, RqBundleEnds end, RqPrepArgs pa, int chunks) {
    __shared__ RqPairLds lds;
    const int bid = (int)blockIdx.x;
    if (bid < end.e0) rq_tail_body<NV>(t0, bid % chunks, bid / chunks, chunks, lds.tail);
    else if (bid < end.e1) rq_tail_body<NV>(t1, (bid - end.e0) % chunks, (bid - end.e0) / chunks, chunks, lds.tail);
    else if (bid < end.e2) rq_tail_body<NV>(t2, (bid - end.e1) % chunks, (bid - end.e1) / chunks, chunks, lds.tail);
    else if (bid < end.e3) rq_tail_body<NV>(t3, (bid - end.e2) % chunks, (bid - end.e2) / chunks, chunks, lds.tail);
    else rq_prep_body(pa, bid - end.e3, lds.prep);
}

template <int NV>
static hipError_t rq_bundle_tail_launch_nv(const RqTailArgs* t, const int* B, int n, const RqPrepArgs& pa, hipStream_t stream) {
    const int64_t chunks = (t[0].nbins + 512 * NV - 1) / (512 * NV);
    int64_t e[RQ_BUNDLE_TAILS], sum = 0;
    for (int j = 0; j < RQ_BUNDLE_TAILS; ++j) e[j] = (sum += j < n ? chunks * B[j] : 0);
    const int64_t grid = sum + pa.nslots;
    if (chunks < 1 || grid > INT32_MAX) return hipErrorInvalidValue;
    const RqTailArgs& last = t[n - 1];   // (an absent tail's workgroup range is empty: its arguments are never read)
    hipLaunchKernelGGL((rq_pair_tail_kernel<NV>), dim3((unsigned)grid), dim3(256), 0, stream, t[0], n > 1 ? t[1] : last, n > 2 ? t[2] : last, n > 3 ? t[3] : last,
                       RqBundleEnds{(int)e[0], (int)e[1], (int)e[2], (int)e[3]}, pa, (int)chunks);
    return hipGetLastError();
}

hipError_t rq_bundle_tail_launch(const RqTailArgs* t, const int* B, int n, const RqPrepArgs& pa, hipStream_t stream) {
    if (!t || !B || n < 1 || n > RQ_BUNDLE_TAILS || pa.nslots < 0 || pa.nslots > 64) return hipErrorInvalidValue;
    int sumB = 0;
    for (int j = 0; j < n; ++j) {
        if (t[j].m < 1 || t[j].m > RQ_FAST_MAX_M || t[j].k < 1 || t[j].k > RQ_FAST_MAX_K) return hipErrorInvalidValue;
        if (t[j].dpad != RQ_DPAD || t[j].nbins != t[0].nbins) return hipErrorInvalidValue;   // (bundles are scanned over rows of 768 elements only)
        if (B[j] < 1 || B[j] > 64) return hipErrorInvalidValue;
        for (int i = 0; i < j; ++i)
            if (t[i].cand == t[j].cand || t[i].rowcount == t[j].rowcount || t[i].done == t[j].done || t[i].ovf == t[j].ovf) return hipErrorInvalidValue;
        sumB += B[j];
    }
    return rq_tail_small_chunks(t[0].nbins, sumB) ? rq_bundle_tail_launch_nv<1>(t, B, n, pa, stream) : rq_bundle_tail_launch_nv<4>(t, B, n, pa, stream);
}

__global__ __launch_bounds__(256) void rq_prep2_queries_kernel(RqPrepArgs a, RqPrepArgs b) {
    __shared__ double part[16];
    const int bid = (int)blockIdx.x;
    if (bid < a.nslots) rq_prep_body(a, bid, part);
    else rq_prep_body(b, bid - a.nslots, part);
}
hipError_t rq_prep2_queries_launch(const RqPrepArgs& a, const RqPrepArgs& b, hipStream_t stream) {
    if (a.nslots <= 0 || b.nslots <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_prep2_queries_kernel, dim3(a.nslots + b.nslots), dim3(256), 0, stream, a, b);
    return hipGetLastError();
}
