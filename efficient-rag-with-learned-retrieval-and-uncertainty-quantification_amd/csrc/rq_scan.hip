// rq_scan.hip -- pass 1 of the search: stream the fp16 corpus once from HBM, score it against a
// block of 64 (or 128) queries on the matrix cores, and keep per (query, bin = quad of 64 rows) the largest
// approximate score, the second largest and the position of the largest.
//
// This is the arithmetic ChromaDB's cosine index performs behind
// reference rag_uq/streaming_index.py:355-359 (collection.query), done exhaustively.
//
// Shape of the work (why it looks like this on MI355X):
//   * HBM-bound: N*1536 B of corpus per query block, 64 FLOP/B -> the matrix cores run ~16% busy.
//   * One workgroup = QW waves (4 or 8); wave w keeps queries 16w..16w+15 in registers as the B operand
//     of v_mfma_f32_16x16x32_f16 (24 fragments x 4 VGPRs), so LDS holds only corpus bytes.
//   * Corpus rows reach LDS by LDS-DMA (global_load_lds_dwordx4): every wave-instruction moves
//     1 KiB contiguous, no VGPRs, and stays in flight across barriers (counted vmcnt, raw s_barrier).
//     A stage = 16 rows x 384 elements (12 KiB, KS = 2) or 16 whole rows (24 KiB, KS = 1); S stages
//     form a ring, S-1 are in flight.  Every variant measured lands within 2 % of the same rate (6.3-6.5 TB/s).
//   * The stage rows alias in LDS banks, so the 16-byte chunks are XOR-swizzled with the row number on
//     the DMA *source* address and on the ds_read_b128 address (LDS image stays lane-linear as
//     LDS-DMA requires).
//   * Accumulator layout of the 16x16 MFMA puts the query on the lane and 4 corpus rows in the 4
//     result registers: max / second max / arg-max over the 16 rows a lane sees of a quad are lane-local (no
//     data-dependent control flow in the streaming loop); the 4 lanes that share a query are merged with two
//     xor-shuffles per quad.
//   * Outputs: ONE 8-byte record per (query, quad) -- largest score, upper bounds of the second and third largest,
//     rows of the largest two (rq_device.h); N/64 * 64 * 8 B = 0.5 % of the corpus bytes -- and
//     wgmax[query][workgroup].  Writes are what the kernel is sensitive to: with a record per 16 rows (65 MB per
//     launch, 16-byte pieces) the stores cost 62 of 289 us (measured by switching them off); a workgroup therefore
//     owns a CONTIGUOUS range of quads and parks its records in LDS until the range is done (see `flush`).
#include <hip/hip_ext.h>

#include "rq_device.h"
#include "rq_kernels.h"
#include "rq_tail_body.h"
#include "rq_scan_body.h"



// EPI of the kernels: 0 / 1 = selection form of the fp16 scan, 2 = the int8 scan (selection form 1), 3 = int8 with split queries,
// 4 = int8 with two query groups per wave (128 queries per pass)
template <int S, bool NT, int PF, int OCC, int KS, int QW, int EPI>
__global__ __launch_bounds__(64 * QW, OCC) void rq_scan_kernel(RqScanArgs a) {
    rq_scan_body<S, NT, PF, KS, QW, (EPI >= 2 ? 1 : EPI), (EPI >= 2 ? EPI - 1 : 0)>(a, (int)blockIdx.x, (int)gridDim.x);
}

// Fused launch: workgroups [0, scan_grid) scan the corpus for THIS batch, the others run the tail (threshold, fp64
// re-score, final top-k) of the PREVIOUS batch of the same stream, whose scan finished with the previous launch.
// One stream, no events: the tail's ~20 us hide under the scan, and the scan launches of consecutive batches never
// overlap each other.  Scan variant: ring of 3 half-row stages, prefetch 1 (36 KB ring + 16.5 KB of record staging =
// 53 760 B of LDS, <= 168 VGPRs), so a CU holds 2 scan workgroups + 1 tail workgroup (3 x 53 760 B <= 160 KB; the
// tail's 16 KB are carved from the ring).
template <bool NT, int NV, int EPI>
__global__ __launch_bounds__(256, 3) void rq_scan_tail_kernel(RqScanArgs sa, RqTailArgs ta, RqPrepArgs pa, int scan_grid, int tail_chunks) {
    unsigned long long t0 = 0;
    if (ta.dbg) t0 = wall_clock64();
    // block ids: [0, scan_grid) scan THIS batch | the tail workgroups of the PREVIOUS batch | pa.nslots workgroups that prepare
    // the queries of the NEXT batch (rq_search_hint_next_device), so that the next call needs no preparation launch
    const int bid = (int)blockIdx.x;
    const int nprep = pa.nslots;
    const int ntail = (int)gridDim.x - scan_grid - nprep;
    if (bid < scan_grid) {
        rq_scan_body<3, NT, 1, 2, 4, (EPI >= 2 ? 1 : EPI), (EPI >= 2 ? EPI - 1 : 0)>(sa, bid, scan_grid);
    } else if (bid < scan_grid + ntail) {
        const int t = bid - scan_grid;
        rq_tail_body<NV>(ta, t % tail_chunks, t / tail_chunks, tail_chunks, *reinterpret_cast<RqTailLds*>(rq_smem));
    } else {
        rq_prep_body(pa, bid - scan_grid - ntail, reinterpret_cast<double*>(rq_smem));
    }
    if (ta.dbg && threadIdx.x == 0) {
        ta.dbg[4 * blockIdx.x] = t0; ta.dbg[4 * blockIdx.x + 1] = wall_clock64();
        // HW_REG_HW_ID (4): wave/simd/cu/sh/se ids;  HW_REG_XCC_ID (20): the XCD
        ta.dbg[4 * blockIdx.x + 2] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        ta.dbg[4 * blockIdx.x + 3] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}

template <int S, bool NT, int PF, int OCC, int KS, int QW, int EPI>
static hipError_t rq_scan_launch_t(const RqScanArgs& a, int grid, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = rq_scan_lds_bytes(S, KS, QW, EPI == 4 ? 2 : 1);
    static unsigned long long attr_done = 0;   // one bit per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!((attr_done >> (dev & 63)) & 1ull)) {
        e = hipFuncSetAttribute((const void*)rq_scan_kernel<S, NT, PF, OCC, KS, QW, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done |= 1ull << (dev & 63);
    }
    // e0 / e1: events attached to the dispatch itself (hipExtLaunchKernel): they read the kernel's own start and end
    // time stamps and cost no extra barrier packets (hipEventRecord around a launch costs ~5 us on each side)
    if (e0 && e1) hipExtLaunchKernelGGL((rq_scan_kernel<S, NT, PF, OCC, KS, QW, EPI>), dim3(grid), dim3(64 * QW), (uint32_t)lds, stream, e0, e1, 0, a);
    else hipLaunchKernelGGL((rq_scan_kernel<S, NT, PF, OCC, KS, QW, EPI>), dim3(grid), dim3(64 * QW), lds, stream, a);
    return hipGetLastError();
}

template <int S, int PF, int OCC, int KS, int QW, int EPI = 0>
static hipError_t rq_scan_launch_r(const RqScanArgs& a, bool nt, int grid, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    return nt ? rq_scan_launch_t<S, true, PF, OCC, KS, QW, EPI>(a, grid, stream, e0, e1) : rq_scan_launch_t<S, false, PF, OCC, KS, QW, EPI>(a, grid, stream, e0, e1);
}

// (ring S, prefetch PF, stages-per-tile KS, waves QW) combinations that are built; anything else is an error.
// qw = 4: 64 queries per pass; qw = 8: 128 queries per pass (one workgroup per CU, whole-row stages).
// epi = 1 (selection with positions inside the scores) exists for the default variant (ring 3, prefetch 1, half-row stages, 4 waves)
hipError_t rq_scan_launch(const RqScanArgs& a, int S, int pf, int ks, int qw, bool nt, int grid, int epi, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    if (grid <= 0) return hipErrorInvalidValue;
    if (a.i8 == 3) return (S == 3 && pf == 1 && ks == 2 && qw == 4) ? rq_scan_launch_r<3, 1, 2, 2, 4, 4>(a, nt, grid, stream, e0, e1) : hipErrorInvalidValue;
    if (a.i8 == 2) return (S == 3 && pf == 1 && ks == 2 && qw == 4) ? rq_scan_launch_r<3, 1, 3, 2, 4, 3>(a, nt, grid, stream, e0, e1) : hipErrorInvalidValue;
    if (a.i8) return (S == 3 && pf == 1 && ks == 2 && qw == 4) ? rq_scan_launch_r<3, 1, 3, 2, 4, 2>(a, nt, grid, stream, e0, e1) : hipErrorInvalidValue;
    if (epi && S == 3 && pf == 1 && ks == 2 && qw == 4) return rq_scan_launch_r<3, 1, 3, 2, 4, 1>(a, nt, grid, stream, e0, e1);
#define RQ_CASE(SS, PP, OO, KK, QQ) if (S == SS && pf == PP && ks == KK && qw == QQ) return rq_scan_launch_r<SS, PP, OO, KK, QQ>(a, nt, grid, stream, e0, e1);
    RQ_CASE(3, 1, 3, 2, 4) RQ_CASE(4, 1, 3, 2, 4)
    RQ_CASE(4, 4, 2, 2, 4) RQ_CASE(6, 4, 2, 2, 4)
    RQ_CASE(5, 6, 2, 2, 4) RQ_CASE(6, 12, 2, 2, 4)
    RQ_CASE(2, 4, 2, 1, 4) RQ_CASE(3, 4, 2, 1, 4) RQ_CASE(3, 12, 2, 1, 4) RQ_CASE(2, 1, 2, 1, 4) RQ_CASE(4, 4, 2, 1, 4)
    RQ_CASE(3, 4, 2, 1, 8)
#undef RQ_CASE
    return hipErrorInvalidValue;
}


// ---- fused scan(batch i) + tail(batch i-1) -------------------------------------------------------------------
template <bool NT, int NV, int EPI>
static hipError_t rq_scan_tail_launch_t(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, int scan_grid, hipStream_t stream,
                                        hipEvent_t e0, hipEvent_t e1) {
    constexpr size_t lds = rq_scan_lds_bytes(3, 2, 4);
    static_assert(sizeof(RqTailLds) <= lds, "tail LDS must fit in the scan's LDS");
    static_assert(3 * lds <= 160 * 1024, "2 scan workgroups + 1 tail workgroup per CU");
    const int64_t chunks = (ta.nbins + 512 * NV - 1) / (512 * NV);
    if (chunks < 1 || chunks * tail_B > (1 << 24)) return hipErrorInvalidValue;
    static unsigned long long attr_done = 0;   // one bit per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!((attr_done >> (dev & 63)) & 1ull)) {
        e = hipFuncSetAttribute((const void*)rq_scan_tail_kernel<NT, NV, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done |= 1ull << (dev & 63);
    }
    const unsigned grid = (unsigned)(scan_grid + chunks * tail_B + pa.nslots);
    if (e0 && e1) hipExtLaunchKernelGGL((rq_scan_tail_kernel<NT, NV, EPI>), dim3(grid), dim3(256), (uint32_t)lds, stream, e0, e1, 0, sa, ta, pa, scan_grid, (int)chunks);
    else hipLaunchKernelGGL((rq_scan_tail_kernel<NT, NV, EPI>), dim3(grid), dim3(256), lds, stream, sa, ta, pa, scan_grid, (int)chunks);
    return hipGetLastError();
}

template <int EPI>
static hipError_t rq_scan_tail_launch_e(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, bool nt, int scan_grid, hipStream_t stream,
                                        hipEvent_t e0, hipEvent_t e1) {
    if (scan_grid <= 0 || tail_B < 0) return hipErrorInvalidValue;   // tail_B = 0: development (the fused kernel without tail workgroups)
    if (ta.m < 1 || ta.m > RQ_FAST_MAX_M || ta.k < 1 || ta.k > RQ_FAST_MAX_K) return hipErrorInvalidValue;
    // Riding tails: as few workgroups as keep every CU's third slot busy once (~256): each tail workgroup costs the
    // scan a little while it is resident (measured at 1M rows: 256 workgroups of 4096 bins 248.7 us per launch, 512 of
    // 2048 bins 252.4 us).  The stand-alone launch (rq_tail_launch) prefers more, smaller ones: lower latency.
    const auto wgs = [&](int nv) { return ((ta.nbins + 512 * nv - 1) / (512 * nv)) * tail_B; };
    const int nv = (ta.fused_nv == 1 || ta.fused_nv == 4 || ta.fused_nv == 8 || ta.fused_nv == 16) ? ta.fused_nv : (wgs(1) <= 384 ? 1 : (wgs(4) <= 384 ? 4 : 8));
    if (nt && nv == 16) return rq_scan_tail_launch_t<true, 16, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1);   // development (fused_nv = 16): 128 riding workgroups at 1M rows
    if (nt) return nv == 1 ? rq_scan_tail_launch_t<true, 1, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                 : nv == 4 ? rq_scan_tail_launch_t<true, 4, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                           : rq_scan_tail_launch_t<true, 8, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1);
    return nv == 1 ? rq_scan_tail_launch_t<false, 1, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
         : nv == 4 ? rq_scan_tail_launch_t<false, 4, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                   : rq_scan_tail_launch_t<false, 8, EPI>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1);
}

// epi: selection form of the scan workgroups (0 = compare / select, 1 = positions inside the scores)
hipError_t rq_scan_tail_launch(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, bool nt, int scan_grid, int epi, hipStream_t stream,
                               hipEvent_t e0, hipEvent_t e1) {
    if (pa.nslots < 0 || pa.nslots > 64) return hipErrorInvalidValue;
    if (sa.i8 == 3) return hipErrorInvalidValue;   // the 128-query form is not fused with a tail (LDS)
    if (sa.i8 == 2) return rq_scan_tail_launch_e<3>(sa, ta, tail_B, pa, nt, scan_grid, stream, e0, e1);
    if (sa.i8) return rq_scan_tail_launch_e<2>(sa, ta, tail_B, pa, nt, scan_grid, stream, e0, e1);
    return epi ? rq_scan_tail_launch_e<1>(sa, ta, tail_B, pa, nt, scan_grid, stream, e0, e1)
               : rq_scan_tail_launch_e<0>(sa, ta, tail_B, pa, nt, scan_grid, stream, e0, e1);
}
