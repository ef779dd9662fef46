// rq_scan_narrow.hip -- pass 1 of the search over rows of 384 elements (rq_index.h dpad = 384; include/rq.h "row_pad").
//
// A row of 384 fp16 elements is 768 bytes: exactly the row of the int8 image that rq_scan_body already streams (I8 != 0).  The
// narrow forms therefore take that form's byte geometry unchanged -- a 12 KiB stage = 16 whole rows, every stage ends a tile, ring
// of 3 stages, 48 chunks of 16 bytes per stage row, the same DMA source offsets, XOR swizzle, LDS read addresses, record staging and
// flush -- and the fp16 form's arithmetic: 12 x v_mfma_f32_16x16x32_f16 per tile and query group, fp16 row scales (2^-12 / norm),
// clamped scores with the row position in the 6 low mantissa bits, no query scale.  A wave holds 48 VGPRs of query fragments per
// 16 queries (96 for rows of 768 elements), which is what lets the 128-query form keep two groups per wave.
//
// Built forms (one each; the tuning options ring / kstage / prefetch / epi do not apply to a narrow index):
//   rq_scan_narrow_kernel<NT, 1>       64 queries per pass, 53 760 B of LDS, up to three workgroups per CU
//   rq_scan_narrow_kernel<NT, 2>       128 queries per pass (two 16-query groups per wave), 70 144 B of LDS, two workgroups per CU
//   rq_scan_narrow_tail_kernel<NT, NV> the fused launch of "pipeline" = 2: scan workgroups of the 64-query form, tail workgroups
//                                      that re-score rows of 768 bytes (rq_tail_body<NV, 384>), preparation workgroups
// Not built for narrow rows: an int8 image, a 256-query pass, the scanned-ahead pair.
// Replaces, like rq_scan.hip, the kNN of reference rag_uq/streaming_index.py:355-359 -- for the embedders whose vectors have 384
// elements or fewer (the reference's own 32-element hash fallback, streaming_index.py:269-273, among them).
#include <hip/hip_ext.h>

#include "rq_device.h"
#include "rq_kernels.h"
#include "rq_tail_body.h"
#include "rq_scan_body.h"

// QG: 16-query groups per wave (1: 64 queries per pass, 2: 128)
template <bool NT, int QG>
__global__ __launch_bounds__(256, QG == 1 ? 3 : 2) void rq_scan_narrow_kernel(RqScanArgs a) {
    rq_scan_body<3, NT, 1, 2, 4, 1, 0, QG>(a, (int)blockIdx.x, (int)gridDim.x);
}

// Block ids as in rq_scan_tail_kernel: [0, scan_grid) scan THIS batch | the tail workgroups of the PREVIOUS batch | pa.nslots
// workgroups that prepare the queries of the NEXT batch.  53 760 B of LDS and <= 168 VGPRs: 2 scan + 1 tail workgroups per CU.
template <bool NT, int NV>
__global__ __launch_bounds__(256, 3) void rq_scan_narrow_tail_kernel(RqScanArgs sa, RqTailArgs ta, RqPrepArgs pa, int scan_grid, int tail_chunks) {
    unsigned long long t0 = 0;
    if (ta.dbg) t0 = wall_clock64();
    const int bid = (int)blockIdx.x;
    const int nprep = pa.nslots;
    const int ntail = (int)gridDim.x - scan_grid - nprep;
    if (bid < scan_grid) {
        rq_scan_body<3, NT, 1, 2, 4, 1, 0, 1>(sa, bid, scan_grid);
    } else if (bid < scan_grid + ntail) {
        const int t = bid - scan_grid;
        rq_tail_body<NV, 384>(ta, t % tail_chunks, t / tail_chunks, tail_chunks, *reinterpret_cast<RqTailLds*>(rq_smem));
    } else {
        rq_prep_body(pa, bid - scan_grid - ntail, reinterpret_cast<double*>(rq_smem));
    }
    if (ta.dbg && threadIdx.x == 0) {   // development stamps (rq_debug_stamps), as in rq_scan_tail_kernel
        ta.dbg[4 * blockIdx.x] = t0; ta.dbg[4 * blockIdx.x + 1] = wall_clock64();
        ta.dbg[4 * blockIdx.x + 2] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        ta.dbg[4 * blockIdx.x + 3] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}

template <bool NT, int QG>
static hipError_t rq_scan_narrow_launch_t(const RqScanArgs& a, int grid, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    constexpr size_t lds = rq_scan_lds_bytes(3, 2, 4, QG);
    static_assert(lds <= 160 * 1024 / (QG == 1 ? 3 : 2), "workgroups per CU the launch bounds ask for");
    static unsigned long long attr_done = 0;   // one bit per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!((attr_done >> (dev & 63)) & 1ull)) {
        e = hipFuncSetAttribute((const void*)rq_scan_narrow_kernel<NT, QG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done |= 1ull << (dev & 63);
    }
    if (e0 && e1) hipExtLaunchKernelGGL((rq_scan_narrow_kernel<NT, QG>), dim3(grid), dim3(256), (uint32_t)lds, stream, e0, e1, 0, a);
    else hipLaunchKernelGGL((rq_scan_narrow_kernel<NT, QG>), dim3(grid), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// queries per pass -> the built form; anything else is an error.
hipError_t rq_scan_narrow_launch(const RqScanArgs& a, int queries, bool nt, int grid, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    if (grid <= 0 || a.i8 != 0) return hipErrorInvalidValue;
    if (queries == 64) return nt ? rq_scan_narrow_launch_t<true, 1>(a, grid, stream, e0, e1) : rq_scan_narrow_launch_t<false, 1>(a, grid, stream, e0, e1);
    if (queries == 128) return nt ? rq_scan_narrow_launch_t<true, 2>(a, grid, stream, e0, e1) : rq_scan_narrow_launch_t<false, 2>(a, grid, stream, e0, e1);
    return hipErrorInvalidValue;
}

// ---- fused scan(batch i) + tail(batch i-1) + prep(batch i+1) --------------------------------------------------
template <bool NT, int NV>
static hipError_t rq_scan_narrow_tail_launch_t(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, int scan_grid, hipStream_t stream,
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
        e = hipFuncSetAttribute((const void*)rq_scan_narrow_tail_kernel<NT, NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done |= 1ull << (dev & 63);
    }
    const unsigned grid = (unsigned)(scan_grid + chunks * tail_B + pa.nslots);
    if (e0 && e1) hipExtLaunchKernelGGL((rq_scan_narrow_tail_kernel<NT, NV>), dim3(grid), dim3(256), (uint32_t)lds, stream, e0, e1, 0, sa, ta, pa, scan_grid, (int)chunks);
    else hipLaunchKernelGGL((rq_scan_narrow_tail_kernel<NT, NV>), dim3(grid), dim3(256), lds, stream, sa, ta, pa, scan_grid, (int)chunks);
    return hipGetLastError();
}

hipError_t rq_scan_narrow_tail_launch(const RqScanArgs& sa, const RqTailArgs& ta, int tail_B, const RqPrepArgs& pa, bool nt, int scan_grid, hipStream_t stream,
                                      hipEvent_t e0, hipEvent_t e1) {
    if (pa.nslots < 0 || pa.nslots > 64 || sa.i8 != 0) return hipErrorInvalidValue;
    if (scan_grid <= 0 || tail_B < 0) return hipErrorInvalidValue;   // tail_B = 0: no tail to carry (first call of a loop)
    if (tail_B > 0 && ta.dpad != 384) return hipErrorInvalidValue;
    if (ta.m < 1 || ta.m > RQ_FAST_MAX_M || ta.k < 1 || ta.k > RQ_FAST_MAX_K) return hipErrorInvalidValue;
    // riding tails: the rule of rq_scan_tail_launch_e (as few workgroups as keep every CU's third slot busy once)
    const auto wgs = [&](int nv) { return ((ta.nbins + 512 * nv - 1) / (512 * nv)) * tail_B; };
    const int nv = (ta.fused_nv == 1 || ta.fused_nv == 4 || ta.fused_nv == 8) ? ta.fused_nv : (wgs(1) <= 384 ? 1 : (wgs(4) <= 384 ? 4 : 8));
    if (nt) return nv == 1 ? rq_scan_narrow_tail_launch_t<true, 1>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                 : nv == 4 ? rq_scan_narrow_tail_launch_t<true, 4>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                           : rq_scan_narrow_tail_launch_t<true, 8>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1);
    return nv == 1 ? rq_scan_narrow_tail_launch_t<false, 1>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
         : nv == 4 ? rq_scan_narrow_tail_launch_t<false, 4>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1)
                   : rq_scan_narrow_tail_launch_t<false, 8>(sa, ta, tail_B, pa, scan_grid, stream, e0, e1);
}
