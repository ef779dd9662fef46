// rq_scan_body.h -- the work of one scan workgroup (rq_scan.hip describes the shape of the work), shared by the kernels of
// rq_scan.hip (rows of 768 elements and their int8 image) and rq_scan_narrow.hip (rows of 384 elements).
#pragma once
#include "rq_device.h"
#include "rq_kernels.h"

extern __shared__ __attribute__((aligned(16))) char rq_smem[];

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

// Records per query a scan workgroup parks in LDS: covers a whole range at the usual grid (1M rows: 30.5 quads per
// workgroup with 64-query workgroups, 61 with the 128-query ones, which run one per CU and have the LDS for it).
__host__ __device__ static constexpr int rq_stage_quads(int QW) { return QW == 8 ? 64 : 32; }

template <int N>
__device__ __forceinline__ void rq_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// S: ring depth; NT: non-temporal corpus loads; PF: A fragments read from LDS ahead of
// their MFMAs (1, 4, 6 or 12); OCC: waves per SIMD the register allocation must allow; KS: stages per
// tile (2: a stage is 16 half rows = 12 KiB; 1: a stage is 16 whole rows = 24 KiB contiguous in HBM);
// QW: waves per workgroup = 16-query groups scored per corpus pass (4: 64 queries, 8: 128 queries).
// EPI: 1 = selection with the row position in the low mantissa bits of the score (rq_device.h rq_insert3: 6 VALU per
//      score, no data-dependent code, no per-score row test -- the pad rows' row scale is NaN); 0 = compare / select form.
// I8: the corpus operand is the int8 image of the shard (rq_select.hip rq_quant_rows_kernel: 768 B per row, per-row scale)
//     and the queries are int8 too (rq_prep_body); v_mfma_i32_16x16x64_i8 sums exactly in int32.  A stage is 16 WHOLE rows
//     (12 KiB, the byte geometry of the fp16 half-row stage, so DMA, swizzle and LDS reads are the same code), every stage
//     ends a tile, and the per-query scale is applied once per quad.  Half the HBM bytes per row; the certificate's bound is
//     the quantisation error measured at add / preparation time (csrc/rq_api.hip scan8_eps).
//     I8 = 2: the queries are TWO int8 images (value and residual, q = s (254 q_hi + q_lo)); every corpus fragment feeds two
//     MFMAs and the score is (254 sum_hi + sum_lo) * scales: the query's share of the error bound drops from ~0.008 to ~3e-5
//     for twice the (idle) matrix-core work and no extra bytes.
//     I8 = 3: 128 queries per pass -- a wave keeps TWO groups of 16 queries (one int8 image each: 2 x 48 VGPRs, where the fp16
//     form would need 2 x 96) and every corpus fragment feeds one MFMA per group; records of 128 queries are parked in LDS
//     (68.5 KB per workgroup: two per CU, so this form is not fused with a tail).
// NARROW: the corpus rows are fp16 rows of 384 elements (rq_index.h dpad = 384): 768 bytes, exactly the row of the int8 image, so the
//     stage geometry, DMA offsets, swizzle, ring and record staging are those of I8 != 0 (a stage = 16 whole rows, every stage ends a
//     tile, 12 fragments per query group) while operand type and epilogue are those of the fp16 form (v_mfma_f32_16x16x32_f16, fp16
//     row scales, clamped scores).  The queries stay in their 768-element slots (the fragments of elements 384.. are never read).
//     NARROW = 2: 128 queries per pass, two groups of 16 queries per wave (2 x 48 VGPRs of fragments), the shape of I8 = 3.
template <int S, bool NT, int PF, int KS, int QW, int EPI = 0, int I8 = 0, int NARROW = 0>
__device__ __forceinline__ void rq_scan_body(const RqScanArgs& a, const int b, const int G) {
    static_assert(S >= 2 && S <= 8, "ring depth");
    static_assert(PF == 1 || PF == 4 || PF == 6 || PF == 12, "fragment prefetch group");
    static_assert(KS == 1 || KS == 2, "stages per tile");
    static_assert(I8 == 0 || (KS == 2 && EPI == 1), "int8 scan: built for the half-row stage geometry and the med3 selection");
    static_assert(NARROW == 0 || (I8 == 0 && KS == 2 && EPI == 1), "narrow rows: the byte geometry of the int8 scan, fp16 operands, med3 selection");
    constexpr bool ROW768B = I8 != 0 || NARROW != 0;   // a corpus row is 768 bytes: the int8 image, or 384 fp16 elements
    constexpr int ROWB = ROW768B ? RQ_DPAD : RQ_DPAD * 2;   // bytes per corpus row
    constexpr int QROWB = I8 ? RQ_DPAD : RQ_DPAD * 2;       // bytes per prepared query (always 768 elements)
    constexpr int KL = ROW768B ? 1 : KS;           // stages per tile
    constexpr int CH = 96 / KS;                    // 16-byte chunks per stage row
    constexpr int STAGE_BYTES = 16 * CH * 16;      // 24576 / KS
    static_assert((24 / KS) % QW == 0, "DMA instructions of a stage must split evenly over the waves");
    constexpr int DPW = 24 / KS / QW;              // DMA wave-instructions per wave per stage
    constexpr int MF = 24 / KS;                    // MFMAs per stage per wave
    constexpr int NSTQ = 4 * KL;                   // stages per quad
    constexpr int VM_KEEP = DPW * (S - 2);         // DMA ops of stages st+1 .. st+S-2 may stay in flight
    constexpr unsigned AUX = NT ? 2u : 0u;
    constexpr int QG = (I8 == 3 || NARROW == 2) ? 2 : 1;   // 16-query groups per wave

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kg = lane >> 4;          // k-group of the MFMA operand / row group of the result
    const int r16 = lane & 15;         // corpus row inside the tile (A operand), query inside the wave (D)

    // (query fragments are built after the DMA prologue has been issued, see below)
    // ---- per-lane DMA source offsets: LDS chunk p = 64*j + lane of a stage holds
    //      row r = p / CH, source chunk c = (p % CH) ^ r   (r < 16, XOR stays inside a 16-chunk group)
    unsigned voff[DPW];
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
        const int p = 64 * (wave * DPW + i) + lane;
        const int r = p / CH, cp = p % CH;
        voff[i] = (unsigned)(r * ROWB + ((cp ^ r) << 4));
    }
    // ---- per-lane LDS read offsets: logical chunk 4*s + kg of row r16 sits at chunk ((4s+kg) ^ r16)
    //      = 4*(s ^ (r16>>2)) + (kg ^ (r16&3));  split s = (s & ~3) | (s & 3): the high part is an immediate, the low
    //      part m = s & 3 enters as ((m ^ (r16>>2)) << 6) = (m << 6) ^ ((r16>>2) << 6).  The row base r16 * CH * 16 is a
    //      multiple of 256, so bits 6..7 of rbase0 hold only that term and rbase(m) = rbase0 ^ (m << 6): one VGPR and
    //      a v_xor per read instead of four VGPRs (the register budget is 168, see rq_scan_tail_kernel).
    static_assert((CH * 16) % 256 == 0, "row pitch must keep bits 6..7 free");
    const unsigned rbase0 = (unsigned)(r16 * (CH * 16) + ((kg ^ (r16 & 3)) << 4) + ((r16 >> 2) << 6));

    // this workgroup's quads: the contiguous range [q_lo, q_lo + nloc)
    const int q_lo = (int)((int64_t)b * a.nquads / G);
    const int nloc = (int)((int64_t)(b + 1) * a.nquads / G) - q_lo;
    const int nst = nloc * NSTQ;
    const char* xb = (const char*)a.x;
    char* norm_lds = rq_smem + S * STAGE_BYTES;                 // [2 parities][64 row scales], shared by the waves
    constexpr int SQ = rq_stage_quads(QW);                      // records per query parked in LDS before they are written out
    uint2* const stg = (uint2*)(norm_lds + 512);                // [16 * QW * QG queries][SQ] finished records

    auto issue = [&](int st, int slot) {
        const int lq = st / NSTQ, t = (st / KL) & 3, kh = st % KL;
        const int64_t quad = (int64_t)q_lo + lq;
        const char* g = xb + (quad * RQ_QUAD_ROWS + t * RQ_TILE_ROWS) * (int64_t)ROWB + kh * (ROWB / KL);
        char* l = rq_smem + slot * STAGE_BYTES + (wave * DPW) * 1024;
#pragma unroll
        for (int i = 0; i < DPW; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(g + voff[i]), (lds_ptr_t)(l + i * 1024), 16, 0, AUX);
        if ((st % NSTQ) == 0 && wave == 0) {   // row scales of the quad (256 B): wave 0's counted wait + the stage barrier
            const float* ns = a.row_scale + quad * RQ_QUAD_ROWS + lane;   // make them visible to all waves
            __builtin_amdgcn_global_load_lds((glb_ptr_t)ns, (lds_ptr_t)(norm_lds + ((lq & 1) << 8)), 4, 0, 0);
        }
    };

    int islot = 0;   // slot the next issued stage goes to
    {
        const int pre = nst < S - 1 ? nst : S - 1;
        for (int st = 0; st < pre; ++st) { issue(st, islot); islot = (islot + 1 == S) ? 0 : islot + 1; }
    }
    int cslot = 0;   // slot of the stage being consumed
    const float NEG_INF = -__builtin_huge_valf();
    float wmax = NEG_INF;   // largest approximate score this lane has produced (feeds the tail's threshold)
    float wmax1 = NEG_INF;  // QG = 2: the same for the second query group

    // ---- query fragments: B[k = 8*kg + j][col = r16] of k-step s == qh[16*wave + r16][32*s + 8*kg + j]
    //      (unit-norm fp16 queries written by rq_prep_queries_kernel); loaded while the first stages are in flight
    //      int8: B[k = 16*kg + j][col = r16] of k-step s == q8[16*wave + r16][64*s + 16*kg + j], 12 fragments
    constexpr int NQF = ROW768B ? 12 : 24;
    rq_half8 qf[NQF];   // (int8: the same 16 bytes per fragment, reinterpreted at the MFMA)
    rq_half8 ql[(I8 >= 2 || QG == 2) ? 12 : 1];   // I8 = 2: fragments of the residual image; QG = 2: of the wave's second query group
    {
        const rq_half8* qsrc = (const rq_half8*)((const char*)a.qh + (size_t)(16 * QG * wave + r16) * QROWB + 16 * kg);
#pragma unroll
        for (int s = 0; s < NQF; ++s) qf[s] = qsrc[4 * s];
#pragma unroll
        for (int s = 0; s < NQF; ++s) asm volatile("" : "+v"(qf[s]));   // ordinary loads retired before the main loop
        if constexpr (I8 >= 2 || QG == 2) {
            const rq_half8* lsrc = I8 == 2 ? (const rq_half8*)((const char*)a.qlo + (size_t)(16 * wave + r16) * QROWB + 16 * kg)
                                           : (const rq_half8*)((const char*)a.qh + (size_t)(16 * QG * wave + 16 + r16) * QROWB + 16 * kg);
#pragma unroll
            for (int s = 0; s < 12; ++s) ql[s] = lsrc[4 * s];
#pragma unroll
            for (int s = 0; s < 12; ++s) asm volatile("" : "+v"(ql[s]));
        }
    }
    float qsc = 1.f;    // int8: s_q / |q| of this lane's query (rq_prep_body), applied once per quad
    float qsc1 = 1.f;   // I8 = 3: scale of the second group's query
    if (I8) qsc = a.qscale[16 * QG * wave + r16];
    if (I8 == 2) qsc *= (1.f / 254.f);
    if (I8 == 3) qsc1 = a.qscale[16 * QG * wave + 16 + r16];

    // Finished records wait in LDS and leave in ONE burst per SQ quads (normally once, at the end of the
    // workgroup's range).  Stores inside the streaming loop are what this kernel is sensitive to: every store
    // instruction that touches 16 different lines holds up the CU's vector-memory address pipe for ~500 cycles
    // (TCP_TCP_TA_ADDR_STALL / _DATA_STALL counters), and the DMA loads queue behind it.  Measured per launch (same
    // box, same run; no store at all = 232 us): a record per 16 rows +62 us, a 16-byte record per quad +45 us, an
    // 8-byte record per quad stored every 4 quads +32 us (non-temporal / write-through / plain alike, any ring depth,
    // any position inside the stage), every quad +60 us.
    auto flush = [&](int quad0, int count) {
        // each wave writes the rows of its own 16 queries: 64 / SQ queries x SQ records (runs of 8 SQ bytes) per instruction
        constexpr int QPI = 64 / SQ;
#pragma unroll 1
        for (int i = 0; i < 16 * QG / QPI; ++i) {
            const int qi = 16 * QG * wave + QPI * i + lane / SQ, j = lane & (SQ - 1);
            if (j < count && qi < a.nq_valid) a.bins[(int64_t)qi * a.bins_stride + quad0 + j] = stg[qi * SQ + j];
        }
    };
    for (int lq = 0; lq < nloc; ++lq) {
        const int quad = q_lo + lq;
        constexpr float EMPTY = I8 ? RQ_TRIPLE_EMPTY8 : -__builtin_huge_valf();   // (int8: finite, see rq_device.h)
        float m1 = EMPTY, m2 = EMPTY, m3 = EMPTY;         // the three largest approximate scores of the lane's 16 rows
        float n1 = EMPTY, n2 = EMPTY, n3 = EMPTY;         // QG = 2: the same for the second query group
        uint32_t ap = 0;                                  // rows (0..63) of the largest [7:0] and second largest [15:8]
        const char* nrow = norm_lds + ((lq & 1) << 8) + kg * 16;

#pragma unroll
        for (int t = 0; t < 4; ++t) {
            rq_float4 acc = {0.f, 0.f, 0.f, 0.f};
            rq_float4 acc1 = {0.f, 0.f, 0.f, 0.f};                // NARROW = 2: the second query group
            rq_int4 iacc = {0, 0, 0, 0}, lacc = {0, 0, 0, 0};
#pragma unroll
            for (int kh = 0; kh < KL; ++kh) {
                const int st = lq * NSTQ + t * KL + kh;
                if (st + S - 2 <= nst - 1) rq_wait_vmcnt<VM_KEEP>(); else rq_wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (st + S - 1 < nst) { issue(st + S - 1, islot); islot = (islot + 1 == S) ? 0 : islot + 1; }
                const char* sb = rq_smem + cslot * STAGE_BYTES;
                cslot = (cslot + 1 == S) ? 0 : cslot + 1;
#pragma unroll
                for (int g = 0; g < MF; g += PF) {
                    rq_half8 av[PF];
#pragma unroll
                    for (int s = 0; s < PF; ++s) av[s] = *(const rq_half8*)(sb + (rbase0 ^ (unsigned)(((g + s) & 3) << 6)) + (((g + s) & ~3) << 6));
#pragma unroll
                    for (int s = 0; s < PF; ++s) {
                        if constexpr (I8 != 0) {
                            iacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(rq_int4, av[s]), __builtin_bit_cast(rq_int4, qf[g + s]), iacc, 0, 0, 0);
                            if constexpr (I8 >= 2) lacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(rq_int4, av[s]), __builtin_bit_cast(rq_int4, ql[g + s]), lacc, 0, 0, 0);
                        } else {
                            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s], qf[kh * MF + g + s], acc, 0, 0, 0);
                            if constexpr (NARROW == 2) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s], ql[g + s], acc1, 0, 0, 0);
                        }
                    }
                }
            }
            if constexpr (I8 != 0) {   // |sum| <= 768 * 127 * 127 < 2^24: the conversions are exact
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = I8 == 2 ? fmaf((float)iacc[i], 254.f, (float)lacc[i]) : (float)iacc[i];
            }
            // tile epilogue: D[row = 4*kg + i][query = r16]
            const rq_float4 nv = *(const rq_float4*)(nrow + t * 64);
            const int64_t row0 = (int64_t)quad * RQ_QUAD_ROWS + t * RQ_TILE_ROWS + 4 * kg;
            if (EPI == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // (int8: the score is an exact int32 sum times a finite row scale, or NaN on pad rows -- no clamp needed, rq_device.h)
                    if constexpr (I8 != 0) rq_insert3(m1, m2, m3, rq_pos_score_finite(acc[i] * nv[i], (uint32_t)(t * 16 + i)));
                    else rq_insert3(m1, m2, m3, rq_pos_score(acc[i] * nv[i], (uint32_t)(t * 16 + i)));
                }
                if constexpr (I8 == 3) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) rq_insert3(n1, n2, n3, rq_pos_score_finite((float)lacc[i] * nv[i], (uint32_t)(t * 16 + i)));
                }
                if constexpr (NARROW == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) rq_insert3(n1, n2, n3, rq_pos_score(acc1[i] * nv[i], (uint32_t)(t * 16 + i)));
                }
            } else
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float sc = acc[i] * nv[i];
                sc = (row0 + i < a.n_rows) ? sc : NEG_INF;
                // comparisons are false for NaN: NaN scores are dropped.  Ties count as separate rows: a tie with m1
                // becomes m2 (with its own position), a tie with m2 becomes m3.
                const bool gt1 = sc > m1, gt2 = sc > m2;
                const uint32_t pos = (uint32_t)(t * 16 + i);
                m3 = gt2 ? m2 : fmaxf(m3, sc);
                ap = gt1 ? ((ap << 8) | pos) : (gt2 ? ((ap & 0xffu) | (pos << 8)) : ap);
                m2 = gt1 ? m1 : fmaxf(m2, sc);
                m1 = gt1 ? sc : m1;
            }
        }
        if (EPI == 1) {
            // per query group: the query's scale (int8; positive, so the order is unchanged and the positions ride through it), the
            // lane's row group into the positions, then the four lanes that share the query insert each other's triples
            auto finish = [&](float x1, float x2, float x3, const float qs, float& wm, const int ql) {
                if constexpr (I8 != 0) { x1 = rq_scale_pos(x1, qs); x2 = rq_scale_pos(x2, qs); x3 = rq_scale_pos(x3, qs); }
                const uint32_t kgb = (uint32_t)kg << 2;
                x1 = __uint_as_float(__float_as_uint(x1) | kgb); x2 = __uint_as_float(__float_as_uint(x2) | kgb); x3 = __uint_as_float(__float_as_uint(x3) | kgb);
#pragma unroll
                for (int off = 16; off <= 32; off <<= 1) {
                    const float o1 = __shfl_xor(x1, off, 64), o2 = __shfl_xor(x2, off, 64), o3 = __shfl_xor(x3, off, 64);
                    rq_insert3(x1, x2, x3, o1);
                    rq_insert3(x1, x2, x3, o2);
                    rq_insert3(x1, x2, x3, o3);
                }
                asm("v_max_f32 %0, %1, %2" : "=v"(wm) : "v"(wm), "v"(x1));
                if (kg == 0) stg[ql * SQ + (lq & (SQ - 1))] = rq_record_from_triple(x1, x2, x3);
            };
            finish(m1, m2, m3, qsc, wmax, 16 * QG * wave + r16);
            if constexpr (QG == 2) finish(n1, n2, n3, qsc1, wmax1, 16 * QG * wave + 16 + r16);
        } else {
        // merge the four lane groups that share this query (lanes r16, r16+16, r16+32, r16+48): all end up equal
        ap = (ap & 0xffffu) + (uint32_t)(4 * kg) * 0x0101u;
        // merge the sorted triples of the two lists (this lane's and the other lane's): both lanes compute the same
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64), o3 = __shfl_xor(m3, off, 64);
            const uint32_t op = (uint32_t)__shfl_xor((int)ap, off, 64);
            // W = the list whose head wins (ties: smaller row), L = the other one
            const bool ow = o1 > m1 || (o1 == m1 && (op & 0xffu) < (ap & 0xffu));
            const float w1 = ow ? o1 : m1, w2 = ow ? o2 : m2, w3 = ow ? o3 : m3;
            const float l1 = ow ? m1 : o1, l2 = ow ? m2 : o2;
            const uint32_t wp = ow ? op : ap, lp = ow ? ap : op;
            const bool tl = l1 > w2 || (l1 == w2 && (lp & 0xffu) < (wp >> 8));   // L's head is the second largest
            m1 = w1;
            m2 = tl ? l1 : w2;
            m3 = tl ? fmaxf(w2, l2) : fmaxf(w3, l1);
            ap = (wp & 0xffu) | (tl ? (lp & 0xffu) << 8 : (wp & 0xff00u));
        }
        wmax = fmaxf(wmax, m1);
        if (kg == 0) {   // the four lane groups hold the same record
            const uint32_t c2 = rq_code16(m2), c3 = rq_code16(m3), d = c2 - c3;   // c3 <= c2
            stg[(16 * wave + r16) * SQ + (lq & (SQ - 1))] =
                make_uint2(rq_up26(m1) | (ap & 63u), (c2 << 16) | ((d < 1023u ? d : 1023u) << 6) | ((ap >> 8) & 63u));
        }
        }
        if ((lq & (SQ - 1)) == SQ - 1 || lq == nloc - 1)
            flush(q_lo + (lq & ~(SQ - 1)), (lq & (SQ - 1)) + 1);
    }
    // per-workgroup maximum of every query: wgmax[query][workgroup]
    wmax = fmaxf(wmax, __shfl_xor(wmax, 16, 64));
    wmax = fmaxf(wmax, __shfl_xor(wmax, 32, 64));
    if (kg == 0 && 16 * QG * wave + r16 < a.nq_valid) a.wgmax[(int64_t)(16 * QG * wave + r16) * a.wgmax_stride + b] = wmax;
    if constexpr (QG == 2) {
        wmax1 = fmaxf(wmax1, __shfl_xor(wmax1, 16, 64));
        wmax1 = fmaxf(wmax1, __shfl_xor(wmax1, 32, 64));
        if (kg == 0 && 16 * QG * wave + 16 + r16 < a.nq_valid) a.wgmax[(int64_t)(16 * QG * wave + 16 + r16) * a.wgmax_stride + b] = wmax1;
    }
}

// ring + [2 parities][64 row scales] + record staging [16 * QW queries][rq_stage_quads(QW)]
static constexpr size_t rq_scan_lds_bytes(int S, int KS, int QW, int QG = 1) {
    return (size_t)S * (24576 / KS) + 512 + (size_t)16 * QW * QG * rq_stage_quads(QW) * 8;
}
