// rq_mmr.hip -- diversified search (include/rq.h rq_mmr_select_device, rq_search_mmr): greedy maximal-marginal-relevance selection
// of k out of m candidate rows per query, next to the rows.
//
// Greedy MMR needs, after every pick, the similarities of the row just picked to the candidates that remain -- k x m row dot
// products per query, not the m x m Gram matrix.  One workgroup per query keeps the candidates' state in LDS and runs the k steps:
// (a) every thread forms v = lambda rel - (1 - lambda) pen of its candidates, the workgroup reduces to the greatest v (lowest
// position on a tie); (b) one thread writes the step's outputs; (c) the picked row is staged in LDS as fp32; (d) every remaining
// candidate's stored row is scored against it with the arithmetic of rq_gather_score_kernel (rq_rowdot.h: 16 lanes per row,
// 16-byte loads, fp64 products in element order, xor butterfly) and pen = max(pen, sim).  The last step skips (d).  The candidate
// rows are re-read from the caches at every step: they are not staged.  Replaces the host loop of a
// max_marginal_relevance_search over the collection.query of reference rag_uq/streaming_index.py:355-359.
#include "rq_mmr_plan.h"
#include "rq_rowdot.h"
#include "rq_stage.h"

// ---- kernel -------------------------------------------------------------------------------------
// (v, position) of the better of two candidates of a step: greater v, then lower position; position -1 = none.  v is never NaN.
__device__ __forceinline__ void rq_mmr_better(double& v, int& p, double ov, int op) {
    const bool take = op >= 0 && (p < 0 || ov > v || (ov == v && op < p));
    v = take ? ov : v;
    p = take ? op : p;
}

template <int DP>
__global__ __launch_bounds__(RQ_MMR_THREADS) void rq_mmr_kernel(RqMmrArgs a) {
    static_assert(DP == 384 || DP == RQ_DPAD, "stored row length");
    constexpr int NP = DP / 128;   // 16-byte loads per lane and row
    constexpr int NW = RQ_MMR_THREADS / 64;
    __shared__ float rel[RQ_MAX_K], pen[RQ_MAX_K];
    __shared__ uint32_t lrow[RQ_MAX_K];          // local row of a present candidate
    __shared__ double rn[RQ_MAX_K];              // its stored fp64 norm
    __shared__ unsigned char live[RQ_MAX_K];     // 1 = present and not yet selected
    __shared__ __attribute__((aligned(16))) float qs[DP];   // the row just picked
    __shared__ double red_v[NW];
    __shared__ int red_p[NW];
    __shared__ int n_present;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x, m = a.m, k = a.k;
    const int64_t* crow = a.cand_rows + (int64_t)q * m;
    const float* crel = a.cand_rel + (int64_t)q * m;
    float* out_s = a.out_scores + (int64_t)q * k;
    int64_t* out_r = a.out_rows + (int64_t)q * k;
    float* out_v = a.out_mmr ? a.out_mmr + (int64_t)q * k : nullptr;
    const char* xb = (const char*)a.x;

    if (tid == 0) n_present = 0;
    __syncthreads();
    for (int i = tid; i < m; i += RQ_MMR_THREADS) {
        const int64_t loc = crow[i] - a.row_offset;
        const float r = crel[i];
        const bool ok = crow[i] >= 0 && loc >= 0 && loc < a.n_rows && r == r;   // an absent candidate is never dereferenced
        rel[i] = r;
        pen[i] = 0.f;
        lrow[i] = ok ? (uint32_t)loc : 0u;
        rn[i] = ok ? a.rownorm64[loc] : 0.0;
        live[i] = ok ? 1 : 0;
        if (ok) atomicAdd(&n_present, 1);
    }
    __syncthreads();
    const int k_eff = min(k, n_present);
    for (int t = k_eff + tid; t < k; t += RQ_MMR_THREADS) {
        out_s[t] = 0.f;
        out_r[t] = -1;
        if (out_v) out_v[t] = 0.f;
    }
    const double lam = a.lambda, oml = 1.0 - a.lambda;
    const int sub = lane & 15, rloc = lane >> 4;

    for (int t = 0; t < k_eff; ++t) {
        // (a) the best (v, lowest position) among the live candidates
        double bv = 0.0;
        int bp = -1;
        for (int i = tid; i < m; i += RQ_MMR_THREADS) {
            if (!live[i]) continue;
            // two products and one subtraction, each rounded; a term whose weight is exactly 0 is 0 whatever its other factor
            // (lambda = 1: v = rel, the search's order also where a penalty is infinite; lambda = 0: v = -pen)
            const double gain = lam == 0.0 ? 0.0 : lam * (double)rel[i], loss = oml == 0.0 ? 0.0 : oml * (double)pen[i];
            double v = gain - loss;
            if (v != v) v = -__builtin_huge_val();   // (inf - inf: ranks last, as rq_sanitize ranks a NaN score)
            rq_mmr_better(bv, bp, v, i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            rq_mmr_better(bv, bp, ov, op);
        }
        if (lane == 0) { red_v[wave] = bv; red_p[wave] = bp; }
        __syncthreads();
        bv = red_v[0]; bp = red_p[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) rq_mmr_better(bv, bp, red_v[w], red_p[w]);
        // (bp >= 0: t < k_eff live candidates have been taken so far)
        const int64_t prow = (int64_t)lrow[bp];
        const double pn = rn[bp];
        // (b) the step's outputs
        if (tid == 0) {
            out_s[t] = rel[bp];
            out_r[t] = prow + a.row_offset;
            if (out_v) out_v[t] = (float)bv;
        }
        if (t + 1 == k_eff) break;   // the last step updates no penalty
        // (c) the picked row as fp32
        if (tid < DP / 8) {
            const rq_half8 h = *(const rq_half8*)(xb + prow * (DP * 2) + tid * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) qs[tid * 8 + e] = (float)h[e];
        }
        __syncthreads();             // (every thread has read live[bp], red_* and lrow[bp] before anything below changes them)
        if (tid == 0) live[bp] = 0;
        // (d) pen = max(pen, sim(candidate, picked row)) for every other live candidate: a wave takes 8 rows per round
        for (int j0 = wave * 8; j0 < m; j0 += NW * 8) {
            rq_half8 xv[2][NP];
            int slot[2];
            bool lv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                slot[u] = j0 + u * 4 + rloc;
                lv[u] = slot[u] < m && slot[u] != bp && live[slot[u]];
                const char* r = xb + (int64_t)lrow[lv[u] ? slot[u] : bp] * (DP * 2) + sub * 16;   // (not live: the picked row, read and dropped)
#pragma unroll
                for (int pp = 0; pp < NP; ++pp) xv[u][pp] = *(const rq_half8*)(r + pp * 256);
            }
            double dot[2];
            rq_rowdot16<NP, 2>(xv, qs, sub, dot);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (sub == 0 && lv[u]) {
                    double sc = dot[u];
                    if (a.metric == 0) sc = dot[u] / (pn * rn[slot[u]] + 1e-30);
                    const float s = rq_sanitize((float)sc);
                    pen[slot[u]] = (t == 0) ? s : fmaxf(pen[slot[u]], s);
                }
            }
        }
        __syncthreads();
    }
}

hipError_t rq_mmr_launch(const RqMmrArgs& a, int B, hipStream_t stream) {
    if (B < 1 || a.m < 1 || a.m > RQ_MAX_K || a.k < 1 || a.k > a.m || (a.dpad != 384 && a.dpad != RQ_DPAD)) return hipErrorInvalidValue;
    if (a.dpad == 384) hipLaunchKernelGGL(rq_mmr_kernel<384>, dim3(B), dim3(RQ_MMR_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(rq_mmr_kernel<RQ_DPAD>, dim3(B), dim3(RQ_MMR_THREADS), 0, stream, a);
    return hipGetLastError();
}

// ---- entry points -------------------------------------------------------------------------------
static int mmr_select(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_rel, int B, int m, int k, double lambda, int metric, float* d_scores,
                      int64_t* d_rows, float* d_mmr, hipStream_t s) {
    const MmrGeometry g = mmr_geometry(idx, B, m);
    RqMmrArgs a;
    a.x = idx->x; a.dpad = g.dp; a.rownorm64 = idx->rownorm64; a.n_rows = idx->n; a.row_offset = idx->row_offset;
    a.cand_rows = d_cand_rows; a.cand_rel = d_cand_rel; a.m = m; a.k = k; a.metric = metric; a.lambda = lambda;
    a.out_scores = d_scores; a.out_rows = d_rows; a.out_mmr = d_mmr;
    HIPCHK(rq_mmr_launch(a, (int)g.grid, s));
    idx->mmr_calls++;
    return RQ_OK;
}

extern "C" int rq_mmr_select_device(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_rel, int B, int m, int k, double lambda, int metric,
                                    float* d_scores, int64_t* d_rows, float* d_mmr, void* stream) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_mmr_select_args(idx, d_cand_rows, d_cand_rel, B, m, k, lambda, metric, d_scores, d_rows)) return r;
    RQ_ON_DEVICE(idx);
    return mmr_select(idx, d_cand_rows, d_cand_rel, B, m, k, lambda, metric, d_scores, d_rows, d_mmr, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h): the exact top m = min(fetch_k, rows in play), repaired
// by the ladder, so the candidates are exact; then the selection and the copies back.
extern "C" int rq_search_mmr(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int fetch_k, double lambda, int metric,
                             float* out_scores, int64_t* out_rows, float* out_mmr) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_mmr_search_args(idx, queries, B, k, fetch_k, lambda, metric, out_scores, out_rows)) return r;
    if (f) if (int r = check_filter(idx, f)) return r;
    RQ_ON_DEVICE(idx);
    hipStream_t s = idx->own_stream;
    if (int r = flush_tails(idx, s)) return r;   // like a "pipeline" = 0 call: what the stream still defers is completed first
    if (idx->n == 0) {                           // nothing to select from: padding
        for (size_t i = 0; i < (size_t)B * k; ++i) { out_scores[i] = 0.f; out_rows[i] = -1; if (out_mmr) out_mmr[i] = 0.f; }
        return RQ_OK;
    }
    const int m = mmr_fetch(k, fetch_k, f ? f->na : idx->n);
    const MmrStaging sz = mmr_staging(idx->dim, B, m, k);
    const size_t bytes[7] = {sz.q, sz.cand_scores, sz.cand_rows, sz.status, sz.out_scores, sz.out_rows, sz.out_mmr};
    Stage st(s);
    if (int r = st.alloc(bytes, out_mmr ? 7 : 6, "an MMR search")) return r;
    float* d_q = st.at<float>(0); float* d_cs = st.at<float>(1); int64_t* d_cr = st.at<int64_t>(2); int* d_status = st.at<int>(3);
    float* d_scores = st.at<float>(4); int64_t* d_rows = st.at<int64_t>(5); float* d_mmr = st.at<float>(6);   // (null without out_mmr)
    if (int r = st.up(d_q, queries, sz.q)) return r;
    if (f) {
        if (int r = search_filtered_device(idx, f, d_q, B, m, metric, {d_cs, d_cr, nullptr, d_status}, s)) return r;
    } else {
        idx->t.searches++;
        idx->t.queries += B;
        if (int r = run_pipeline(idx, d_q, B, m, metric, nb_default(idx, m), {d_cs, d_cr, nullptr, d_status}, s, CALL_ALLOW8 | CALL_FETCH)) return r;
    }
    if (int r = fixup_ladder(idx, f, d_q, B, m, metric, d_cs, d_cr, nullptr, d_status, s); r < 0) return r;
    if (int r = mmr_select(idx, d_cr, d_cs, B, m, k, lambda, metric, d_scores, d_rows, d_mmr, s)) return r;
    st.down(out_scores, d_scores, sz.out_scores);
    st.down(out_rows, d_rows, sz.out_rows);
    if (out_mmr) st.down(out_mmr, d_mmr, sz.out_mmr);
    return st.finish();
}
