// rq_score.hip -- scoring given rows (include/rq.h rq_score_rows_device, rq_score_rows): the exact score of every (query, row) pair
// of one list of rows per query, next to the rows.
//
// A search ranks the shard for a query; hybrid retrieval then asks for the dense score of passages that came from the OTHER
// retriever (reference rag_uq/streaming_index.py:485-523 writes 0.0 for them, :498-499: Chroma scores only what its query returns).
// Here that is one row read per pair: the queries are prepared as for every other call (rq_prep_queries_launch: fp32 padded query,
// fp64 norm), and every dot product is rq_rowdot.h's -- 16 lanes per row, fp64 products in element order, xor butterfly -- so a
// pair's score has the bits rq_search and the filter's gather route return for it.  Unlike the gather route (one list for all
// queries, re-read from the caches by the workgroups in flight together) every query has its own list: a random whole-row gather.
#include "rq_score_plan.h"
#include "rq_rowdot.h"
#include "rq_stage.h"

// ---- kernel -------------------------------------------------------------------------------------
// grid (queries of the group, ceil(m / RQ_SCORE_TILE)), 256 threads.  The workgroup keeps its query in LDS; a wave takes 8 list
// positions per round (lane group rloc = lane >> 4 owns positions j0 + rloc and j0 + 4 + rloc: NP x 2 sixteen-byte loads per lane
// before the first product).  An absent entry (outside the shard, or beyond m) loads stored row 0 -- a valid address, the shard
// holds a row -- and drops it; its score is 0.0.
template <int DP>
__global__ __launch_bounds__(RQ_SCORE_THREADS) void rq_score_rows_kernel(RqScoreArgs a) {
    static_assert(DP == 384 || DP == RQ_DPAD, "stored row length");
    static_assert(RQ_SCORE_THREADS == 256 && RQ_SCORE_TILE % 32 == 0, "4 waves x 8 positions per round");
    constexpr int NP = DP / 128;   // 16-byte loads per lane and row
    __shared__ __attribute__((aligned(16))) float qs[RQ_DPAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x;
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) qs[pp * 256 + tid] = a.q32[(size_t)q * RQ_DPAD + pp * 256 + tid];
    __syncthreads();
    const double qn = a.qnorm64[q];
    const int sub = lane & 15, rloc = lane >> 4;
    const char* xb = (const char*)a.x;
    const int base = (int)blockIdx.y * RQ_SCORE_TILE;
    const int64_t* list = a.rows + (int64_t)q * a.m;
    float* out = a.scores + (int64_t)q * a.m;
    const int64_t lo = a.row_offset, hi = a.row_offset + a.n_rows;
    for (int j0 = wave * 8; j0 < RQ_SCORE_TILE; j0 += RQ_SCORE_THREADS / 8) {
        if (base + j0 >= a.m) break;   // uniform over the wave
        rq_half8 xv[2][NP];
        int pos[2];
        double rn[2];
        bool inlist[2], present[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pos[u] = base + j0 + u * 4 + rloc;
            inlist[u] = pos[u] < a.m;
            const int64_t g = inlist[u] ? list[pos[u]] : (int64_t)-1;
            present[u] = inlist[u] && g >= lo && g < hi;
            const int64_t row = present[u] ? g - lo : 0;   // (never an address outside the shard)
            rn[u] = a.rownorm64[row];
            const char* r = xb + row * (DP * 2) + sub * 16;
#pragma unroll
            for (int pp = 0; pp < NP; ++pp) xv[u][pp] = *(const rq_half8*)(r + pp * 256);
        }
        double dot[2];
        rq_rowdot16<NP, 2>(xv, qs, sub, dot);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (sub == 0 && inlist[u]) {
                double sc = dot[u];
                if (a.metric == 0) sc = dot[u] / (qn * rn[u] + 1e-30);
                if (qn == 0.0) sc = 0.0;   // a zero-norm query scores every row 0 (include/rq.h), as rq_gather_score_kernel
                float s = rq_sanitize((float)sc);
                if (s == 0.f) s = 0.f;     // -0.0 leaves as +0.0, as from every key (rq_make_key)
                out[pos[u]] = present[u] ? s : 0.f;
            }
        }
    }
}

hipError_t rq_score_rows_launch(const RqScoreArgs& a, int queries, hipStream_t stream) {
    if (queries < 1 || queries > 65535 || a.m < 1 || a.m > RQ_MAX_SCORE_ROWS || a.n_rows < 1 || (a.dpad != 384 && a.dpad != RQ_DPAD)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)queries, (unsigned)((a.m + RQ_SCORE_TILE - 1) / RQ_SCORE_TILE));
    if (a.dpad == 384) hipLaunchKernelGGL(rq_score_rows_kernel<384>, grid, dim3(RQ_SCORE_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(rq_score_rows_kernel<RQ_DPAD>, grid, dim3(RQ_SCORE_THREADS), 0, stream, a);
    return hipGetLastError();
}

// ---- entry points -------------------------------------------------------------------------------
static int score_rows_device(rq_index* idx, const float* d_q, int B, const int64_t* d_rows, int m, int metric, float* d_scores, hipStream_t s) {
    // like a "pipeline" = 0 call: whatever the stream still defers is completed first (the prepared-query slots are the stream's)
    if (int r = flush_tails(idx, s)) return r;
    idx->score_calls++;
    idx->score_pairs += (int64_t)B * m;
    if (idx->n == 0) {   // every entry is absent
        if (int r = mark_no_scan(idx, s)) return r;
        HIPCHK(hipMemsetAsync(d_scores, 0, (size_t)B * (size_t)m * sizeof(float), s));
        return RQ_OK;
    }
    const ScoreGroups g = score_groups(B);
    const QuerySet* qs = nullptr;
    if (int r = scanless_workspace(idx, s, g.slots, 0, &qs, nullptr)) return r;
    for (int i = 0; i < g.count; ++i) {
        const int off = i * g.group, nq = std::min(g.group, B - off);
        const RqPrepArgs pa = prep_args(*qs, d_q + (size_t)off * idx->dim, idx->dim, nq, (nq + 63) / 64 * 64, false);
        const ScoreGeometry geo = score_geometry(idx, nq, m);
        RqScoreArgs a;
        a.x = idx->x; a.dpad = geo.dp; a.rownorm64 = idx->rownorm64; a.n_rows = idx->n; a.row_offset = idx->row_offset;
        a.q32 = qs->q32; a.qnorm64 = qs->qn; a.rows = d_rows + (size_t)off * (size_t)m; a.m = m; a.metric = metric;
        a.scores = d_scores + (size_t)off * (size_t)m;
        HIPCHK(rq_prep_queries_launch(pa, s));
        HIPCHK(rq_score_rows_launch(a, (int)geo.grid_x, s));
    }
    return RQ_OK;
}

extern "C" int rq_score_rows_device(rq_index* idx, const float* d_queries, int B, const int64_t* d_rows, int m, int metric, float* d_scores, void* stream) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_score_args(idx, d_queries, B, d_rows, m, metric, d_scores)) return r;
    RQ_ON_DEVICE(idx);
    return score_rows_device(idx, d_queries, B, d_rows, m, metric, d_scores, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h).
extern "C" int rq_score_rows(rq_index* idx, const float* queries, int B, const int64_t* rows, int m, int metric, float* out_scores) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_score_args(idx, queries, B, rows, m, metric, out_scores)) return r;
    RQ_ON_DEVICE(idx);
    const ScoreStaging sz = score_staging(idx->dim, B, m);
    const size_t bytes[3] = {sz.q, sz.rows, sz.scores};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 3, "scoring given rows")) return r;
    float* d_q = st.at<float>(0); int64_t* d_rows = st.at<int64_t>(1); float* d_scores = st.at<float>(2);
    st.up(d_q, queries, sz.q);
    if (int r = st.up(d_rows, rows, sz.rows)) return r;
    if (int r = score_rows_device(idx, d_q, B, d_rows, m, metric, d_scores, st.s)) return r;
    st.down(out_scores, d_scores, sz.scores);
    return st.finish();
}
