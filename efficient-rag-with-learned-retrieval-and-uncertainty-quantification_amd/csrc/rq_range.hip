// rq_range.hip -- range searches (include/rq.h rq_search_range*): every row whose score reaches a per-query threshold -- the exact
// count, and the best min(count, cap) of them in the canonical order.
//
// The top-k routes ask "which bins can hold one of the k best rows"; a range search asks the simpler question "which bins can hold
// a row that reaches thr", and the scan has already written the answer's proof: per query and 64-row bin an upper bound m1 of the
// bin's best approximate score (rq_device.h).  rq_certified(m1, eps, ..., thr) -- the certificate's last step with the threshold
// in the place of the k-th score -- proves that no row of the bin has an fp32 score >= thr; such a bin is skipped, every other
// bin's rows are re-scored with rq_rowdot.h (the bits of every other route) and compared with thr as fp32 values.  What a call does
// is decided by rq_range_plan.h: nothing (no row to return), the scan route (run_pipeline stopped after its scan passes, then
// rq_range_tail_kernel), for filtered calls the gather route (rq_gather_score_kernel over the listed rows) or the exact scan of the
// shard (rq_exact_scan_kernel); the last two empty the keys below the threshold (rq_range_thr_kernel).  Every route ends in
// rq_final_kernel with k = cap over the query's qualifying keys.  The `where`-less "all passages at least this similar" a vector
// store offers next to the collection.query of reference rag_uq/streaming_index.py:355-359.
#include "rq_range_plan.h"
#include "rq_final_body.h"   // RQ_TINY_QUERY_NORM
#include "rq_rowdot.h"
#include "rq_repair.h"

// ---- kernels ------------------------------------------------------------------------------------
struct RqRangeTailArgs {
    const void* x; int dpad;          // stored rows and their length in elements (768 or 384)
    const double* rownorm64;
    int64_t n_rows;
    const uint2* bins; int64_t bins_stride; int64_t nbins;   // the scan's records of the group's queries
    const float* q32;                 // [queries][768] raw fp32 queries, zero padded (rq_prep_body)
    const double* qnorm64;            // [queries]
    const float* thr;                 // [queries]
    const uint32_t* bits;             // a filtered call: the allowed rows' bitmap, else null
    const uint32_t* first;            // a filtered call: its first min(na, RQ_MAX_K) allowed rows
    int64_t n_allowed;                // rows that can qualify: the filter's allowed rows, else n_rows
    int metric;
    float eps, max_row_norm;          // the scan's bound (rq_plan.h scan_eps) and the largest row norm, as the certificate takes them
    int cap, ccap;                    // results per query; candidate keys per query (>= cap)
    uint64_t* cand;                   // [queries][ccap], zero before the launch
    unsigned* slot;                   // [queries] qualifying rows that asked for a place in cand, zero before the launch
    int64_t* count;                   // [queries] zero before the launch
    int* status;                      // [queries] zero before the launch; 1 = overflow or a non-finite query: the fixup's
    unsigned long long* bins_rescored;   // the call's re-scored bins, all queries ("range_bins_last")
};

__device__ __forceinline__ bool rq_range_bit(const uint32_t* bits, int64_t row) { return (bits[row >> 5] >> (row & 31)) & 1u; }
__device__ __forceinline__ bool rq_finite32(float v) { return v - v == 0.f; }

// grid (queries of the group, ceil(nbins / RQ_RANGE_CHUNK)), 256 threads.  Phase 1: the workgroup walks its chunk of the query's
// bin records and lists the bins that rq_certified cannot rule out.  Phase 2: the listed bins' rows, 64 per bin, are re-scored as
// rq_gather_score_kernel re-scores its list: 16 lanes per row, a wave takes 8 rows per round, the summation order of rq_rowdot.h.
// A row at or beyond n_rows (the ragged last bin) loads the shard's last row -- a valid address -- and is dropped.
template <int DP, bool FILT>
__global__ __launch_bounds__(256) void rq_range_tail_kernel(RqRangeTailArgs a) {
    static_assert(DP == 384 || DP == RQ_DPAD, "stored row length");
    constexpr int NP = DP / 128;   // 16-byte loads per lane and row
    __shared__ __attribute__((aligned(16))) float qs[RQ_DPAD];
    __shared__ int list[RQ_RANGE_CHUNK];
    __shared__ int nlist;
    __shared__ unsigned lcount;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x, chunk = (int)blockIdx.y;
    const float thr = a.thr[q];
    const double qn = a.qnorm64[q];
    if (!rq_finite32(thr)) return;   // (uniform) such a query returns nothing: count 0, status 0 (include/rq.h)
    if (!(qn - qn == 0.0)) {         // a NaN or infinite query: the scan's records say nothing about it -> the fixup's exact route
        if (chunk == 0 && tid == 0) a.status[q] = 1;
        return;
    }
    if (qn == 0.0) {                 // every row scores 0.0: all of them qualify, or none
        if (chunk == 0 && thr <= 0.f) {
            const int64_t kk = a.n_allowed < a.cap ? a.n_allowed : a.cap;
            for (int j = tid; j < kk; j += 256) a.cand[(int64_t)q * a.ccap + j] = rq_make_key(0.f, FILT ? a.first[j] : (uint32_t)j);
            if (tid == 0) a.count[q] = a.n_allowed;
        }
        return;
    }
    // (cosine: below RQ_TINY_QUERY_NORM the 1e-30 of the score definition is no longer negligible against the scan's pure cosine:
    // nothing is skipped for such a query, which makes its answer exact by construction)
    const bool may_skip = !(a.metric == 0 && qn < RQ_TINY_QUERY_NORM);
    if (tid == 0) { nlist = 0; lcount = 0; }
    __syncthreads();
    const int64_t b0 = (int64_t)chunk * RQ_RANGE_CHUNK;
    const int64_t b1 = b0 + RQ_RANGE_CHUNK < a.nbins ? b0 + RQ_RANGE_CHUNK : a.nbins;
    const uint2* rec = a.bins + (int64_t)q * a.bins_stride;
    for (int64_t b = b0 + tid; b < b1; b += 256) {
        const float m1 = rq_rec_m1(rec[b].x);
        // skipped iff the bound proves that every row of the bin scores below thr (a NaN m1 proves nothing: not skipped)
        if (!(may_skip && rq_certified((double)m1, a.eps, a.max_row_norm, qn, a.metric, thr))) list[atomicAdd(&nlist, 1)] = (int)(b - b0);
    }
    __syncthreads();
    const int n = nlist;
    if (n == 0) return;   // uniform over the workgroup
    if (tid == 0) atomicAdd(a.bins_rescored, (unsigned long long)n);
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) qs[pp * 256 + tid] = a.q32[(size_t)q * RQ_DPAD + pp * 256 + tid];
    __syncthreads();
    const int sub = lane & 15, rloc = lane >> 4;
    const char* xb = (const char*)a.x;
    uint64_t* out = a.cand + (int64_t)q * a.ccap;
    const int jobs = n * RQ_BIN_ROWS;   // <= 2048 x 64
    for (int j0 = wave * 8; j0 < jobs; j0 += 32) {
        rq_half8 xv[2][NP];
        int64_t rows[2];
        double rn[2];
        bool lv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int job = j0 + u * 4 + rloc;   // < jobs: a multiple of 64
            rows[u] = (b0 + list[job >> 6]) * RQ_BIN_ROWS + (job & 63);
            lv[u] = rows[u] < a.n_rows;
            if (!lv[u]) rows[u] = a.n_rows - 1;   // (never an address outside the shard)
            if (FILT) lv[u] = lv[u] && rq_range_bit(a.bits, rows[u]);
            rn[u] = a.rownorm64[rows[u]];
            const char* r = xb + rows[u] * (DP * 2) + sub * 16;
#pragma unroll
            for (int pp = 0; pp < NP; ++pp) xv[u][pp] = *(const rq_half8*)(r + pp * 256);
        }
        double dot[2];
        rq_rowdot16<NP, 2>(xv, qs, sub, dot);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (sub == 0 && lv[u]) {
                double sc = dot[u];
                if (a.metric == 0) sc = dot[u] / (qn * rn[u] + 1e-30);
                float s = rq_sanitize((float)sc);
                if (s == 0.f) s = 0.f;   // -0.0 is +0.0, as in every key (rq_make_key)
                if (s >= thr) {          // the comparison of include/rq.h: on the fp32 values
                    atomicAdd(&lcount, 1u);
                    const unsigned pos = atomicAdd(&a.slot[q], 1u);
                    if (pos < (unsigned)a.ccap) out[pos] = rq_make_key(s, (uint32_t)rows[u]);
                    else a.status[q] = 1;   // overflow: the count stays exact, the fixup re-runs the query on the exact route
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0 && lcount) atomicAdd((unsigned long long*)&a.count[q], (unsigned long long)lcount);
}

// The exact and gather routes: cand[q][0 .. per) holds a key (score, LOCAL row) or 0 for every row in play.  Keys below the query's
// threshold are emptied and the others counted; a non-finite threshold empties all of them.  grid (queries, tiles of 4096 keys).
#define RQ_RANGE_THR_TILE 4096
__global__ __launch_bounds__(256) void rq_range_thr_kernel(uint64_t* cand, int64_t per, const float* thr_all, int64_t* count) {
    __shared__ unsigned lcount;
    const int tid = threadIdx.x;
    const int q = (int)blockIdx.x;
    const float thr = thr_all[q];
    const bool live = rq_finite32(thr);
    if (tid == 0) lcount = 0;
    __syncthreads();
    uint64_t* c = cand + (int64_t)q * per;
    unsigned mine = 0;
    for (int64_t base = (int64_t)blockIdx.y * RQ_RANGE_THR_TILE; base < per; base += (int64_t)gridDim.y * RQ_RANGE_THR_TILE) {
        for (int i = tid; i < RQ_RANGE_THR_TILE; i += 256) {
            const int64_t j = base + i;
            if (j >= per) break;
            const uint64_t key = c[j];
            if (key == 0) continue;
            if (live && rq_key_score(key) >= thr) mine++;
            else c[j] = 0;
        }
    }
    if (mine) atomicAdd(&lcount, mine);
    __syncthreads();
    if (tid == 0 && lcount) atomicAdd((unsigned long long*)&count[q], (unsigned long long)lcount);
}

static hipError_t rq_range_tail_launch(const RqRangeTailArgs& a, int queries, hipStream_t stream) {
    if (queries < 1 || queries > 65535 || a.nbins < 1 || a.n_rows < 1 || a.cap < 1 || a.ccap < a.cap || (a.dpad != 384 && a.dpad != RQ_DPAD)) return hipErrorInvalidValue;
    if (a.nbins > a.bins_stride) return hipErrorInvalidValue;
    const dim3 grid((unsigned)queries, range_chunks(a.nbins));
    if (grid.y > 65535) return hipErrorInvalidValue;   // (134M bins: beyond a shard's 2^32 rows)
    const bool filt = a.bits != nullptr;
    if (a.dpad == 384) {
        if (filt) hipLaunchKernelGGL((rq_range_tail_kernel<384, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((rq_range_tail_kernel<384, false>), grid, dim3(256), 0, stream, a);
    } else {
        if (filt) hipLaunchKernelGGL((rq_range_tail_kernel<RQ_DPAD, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((rq_range_tail_kernel<RQ_DPAD, false>), grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

static hipError_t rq_range_thr_launch(uint64_t* cand, int64_t per, int queries, const float* thr, int64_t* count, hipStream_t stream) {
    if (queries < 1 || queries > 65535 || per < 1) return hipErrorInvalidValue;
    const int64_t tiles = std::min<int64_t>((per + RQ_RANGE_THR_TILE - 1) / RQ_RANGE_THR_TILE, 65535);   // (a workgroup strides beyond)
    hipLaunchKernelGGL(rq_range_thr_kernel, dim3((unsigned)queries, (unsigned)tiles), dim3(256), 0, stream, cand, per, thr, count);
    return hipGetLastError();
}

// ---- routes -------------------------------------------------------------------------------------
struct RangeOut {   // a call's device outputs (keys may be null); from: those of its queries from `off` on
    float* scores; int64_t* rows; uint64_t* keys; int64_t* count; int* status;
    RangeOut from(int off, int cap) const {
        return {scores + (size_t)off * cap, rows + (size_t)off * cap, keys ? keys + (size_t)off * cap : nullptr, count + off, status + off};
    }
};

// The sorted outputs of g queries from their qualifying keys (per each, 0 = empty): rq_final_kernel with k = cap.  Every row in
// play was scored (nbins <= nb: nothing to certify); the norms it is given are 1.0, because the keys of a zero-norm query are
// already its answer -- the kernel's own shortcut would return rows at 0.0 also when thr > 0.
static int range_final(rq_index* idx, const Workspace& w, const uint64_t* cand, int64_t per, int g, int cap, const RangeOut& o, hipStream_t s) {
    RqFinalArgs fa{};
    fa.cand = cand; fa.ncand = (int)per; fa.binkeys = nullptr; fa.binkeys_stride = 0; fa.nb = 1; fa.nbins = 1;
    fa.qnorm64 = w.rg_one; fa.metric = 0; fa.eps = 0.f; fa.max_row_norm = 0.f; fa.k = cap; fa.row_offset = idx->row_offset; fa.n_rows = per;
    fa.first = nullptr;
    fa.out_scores = o.scores; fa.out_rows = o.rows; fa.out_keys = o.keys; fa.out_status = w.rg_status;
    HIPCHK(rq_final_launch(fa, g, s));
    return RQ_OK;
}

static int range_scan_route(rq_index* idx, const rq_filter* f, const float* d_q, int B, const float* d_thr, int cap, int metric, const RangeOut& out, hipStream_t s) {
    const int ccap = range_cand_capacity(cap, idx->range_cand_cap);
    if (!idx->range_bins) HIPCHK(hipMalloc((void**)&idx->range_bins, sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(idx->range_bins, 0, sizeof(unsigned long long), s));
    idx->range_bins_valid = true;
    const RangeGroups gr = range_groups(RROUTE_SCAN, B, 0);
    for (int i = 0; i < gr.count; ++i) {
        const int off = i * gr.group, g = std::min(gr.group, B - off);
        const RangeOut o = out.from(off, cap);
        ScanOnly so;
        so.cand_elems = (size_t)g * (size_t)ccap;
        // the call's usual fp16 scan passes: use8 = false, flags 0, the masked scale when filtered; no tail follows
        if (int r = run_pipeline(idx, d_q + (size_t)off * idx->dim, g, 1, metric, 0, {o.scores, o.rows, o.keys, o.status}, s, 0, f, &so)) return r;
        Workspace& w = *so.w;
        if (int r = ensure_range_ws(w, w.bcap)) return r;
        HIPCHK(hipMemsetAsync(w.cand, 0, so.cand_elems * sizeof(uint64_t), s));
        HIPCHK(hipMemsetAsync(w.rg_slot, 0, (size_t)g * sizeof(unsigned), s));
        RqRangeTailArgs a;
        a.x = idx->x; a.dpad = idx->dpad; a.rownorm64 = idx->rownorm64; a.n_rows = idx->n;
        a.bins = w.bins; a.bins_stride = w.bins_stride; a.nbins = (idx->n + 63) / 64;
        a.q32 = w.qs.q32; a.qnorm64 = w.qs.qn; a.thr = d_thr + off;
        a.bits = f ? f->d_bits : nullptr; a.first = f ? f->d_first : nullptr; a.n_allowed = f ? f->na : idx->n;
        a.metric = metric; a.eps = scan_eps(idx, metric); a.max_row_norm = (float)(idx->max_row_norm * (1.0 + 1e-6));
        a.cap = cap; a.ccap = ccap; a.cand = w.cand; a.slot = w.rg_slot; a.count = o.count; a.status = o.status;
        a.bins_rescored = idx->range_bins;
        HIPCHK(rq_range_tail_launch(a, g, s));
        if (int r = range_final(idx, w, w.cand, ccap, g, cap, o, s)) return r;
    }
    return RQ_OK;
}

// The exact route (f: excluded rows' keys emptied first) and, with `gather`, the filter's listed rows instead of the shard.
static int range_keyed_route(rq_index* idx, const rq_filter* cf, bool gather, const float* d_q, int B, const float* d_thr, int cap, int metric,
                             const RangeOut& out, hipStream_t s) {
    rq_filter* f = const_cast<rq_filter*>(cf);
    if (gather)
        if (int r = ensure_filter_list(f)) return r;
    const int64_t nbins = (idx->n + 63) / 64;
    const int64_t per = gather ? f->na : nbins * RQ_BIN_ROWS;
    if (per > INT32_MAX) return set_err(RQ_EUNSUPPORTED, "a range search over %lld keys per query", (long long)per);
    const RangeGroups gr = range_groups(gather ? RROUTE_GATHER : RROUTE_EXACT, B, per);
    const int slots = (gr.group + 63) / 64 * 64;
    const QuerySet* qs = nullptr;
    uint64_t* cand = nullptr;
    if (int r = scanless_workspace(idx, s, slots, (size_t)gr.group * (size_t)per, &qs, &cand)) return r;
    Workspace& w = idx->ctx[s].w[0];
    if (int r = ensure_range_ws(w, w.bcap)) return r;
    for (int i = 0; i < gr.count; ++i) {
        const int off = i * gr.group, g = std::min(gr.group, B - off);
        const RangeOut o = out.from(off, cap);
        HIPCHK(rq_prep_queries_launch(prep_args(*qs, d_q + (size_t)off * idx->dim, idx->dim, g, (g + 63) / 64 * 64, false), s));
        if (gather) {
            RqGatherArgs ga;
            ga.x = idx->x; ga.dpad = idx->dpad; ga.rownorm64 = idx->rownorm64; ga.q32 = qs->q32; ga.qnorm64 = qs->qn;
            ga.list = f->d_list; ga.nlist = per; ga.metric = metric; ga.cand = cand; ga.cand_stride = per;
            HIPCHK(rq_gather_score_launch(ga, g, s));
        } else {
            RqRescoreArgs ra;
            ra.x = idx->x; ra.dpad = idx->dpad; ra.q32 = qs->q32; ra.qnorm64 = qs->qn; ra.rownorm64 = idx->rownorm64;
            ra.binkeys = nullptr; ra.binkeys_stride = 1; ra.nb = (int)nbins; ra.metric = metric; ra.n_rows = idx->n; ra.cand = cand;
            if (idx->exact_mfma) HIPCHK(rq_exact_scan_launch(ra, g, idx->cu_count, s));
            else HIPCHK(rq_rescore_launch(ra, g, s));
            if (f) HIPCHK(rq_mask_keys_launch(cand, (int64_t)g * per, f->d_bits, s));
        }
        HIPCHK(rq_range_thr_launch(cand, per, g, d_thr + off, o.count, s));
        if (int r = range_final(idx, w, cand, per, g, cap, o, s)) return r;
    }
    return RQ_OK;
}

static int range_fill_empty(int B, int cap, const RangeOut& out, hipStream_t s) {
    HIPCHK(hipMemsetAsync(out.scores, 0, (size_t)B * cap * sizeof(float), s));
    HIPCHK(hipMemsetAsync(out.rows, 0xff, (size_t)B * cap * sizeof(int64_t), s));
    if (out.keys) HIPCHK(hipMemsetAsync(out.keys, 0, (size_t)B * cap * sizeof(uint64_t), s));
    return RQ_OK;
}

// forced: the route to take (-1 = option "range_route", then the rule).  count: one more call for "range_calls" / rq_timing.
static int search_range_device(rq_index* idx, const rq_filter* f, const float* d_q, int B, const float* d_thr, int cap, int metric, const RangeOut& out,
                               hipStream_t s, int forced, bool count) {
    // like a "pipeline" = 0 call: whatever the stream still defers (fused tail, scanned-ahead pair, hint) is completed first
    if (int r = flush_tails(idx, s)) return r;
    if (count) {
        idx->t.searches++;
        idx->t.queries += B;
        idx->range_calls++;
    }
    FilterShape shape;
    if (f) shape = FilterShape{f->n, f->na, f->occ_prefix.data()};
    const int route = plan_range(idx, f ? &shape : nullptr, B, metric, forced >= 0 ? forced : idx->range_route);
    if (count) idx->range_route_last = route;
    HIPCHK(hipMemsetAsync(out.count, 0, (size_t)B * sizeof(int64_t), s));
    HIPCHK(hipMemsetAsync(out.status, 0, (size_t)B * sizeof(int), s));
    if (count && route != RROUTE_SCAN) idx->range_bins_valid = false;   // (a repair leaves the statistic of the call it repairs)
    if (route == RROUTE_EMPTY) {
        if (int r = mark_no_scan(idx, s)) return r;
        return range_fill_empty(B, cap, out, s);
    }
    if (route == RROUTE_SCAN) return range_scan_route(idx, f, d_q, B, d_thr, cap, metric, out, s);
    return range_keyed_route(idx, f, route == RROUTE_GATHER, d_q, B, d_thr, cap, metric, out, s);
}

// Synchronises `s`, re-runs the queries whose status is non-zero (overflowed candidate lists, non-finite queries) on the exact
// route and patches the outputs in place.  Returns how many.
static int range_fixup(rq_index* idx, const rq_filter* f, const float* d_q, int B, const float* d_thr, int cap, int metric, const RangeOut& out, hipStream_t s) {
    if (int r = flush_tails(idx, s)) return r;
    Stage fx(s);
    RepairList bad;
    if (int r = repair_flagged(fx, out.status, B, bad)) return r;
    if (bad.empty()) return 0;
    const int nb = (int)bad.size();
    idx->range_repaired += nb;
    idx->repaired_total += nb;
    idx->t.exact_scans += nb;
    const RangeStaging sz = range_staging(idx->dim, nb, cap);
    const size_t bytes[7] = {sz.q, sz.thr, sz.scores, sz.rows, sz.rows, sz.count, sz.status};
    if (int r = fx.alloc(bytes, 7, "the repair of a range search")) return r;
    float* fq = fx.at<float>(0); float* fthr = fx.at<float>(1);
    const RangeOut fo{fx.at<float>(2), fx.at<int64_t>(3), out.keys ? fx.at<uint64_t>(4) : nullptr, fx.at<int64_t>(5), fx.at<int>(6)};
    if (int r = repair_pack(fx, bad, {repair_col(d_q, fq, (size_t)idx->dim), repair_col(d_thr, fthr, 1)})) return r;
    if (int r = search_range_device(idx, f, fq, nb, fthr, cap, metric, fo, s, RROUTE_EXACT, false)) return r;
    const size_t c = (size_t)cap;   // (the re-run's status comes back as a column)
    if (int r = repair_unpack(fx, bad, {repair_col(out.scores, fo.scores, c), repair_col(out.rows, fo.rows, c), repair_col(out.keys, fo.keys, c),
                                        repair_col(out.count, fo.count, 1), repair_col(out.status, fo.status, 1)})) return r;
    if (int r = fx.finish()) return r;
    return nb;
}

// ---- entry points -------------------------------------------------------------------------------
static int check_range_call(const rq_index* idx, const rq_filter* f, const void* q, int B, const void* thr, const float* host_thr, int cap, int metric,
                            const void* scores, const void* rows, const void* count) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_range_args(idx, q, B, thr, host_thr, cap, metric, scores, rows, count)) return r;
    if (f)
        if (int r = check_filter(idx, f)) return r;
    return RQ_OK;
}

extern "C" int rq_search_range_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, const float* d_thr, int cap, int metric,
                                      float* d_scores, int64_t* d_rows, uint64_t* d_keys, int64_t* d_count, int* d_status, void* stream) {
    if (int r = check_range_call(idx, f, d_queries, B, d_thr, nullptr, cap, metric, d_scores, d_rows, d_count)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return search_range_device(idx, f, d_queries, B, d_thr, cap, metric, {d_scores, d_rows, d_keys, d_count, d_status}, (hipStream_t)stream, -1, true);
}

extern "C" int rq_search_range_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, const float* d_thr, int cap, int metric,
                                            float* d_scores, int64_t* d_rows, uint64_t* d_keys, int64_t* d_count, int* d_status, void* stream) {
    if (int r = check_range_call(idx, f, d_queries, B, d_thr, nullptr, cap, metric, d_scores, d_rows, d_count)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return range_fixup(idx, f, d_queries, B, d_thr, cap, metric, {d_scores, d_rows, d_keys, d_count, d_status}, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h).
extern "C" int rq_search_range(rq_index* idx, const rq_filter* f, const float* queries, int B, const float* thr, int cap, int metric,
                               float* out_scores, int64_t* out_rows, int64_t* out_count) {
    if (int r = check_range_call(idx, f, queries, B, thr, thr, cap, metric, out_scores, out_rows, out_count)) return r;
    RQ_ON_DEVICE(idx);
    const RangeStaging sz = range_staging(idx->dim, B, cap);
    const size_t bytes[6] = {sz.q, sz.thr, sz.scores, sz.rows, sz.count, sz.status};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 6, "a range search")) return r;
    float* d_q = st.at<float>(0); float* d_thr = st.at<float>(1);
    const RangeOut o{st.at<float>(2), st.at<int64_t>(3), nullptr, st.at<int64_t>(4), st.at<int>(5)};
    st.up(d_q, queries, sz.q);
    if (int r = st.up(d_thr, thr, sz.thr)) return r;
    if (int r = search_range_device(idx, f, d_q, B, d_thr, cap, metric, o, st.s, -1, true)) return r;
    if (int r = range_fixup(idx, f, d_q, B, d_thr, cap, metric, o, st.s); r < 0) return r;
    st.down(out_scores, o.scores, sz.scores);
    st.down(out_rows, o.rows, sz.rows);
    st.down(out_count, o.count, sz.count);
    return st.finish();
}
