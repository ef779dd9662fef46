// rq_filter.hip -- filtered searches (include/rq.h rq_filter, rq_search_filtered*): the top-k over an allowed set of rows.
//
// A filter is a bitmap over the LOCAL rows of one index.  Nothing stored changes: the scan kernels never test a row's validity
// -- pad rows carry a NaN row scale and sort last -- so a filtered scan is the same kernels over a second
// row-scale array in which excluded rows are NaN too (rq_mask_scale_kernel, the one creation kernel).  What a call does is
// decided by rq_filter_plan.h: nothing (no row allowed), the gather route (rq_gather_score_kernel: exactly the listed rows,
// re-scored in fp64 with the tail's own arithmetic, cost B x na), the scan route (run_pipeline with the filter: masked scale,
// rq_tail_kernel<NV, DP, true>, the certificate; rq_mask_keys_kernel in the generic tail) or the exact scan of the shard with the
// excluded rows' keys emptied.  Replaces the `where` restriction of the collection.query of reference
// rag_uq/streaming_index.py:355-359.
#include "rq_filter_plan.h"
#include "rq_gather_body.h"
#include "rq_stage.h"

// ---- kernels ------------------------------------------------------------------------------------
__device__ __forceinline__ bool rq_filter_bit(const uint32_t* bits, int64_t row) { return (bits[row >> 5] >> (row & 31)) & 1u; }

__global__ __launch_bounds__(256) void rq_mask_scale_kernel(const float* src, const uint32_t* bits, int64_t n_rows, int64_t cap, float* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    out[i] = (i < n_rows && rq_filter_bit(bits, i)) ? src[i] : __uint_as_float(0xffffffffu);   // the pad rows' NaN (rq_api.hip grow)
}
hipError_t rq_mask_scale_launch(const float* src, const uint32_t* bits, int64_t n_rows, int64_t cap, float* out, hipStream_t stream) {
    if (cap <= 0 || n_rows > cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_mask_scale_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, stream, src, bits, n_rows, cap, out);
    return hipGetLastError();
}

// Candidate keys carry their LOCAL row (rq_rescore_kernel, rq_exact_scan_kernel): key 0 already means "no row" to rq_final_kernel.
__global__ __launch_bounds__(256) void rq_mask_keys_kernel(uint64_t* cand, int64_t n, const uint32_t* bits) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t key = cand[i];
        if (key != 0 && !rq_filter_bit(bits, (int64_t)rq_key_index(key))) cand[i] = 0;
    }
}
hipError_t rq_mask_keys_launch(uint64_t* cand, int64_t n, const uint32_t* bits, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 16384);
    hipLaunchKernelGGL(rq_mask_keys_kernel, dim3(grid), dim3(256), 0, stream, cand, n, bits);
    return hipGetLastError();
}

// grid (B, ceil(nlist / 256)): query = blockIdx.x, so that the workgroups in flight together re-score the SAME 256 rows for
// different queries (the rows come from the caches after their first reader); 256 threads.  The arithmetic of one row is
// rq_tail_body.h phase C's: 16 lanes per row (sub = lane & 15 owns elements pp * 128 + 8 * sub + e), a wave takes 8 rows per
// round, fp64 products in element order, xor butterfly over the 16 lanes -- the same summation order, hence the same bits
// (rq_rowdot.h, shared with rq_mmr.hip).  The body is rq_gather_body.h's, shared with the ragged gather of rq_filter_each.hip.
template <int DP>
__global__ __launch_bounds__(256) void rq_gather_score_kernel(RqGatherArgs a) {
    __shared__ __attribute__((aligned(16))) float qs[RQ_DPAD];
    const int q = (int)blockIdx.x;
    rq_gather_chunk<DP>(a.x, a.rownorm64, a.q32 + (size_t)q * RQ_DPAD, a.qnorm64[q], a.list, a.nlist, (int64_t)blockIdx.y * 256, a.metric,
                        a.cand + (int64_t)q * a.cand_stride, qs);
}
hipError_t rq_gather_score_launch(const RqGatherArgs& a, int B, hipStream_t stream) {
    if (B < 1 || a.nlist < 1 || a.cand_stride < a.nlist || (a.dpad != 384 && a.dpad != RQ_DPAD)) return hipErrorInvalidValue;
    // a grid holds 65 535 chunks of 256 rows in y: longer lists take several launches, each over its own stretch of the list
    const int64_t per_launch = (int64_t)RQ_GATHER_MAX_CHUNKS * 256;
    for (int64_t off = 0; off < a.nlist; off += per_launch) {
        RqGatherArgs part = a;
        part.list = a.list + off; part.cand = a.cand + off; part.nlist = std::min(per_launch, a.nlist - off);
        const unsigned chunks = (unsigned)((part.nlist + 255) / 256);
        if (a.dpad == 384) hipLaunchKernelGGL(rq_gather_score_kernel<384>, dim3(B, chunks), dim3(256), 0, stream, part);
        else hipLaunchKernelGGL(rq_gather_score_kernel<RQ_DPAD>, dim3(B, chunks), dim3(256), 0, stream, part);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- the filter object ----------------------------------------------------------------------------
static void free_filter(rq_filter* f) {
    free_dev(f->d_bits, f->d_first, f->d_list, f->scale[0], f->scale[1]);
    delete f;
}
void free_filters(rq_index* idx) {
    for (rq_filter* f : idx->filters) free_filter(f);
    idx->filters.clear();
}

// The host bookkeeping of a filter from its bitmap (bits beyond n_rows are ignored): count, occupancy of the bins.
static void filter_host_state(rq_filter* f, const uint32_t* bits, int64_t n) {
    const int64_t words = (n + 31) / 32, nbins = (n + 63) / 64;
    f->n = n;
    f->bits.assign(bits, bits + words);
    if (n & 31) f->bits[(size_t)words - 1] &= (1u << (n & 31)) - 1u;
    f->occ_prefix.assign((size_t)nbins + 1, 0);
    int64_t na = 0;
    for (int64_t b = 0; b < nbins; ++b) {
        const uint32_t lo = f->bits[(size_t)(2 * b)], hi = 2 * b + 1 < words ? f->bits[(size_t)(2 * b + 1)] : 0u;
        na += __builtin_popcount(lo) + __builtin_popcount(hi);
        f->occ_prefix[(size_t)b + 1] = f->occ_prefix[(size_t)b] + ((lo | hi) ? 1 : 0);
    }
    f->na = na;
}
// Allowed rows in ascending order, the first `limit` of them.
static std::vector<uint32_t> filter_rows(const rq_filter* f, int64_t limit) {
    std::vector<uint32_t> rows;
    rows.reserve((size_t)std::min(limit, f->na));
    for (size_t w = 0; w < f->bits.size() && (int64_t)rows.size() < limit; ++w)
        for (uint32_t v = f->bits[w]; v && (int64_t)rows.size() < limit; v &= v - 1) rows.push_back((uint32_t)(w * 32 + __builtin_ctz(v)));
    return rows;
}

static rq_filter* filter_create(rq_index* idx, const uint32_t* bits, int64_t n_rows, bool on_device, hipStream_t stream) {
    if (rq_device_count() <= 0) { err_no_device(); return nullptr; }
    if (!idx || (!bits && n_rows > 0)) { set_err(RQ_EINVAL, "null argument"); return nullptr; }
    if (!idx->shards.empty()) { set_err(RQ_EUNSUPPORTED, "RQ_EUNSUPPORTED: filters on a multi-device index: use one index per device"); return nullptr; }
    if (n_rows != idx->n) { set_err(RQ_EINVAL, "the filter covers %lld rows, the index holds %lld", (long long)n_rows, (long long)idx->n); return nullptr; }
    DeviceGuard dg_(idx->device);
    if (!dg_.ok) { set_err(RQ_EHIP, "cannot select device %d", idx->device); return nullptr; }
    const size_t words = (size_t)((n_rows + 31) / 32);
    std::vector<uint32_t> host;
    if (on_device && words) {   // the device form copies its N / 8 bytes back once
        host.resize(words);
        if (hipMemcpyAsync(host.data(), bits, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            set_err(RQ_EHIP, "copy of the device bitmap failed");
            return nullptr;
        }
        bits = host.data();
    }
    rq_filter* f = new rq_filter();
    f->idx = idx;
    filter_host_state(f, bits, n_rows);
    const std::vector<uint32_t> first = filter_rows(f, RQ_MAX_K);
    bool ok = true;
    if (words) {
        ok = hipMalloc((void**)&f->d_bits, words * sizeof(uint32_t)) == hipSuccess &&
             hipMemcpy(f->d_bits, f->bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok && !first.empty())
        ok = hipMalloc((void**)&f->d_first, first.size() * sizeof(uint32_t)) == hipSuccess &&
             hipMemcpy(f->d_first, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { set_err(RQ_ENOMEM, "device memory for a filter over %lld rows", (long long)n_rows); free_filter(f); return nullptr; }
    idx->filters.push_back(f);
    return f;
}

extern "C" rq_filter* rq_filter_create(rq_index* idx, const uint32_t* bits, int64_t n_rows) { return filter_create(idx, bits, n_rows, false, nullptr); }
extern "C" rq_filter* rq_filter_create_device(rq_index* idx, const uint32_t* d_bits, int64_t n_rows, void* stream) {
    return filter_create(idx, d_bits, n_rows, true, (hipStream_t)stream);
}
extern "C" int64_t rq_filter_count(const rq_filter* f) { return f ? f->na : RQ_EINVAL; }
extern "C" void rq_filter_destroy(rq_filter* f) {
    if (!f) return;
    rq_index* idx = f->idx;
    DeviceGuard dg_(idx->device);
    (void)hipDeviceSynchronize();   // searches in flight on any stream may still read the filter's arrays
    idx->filters.erase(std::remove(idx->filters.begin(), idx->filters.end(), f), idx->filters.end());
    free_filter(f);
}

// The masked row scale of `metric`, built by the first search that scans with the filter.  A filter belongs to its index, not to a
// stream: the array is published (f->scale) only when it is complete, so a call on any other stream that finds it may scan at once
// -- as ensure_ones and ensure_x8 complete their builds before marking them valid.  The rebuild after a reservation waits for the
// whole device first: scans of other streams may still read the old array.
int ensure_filter_scale(rq_index* idx, const rq_filter* cf, int metric, hipStream_t s) {
    rq_filter* f = const_cast<rq_filter*>(cf);   // a cache: the filter's meaning does not change
    const int m = metric == RQ_METRIC_IP ? 1 : 0;
    if (f->scale[m] && f->scale_cap[m] == idx->cap) return RQ_OK;
    if (f->scale[m]) { HIPCHK(hipDeviceSynchronize()); free_dev(f->scale[m]); f->scale_cap[m] = 0; }   // (a reservation made since: the scan reads whole quads)
    const float* src = idx->inv_norm;
    if (m) { if (int r = ensure_ones(idx, s)) return r; src = idx->ones; }
    float* built = nullptr;
    if (hipMalloc((void**)&built, (size_t)idx->cap * sizeof(float)) != hipSuccess) return set_err(RQ_ENOMEM, "hipMalloc of %lld masked row scales failed", (long long)idx->cap);
    hipError_t e = rq_mask_scale_launch(src, f->d_bits, f->n, idx->cap, built, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(built); return set_err(RQ_EHIP, "building the masked row scales failed: %s", hipGetErrorString(e)); }
    f->scale[m] = built;
    f->scale_cap[m] = idx->cap;
    return RQ_OK;
}

int ensure_filter_list(rq_filter* f) {
    if (f->d_list) return RQ_OK;
    const std::vector<uint32_t> rows = filter_rows(f, f->na);
    if (hipMalloc((void**)&f->d_list, rows.size() * sizeof(uint32_t)) != hipSuccess) return set_err(RQ_ENOMEM, "hipMalloc of %zu listed rows failed", rows.size());
    HIPCHK(hipMemcpy(f->d_list, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RQ_OK;
}

// ---- searches -------------------------------------------------------------------------------------
int check_filter(const rq_index* idx, const rq_filter* f) {
    if (!f) return set_err(RQ_EINVAL, "null filter");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "filtered searches on a multi-device index: use one index per device");
    if (f->idx != idx) return set_err(RQ_EINVAL, "the filter belongs to another index");
    if (f->n != idx->n) return set_err(RQ_EINVAL, "stale filter: made for %lld rows, the index holds %lld", (long long)f->n, (long long)idx->n);
    return RQ_OK;
}

// The gather route: groups of queries whose candidate keys (na each) stay within 1 GiB, as the exact rung bounds its own; the
// prepared queries and the keys live in the stream's workspace like those of any other call.
static int gather_route(rq_index* idx, rq_filter* f, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s) {
    if (int r = ensure_filter_list(f)) return r;
    const int64_t na = f->na;
    const int group = queries_per_gib(B, na);
    const QuerySet* qs = nullptr;
    uint64_t* cand = nullptr;
    if (int r = scanless_workspace(idx, s, (group + 63) / 64 * 64, (size_t)group * (size_t)na, &qs, &cand)) return r;
    for (int off = 0; off < B; off += group) {
        const int g = std::min(group, B - off);
        const RqPrepArgs pa = prep_args(*qs, d_q + (size_t)off * idx->dim, idx->dim, g, (g + 63) / 64 * 64, false);
        const SearchOut o = out.from(off, k);
        RqGatherArgs ga;
        ga.x = idx->x; ga.dpad = idx->dpad; ga.rownorm64 = idx->rownorm64; ga.q32 = qs->q32; ga.qnorm64 = qs->qn;
        ga.list = f->d_list; ga.nlist = na; ga.metric = metric; ga.cand = cand; ga.cand_stride = na;
        RqFinalArgs fa{};
        fa.cand = cand; fa.ncand = (int)na; fa.binkeys = nullptr; fa.binkeys_stride = 0; fa.nb = 1; fa.nbins = 1;   // nbins <= nb: every row in play was re-scored
        fa.qnorm64 = qs->qn; fa.metric = metric; fa.eps = 0.f; fa.max_row_norm = 0.f; fa.k = k; fa.row_offset = idx->row_offset; fa.n_rows = na;
        fa.first = f->d_first;
        fa.out_scores = o.scores; fa.out_rows = o.rows; fa.out_keys = o.keys; fa.out_status = o.status;
        HIPCHK(rq_prep_queries_launch(pa, s));
        HIPCHK(rq_gather_score_launch(ga, g, s));
        HIPCHK(rq_final_launch(fa, g, s));
    }
    return RQ_OK;
}

int search_filtered_device(rq_index* idx, const rq_filter* cf, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s) {
    rq_filter* f = const_cast<rq_filter*>(cf);
    // like a "pipeline" = 0 call: whatever the stream still defers (fused tail, scanned-ahead pair, hint) is completed first
    if (int r = flush_tails(idx, s)) return r;
    idx->t.searches++;
    idx->t.queries += B;
    const FilterShape shape{f->n, f->na, f->occ_prefix.data()};
    const int route = plan_filter(idx, shape, B, k, metric, idx->filter_route);
    idx->filter_route_last = route;
    return run_filter_route(idx, f, route, d_q, B, k, metric, out, s);
}

// One filter's queries down the route the plan chose (search_filtered_device; the pass groups of rq_filter_each.hip).
int run_filter_route(rq_index* idx, rq_filter* f, int route, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s) {
    if (route == FROUTE_EMPTY) {
        if (int r = mark_no_scan(idx, s)) return r;
        return fill_empty(B, k, out, s);
    }
    if (route == FROUTE_GATHER) return gather_route(idx, f, d_q, B, k, metric, out, s);
    if (route == FROUTE_SCAN) return run_pipeline(idx, d_q, B, k, metric, nb_default(idx, k), out, s, 0, f);
    // exact: the shard's fp64 scan in groups of queries (1 GiB of candidate keys, as rq_search_fixup_device's last rung)
    const int group = queries_per_gib(B, (idx->n + 63) / 64 * 64);
    for (int off = 0; off < B; off += group) {
        const int g = std::min(group, B - off);
        if (int r = run_pipeline(idx, d_q + (size_t)off * idx->dim, g, k, metric, -1, out.from(off, k), s, 0, f)) return r;
    }
    return RQ_OK;
}

extern "C" int rq_search_filtered_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores,
                                         int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_search_args(idx, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    if (int r = check_filter(idx, f)) return r;
    RQ_ON_DEVICE(idx);
    return search_filtered_device(idx, f, d_queries, B, k, metric, {d_scores, d_rows, d_keys, d_status}, (hipStream_t)stream);
}

extern "C" int rq_search_fixup_filtered_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores,
                                               int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_search_args(idx, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    if (int r = check_filter(idx, f)) return r;
    RQ_ON_DEVICE(idx);
    return fixup_ladder(idx, f, d_queries, B, k, metric, d_scores, d_rows, d_keys, d_status, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h).
extern "C" int rq_search_filtered(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows) {
    if (int r = check_search_args(idx, queries, B, k, metric, out_scores, out_rows)) return r;
    if (int r = check_filter(idx, f)) return r;
    RQ_ON_DEVICE(idx);
    const SearchStaging sz = search_staging(idx->dim, B, k);
    const size_t bytes[4] = {sz.q, sz.scores, sz.rows, sz.status};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 4, "a filtered search")) return r;
    float* d_q = st.at<float>(0); float* d_scores = st.at<float>(1); int64_t* d_rows = st.at<int64_t>(2); int* d_status = st.at<int>(3);
    if (int r = st.up(d_q, queries, sz.q)) return r;
    if (int r = search_filtered_device(idx, f, d_q, B, k, metric, {d_scores, d_rows, nullptr, d_status}, st.s)) return r;
    if (int r = fixup_ladder(idx, f, d_q, B, k, metric, d_scores, d_rows, nullptr, d_status, st.s); r < 0) return r;
    st.down(out_scores, d_scores, sz.scores);
    st.down(out_rows, d_rows, sz.rows);
    return st.finish();
}
