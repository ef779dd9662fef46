// rq_filter_each.hip -- searches with one filter per query (include/rq.h rq_search_filtered_each*): query q ranks the rows of
// filters[q] only, in ONE call, instead of one rq_search_filtered_device call per distinct filter.  What a call does is decided by
// rq_filter_each_plan.h: the queries are grouped by filter, every group is routed by plan_filter with its own number of queries, and
//   - the groups of the gather route together are the RAGGED SET: the whole batch is prepared once, rq_gather_ragged_kernel re-scores
//     each query's own listed rows (rq_gather_body.h: the bits of rq_gather_score_kernel), and rq_final_kernel with a per-query
//     descriptor (RqFinalArgs::each) ranks each query's keys -- three launches per round whatever the number of filters;
//   - groups of the scan and exact routes, and the unrestricted (NULL) queries, run the existing call of their route, through pointer
//     offsets when their queries are one contiguous run and through a staging sub-batch (gather rows, scatter results) otherwise;
//   - many broad filters in one batch share ONE exact fp64 scan of the shard (as generic_tail runs it), rq_mask_keys_each_kernel
//     empties each query's keys by its own bitmap, and the per-query final ranks them.
// A batch whose entries are all the same filter is exactly the existing call.
#include "rq_filter_each_plan.h"
#include "rq_gather_body.h"
#include "rq_repair.h"

// ---- kernels ------------------------------------------------------------------------------------
// One workgroup per work item (run, chunk, query of the run), the query running fastest (rq_kernels.h RqRaggedArgs).  Everything
// that selects the item is uniform over the workgroup.
template <int DP>
__global__ __launch_bounds__(256) void rq_gather_ragged_kernel(RqRaggedArgs a, int64_t item0) {
    __shared__ __attribute__((aligned(16))) float qs[RQ_DPAD];
    const int64_t item = item0 + (int64_t)blockIdx.x;
    int lo = 0, hi = a.nruns;   // runs[lo].item_base <= item < runs[hi].item_base (the sentinel)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.runs[mid].item_base <= item) lo = mid; else hi = mid;
    }
    const RqEachRun r = a.runs[lo];
    const int64_t local = item - r.item_base;
    const int64_t chunk = local / r.count;
    const RqEachDesc d = a.each[r.first + (int)(local - chunk * r.count)];
    rq_gather_chunk<DP>(a.x, a.rownorm64, a.q32 + (size_t)d.q * RQ_DPAD, a.qnorm64[d.q], d.list, r.na, chunk * 256, a.metric, a.cand + d.key_off, qs);
}
hipError_t rq_gather_ragged_launch(const RqRaggedArgs& a, int64_t items, hipStream_t stream) {
    if (items < 1 || a.nruns < 1 || (a.dpad != 384 && a.dpad != RQ_DPAD)) return hipErrorInvalidValue;
    // a grid holds 2^31 - 1 workgroups in x: more items take several launches, each from its own first item
    for (int64_t item0 = 0; item0 < items; item0 += RQ_RAGGED_MAX_ITEMS) {
        const unsigned grid = (unsigned)std::min<int64_t>(RQ_RAGGED_MAX_ITEMS, items - item0);
        if (a.dpad == 384) hipLaunchKernelGGL(rq_gather_ragged_kernel<384>, dim3(grid), dim3(256), 0, stream, a, item0);
        else hipLaunchKernelGGL(rq_gather_ragged_kernel<RQ_DPAD>, dim3(grid), dim3(256), 0, stream, a, item0);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// rq_mask_keys_kernel (rq_filter.hip) with a bitmap per query: blockIdx.y is the query.
__global__ __launch_bounds__(256) void rq_mask_keys_each_kernel(uint64_t* cand, const RqEachDesc* each) {
    const RqEachDesc d = each[blockIdx.y];
    uint64_t* c = cand + d.key_off;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < d.ncand; i += stride) {
        const uint64_t key = c[i];
        if (key == 0) continue;
        const int64_t row = (int64_t)rq_key_index(key);
        if (!((d.bits[row >> 5] >> (row & 31)) & 1u)) c[i] = 0;
    }
}
hipError_t rq_mask_keys_each_launch(uint64_t* cand, const RqEachDesc* each, int nq, int64_t max_ncand, hipStream_t stream) {
    if (nq < 1 || nq > 65535) return hipErrorInvalidValue;
    if (max_ncand <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<int64_t>((max_ncand + 255) / 256, 1024);
    hipLaunchKernelGGL(rq_mask_keys_each_kernel, dim3(gx, (unsigned)nq), dim3(256), 0, stream, cand, each);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rq_each_gather_rows_kernel(const float* src, const int* pos, int dim, float* dst) {
    const float* s = src + (size_t)pos[blockIdx.x] * dim;
    float* d = dst + (size_t)blockIdx.x * dim;
    for (int e = threadIdx.x; e < dim; e += 256) d[e] = s[e];
}
hipError_t rq_each_gather_rows_launch(const float* src, const int* pos, int n, int dim, float* dst, hipStream_t stream) {
    if (n < 1 || dim < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_each_gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, stream, src, pos, dim, dst);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rq_each_scatter_kernel(RqEachScatterArgs a) {
    const int i = blockIdx.x;
    const int64_t o = (int64_t)a.pos[i] * a.k, in = (int64_t)i * a.k;
    for (int j = threadIdx.x; j < a.k; j += 256) {
        a.scores[o + j] = a.src_scores ? a.src_scores[in + j] : 0.f;
        a.rows[o + j] = a.src_scores ? a.src_rows[in + j] : -1;
        if (a.keys) a.keys[o + j] = a.src_scores && a.src_keys ? a.src_keys[in + j] : 0;
    }
    if (threadIdx.x == 0) a.status[a.pos[i]] = a.src_scores ? a.src_status[i] : 0;
}
hipError_t rq_each_scatter_launch(const RqEachScatterArgs& a, hipStream_t stream) {
    if (a.n < 1 || a.k < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_each_scatter_kernel, dim3((unsigned)a.n), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- the call's tables and staging ------------------------------------------------------------------
// The tables of one call, laid out in one block (16-byte aligned pieces) that goes to the device in one copy.
struct EachTables {
    std::vector<char> blob;
    size_t put(const void* data, size_t bytes) {
        const size_t off = (blob.size() + 15) / 16 * 16;
        blob.resize(off + bytes);
        if (bytes) std::memcpy(blob.data() + off, data, bytes);
        return off;
    }
};

template <class T>
static int each_ensure(T*& p, size_t elems) {   // (hipFree waits for the device: nothing still reads the old buffer)
    if (p) (void)hipFree(p);
    p = nullptr;
    if (hipMalloc((void**)&p, std::max(elems, (size_t)1) * sizeof(T)) != hipSuccess) return set_err(RQ_ENOMEM, "hipMalloc of %zu staging bytes failed", elems * sizeof(T));
    return RQ_OK;
}

// The staging sub-batch of `nq` queries with k results each.
static int each_staging(StreamCtx& cx, int nq, int k) {
    if (nq <= cx.each_bcap && k <= cx.each_k) return RQ_OK;
    const int nb = std::max(nq, cx.each_bcap), nk = std::max(k, cx.each_k);
    cx.each_bcap = cx.each_k = 0;
    if (int r = each_ensure(cx.each_q, (size_t)nb * RQ_MAX_DIM)) return r;
    if (int r = each_ensure(cx.each_scores, (size_t)nb * nk)) return r;
    if (int r = each_ensure(cx.each_rows, (size_t)nb * nk)) return r;
    if (int r = each_ensure(cx.each_keys, (size_t)nb * nk)) return r;
    if (int r = each_ensure(cx.each_status, (size_t)nb)) return r;
    cx.each_bcap = nb; cx.each_k = nk;
    return RQ_OK;
}

// The call's tables on the device: pinned block -> each_tab, on the stream.  The copy before this one has finished when the pinned
// block is written again (each_ev).
static int each_upload(StreamCtx& cx, const EachTables& t, hipStream_t s) {
    if (t.blob.empty()) return RQ_OK;
    if (cx.each_ev_pending) { HIPCHK(hipEventSynchronize(cx.each_ev)); cx.each_ev_pending = false; }
    if (!cx.each_ev) HIPCHK(hipEventCreateWithFlags(&cx.each_ev, hipEventDisableTiming));
    if (t.blob.size() > cx.each_tab_bytes) {
        const size_t want = std::max(t.blob.size(), 2 * cx.each_tab_bytes);
        if (cx.each_pin) (void)hipHostFree(cx.each_pin);
        cx.each_pin = nullptr; cx.each_tab_bytes = 0;
        if (int r = each_ensure(cx.each_tab, want)) return r;
        if (hipHostMalloc((void**)&cx.each_pin, want, hipHostMallocDefault) != hipSuccess) return set_err(RQ_ENOMEM, "hipHostMalloc of %zu table bytes failed", want);
        cx.each_tab_bytes = want;
    }
    std::memcpy(cx.each_pin, t.blob.data(), t.blob.size());
    HIPCHK(hipMemcpyAsync(cx.each_tab, cx.each_pin, t.blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(cx.each_ev, s));
    cx.each_ev_pending = true;
    return RQ_OK;
}

// ---- the call -------------------------------------------------------------------------------------
static int check_each_args(const rq_index* idx, const rq_filter* const* filters, const void* q, int B, int k, int metric, const void* sc, const void* rows) {
    if (int r = check_search_args(idx, q, B, k, metric, sc, rows)) return r;
    if (!filters) return set_err(RQ_EINVAL, "null filter array");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "RQ_EUNSUPPORTED: per-query filters on a multi-device index: use one index per device");
    for (int i = 0; i < B; ++i)
        if (filters[i])
            if (int r = check_filter(idx, filters[i])) return r;
    return RQ_OK;
}

static int roundup64(int v) { return (v + 63) / 64 * 64; }

// One pass group: the existing call of its route over the group's queries, in place or through the staging sub-batch.
static int each_pass_group(rq_index* idx, StreamCtx& cx, const EachGroup& g, const int* d_pos, const float* d_q, int k, int metric, const SearchOut& out, hipStream_t s) {
    const int bg = (int)g.q.size();
    const float* gq = d_q + (size_t)g.q[0] * idx->dim;
    SearchOut go = out.from(g.q[0], k);
    if (!g.contiguous) {
        HIPCHK(rq_each_gather_rows_launch(d_q, d_pos, bg, idx->dim, cx.each_q, s));
        gq = cx.each_q;
        go = SearchOut{cx.each_scores, cx.each_rows, out.keys ? cx.each_keys : nullptr, cx.each_status};
    }
    if (!g.f) { if (int r = run_pipeline(idx, gq, bg, k, metric, nb_default(idx, k), go, s, 0, nullptr)) return r; }
    else if (int r = run_filter_route(idx, const_cast<rq_filter*>(g.f), g.route, gq, bg, k, metric, go, s)) return r;
    if (!g.contiguous) {
        RqEachScatterArgs sa{d_pos, bg, k, go.scores, go.rows, go.keys, go.status, out.scores, out.rows, out.keys, out.status};
        HIPCHK(rq_each_scatter_launch(sa, s));
    }
    return RQ_OK;
}

static int search_filtered_each_device(rq_index* idx, const rq_filter* const* filters, const float* d_q, int B, int k, int metric, const SearchOut& out, hipStream_t s) {
    EachPlan p;
    if (int r = plan_filter_each(idx, filters, B, k, metric, idx->filter_route, idx->each_key_cap, &p)) return r;
    idx->each_calls++;
    idx->each_groups_last = (int64_t)p.groups.size();
    idx->each_ragged_last = idx->each_rounds_last = idx->each_shared_last = 0;
    idx->each_routes_last = p.routes;
    // one filter for the whole batch: exactly the existing call (same route, same launches)
    if (p.groups.size() == 1 && p.groups[0].f) return search_filtered_device(idx, p.groups[0].f, d_q, B, k, metric, out, s);
    // like a "pipeline" = 0 call: whatever the stream still defers (fused tail, scanned-ahead pair, hint) is completed first
    if (int r = flush_tails(idx, s)) return r;
    idx->t.searches++;
    idx->t.queries += B;
    idx->filter_route_last = p.last_route == EACH_ROUTE_NULL ? -1 : p.last_route;
    if (p.groups.size() == 1) return run_pipeline(idx, d_q, B, k, metric, nb_default(idx, k), out, s, 0, nullptr);   // every entry NULL: the unfiltered search

    // ---- tables: descriptors and runs of every ragged round, descriptors of the shared exact route, positions of scattered groups
    EachTables t;
    const int64_t ncand_x = (idx->n + 63) / 64 * 64;   // keys per query of an exact scan
    const int S = (int)p.shared_q.size();
    const int xg = S ? queries_per_gib(S, ncand_x) : 0;   // queries per exact scan of the shared route
    struct RoundTab { size_t desc, runs; int nruns; int64_t items; };
    std::vector<RoundTab> rtab;
    for (const EachGroup& g : p.groups)
        if (g.kind == EACH_RAGGED)
            if (int r = ensure_filter_list(const_cast<rq_filter*>(g.f))) return r;
    int64_t max_keys = 0;
    for (const EachRound& rd : p.rounds) {
        std::vector<RqEachDesc> desc((size_t)rd.count);
        std::vector<RqEachRun> runs;
        int64_t off = 0, items = 0;
        for (int i = 0; i < rd.count; ++i) {
            const int gi = p.ragged_g[(size_t)(rd.first + i)], q = p.ragged_q[(size_t)(rd.first + i)];
            const rq_filter* f = p.groups[(size_t)gi].f;
            if (i == 0 || gi != p.ragged_g[(size_t)(rd.first + i - 1)]) runs.push_back(RqEachRun{0, f->na, i, 0});
            runs.back().count++;
            desc[(size_t)i] = RqEachDesc{f->d_list, f->d_first, f->d_bits, off, f->na, f->na, q, q};
            off += f->na;
        }
        for (RqEachRun& r : runs) { r.item_base = items; items += (r.na + 255) / 256 * (int64_t)r.count; }
        const int nruns = (int)runs.size();
        runs.push_back(RqEachRun{items, 0, 0, 0});   // the sentinel
        rtab.push_back(RoundTab{t.put(desc.data(), desc.size() * sizeof(RqEachDesc)), t.put(runs.data(), runs.size() * sizeof(RqEachRun)), nruns, items});
        max_keys = std::max(max_keys, rd.keys);
    }
    size_t shared_desc = 0, shared_pos = 0;
    if (S) {
        std::vector<RqEachDesc> desc((size_t)S);
        for (int i = 0; i < S; ++i) {
            const rq_filter* f = p.groups[(size_t)p.shared_g[(size_t)i]].f;
            const int slot = i % xg;   // its place in its exact scan
            desc[(size_t)i] = RqEachDesc{nullptr, f->d_first, f->d_bits, (int64_t)slot * ncand_x, ncand_x, f->na, slot, p.shared_q[(size_t)i]};
        }
        shared_desc = t.put(desc.data(), desc.size() * sizeof(RqEachDesc));
        shared_pos = t.put(p.shared_q.data(), p.shared_q.size() * sizeof(int));
    }
    std::vector<size_t> gpos(p.groups.size(), 0);
    int stage_q = S;
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const EachGroup& g = p.groups[gi];
        if (g.contiguous || (g.kind != EACH_PASS && g.kind != EACH_EMPTY)) continue;
        gpos[gi] = t.put(g.q.data(), g.q.size() * sizeof(int));
        if (g.kind == EACH_PASS) stage_q = std::max(stage_q, (int)g.q.size());
    }

    // ---- the stream's workspace, staging and tables
    const QuerySet* qs = nullptr;
    uint64_t* cand = nullptr;
    if (!p.ragged_q.empty()) { if (int r = scanless_workspace(idx, s, roundup64(B), (size_t)max_keys, &qs, &cand)) return r; }
    else if (int r = mark_no_scan(idx, s)) return r;
    StreamCtx& cx = idx->ctx[s];
    if (stage_q > 0)
        if (int r = each_staging(cx, stage_q, k)) return r;
    if (int r = each_upload(cx, t, s)) return r;
    const char* tab = cx.each_tab;

    // ---- groups with no row to return: padding
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const EachGroup& g = p.groups[gi];
        if (g.kind != EACH_EMPTY) continue;
        if (g.contiguous) { if (int r = fill_empty((int)g.q.size(), k, out.from(g.q[0], k), s)) return r; }
        else {
            RqEachScatterArgs sa{(const int*)(tab + gpos[gi]), (int)g.q.size(), k, nullptr, nullptr, nullptr, nullptr, out.scores, out.rows, out.keys, out.status};
            HIPCHK(rq_each_scatter_launch(sa, s));
        }
    }

    // ---- the ragged set: the batch prepared once, then a gather and a final launch per round
    if (!p.ragged_q.empty()) {
        HIPCHK(rq_prep_queries_launch(prep_args(*qs, d_q, idx->dim, B, roundup64(B), false), s));
        for (size_t ri = 0; ri < p.rounds.size(); ++ri) {
            const EachRound& rd = p.rounds[ri];
            const RqEachDesc* d_desc = (const RqEachDesc*)(tab + rtab[ri].desc);
            RqRaggedArgs ga;
            ga.x = idx->x; ga.dpad = idx->dpad; ga.rownorm64 = idx->rownorm64; ga.q32 = qs->q32; ga.qnorm64 = qs->qn;
            ga.each = d_desc; ga.runs = (const RqEachRun*)(tab + rtab[ri].runs); ga.nruns = rtab[ri].nruns; ga.metric = metric; ga.cand = cand;
            RqFinalArgs fa{};
            fa.cand = cand; fa.ncand = 0; fa.binkeys = nullptr; fa.binkeys_stride = 0; fa.nb = 1; fa.nbins = 1;   // nbins <= nb: every row in play was re-scored
            fa.qnorm64 = qs->qn; fa.metric = metric; fa.eps = 0.f; fa.max_row_norm = 0.f; fa.k = k; fa.row_offset = idx->row_offset; fa.n_rows = 0;
            fa.each = d_desc;
            fa.out_scores = out.scores; fa.out_rows = out.rows; fa.out_keys = out.keys; fa.out_status = out.status;
            HIPCHK(rq_gather_ragged_launch(ga, rtab[ri].items, s));
            HIPCHK(rq_final_launch(fa, rd.count, s));
        }
        idx->each_ragged_last = (int64_t)p.ragged_q.size();
        idx->each_rounds_last = (int64_t)p.rounds.size();
    }

    // ---- pass groups: one existing call each
    for (size_t gi = 0; gi < p.groups.size(); ++gi)
        if (p.groups[gi].kind == EACH_PASS)
            if (int r = each_pass_group(idx, cx, p.groups[gi], (const int*)(tab + gpos[gi]), d_q, k, metric, out, s)) return r;

    // ---- the shared exact route: one fp64 scan of the shard per xg queries (as generic_tail runs it), each query's keys masked by
    // its own bitmap, the per-query final
    if (S) {
        HIPCHK(rq_each_gather_rows_launch(d_q, (const int*)(tab + shared_pos), S, idx->dim, cx.each_q, s));
        CallPlan cp;
        if (int r = plan_call(idx, xg, k, metric, -1, false, 0, &cp)) return r;
        if (int r = scanless_workspace(idx, s, roundup64(xg), (size_t)xg * (size_t)cp.ncand, &qs, &cand)) return r;
        for (int off = 0; off < S; off += xg) {
            const int g = std::min(xg, S - off);
            const RqEachDesc* d_desc = (const RqEachDesc*)(tab + shared_desc) + off;
            HIPCHK(rq_prep_queries_launch(prep_args(*qs, cx.each_q + (size_t)off * idx->dim, idx->dim, g, roundup64(g), false), s));
            RqRescoreArgs ra;
            ra.x = idx->x; ra.dpad = idx->dpad; ra.q32 = qs->q32; ra.qnorm64 = qs->qn; ra.rownorm64 = idx->rownorm64;
            ra.binkeys = nullptr; ra.binkeys_stride = cp.m; ra.nb = cp.nb; ra.metric = metric; ra.n_rows = idx->n; ra.cand = cand;
            if (idx->exact_mfma) HIPCHK(rq_exact_scan_launch(ra, g, idx->cu_count, s));
            else HIPCHK(rq_rescore_launch(ra, g, s));
            HIPCHK(rq_mask_keys_each_launch(cand, d_desc, g, cp.ncand, s));
            RqFinalArgs fa{};
            fa.cand = cand; fa.ncand = (int)cp.ncand; fa.binkeys = nullptr; fa.binkeys_stride = cp.m; fa.nb = cp.nb; fa.nbins = cp.nb;
            fa.qnorm64 = qs->qn; fa.metric = metric; fa.eps = scan_eps(idx, metric); fa.max_row_norm = (float)(idx->max_row_norm * (1.0 + 1e-6));
            fa.k = k; fa.row_offset = idx->row_offset; fa.n_rows = idx->n;
            fa.each = d_desc;
            fa.out_scores = out.scores; fa.out_rows = out.rows; fa.out_keys = out.keys; fa.out_status = out.status;
            HIPCHK(rq_final_launch(fa, g, s));
        }
        idx->each_shared_last = S;
    }
    return RQ_OK;
}

// The repair of an each-call: the flagged queries of every group climb the existing ladder under that group's filter.
static int fixup_filtered_each(rq_index* idx, const rq_filter* const* filters, const float* d_q, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                               uint64_t* d_keys, int* d_status, hipStream_t s) {
    if (int r = flush_tails(idx, s)) return r;
    Stage fx(s);   // (owns no buffer)
    std::vector<int> st;
    if (int r = repair_status(fx, d_status, B, st)) return r;
    EachPlan p;
    if (int r = plan_filter_each(idx, filters, B, k, metric, idx->filter_route, idx->each_key_cap, &p)) return r;
    int total = 0;
    for (const EachGroup& g : p.groups) {
        RepairList bad;
        for (int q : g.q) if (st[(size_t)q] != 0) bad.push_back({(int)bad.size(), q});
        if (bad.empty()) continue;
        // (the unrestricted group climbs the unfiltered ladder, but an each-call never touches the int8 image or its accounting)
        const bool keep8 = idx->last_use8;
        if (!g.f) idx->last_use8 = false;
        int r;
        if (g.contiguous) {
            const size_t q0 = (size_t)g.q[0];
            r = fixup_ladder(idx, g.f, d_q + q0 * idx->dim, (int)g.q.size(), k, metric, d_scores + q0 * k, d_rows + q0 * k, d_keys ? d_keys + q0 * k : nullptr, d_status + q0, s);
        } else {
            if (idx->ctx.find(s) == idx->ctx.end())
                if (int e = mark_no_scan(idx, s)) { idx->last_use8 = keep8; return e; }
            StreamCtx& cx = idx->ctx[s];
            r = each_staging(cx, (int)bad.size(), k);
            uint64_t* sk = d_keys ? cx.each_keys : nullptr;
            if (r == RQ_OK) r = repair_pack(fx, bad, {repair_col(d_q, cx.each_q, (size_t)idx->dim), repair_col(d_status, cx.each_status, 1)});
            if (r == RQ_OK) r = fixup_ladder(idx, g.f, cx.each_q, (int)bad.size(), k, metric, cx.each_scores, cx.each_rows, sk, cx.each_status, s);
            if (r >= 0) {
                repair_unpack(fx, bad, {repair_col(d_scores, cx.each_scores, k), repair_col(d_rows, cx.each_rows, k), repair_col(d_keys, sk, k)}, d_status);
                if (int e = fx.finish()) r = e;
            }
        }
        idx->last_use8 = keep8;
        if (r < 0) return r;
        if (!g.f) idx->filter_repaired += r;   // (fixup_ladder counts the filtered groups' itself)
        total += r;
    }
    return total;
}

extern "C" int rq_search_filtered_each_device(rq_index* idx, const rq_filter* const* filters, const float* d_queries, int B, int k, int metric,
                                              float* d_scores, int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_each_args(idx, filters, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return search_filtered_each_device(idx, filters, d_queries, B, k, metric, {d_scores, d_rows, d_keys, d_status}, (hipStream_t)stream);
}

extern "C" int rq_search_fixup_filtered_each_device(rq_index* idx, const rq_filter* const* filters, const float* d_queries, int B, int k, int metric,
                                                    float* d_scores, int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_each_args(idx, filters, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return fixup_filtered_each(idx, filters, d_queries, B, k, metric, d_scores, d_rows, d_keys, d_status, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h), repair included.
extern "C" int rq_search_filtered_each(rq_index* idx, const rq_filter* const* filters, const float* queries, int B, int k, int metric, float* out_scores,
                                       int64_t* out_rows) {
    if (int r = check_each_args(idx, filters, queries, B, k, metric, out_scores, out_rows)) return r;
    RQ_ON_DEVICE(idx);
    const SearchStaging sz = search_staging(idx->dim, B, k);
    const size_t bytes[4] = {sz.q, sz.scores, sz.rows, sz.status};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 4, "a search with per-query filters")) return r;
    float* d_q = st.at<float>(0); float* d_scores = st.at<float>(1); int64_t* d_rows = st.at<int64_t>(2); int* d_status = st.at<int>(3);
    if (int r = st.up(d_q, queries, sz.q)) return r;
    if (int r = search_filtered_each_device(idx, filters, d_q, B, k, metric, {d_scores, d_rows, nullptr, d_status}, st.s)) return r;
    if (int r = fixup_filtered_each(idx, filters, d_q, B, k, metric, d_scores, d_rows, nullptr, d_status, st.s); r < 0) return r;
    st.down(out_scores, d_scores, sz.scores);
    st.down(out_rows, d_rows, sz.rows);
    return st.finish();
}
