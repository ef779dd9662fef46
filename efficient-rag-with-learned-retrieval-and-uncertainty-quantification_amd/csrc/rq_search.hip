// rq_search.hip -- search orchestration of the single-device index: per-stream workspaces, the pipeline of one call
// (run_pipeline: plan -> prepare -> scan passes -> tail), deferred tails and bundles of scanned-ahead calls, the repair ladder,
// the blocking host-buffer search.  What a call will do is decided by rq_plan.h, what it is to the calls before it on its stream by
// rq_bundle_plan.h; the kernels are rq_kernels.h's launchers.
#include "rq_plan.h"
#include "rq_repair.h"

static const size_t RQ_MAX_STREAM_CTX = 8;
static_assert(RQ_BUNDLE_MAX == RQ_BUNDLE_TAILS, "a bundle's tails run in one rq_bundle_tail_launch");

// ---- workspaces --------------------------------------------------------------------------------
// (Re)allocate a device buffer of want_elems elements; the old contents are dropped.  hipFree waits for the
// device, so kernels still using the old buffer have finished.
template <class T>
static int ensure(T*& p, size_t want_elems) {
    if (p) (void)hipFree(p);
    p = nullptr;
    hipError_t e = hipMalloc((void**)&p, want_elems * sizeof(T));
    if (e != hipSuccess) return set_err(RQ_ENOMEM, "workspace hipMalloc of %zu bytes failed: %s", want_elems * sizeof(T), hipGetErrorString(e));
    return RQ_OK;
}

static void free_queries(QuerySet& q) { free_dev(q.qh, q.q32, q.qn, q.q8, q.qscale8, q.qeps8, q.q8lo, q.qeps8s); }

// Buffers for nslots prepared queries, all or none; a set that exists is dropped first (see ensure).  *bytes (if wanted):
// the size of the last request made, on failure the one that failed.
static hipError_t alloc_queries(QuerySet& q, size_t nslots, size_t* bytes) {
    free_queries(q);
    hipError_t e = hipSuccess;
    auto get = [&](auto*& p, size_t per_slot) {
        if (e != hipSuccess) return;
        const size_t b = nslots * per_slot * sizeof(*p);
        if (bytes) *bytes = b;
        e = hipMalloc((void**)&p, b);
    };
    get(q.qh, RQ_DPAD); get(q.q32, RQ_DPAD); get(q.qn, 1); get(q.q8, RQ_DPAD); get(q.qscale8, 1); get(q.qeps8, 1); get(q.q8lo, RQ_DPAD); get(q.qeps8s, 1);
    if (e != hipSuccess) free_queries(q);
    return e;
}

// Preparation of B queries at q into the first nslots slots of qs (one workgroup per slot: slots >= B are written as zero).
RqPrepArgs prep_args(const QuerySet& qs, const float* q, int dim, int B, int nslots, bool with_int8) {
    RqPrepArgs pa{};
    pa.q = q; pa.dim = dim; pa.B = B; pa.nslots = nslots;
    pa.qh = qs.qh; pa.q32pad = qs.q32; pa.qnorm64 = qs.qn;
    if (with_int8) { pa.q8 = qs.q8; pa.qscale8 = qs.qscale8; pa.qeps8 = qs.qeps8; pa.q8lo = qs.q8lo; pa.qeps8s = qs.qeps8s; }
    return pa;
}

// Slot i of the stream's ring: 64 prepared queries.
static QuerySet ring_slot(const StreamCtx& cx, int i) {
    const QuerySet& r = cx.ring;
    const size_t q = (size_t)i * 64, e = q * RQ_DPAD;
    return QuerySet{r.qh + e, r.q32 + e, r.qn + q, r.q8 + e, r.qscale8 + q, r.qeps8 + q, r.q8lo + e, r.qeps8s + q};
}

static int ensure_ws(Workspace& w, int bpad, int64_t stride, int64_t m, size_t cand_elems) {
    const bool regrow_b = bpad > w.bcap;
    const int bcap = std::max(bpad, w.bcap);
    if (regrow_b) {
        w.bcap = 0;   // (a regrow that fails part-way is made again by the next call)
        size_t bytes = 0;
        if (hipError_t e = alloc_queries(w.qs, (size_t)bcap, &bytes); e != hipSuccess)
            return set_err(RQ_ENOMEM, "workspace hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        if (int r = ensure(w.wgmax, (size_t)bcap * RQ_WGMAX_STRIDE)) return r;
        if (int r = ensure(w.rowcount, (size_t)bcap)) return r;
        if (int r = ensure(w.thr, (size_t)bcap)) return r;
        if (int r = ensure(w.done, (size_t)bcap)) return r;
        if (int r = ensure(w.ovf, (size_t)bcap)) return r;
        w.counters_zero = false;
    }
    if (regrow_b || stride > w.bins_stride) {
        const int64_t st = std::max(stride, w.bins_stride);
        if (int r = ensure(w.bins, (size_t)bcap * st)) return r;
        w.bins_stride = st;
    }
    if (regrow_b || m > w.binkeys_cap) {
        const int64_t mm = std::max(m, w.binkeys_cap);
        if (int r = ensure(w.binkeys, (size_t)bcap * mm)) return r;
        w.binkeys_cap = mm;
    }
    if (cand_elems > w.cand_elems) {   // sized by the queries of the call, not by the padded slot count: an exact scan of
        if (int r = ensure(w.cand, cand_elems)) return r;   // one query holds a key for every row of the shard
        w.cand_elems = cand_elems;
    }
    w.bcap = bcap;
    return RQ_OK;
}

int ensure_range_ws(Workspace& w, int bpad) {
    if (bpad <= w.rg_bcap) return RQ_OK;
    w.rg_bcap = 0;
    if (int r = ensure(w.rg_slot, (size_t)bpad)) return r;
    if (int r = ensure(w.rg_status, (size_t)bpad)) return r;
    if (int r = ensure(w.rg_one, (size_t)bpad)) return r;
    const std::vector<double> one((size_t)bpad, 1.0);
    HIPCHK(hipMemcpy(w.rg_one, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice));
    w.rg_bcap = bpad;
    return RQ_OK;
}

int ensure_ones(rq_index* idx, hipStream_t s) {
    if (idx->ones && idx->ones_valid == idx->n) return RQ_OK;
    if (!idx->ones) HIPCHK(hipMalloc((void**)&idx->ones, (size_t)idx->cap * sizeof(float)));
    std::vector<float> h((size_t)idx->cap, std::nanf(""));   // pad rows: NaN, like inv_norm (see grow)
    std::fill(h.begin(), h.begin() + idx->n, RQ_QSCALE_INV);  // the queries carry 2^12 (rq_select.hip)
    HIPCHK(hipMemcpy(idx->ones, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    idx->ones_valid = idx->n;
    return RQ_OK;
}

static void free_ws(Workspace& w) {
    free_queries(w.qs);
    free_dev(w.bins, w.binkeys, w.cand, w.wgmax, w.rowcount, w.thr, w.done, w.ovf, w.fix_q, w.fix_scores, w.fix_rows, w.fix_keys, w.fix_status);
    free_dev(w.rg_slot, w.rg_status, w.rg_one);
    w = Workspace();
}

void free_ctx(StreamCtx& c) {
    free_ws(c.w[0]);
    free_ws(c.w[1]);
    free_queries(c.ring);
    free_dev(c.grp_scores, c.grp_rows, c.grp_status, c.gm_scores, c.gm_rows);
    free_dev(c.each_tab, c.each_q, c.each_scores, c.each_rows, c.each_keys, c.each_status);
    if (c.each_pin) (void)hipHostFree(c.each_pin);
    if (c.each_ev) (void)hipEventDestroy(c.each_ev);
    if (c.tail) (void)hipStreamDestroy(c.tail);
    for (int p = 0; p < 2; ++p) {
        if (c.ev_scan[p]) (void)hipEventDestroy(c.ev_scan[p]);
        if (c.ev_tail[p]) (void)hipEventDestroy(c.ev_tail[p]);
    }
    c = StreamCtx();
}

// The next pair of timing events ("profile"), created on first use; null events once 16384 pairs are in use (rq_reset_timing
// starts over).  The caller advances ev_used when it has recorded the pair.
static int next_event_pair(rq_index* idx, hipEvent_t& e0, hipEvent_t& e1) {
    e0 = e1 = nullptr;
    if (idx->ev_used >= 16384) return RQ_OK;
    if (idx->ev_used == idx->events.size()) {
        hipEvent_t n0, n1;
        HIPCHK(hipEventCreate(&n0));
        HIPCHK(hipEventCreate(&n1));
        idx->events.push_back({n0, n1});
    }
    e0 = idx->events[idx->ev_used].first; e1 = idx->events[idx->ev_used].second;
    return RQ_OK;
}

// ---- one call ------------------------------------------------------------------------------------
int fill_empty(int B, int k, const SearchOut& out, hipStream_t s) {
    HIPCHK(hipMemsetAsync(out.scores, 0, (size_t)B * k * sizeof(float), s));
    HIPCHK(hipMemsetAsync(out.rows, 0xff, (size_t)B * k * sizeof(int64_t), s));
    if (out.keys) HIPCHK(hipMemsetAsync(out.keys, 0, (size_t)B * k * sizeof(uint64_t), s));
    HIPCHK(hipMemsetAsync(out.status, 0, (size_t)B * sizeof(int), s));
    return RQ_OK;
}

// Test hook ("poison_cand"): before a tail runs, its queries' candidate lists are overwritten with the largest
// possible key.  A consumer that reads a candidate slot it was not handed (a stale line) then returns row 0 with a NaN
// score at rank 1, which no oracle comparison can miss -- instead of a plausible key of an earlier batch.
static int poison_cand(const rq_index* idx, const RqTailArgs& t, int B, hipStream_t s) {
    if (!idx->poison_cand || !t.cand || B <= 0) return RQ_OK;
    HIPCHK(hipMemsetAsync(t.cand, 0xff, (size_t)B * RQ_CAND_CAP * sizeof(uint64_t), s));
    return RQ_OK;
}

// Where a call's bin records are (test hooks rq_debug_bin_records / rq_debug_pooled); bins == nullptr: it scanned nothing.
static void set_records(StreamCtx& c, const uint2* bins, int64_t stride, int B, int slots) {
    c.rec_bins = bins; c.rec_stride = stride; c.rec_B = B; c.rec_slots = slots;
}

// Test hook ("poison_bins"): before a call's scan, the records of every query slot its passes cover are filled with 0xff bytes.
// A record no workgroup wrote then decodes to a NaN maximum, and a pass that writes slots beyond its valid queries shows.
static int poison_bins(const rq_index* idx, uint2* bins, int64_t stride, int slots, hipStream_t s) {
    if (!idx->poison_bins || slots <= 0) return RQ_OK;
    HIPCHK(hipMemsetAsync(bins, 0xff, (size_t)slots * (size_t)stride * sizeof(uint2), s));
    return RQ_OK;
}

// What becomes of a bundle that an event does not continue (rq_bundle_plan.h BundleStep::brk; defined below, behind the pieces
// of a call it is made of).  The ONE place where gathered calls are scanned late and unclaimed tails complete: flush_tails and
// flush_all, which every other route and every mutation of the index goes through, and run_pipeline call it.
static int break_bundle(rq_index* idx, StreamCtx& c, const BundleStep& st, hipStream_t s);

static int ensure_ring(StreamCtx& cx) {
    if (!cx.ring.qh) HIPCHK(alloc_queries(cx.ring, (size_t)RQ_RING_SLOTS * 64, nullptr));
    return RQ_OK;
}

// The tail that is waiting for the stream's next scan launch ("pipeline" = 2) runs on its own instead, on `s`.
static int launch_waiting_tail(const rq_index* idx, StreamCtx& c, hipStream_t s) {
    if (!c.fused_pending) return RQ_OK;
    c.fused_pending = false;
    if (int r = poison_cand(idx, c.fused_tail, c.fused_B, s)) return r;
    HIPCHK(rq_tail_launch(c.fused_tail, c.fused_B, s));
    return RQ_OK;
}

// Make `s` wait for every tail still running on the internal tail stream of `s` (pipeline = 1) and launch the
// tail that was waiting for the next scan (pipeline = 2).
int flush_tails(rq_index* idx, hipStream_t s) {
    auto it = idx->ctx.find(s);
    if (it == idx->ctx.end()) return RQ_OK;
    StreamCtx& c = it->second;
    c.hint_q = nullptr;   // a flush ends the loop the hint belonged to (queries already prepared stay usable)
    if (int r = break_bundle(idx, c, bundle_end(c.bs), s)) return r;
    if (int r = launch_waiting_tail(idx, c, s)) return r;
    for (int p = 0; p < 2; ++p)
        if (c.tail_pending[p]) {
            HIPCHK(hipStreamWaitEvent(s, c.ev_tail[p], 0));
            c.tail_pending[p] = false;
        }
    return RQ_OK;
}

bool bundles_open(const rq_index* idx) {
    for (auto& kv : idx->ctx)
        if (kv.second.bs.phase == BUNDLE_GATHER) return true;
    return false;
}

// Every bundle still open and every tail still waiting for a scan ("pipeline" = 2), of every stream the index remembers.  The callers' stream handles are
// NOT used for it (a caller may have destroyed a stream it no longer searches on; only rq_stream_release tells us): the device
// is drained first -- every scan those tails depend on has then finished -- and the tails run on the index's own stream.
int flush_all(rq_index* idx) {
    bool any = false;
    for (auto& kv : idx->ctx) any = any || kv.second.fused_pending || kv.second.bs.phase != BUNDLE_IDLE || kv.second.tail_pending[0] || kv.second.tail_pending[1];
    if (!any) return RQ_OK;
    RQ_ON_DEVICE(idx);
    HIPCHK(hipDeviceSynchronize());
    for (auto& kv : idx->ctx) {
        StreamCtx& c = kv.second;
        c.hint_q = nullptr;
        c.tail_pending[0] = c.tail_pending[1] = false;   // (their events have fired: the device is idle)
        // (gathered calls are scanned here, on the index's own stream: their queries were prepared by launches that have drained)
        if (int r = break_bundle(idx, c, bundle_end(c.bs), idx->own_stream)) return r;
        if (int r = launch_waiting_tail(idx, c, idx->own_stream)) return r;
    }
    HIPCHK(hipStreamSynchronize(idx->own_stream));
    return RQ_OK;
}

// Drop the workspace of *only (null: of every stream) after the device has drained.
static int release_contexts(rq_index* idx, const hipStream_t* only) {
    if (int r = flush_all(idx)) return r;
    HIPCHK(hipDeviceSynchronize());
    for (auto it = idx->ctx.begin(); it != idx->ctx.end();) {
        if (!only || it->first == *only) { free_ctx(it->second); it = idx->ctx.erase(it); }
        else ++it;
    }
    return RQ_OK;
}

extern "C" int rq_stream_release(rq_index* idx, void* stream) {
    if (!idx) return set_err(RQ_EINVAL, "null index");
    if (!idx->shards.empty()) return RQ_OK;
    RQ_ON_DEVICE(idx);
    const hipStream_t s = (hipStream_t)stream;
    if (idx->ctx.find(s) == idx->ctx.end()) return RQ_OK;
    return release_contexts(idx, &s);
}

// How a call's tail runs: right behind its scan, on the stream's internal tail stream ("pipeline" = 1), or with the stream's
// next scan launch ("pipeline" = 2, fused: one scan launch per call of <= 64 queries, which carries the tail of the previous call).
enum CallMode { CALL_PLAIN, CALL_PIPED, CALL_FUSED };

// What the steps of one run_pipeline call share on top of its plan.
struct Call {
    const float* d_q; int B, k, metric; SearchOut out; hipStream_t s;
    CallPlan p;
    CallMode mode = CALL_PLAIN;
    bool pair = false;               // this call's pass also scans the batch its stream announced ("scan_ahead")
    int par = 0, slot = -1;          // workspace of the stream, ring slot of the queries (fused)
    int next_slot = -1;              // ring slot of the batch the stream announced (fused; rq_bundle_plan.h)
    const float* scale = nullptr;    // row scales of the metric (a filtered call: the filter's masked copy)
    const rq_filter* filt = nullptr; // the call ranks these rows only (include/rq.h rq_search_filtered)
    int grid_narrow = 0, nwg_split = 0;
};

// The stream's turn: which of its two workspaces (and, fused, which ring slot) the call takes, after whatever has to be
// ordered before it.
static int enter_stream(rq_index* idx, StreamCtx& cx, Call& c) {
    hipStream_t s = c.s;
    if (c.mode == CALL_FUSED) {
        c.par = (int)(cx.calls++ & 1);   // (c.slot: the bundle plan's)
        if (int r = ensure_ring(cx)) return r;
    } else if (c.mode == CALL_PIPED) {
        if (cx.fused_pending) { if (int r = flush_tails(idx, s)) return r; }
        if (!cx.tail) {
            // plain priority: a high-priority tail stream was measured to slow the scan it overlaps
            HIPCHK(hipStreamCreateWithFlags(&cx.tail, hipStreamNonBlocking));
            for (int p = 0; p < 2; ++p) {
                HIPCHK(hipEventCreateWithFlags(&cx.ev_scan[p], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&cx.ev_tail[p], hipEventDisableTiming));
            }
        }
        c.par = (int)(cx.calls++ & 1);
        // this workspace was last used two calls ago: its tail must have finished before it is overwritten
        if (cx.tail_pending[c.par]) { HIPCHK(hipStreamWaitEvent(s, cx.ev_tail[c.par], 0)); cx.tail_pending[c.par] = false; }
    } else {
        if (int r = flush_tails(idx, s)) return r;   // order after anything still on the tail stream
    }
    if (c.mode != CALL_FUSED) cx.hint_q = nullptr;   // a hint is for the next FUSED call of the stream only
    return RQ_OK;
}

// Workgroups per CU of the 64-query grid.
// Small int8 shards searched from SEVERAL caller streams (the per-rank shape of a multi-GPU run: 125k rows, two streams): two fused
// launches are resident at once, so ONE scan workgroup per CU and launch already keeps two per CU streaming, and each lives twice as
// long -- the prologue (48 KB of query fragments + the ring fill) is paid half as often.  Measured, two streams + exchange, us per
// batch with 2 / 1 workgroups per CU: 125k rows 24.2 / 20.5, 250k rows 32.5 / 31.4; the fp16 rows are at the streaming rate either way
// (28.7 / 29.7): int8 only, below 8 quads per workgroup, and only while another stream has a fused tail pending.
static int scan_wg_per_cu(const rq_index* idx, const Call& c) {
    if (c.mode == CALL_FUSED && c.p.use8 && idx->wg_auto && idx->wg_per_cu == 2 && (int64_t)c.p.nquads < (int64_t)16 * idx->cu_count)
        for (auto& kv : idx->ctx)
            if (kv.first != c.s && kv.second.fused_pending) return 1;
    return idx->wg_per_cu;
}

// The scan of the pass that starts at query slot q0.
static RqScanArgs scan_args(const rq_index* idx, const Call& c, const Workspace& w, const QuerySet& qs, int q0, int qb) {
    const CallPlan& p = c.p;
    RqScanArgs a;
    a.i8 = 0; a.qscale = nullptr; a.qlo = nullptr; a.qh_hi = nullptr;
    a.x = idx->x;
    a.row_scale = c.scale;
    a.qh = qs.qh + (size_t)q0 * RQ_DPAD;
    a.bins = w.bins + (size_t)q0 * w.bins_stride;
    a.bins_stride = w.bins_stride;
    a.n_rows = idx->n;
    a.nquads = p.nquads;
    a.nq_valid = idx->scan_nostore == 1 ? 0 : std::min(qb, c.B - q0);
    a.wgmax = w.wgmax + (size_t)q0 * RQ_WGMAX_STRIDE;
    a.wgmax_stride = RQ_WGMAX_STRIDE;
    if (p.use8) {
        a.i8 = qb == 256 ? 4 : (qb == 128 ? 3 : (p.split8 ? 2 : 1)); a.qlo = qs.q8lo; a.x = idx->x8; a.row_scale = c.metric == RQ_METRIC_IP ? idx->scale8_ip : idx->scale8_cos;
        a.qh = (const _Float16*)(qs.q8 + (size_t)q0 * RQ_DPAD); a.qscale = qs.qscale8 + q0;
    }
    return a;
}

// The call's scan passes.  pa: the preparation of the stream's announced batch that rides with a fused launch (nslots 0: none).
static int scan_passes(rq_index* idx, StreamCtx& cx, const Workspace& w, const QuerySet& qs, const Call& c, const RqPrepArgs& pa) {
    const CallPlan& p = c.p;
    hipStream_t s = c.s;
    const bool fused = c.mode == CALL_FUSED, narrow = p.narrow, nt = p.nt;
    // a filtered call masks rows by their NaN scale, which the compare / select form ("epi" = 0, and with it "wide_batch" = 2's
    // 8-wave pass) does not honour beyond the shard's end: it keeps to the forms that do
    const int epi = c.filt ? 1 : idx->epi;
    const bool wave8 = idx->wide_batch == 2 && !c.filt;
    // the fused launch of this layout
    auto scan_tail = [&](const RqScanArgs& sa, const RqTailArgs& t, int tb, int grid, hipEvent_t e0, hipEvent_t e1) {
        return narrow ? rq_scan_narrow_tail_launch(sa, t, tb, pa, nt, grid, s, e0, e1) : rq_scan_tail_launch(sa, t, tb, pa, nt, grid, idx->epi, s, e0, e1);
    };
    for (int blk = 0, q0 = 0; blk < p.npass; q0 += p.pass_q[blk], ++blk) {
        const int qb = p.pass_q[blk];
        const int grid = q0 >= c.nwg_split ? c.grid_narrow : p.grid_wide;
        RqScanArgs a = scan_args(idx, c, w, qs, q0, qb);
        if (c.pair) {   // queries 64..127 of the pass: the announced batch, from the next ring slot
            a.qh_hi = ring_slot(cx, c.next_slot).qh;
            if (idx->scan_nostore != 1) a.nq_valid = 64 + cx.await_B;
        }
        hipEvent_t t0 = nullptr, t1 = nullptr;   // "profile" = 1: every profile_stride-th scan is timed
        if (idx->profile == 1) {
            if (int r = next_event_pair(idx, t0, t1)) return r;
            if (t0 && (idx->scan_seq++ % (uint64_t)idx->profile_stride) != 0) t0 = t1 = nullptr;
        }
        // the event pair rides on the scan dispatch itself (kernel start / end time stamps, no barrier packets)
        const bool legacy = t0 && idx->profile_legacy;   // A/B: hipEventRecord around the launch
        const hipEvent_t e0 = legacy ? nullptr : t0, e1 = legacy ? nullptr : t1;
        if (legacy) HIPCHK(hipEventRecord(t0, s));
        if (c.pair) HIPCHK(rq_scan_wide_launch(a, 0, 128, nt, grid, s, e0, e1));   // compiler-scheduled LDS reads only (never 8: DESIGN 4.4)
        else if (fused && cx.fused_pending) {
            cx.fused_pending = false;
            if (int r = poison_cand(idx, cx.fused_tail, cx.fused_B, s)) return r;
            if (idx->tail_stop == 9) {   // development: fused kernel without its tail workgroups, tail launched after it
                HIPCHK(scan_tail(a, cx.fused_tail, 0, grid, e0, e1));
                RqTailArgs t9 = cx.fused_tail; t9.stop_after = 0;
                HIPCHK(rq_tail_launch(t9, cx.fused_B, s));
            } else
            HIPCHK(scan_tail(a, cx.fused_tail, cx.fused_B, grid, e0, e1));
        } else if (fused && pa.nslots) {   // first call of a loop: no tail to carry yet, but queries to prepare
            RqTailArgs none{};
            none.nbins = p.nbins; none.m = none.k = 1; none.thr_mult = 2.25f; none.thr_slack = 0.f;
            HIPCHK(scan_tail(a, none, 0, grid, e0, e1));
        } else if (narrow) HIPCHK(rq_scan_narrow_launch(a, qb, nt, grid, s, e0, e1));   // 64 queries, or 128 (two query groups per wave)
        else if (fused) HIPCHK(rq_scan_launch(a, 3, 1, 2, 4, nt, grid, idx->epi, s, e0, e1));
        else if (p.use8 && qb == 256) HIPCHK(rq_scan_wide_launch(a, idx->wide256_8, 256, nt, grid, s, e0, e1));   // 256 queries over the int8 image
        else if (p.use8) HIPCHK(rq_scan_launch(a, 3, 1, 2, 4, nt, grid, 1, s, e0, e1));   // 64 queries, or 128 (a.i8 = 3)
        else if (qb == 256) HIPCHK(rq_scan_wide_launch(a, idx->wide256, 256, nt, grid, s, e0, e1));
        else if (qb == 128 && wave8) HIPCHK(rq_scan_launch(a, 3, 4, 1, 8, nt, grid, 0, s, e0, e1));   // round 1's 8-wave pass
        else if (qb == 128) HIPCHK(rq_scan_wide_launch(a, idx->wide128, 128, nt, grid, s, e0, e1));
        else HIPCHK(rq_scan_launch(a, idx->ring, idx->prefetch, idx->kstage, 4, nt, grid, epi, s, e0, e1));
        if (fused && pa.nslots) {
            cx.prepped_q = cx.hint_q; cx.prepped_B = cx.hint_B; cx.prepped_slot = c.next_slot;
            cx.hint_q = nullptr;
        }
        if (legacy) HIPCHK(hipEventRecord(t1, s));
        if (t0) { idx->ev_used++; idx->ev_bytes += idx->n * p.scan_rowb; }
    }
    return RQ_OK;
}

// The fast tail of the call (rq_tail.hip) over workspace w.
static RqTailArgs tail_args(const rq_index* idx, const Call& c, const Workspace& w, const QuerySet& qs) {
    const CallPlan& p = c.p;
    const bool use8 = p.use8;
    RqTailArgs ta;
    ta.q = c.d_q; ta.dim = idx->dim; ta.x = idx->x; ta.dpad = idx->dpad; ta.rownorm64 = idx->rownorm64; ta.n_rows = idx->n;
    ta.bins = w.bins; ta.bins_stride = w.bins_stride; ta.nbins = p.nbins;
    ta.wgmax = w.wgmax; ta.wgmax_stride = RQ_WGMAX_STRIDE; ta.nwg = p.grid_wide; ta.nwg_split = c.nwg_split; ta.nwg2 = c.grid_narrow;
    ta.m = (int)std::min<int64_t>(c.k, c.filt ? c.filt->na : idx->n); ta.metric = c.metric; ta.k = c.k;
    ta.eps = use8 ? scan8_eps(idx) : scan_eps(idx, c.metric);
    ta.qeps = use8 ? (p.split8 ? qs.qeps8s : qs.qeps8) : nullptr;
    ta.binerr = use8 && idx->bin_bound ? idx->binerr8 : nullptr;
    ta.eps_rows_max = use8 ? (float)idx->max_e8 : 0.f;
    // int8 scan: T = P - bound - slack.  The slack covers how far the k-th EXACT score may sit below P (= a k-th largest
    // APPROXIMATE score, biased upward by the errors of the rows that won); it is (thr_mult8 - 1) x the larger of the
    // query's own bound and the one-image bound of a typical query -- also when the queries are split (their bound is
    // smaller, the rows' errors are not)
    ta.thr_mult = use8 ? (float)idx->thr_mult8 : 2.25f;
    ta.thr_slack = use8 ? (float)(idx->max_e8 + 0.009) : 0.f;
    ta.local_topk = idx->tail_local;
    ta.max_row_norm = (float)(idx->max_row_norm * (1.0 + 1e-6)); ta.row_offset = idx->row_offset;
    ta.cand = w.cand; ta.rowcount = w.rowcount; ta.done = w.done; ta.ovf = w.ovf;
    ta.out_scores = c.out.scores; ta.out_rows = c.out.rows; ta.out_keys = c.out.keys; ta.out_status = c.out.status;
    ta.dbg = idx->dbg_stamps;
    ta.stop_after = idx->tail_stop;
    ta.fused_nv = idx->fused_nv;
    return ta;
}

// Member j of a bundle whose pass wrote workspace w: the tail `ta` of the pass moved to the member's quarter -- query slots
// 64 j .. 64 j + 63 of the records, maxima, candidates and counters -- and to the ring's own copy of the member's queries.
static RqTailArgs member_tail(const StreamCtx& cx, const Workspace& w, RqTailArgs ta, int j, int slot) {
    const size_t q0 = (size_t)64 * j;
    ta.q = ring_slot(cx, slot).q32; ta.dim = RQ_DPAD;
    ta.bins = w.bins + q0 * w.bins_stride; ta.wgmax = w.wgmax + q0 * RQ_WGMAX_STRIDE;
    ta.cand = w.cand + q0 * RQ_CAND_CAP; ta.rowcount = w.rowcount + q0; ta.done = w.done + q0; ta.ovf = w.ovf + q0;
    return ta;
}
// What a member's own call says of its tail: k and the outputs.
static void member_call(const rq_index* idx, RqTailArgs& t, int k, const SearchOut& out) {
    t.k = k; t.m = (int)std::min<int64_t>(k, idx->n);
    t.out_scores = out.scores; t.out_rows = out.rows; t.out_keys = out.keys; t.out_status = out.status;
}

// Fused: the tail runs with the NEXT scan launch of the stream (or at the flush).  It reads the ring's own copy of the
// queries, so the caller's buffer is free as soon as this call's work has run.
static void defer_tail(StreamCtx& cx, const Workspace& w, const QuerySet& qs, const Call& c, RqTailArgs ta) {
    ta.q = qs.q32; ta.dim = RQ_DPAD;
    if (!c.pair) { cx.fused_tail = ta; cx.fused_B = c.B; cx.fused_pending = true; return; }
    // a pair: this call is member 0; the announced batch took slots 64..127 of the pass and of the workspace (member 1, whose k
    // and outputs its own call brings: bundle_member, ROLE_CLAIM)
    cx.b_tail[0] = ta; cx.b_B[0] = c.B;
    cx.b_tail[1] = member_tail(cx, w, ta, 1, c.next_slot);
    cx.b_par = c.par; cx.b_metric = c.metric;
}

// The tails of the first n members of the stream's bundle in ONE launch, with the preparation pa (nslots 0: none).
static int launch_bundle_tails(const rq_index* idx, StreamCtx& cx, int n, const RqPrepArgs& pa, hipStream_t s) {
    for (int j = 0; j < n; ++j)
        if (int r = poison_cand(idx, cx.b_tail[j], cx.b_B[j], s)) return r;
    HIPCHK(rq_bundle_tail_launch(cx.b_tail, cx.b_B, n, pa, s));
    return RQ_OK;
}

// ONE pass over the first n members of the stream's bundle (ring slots base ..; nq_valid queries in all) into the quarters of
// workspace cx.w[c.par], by the narrowest form: 64 queries (the plain pass), 128 (rq_scan_wide.hip variant 0, as a pair's) or 256
// (variant 2: compiler-scheduled LDS reads only; three members leave the last quarter invalid).  c: the plan, metric and
// row scales of a 64-query call on this shard.  Afterwards b_tail[0 .. n) are complete but for the k and outputs of members whose
// own call is still to come.
static int bundle_scan(rq_index* idx, StreamCtx& cx, Call& c, int n, int base, int nq_valid) {
    const CallPlan& p = c.p;
    hipStream_t s = c.s;
    Workspace& w = cx.w[c.par];
    const int slots = n == 1 ? 64 : (n == 2 ? 128 : 256);
    // a tail still waiting for a scan (the call before the bundle was on its own) runs first: the wide passes carry none
    if (int r = launch_waiting_tail(idx, cx, s)) return r;
    set_records(cx, w.bins, w.bins_stride, nq_valid, slots);
    if (int r = poison_bins(idx, w.bins, w.bins_stride, slots, s)) return r;
    c.grid_narrow = scan_grid(idx, p.nquads, idx->wg_per_cu);
    c.nwg_split = n == 1 ? 0 : 64;   // (every member's tail counts its queries from 0: all of them on the wide grid)
    RqScanArgs a = scan_args(idx, c, w, ring_slot(cx, base), 0, slots);
    a.nq_valid = idx->scan_nostore == 1 ? 0 : nq_valid;
    if (n == 2) a.qh_hi = ring_slot(cx, bundle_slot_after(base)).qh;   // (three and four members: an aligned quarter of the ring, one block)
    hipEvent_t t0 = nullptr, t1 = nullptr;   // "profile" = 1, as scan_passes
    if (idx->profile == 1) {
        if (int r = next_event_pair(idx, t0, t1)) return r;
        if (t0 && (idx->scan_seq++ % (uint64_t)idx->profile_stride) != 0) t0 = t1 = nullptr;
    }
    const bool legacy = t0 && idx->profile_legacy;
    const hipEvent_t e0 = legacy ? nullptr : t0, e1 = legacy ? nullptr : t1;
    if (legacy) HIPCHK(hipEventRecord(t0, s));
    if (n == 1) HIPCHK(rq_scan_launch(a, 3, 1, 2, 4, p.nt, c.grid_narrow, idx->epi, s, e0, e1));
    else if (n == 2) HIPCHK(rq_scan_wide_launch(a, 0, 128, p.nt, p.grid_wide, s, e0, e1));
    else { HIPCHK(rq_scan_wide_launch(a, 2, 256, p.nt, p.grid_wide, s, e0, e1)); idx->bundles4++; }
    if (legacy) HIPCHK(hipEventRecord(t1, s));
    if (t0) { idx->ev_used++; idx->ev_bytes += idx->n * p.scan_rowb; }
    const RqTailArgs ta = tail_args(idx, c, w, ring_slot(cx, base));
    for (int j = 0; j < n; ++j) {
        RqTailArgs t = member_tail(cx, w, ta, j, (base + j) % RQ_RING_SLOTS);
        const RqTailArgs& own = cx.b_tail[j];
        t.k = own.k; t.m = own.m; t.out_scores = own.out_scores; t.out_rows = own.out_rows; t.out_keys = own.out_keys; t.out_status = own.out_status;
        cx.b_tail[j] = t;
    }
    return RQ_OK;
}

static int break_bundle(rq_index* idx, StreamCtx& cx, const BundleStep& st, hipStream_t s) {
    if (st.brk == BREAK_NONE) return RQ_OK;
    cx.await_q = nullptr;
    if (st.brk == BREAK_SCAN) {   // gathered, not scanned: the plan of a 64-query call on the shard as it is (every mutation completes bundles first)
        Call c{nullptr, 64, cx.b_tail[0].k, cx.b_metric, SearchOut{}, s};
        if (int r = plan_call(idx, 64, c.k, c.metric, nb_default(idx, c.k), false, CALL_MAY_DEFER, &c.p)) return r;
        c.mode = CALL_FUSED; c.par = cx.b_par;
        c.scale = c.metric == RQ_METRIC_IP ? idx->ones : idx->inv_norm;
        if (int r = bundle_scan(idx, cx, c, st.brk_n, st.brk_base, 64 * st.brk_n)) return r;
    }
    // one tail: it rides with the next fused launch of the stream or runs at the flush, as a lone call's; several run now
    if (st.brk_n == 1) { cx.fused_tail = cx.b_tail[0]; cx.fused_B = cx.b_B[0]; cx.fused_pending = true; return RQ_OK; }
    return launch_bundle_tails(idx, cx, st.brk_n, RqPrepArgs{}, s);
}

// A call that the plan made a member of a bundle of four (ROLE_OPEN .. ROLE_JOIN_PASS), the last member of one cut short
// (ROLE_CLOSE) or the claim of a batch that was scanned ahead (ROLE_CLAIM: a pair's second call, a bundle's fourth).
static int bundle_member(rq_index* idx, StreamCtx& cx, Call& c, const BundleStep& st) {
    hipStream_t s = c.s;
    const CallPlan& p = c.p;
    const int j = (st.slot - st.base + RQ_RING_SLOTS) % RQ_RING_SLOTS;   // member number
    if (st.role == ROLE_OPEN) { cx.b_par = (int)(cx.calls & 1); cx.b_metric = c.metric; }
    cx.calls++;
    c.mode = CALL_FUSED; c.par = cx.b_par; c.slot = st.slot; c.next_slot = st.next_slot;
    idx->last_use8 = false; idx->last_wide1 = false;
    if (st.role != ROLE_OPEN || !st.prep_self) idx->hints_used++;
    if (int r = ensure_ring(cx)) return r;
    Workspace& w = cx.w[c.par];
    if (st.role == ROLE_OPEN) {
        // the workspace holds the four quarters before any member's tail is planned; a tail that still waits reads the old one
        if (int r = launch_waiting_tail(idx, cx, s)) return r;
        if (int r = ensure_ws(w, 64 * RQ_BUNDLE_MAX, p.stride, p.m, (size_t)64 * RQ_BUNDLE_MAX * (size_t)p.ncand)) return r;
        if (!w.counters_zero) {
            HIPCHK(hipMemsetAsync(w.rowcount, 0, (size_t)w.bcap * sizeof(int), s));
            HIPCHK(hipMemsetAsync(w.done, 0, (size_t)w.bcap * sizeof(int), s));
            HIPCHK(hipMemsetAsync(w.ovf, 0, (size_t)w.bcap * sizeof(int), s));
            w.counters_zero = true;
        }
    }
    c.scale = idx->inv_norm;
    if (c.metric == RQ_METRIC_IP) { if (int r = ensure_ones(idx, s)) return r; c.scale = idx->ones; }
    member_call(idx, cx.b_tail[j], c.k, c.out);
    cx.b_B[j] = c.B;
    // preparations: the member's own queries unless an earlier launch made them, and the batch it announces -- with the tail
    // launch where this call makes one, else now, both in ONE launch
    const bool tails_now = st.role == ROLE_CLOSE || st.role == ROLE_CLAIM;
    RqPrepArgs self{}, next{};
    if (st.prep_self) self = prep_args(ring_slot(cx, st.slot), c.d_q, idx->dim, c.B, 64, true);
    if (st.next_slot >= 0) next = prep_args(ring_slot(cx, st.next_slot), cx.hint_q, idx->dim, cx.hint_B, 64, true);
    if (self.nslots && next.nslots && !tails_now) HIPCHK(rq_prep2_queries_launch(self, next, s));
    else {
        if (self.nslots) HIPCHK(rq_prep_queries_launch(self, s));
        if (next.nslots && !tails_now) HIPCHK(rq_prep_queries_launch(next, s));
    }
    cx.prepped_q = nullptr;
    if (next.nslots) { cx.prepped_q = cx.hint_q; cx.prepped_B = cx.hint_B; cx.prepped_slot = st.next_slot; }
    cx.await_q = nullptr;
    if (!tails_now) { cx.await_q = cx.hint_q; cx.await_B = cx.hint_B; cx.await_metric = c.metric; }   // (these roles need an announcement)
    cx.hint_q = nullptr;
    switch (st.role) {
    case ROLE_OPEN: case ROLE_JOIN:
        set_records(cx, nullptr, 0, 0, 0);   // gathered: nothing of this call has been scanned yet
        return RQ_OK;
    case ROLE_JOIN_PASS:
        return bundle_scan(idx, cx, c, st.n, st.base, 64 * (st.n - 1) + cx.await_B);
    case ROLE_CLOSE:
        if (int r = bundle_scan(idx, cx, c, st.n, st.base, 64 * (st.n - 1) + c.B)) return r;
        return launch_bundle_tails(idx, cx, st.n, next, s);
    default:   // ROLE_CLAIM: this call's records are its quarter of the pass made ahead
        set_records(cx, cx.b_tail[j].bins, cx.b_tail[j].bins_stride, c.B, 64);
        return launch_bundle_tails(idx, cx, st.n, next, s);
    }
}

// Plain and piped: the tail runs now, behind the scan (piped: on the stream's tail stream).
static int launch_tail(rq_index* idx, StreamCtx& cx, const Call& c, const RqTailArgs& ta) {
    hipStream_t ts = c.s;
    if (c.mode == CALL_PIPED) {
        HIPCHK(hipEventRecord(cx.ev_scan[c.par], c.s));
        HIPCHK(hipStreamWaitEvent(cx.tail, cx.ev_scan[c.par], 0));
        ts = cx.tail;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (idx->profile == 2) {   // profile = 2: time the tail instead of the scan
        if (int r = next_event_pair(idx, e0, e1)) return r;
        if (e0) HIPCHK(hipEventRecord(e0, ts));
    }
    if (int r = poison_cand(idx, ta, c.B, ts)) return r;
    if (c.filt) HIPCHK(rq_tail_filtered_launch(ta, RqFilterArgs{c.filt->d_bits, c.filt->d_first, c.filt->na}, c.B, ts));
    else HIPCHK(rq_tail_launch(ta, c.B, ts));
    if (e0) { HIPCHK(hipEventRecord(e1, ts)); idx->ev_used++; idx->ev_bytes += idx->n * c.p.scan_rowb; }
    if (c.mode == CALL_PIPED) { HIPCHK(hipEventRecord(cx.ev_tail[c.par], cx.tail)); cx.tail_pending[c.par] = true; }
    return RQ_OK;
}

// The generic tail: the m best bins of every query (exact: every bin), their rows re-scored in fp64, top k of those.
static int generic_tail(rq_index* idx, const Call& c, const Workspace& w) {
    const CallPlan& p = c.p;
    hipStream_t s = c.s;
    if (!p.exact) HIPCHK(rq_select_bins_launch(w.bins, w.bins_stride, p.nbins, c.B, p.m, w.binkeys, s));
    RqRescoreArgs ra;
    ra.x = idx->x; ra.dpad = idx->dpad; ra.q32 = w.qs.q32; ra.qnorm64 = w.qs.qn; ra.rownorm64 = idx->rownorm64;
    ra.binkeys = p.exact ? nullptr : w.binkeys; ra.binkeys_stride = p.m; ra.nb = p.nb; ra.metric = c.metric;
    ra.n_rows = idx->n; ra.cand = w.cand;
    if (p.exact && idx->exact_mfma) HIPCHK(rq_exact_scan_launch(ra, c.B, idx->cu_count, s));   // the whole shard: fp64 contraction on the matrix cores
    else HIPCHK(rq_rescore_launch(ra, c.B, s));
    // a filtered call: the keys of excluded rows become 0 = "no row" before anything ranks them
    if (c.filt) HIPCHK(rq_mask_keys_launch(w.cand, (int64_t)c.B * p.ncand, c.filt->d_bits, s));
    RqFinalArgs fa;
    fa.cand = w.cand; fa.ncand = (int)p.ncand; fa.binkeys = w.binkeys; fa.binkeys_stride = p.m; fa.nb = p.nb; fa.nbins = p.exact ? p.nb : p.nbins;
    fa.qnorm64 = w.qs.qn; fa.metric = c.metric; fa.eps = scan_eps(idx, c.metric);
    fa.max_row_norm = (float)(idx->max_row_norm * (1.0 + 1e-6)); fa.k = c.k; fa.row_offset = idx->row_offset; fa.n_rows = c.filt ? c.filt->na : idx->n;   // (n_rows: the rows that can be returned)
    fa.first = c.filt ? c.filt->d_first : nullptr;
    fa.out_scores = c.out.scores; fa.out_rows = c.out.rows; fa.out_keys = c.out.keys; fa.out_status = c.out.status;
    HIPCHK(rq_final_launch(fa, c.B, s));
    return RQ_OK;
}

int scanless_workspace(rq_index* idx, hipStream_t s, int bpad, size_t cand_elems, const QuerySet** qs, uint64_t** cand) {
    if (idx->ctx.find(s) == idx->ctx.end() && idx->ctx.size() >= RQ_MAX_STREAM_CTX)
        if (int r = release_contexts(idx, nullptr)) return r;
    StreamCtx& cx = idx->ctx[s];
    Workspace& w = cx.w[0];
    if (bpad > 0)
        if (int r = ensure_ws(w, bpad, 64, 1, cand_elems)) return r;
    set_records(cx, nullptr, 0, 0, 0);
    if (qs) *qs = &w.qs;
    if (cand) *cand = w.cand;
    return RQ_OK;
}
int mark_no_scan(rq_index* idx, hipStream_t s) { return scanless_workspace(idx, s, 0, 0, nullptr, nullptr); }   // (the debug hooks say so)

// One pass of the pipeline for B queries.  nb < 0: exact scan (every bin re-scored, no corpus scan).  flags: CallFlags (rq_index.h).
int run_pipeline(rq_index* idx, const float* d_q, int B, int k, int metric, int nb, const SearchOut& out, hipStream_t s, unsigned flags,
                 const rq_filter* filt, ScanOnly* scan_only) {
    if (idx->n == 0) {
        if (auto it = idx->ctx.find(s); it != idx->ctx.end()) set_records(it->second, nullptr, 0, 0, 0);
        return fill_empty(B, k, out, s);
    }
    // the int8 image (rq_plan.h scan8_wanted): brought up to date first, which may build it and calibrate the ladder
    bool use8 = false;
    if (scan8_wanted(idx, B, k, nb, flags)) {
        if (int r = ensure_x8(idx, s)) return r;
        use8 = scan8_usable(idx, B, k);
    }
    Call c{d_q, B, k, metric, out, s};
    c.filt = filt;
    if (int r = plan_call(idx, B, k, metric, nb, use8, flags, &c.p)) return r;
    const CallPlan& p = c.p;
    // Workspaces are kept per caller stream.  A caller that keeps creating streams (torch hands out a pool of 32) would
    // pile them up: beyond RQ_MAX_STREAM_CTX streams everything idle is dropped (rare; costs one device synchronisation).
    if (idx->ctx.find(s) == idx->ctx.end() && idx->ctx.size() >= RQ_MAX_STREAM_CTX)
        if (int r = release_contexts(idx, nullptr)) return r;
    StreamCtx& cx = idx->ctx[s];
    const bool may_defer = flags & CALL_MAY_DEFER;
    if (p.fast && may_defer && idx->pipeline == 1) c.mode = CALL_PIPED;
    if (p.fast && may_defer && idx->pipeline == 2 && p.bpad == 64) c.mode = CALL_FUSED;
    const bool fused = c.mode == CALL_FUSED;
    // Options "scan_ahead" / "scan_bundle": a fused call over the fp16 rows whose stream has announced its next batch
    // (rq_search_hint_next_device) is scanned together with it in one 128-query pass (rq_scan_wide.hip variant 0: 266-268 us at 1M
    // rows against 237 us for 64 queries) and, once the loop has proven steady, four consecutive calls in one 256-query pass; the
    // call that brings a batch scanned ahead only runs the tails.  Only on shards the Infinity Cache cannot hold (the rule of the
    // non-temporal loads): smaller shards are not bound by HBM bytes.  What this call is to the calls before it: rq_bundle_plan.h.
    BundleCall bc;
    bc.fused = fused;
    bc.eligible = fused && !use8 && !p.narrow && !filt && !scan_only && idx->scan_ahead && beyond_cache(idx->n, (int64_t)idx->rowb());
    bc.matches = cx.await_q && d_q == cx.await_q && B == cx.await_B && metric == cx.await_metric;
    bc.announces = fused && cx.hint_q && cx.hint_B <= 64;
    bc.full = B == 64;
    bc.next_full = cx.hint_B == 64;
    bc.prepped_slot = fused && cx.prepped_q == d_q && cx.prepped_B == B ? cx.prepped_slot : -1;
    bc.other = (cx.await_q || cx.prepped_q) && !bc.matches && bc.prepped_slot < 0;
    const BundleStep step = bundle_call(cx.bs, bc, idx->scan_bundle);
    if (int r = break_bundle(idx, cx, step, s)) return r;
    if (step.role >= ROLE_OPEN) return bundle_member(idx, cx, c, step);
    c.pair = step.role == ROLE_PAIR_FIRST;
    c.slot = step.slot; c.next_slot = step.next_slot;
    if (int r = enter_stream(idx, cx, c)) return r;
    Workspace& w = cx.w[c.par];
    // (a pair: the announced batch's records, candidates and counters take query slots 64..127 of the same workspace)
    // (... sized at once for the widest bundle the stream may come to, so that a steady loop never regrows it)
    const int ws_slots = c.pair ? 64 * std::max(2, idx->scan_bundle) : p.bpad;
    if (int r = ensure_ws(w, ws_slots, p.exact ? 64 : p.stride, p.exact ? 1 : p.m, std::max((size_t)(c.pair ? ws_slots : B) * (size_t)p.ncand, scan_only ? scan_only->cand_elems : (size_t)0))) return r;
    c.scale = idx->inv_norm;
    if (metric == RQ_METRIC_IP) { if (int r = ensure_ones(idx, s)) return r; c.scale = idx->ones; }
    if (filt) {   // excluded rows get a NaN scale, like pad rows: no scan form tests a row's validity
        if (int r = ensure_filter_scale(idx, filt, metric, s)) return r;
        c.scale = filt->scale[metric];
    }

    // counter protocol of the tail kernel: rowcount/done/ovf are zero on entry and the kernel leaves them zero
    if (p.fast && !w.counters_zero) {
        HIPCHK(hipMemsetAsync(w.rowcount, 0, (size_t)w.bcap * sizeof(int), s));
        HIPCHK(hipMemsetAsync(w.done, 0, (size_t)w.bcap * sizeof(int), s));
        HIPCHK(hipMemsetAsync(w.ovf, 0, (size_t)w.bcap * sizeof(int), s));
        w.counters_zero = true;
    }
    if (use8) idx->scan8_used++;
    // (may_defer: the caller's own search; CALL_FETCH: the fetch of a route -- not a repair pass of rq_search_fixup_device)
    if (may_defer || (flags & CALL_FETCH)) { idx->last_use8 = use8; idx->last_wide1 = use8 && B > 64 && idx->scan8_level[p.kclass] == 1; }
    // unit-norm fp16 query fragments for the scan (+ padded fp32 queries / fp64 norms for the generic tail)
    // ... unless the previous launch of this stream has already prepared exactly these queries (rq_search_hint_next_device)
    const QuerySet qs = fused ? ring_slot(cx, c.slot) : w.qs;
    const bool prepared = fused && !step.prep_self;
    cx.prepped_q = nullptr;
    if (prepared) idx->hints_used++;
    else HIPCHK(rq_prep_queries_launch(prep_args(qs, d_q, idx->dim, B, p.bpad, true), s));
    // the queries announced for the NEXT call are prepared by extra workgroups of this call's fused launch
    RqPrepArgs pa{};
    if (fused && cx.hint_q) pa = prep_args(ring_slot(cx, c.next_slot), cx.hint_q, idx->dim, cx.hint_B, 64, true);
    if (c.pair) {
        // the pass reads the announced batch from the next ring slot: it is prepared first, by a launch of its own; and a tail
        // still waiting for a scan (the call before this one was not paired) runs on its own, as the wide pass carries none
        HIPCHK(rq_prep_queries_launch(pa, s));
        cx.prepped_q = cx.hint_q; cx.prepped_B = cx.hint_B; cx.prepped_slot = c.next_slot;
        cx.await_q = cx.hint_q; cx.await_B = cx.hint_B; cx.await_metric = metric;
        cx.hint_q = nullptr;
        pa.nslots = 0;
        if (int r = launch_waiting_tail(idx, cx, s)) return r;
    }
    c.grid_narrow = scan_grid(idx, p.nquads, scan_wg_per_cu(idx, c));
    c.nwg_split = c.pair ? 64 : p.nwg_split;   // both batches of a pair: the wide grid
    if (p.exact) {
        if (scan_only) return set_err(RQ_EINVAL, "internal: a scan-only call on a shard whose plan is the exact scan");   // (rq_range_plan.h asks plan_call first)
        set_records(cx, nullptr, 0, 0, 0);
        return generic_tail(idx, c, w);
    }
    const int slots = c.pair ? 128 : p.bpad;   // (a pair: both halves; the upper one is the next call's, bundle_member)
    set_records(cx, w.bins, w.bins_stride, c.pair ? 64 + cx.await_B : B, slots);
    if (int r = poison_bins(idx, w.bins, w.bins_stride, slots, s)) return r;
    if (int r = scan_passes(idx, cx, w, qs, c, pa)) return r;
    if (scan_only) { scan_only->w = &w; return RQ_OK; }   // a range search: its own tail reads the records (rq_range.hip)
    if (!p.fast) return generic_tail(idx, c, w);
    if (idx->tail_stop) w.counters_zero = false;   // a truncated tail does not reset its counters
    const RqTailArgs ta = tail_args(idx, c, w, qs);
    if (fused) { defer_tail(cx, w, qs, c, ta); return RQ_OK; }
    return launch_tail(idx, cx, c, ta);
}

// ---- entry points -------------------------------------------------------------------------------
int check_search_args(const rq_index* idx, const void* q, int B, int k, int metric, const void* sc, const void* rows) {
    if (!idx || !q || !sc || !rows) return set_err(RQ_EINVAL, "null argument");
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (k < 1 || k > RQ_MAX_K) return set_err(RQ_EINVAL, "k %d outside 1..%d", k, RQ_MAX_K);
    if (metric != RQ_METRIC_COSINE && metric != RQ_METRIC_IP) return set_err(RQ_EINVAL, "unknown metric %d", metric);
    return RQ_OK;
}

extern "C" int rq_search_device(rq_index* idx, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                                uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_search_args(idx, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "device-pointer searches on a multi-device index: use rq_search (host buffers), or one index per device");
    RQ_ON_DEVICE(idx);
    idx->t.searches++;
    idx->t.queries += B;
    return run_pipeline(idx, d_queries, B, k, metric, nb_default(idx, k), {d_scores, d_rows, d_keys, d_status}, (hipStream_t)stream, CALL_MAY_DEFER | CALL_ALLOW8);
}

// The queries of the NEXT rq_search_device call on `stream` ("pipeline" = 2 loops): the call made right after this one
// prepares them with 64 extra workgroups of its own launch, and the call after that -- if it is given exactly d_next_queries
// and B -- skips its preparation launch.  Advisory: anything else simply prepares its queries itself.
extern "C" int rq_search_hint_next_device(rq_index* idx, const float* d_next_queries, int B, void* stream) {
    if (!idx) return set_err(RQ_EINVAL, "null index");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "device-pointer searches on a multi-device index: use rq_search (host buffers), or one index per device");
    if (B < 0 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 0..65535", B);
    // Advisory.  A hint for a stream no search has run on yet only makes a host-side record (no device memory, no device call:
    // hence no device guard here); the workspace is allocated by the search that follows.  Beyond RQ_MAX_STREAM_CTX remembered
    // streams the hint is dropped instead (the call then prepares its own queries).  Remembered stream handles are never used
    // again by the library on its own account (flush_all runs pending tails on the index's own stream), so a record for a stream
    // the caller destroys later is harmless.
    if (idx->ctx.find((hipStream_t)stream) == idx->ctx.end() && idx->ctx.size() >= RQ_MAX_STREAM_CTX) return RQ_OK;
    StreamCtx& c = idx->ctx[(hipStream_t)stream];
    const bool usable = d_next_queries && B >= 1 && B <= 64 && idx->use_hint && idx->pipeline == 2;
    c.hint_q = usable ? d_next_queries : nullptr;
    c.hint_B = usable ? B : 0;
    return RQ_OK;
}

extern "C" int rq_search_train_device(rq_index* idx, int n_batches, const float* const* d_queries, int B, int k, int metric,
                                      float* const* d_scores, int64_t* const* d_rows, uint64_t* const* d_keys, int* const* d_status,
                                      void* const* streams, int n_streams) {
    if (!idx || n_batches < 0 || !d_queries || !d_scores || !d_rows || !d_status || !streams || n_streams < 1 || n_streams > 8)
        return set_err(RQ_EINVAL, "bad train arguments");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "device-pointer searches on a multi-device index: use rq_search (host buffers), or one index per device");
    for (int i = 0; i < n_batches; ++i) {
        if (int r = check_search_args(idx, d_queries[i], B, k, metric, d_scores[i], d_rows[i])) return r;
        if (!d_status[i]) return set_err(RQ_EINVAL, "d_status is required");
    }
    RQ_ON_DEVICE(idx);
    for (int i = 0; i < n_batches; ++i) {
        hipStream_t s = (hipStream_t)streams[i % n_streams];
        if (const float* nxt = d_queries[i + n_streams])
            if (int r = rq_search_hint_next_device(idx, nxt, B, s)) return r;
        idx->t.searches++;
        idx->t.queries += B;
        if (int r = run_pipeline(idx, d_queries[i], B, k, metric, nb_default(idx, k), {d_scores[i], d_rows[i], d_keys ? d_keys[i] : nullptr, d_status[i]}, s, CALL_MAY_DEFER | CALL_ALLOW8))
            return r;
    }
    return RQ_OK;
}

extern "C" int rq_search_flush_device(rq_index* idx, void* stream) {
    if (!idx) return set_err(RQ_EINVAL, "null index");
    if (!idx->shards.empty()) return RQ_OK;
    RQ_ON_DEVICE(idx);
    return flush_tails(idx, (hipStream_t)stream);
}

extern "C" int rq_search_fixup_device(rq_index* idx, const float* d_queries, int B, int k, int metric, float* d_scores,
                                      int64_t* d_rows, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_search_args(idx, d_queries, B, k, metric, d_scores, d_rows)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "device-pointer searches on a multi-device index: use rq_search (host buffers), or one index per device");
    RQ_ON_DEVICE(idx);
    return fixup_ladder(idx, nullptr, d_queries, B, k, metric, d_scores, d_rows, d_keys, d_status, (hipStream_t)stream);
}

int fixup_ladder(rq_index* idx, const rq_filter* filt, const float* d_queries, int B, int k, int metric, float* d_scores,
                 int64_t* d_rows, uint64_t* d_keys, int* d_status, hipStream_t s) {
    if (int r = flush_tails(idx, s)) return r;
    Stage fx(s);   // (owns no buffer: the workspace's grow-only fix_* are the packed ones)
    RepairList bad;
    if (int r = repair_flagged(fx, d_status, B, bad)) return r;
    if (!filt) scan8_account(idx, k, B, (int)bad.size());   // (filtered calls never touch the int8 image or its ladder)
    if (bad.empty()) return 0;
    const int repaired = (int)bad.size();
    idx->repaired_total += repaired;
    if (filt) idx->filter_repaired += repaired;
    Workspace& w = idx->ctx[s].w[0];
    if (repaired > w.fix_bcap || k > w.fix_k) {
        const int nb_ = std::max(repaired, w.fix_bcap), nk = std::max(k, w.fix_k);
        if (int r = ensure(w.fix_q, (size_t)nb_ * RQ_MAX_DIM)) return r;
        if (int r = ensure(w.fix_scores, (size_t)nb_ * nk)) return r;
        if (int r = ensure(w.fix_rows, (size_t)nb_ * nk)) return r;
        if (int r = ensure(w.fix_keys, (size_t)nb_ * nk)) return r;
        if (int r = ensure(w.fix_status, (size_t)nb_)) return r;
        w.fix_bcap = nb_; w.fix_k = nk;
    }
    // ladder: (queries that came from the int8 scan: the fp16 scan, whose threshold certifies by construction,) 4x wider
    // candidate set, then the full fp64 scan
    const int nb1 = std::min(RQ_NB_MAX, 4 * nb_default(idx, k));
    const bool from8 = !filt && idx->last_use8 && idx->x8 && idx->scan8;
    const unsigned allow8 = filt ? 0u : (unsigned)CALL_ALLOW8;
    const SearchOut fix_out{w.fix_scores, w.fix_rows, w.fix_keys, w.fix_status};
    for (int level = from8 ? -1 : 0; level < 2 && !bad.empty(); ++level) {
        const int nbq = (int)bad.size();
        if (int r = repair_pack(fx, bad, {repair_col(d_queries, w.fix_q, (size_t)idx->dim)})) return r;
        if (level < 0) {
            if (int r = run_pipeline(idx, w.fix_q, nbq, k, metric, nb_default(idx, k), fix_out, s, 0, filt)) return r;
        } else if (level == 0) {
            idx->t.widened += nbq;
            // (the fast tail fails only when its candidate lists overflow: the wider pass uses the generic sorted tail)
            if (int r = run_pipeline(idx, w.fix_q, nbq, k, metric, nb1, fix_out, s, CALL_FORCE_GENERIC | allow8, filt)) return r;
        } else {
            idx->t.exact_scans += nbq;
            // bound the candidate memory: a few queries per exact pass
            const int group = queries_per_gib(nbq, (idx->n + 63) / 64 * 64);
            for (int off = 0; off < nbq; off += group) {
                const int g = std::min(group, nbq - off);
                if (int r = run_pipeline(idx, w.fix_q + (size_t)off * idx->dim, g, k, metric, -1, fix_out.from(off, k), s, allow8, filt)) return r;
            }
        }
        // the slots that certified at this rung go back, the others climb on in slots 0, 1, ...
        std::vector<int> st2;
        if (int r = repair_status(fx, w.fix_status, nbq, st2)) return r;
        RepairList done, still;
        for (const RepairPair& p : bad) {
            if (st2[(size_t)p.slot] == 0) done.push_back(p);
            else still.push_back({(int)still.size(), p.q});
        }
        repair_unpack(fx, done, {repair_col(d_scores, w.fix_scores, k), repair_col(d_rows, w.fix_rows, k), repair_col(d_keys, w.fix_keys, k)}, d_status);
        if (int r = fx.finish()) return r;
        bad.swap(still);
    }
    if (!bad.empty()) return set_err(RQ_EHIP, "internal: %zu queries uncertified after the exact scan", bad.size());
    return repaired;
}

// The blocking host-buffer search in two halves, so that a multi-device parent can enqueue on every device before it
// waits for any: search_begin stages the queries and enqueues the search on the index's own stream, search_end waits,
// repairs uncertified queries and hands the results over.
int rq_search_begin(rq_index* idx, const float* queries, int B, int k, int metric) {
    RQ_ON_DEVICE(idx);
    if (B > idx->h_bcap || k > idx->h_kcap) {
        const int nb = std::max(B, idx->h_bcap), nk = std::max(k, idx->h_kcap);
        if (int r = ensure(idx->h_dq, (size_t)nb * RQ_MAX_DIM)) return r;
        if (int r = ensure(idx->h_dscores, (size_t)nb * nk)) return r;
        if (int r = ensure(idx->h_drows, (size_t)nb * nk)) return r;
        if (int r = ensure(idx->h_dstatus, (size_t)nb)) return r;
        idx->h_bcap = nb; idx->h_kcap = nk;
    }
    hipStream_t s = idx->own_stream;
    idx->hs_small = (size_t)B * k <= 65536;
    if (idx->hs_small) {
        // one device block [rows int64 | scores fp32 | status int32] -> one copy into pinned memory -> one synchronisation
        const size_t off_s = (size_t)B * k * sizeof(int64_t), off_t = off_s + (size_t)B * k * sizeof(float);
        const size_t bytes = off_t + (size_t)B * sizeof(int), qfloats = (size_t)B * idx->dim;
        if (bytes > idx->hs_bytes) {
            if (idx->hs_dev) (void)hipFree(idx->hs_dev);
            if (idx->hs_pin) (void)hipHostFree(idx->hs_pin);
            idx->hs_dev = nullptr; idx->hs_pin = nullptr; idx->hs_bytes = 0;
            HIPCHK(hipMalloc((void**)&idx->hs_dev, bytes));
            HIPCHK(hipHostMalloc((void**)&idx->hs_pin, bytes, hipHostMallocDefault));
            idx->hs_bytes = bytes;
        }
        if (qfloats > idx->hs_qfloats) {
            if (idx->hs_pin_q) (void)hipHostFree(idx->hs_pin_q);
            idx->hs_pin_q = nullptr; idx->hs_qfloats = 0;
            HIPCHK(hipHostMalloc((void**)&idx->hs_pin_q, qfloats * sizeof(float), hipHostMallocDefault));
            idx->hs_qfloats = qfloats;
        }
        int64_t* d_rows = (int64_t*)idx->hs_dev;
        float* d_scores = (float*)(idx->hs_dev + off_s);
        int* d_status = (int*)(idx->hs_dev + off_t);
        std::memcpy(idx->hs_pin_q, queries, qfloats * sizeof(float));
        HIPCHK(hipMemcpyAsync(idx->h_dq, idx->hs_pin_q, qfloats * sizeof(float), hipMemcpyHostToDevice, s));
        if (int r = rq_search_device(idx, idx->h_dq, B, k, metric, d_scores, d_rows, nullptr, d_status, s)) return r;
        if (int r = flush_tails(idx, s)) return r;   // (option "pipeline": the tail must have run before the copy)
        HIPCHK(hipMemcpyAsync(idx->hs_pin, idx->hs_dev, bytes, hipMemcpyDeviceToHost, s));
        return RQ_OK;
    }
    HIPCHK(hipMemcpyAsync(idx->h_dq, queries, (size_t)B * idx->dim * sizeof(float), hipMemcpyHostToDevice, s));
    return rq_search_device(idx, idx->h_dq, B, k, metric, idx->h_dscores, idx->h_drows, nullptr, idx->h_dstatus, s);
}

int rq_search_end(rq_index* idx, int B, int k, int metric, float* out_scores, int64_t* out_rows) {
    RQ_ON_DEVICE(idx);
    hipStream_t s = idx->own_stream;
    if (idx->hs_small) {
        const size_t off_s = (size_t)B * k * sizeof(int64_t), off_t = off_s + (size_t)B * k * sizeof(float);
        int64_t* d_rows = (int64_t*)idx->hs_dev;
        float* d_scores = (float*)(idx->hs_dev + off_s);
        int* d_status = (int*)(idx->hs_dev + off_t);
        HIPCHK(hipStreamSynchronize(s));
        const int* st = (const int*)(idx->hs_pin + off_t);
        bool clean = true;
        for (int q = 0; q < B; ++q) clean = clean && st[q] == 0;
        if (!clean) {   // rare: repair on the device, fetch again
            const int fr = rq_search_fixup_device(idx, idx->h_dq, B, k, metric, d_scores, d_rows, nullptr, d_status, s);
            if (fr < 0) return fr;
            HIPCHK(hipMemcpyAsync(idx->hs_pin, idx->hs_dev, off_t, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        } else scan8_account(idx, k, B, 0);   // the int8 ladder sees the clean calls too
        std::memcpy(out_rows, idx->hs_pin, off_s);
        std::memcpy(out_scores, idx->hs_pin + off_s, off_t - off_s);
        return RQ_OK;
    }
    const int fr = rq_search_fixup_device(idx, idx->h_dq, B, k, metric, idx->h_dscores, idx->h_drows, nullptr, idx->h_dstatus, s);
    if (fr < 0) return fr;
    HIPCHK(hipMemcpyAsync(out_scores, idx->h_dscores, (size_t)B * k * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_rows, idx->h_drows, (size_t)B * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RQ_OK;
}

extern "C" int rq_search(rq_index* idx, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows) {
    if (int r = check_search_args(idx, queries, B, k, metric, out_scores, out_rows)) return r;
    if (!idx->shards.empty()) return rq_multi_search(idx, queries, B, k, metric, out_scores, out_rows);
    if (int r = rq_search_begin(idx, queries, B, k, metric)) return r;
    return rq_search_end(idx, B, k, metric, out_scores, out_rows);
}

extern "C" int rq_merge_keys_device(const uint64_t* d_keys_in, int n_per_query, int B, int k, float* d_scores, int64_t* d_rows,
                                    uint64_t* d_keys_out, void* stream) {
    if (!d_keys_in || !d_scores || !d_rows || B < 1 || k < 1 || k > RQ_MAX_K || n_per_query < 0) return set_err(RQ_EINVAL, "bad merge arguments");
    HIPCHK(rq_merge_keys_launch(d_keys_in, n_per_query, B, k, d_scores, d_rows, d_keys_out, (hipStream_t)stream));
    return RQ_OK;
}
