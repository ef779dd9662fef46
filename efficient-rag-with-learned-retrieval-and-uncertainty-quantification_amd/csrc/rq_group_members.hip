// rq_group_members.hip -- the members of the top groups (include/rq.h rq_group_fill_device, rq_search_group_members*): the best s
// rows of each of the k best groups -- "the top k articles, each with its best passages" -- next to the rows.
//
// A grouped search (rq_group.hip) returns each group's winner.  Its other members cannot come from the ranking: a group's third
// best row may rank anywhere, so no list of RQ_MAX_K rows is sure to hold it.  They are fetched THROUGH THE GROUP: a member table
// (rq_group_members_plan.h: the grouped rows sorted by (id, row), the distinct ids, their offsets) is built from the host copy of
// the ids by the first call that needs it, and one workgroup per (query, group slot) scores the rows of the slot's group -- every
// one of them, so the best s of them are exact -- with rq_rowdot.h's dot product, sorts their keys in LDS and writes the first s.
// A group with more rows than the LDS sort holds is left to rq_search_group_members_fixup_device, which searches that group's
// rows through a temporary rq_filter.  No scan kernel is touched.
#include "rq_group_members_plan.h"
#include "rq_repair.h"
#include "rq_rowdot.h"
#include "rq_score_plan.h"   // score_groups: the queries of a call in groups of prepared-query slots

// ---- kernel -------------------------------------------------------------------------------------
struct RqGroupFillArgs {
    const void* x; const double* rownorm64;   // stored rows (DP elements each) and their norms
    int64_t n_rows, row_offset;               // n_rows >= 1
    const float* q32; const double* qnorm64;  // [queries][768] raw fp32 queries, zero padded, and their norms (rq_prep_body)
    const uint32_t* fbits;                    // the filter's bitmap over local rows, null = every row is in play
    const int32_t* gt_ids; const uint32_t* gt_off; const uint32_t* gt_rows; int64_t gt_groups;   // the member table (gt_groups may be 0)
    const int64_t* win_rows;                  // [queries][k] GLOBAL rows; -1 / outside the shard = an absent slot
    const int32_t* win_groups;                // [queries][k] the slots' group ids; negative = the row is a group of its own
    int k, s, metric, cap, sort_n;            // cap <= sort_n, a power of two <= RQ_GROUP_FILL_MAX
    float* out_scores; int64_t* out_rows;     // [queries][k][s]
    int32_t* out_count;                       // [queries][k]
    int* out_status;                          // [queries]: only ever SET to 1 here (plain stores of the same value: no atomics)
    int* scored;                              // [queries][k] members scored
};

// grid (k, queries), 256 threads, 3 KiB + sort_n x 8 bytes of dynamic LDS (the query, the keys).  (a) the slot's member list: nothing (absent slot, an id no row
// carries), the row itself (ungrouped), or the id's range of the table by binary search; more rows than cap: count -1, status 1;
// (b) the query into LDS; a wave scores 8 members per round exactly as rq_score_rows_kernel does (lane group rloc owns members
// j0 + rloc and j0 + 4 + rloc); a member outside the list or the filter loads the slot's own row -- a valid address -- and leaves
// key 0; (c) bitonic sort, keys descending: present keys are distinct (they carry their row), so the order is the canonical one
// whatever the schedule, and key 0 (no score maps to it: rq_make_key of -inf is 0x007fffff........) sorts last; (d) the first s.
template <int DP>
__global__ __launch_bounds__(RQ_GROUP_FILL_THREADS) void rq_group_members_kernel(RqGroupFillArgs a) {
    static_assert(DP == 384 || DP == RQ_DPAD, "stored row length");
    static_assert(RQ_GROUP_FILL_THREADS == 256, "4 waves x 8 members per round; 3 query elements per thread");
    constexpr int NP = DP / 128;   // 16-byte loads per lane and row
    extern __shared__ __attribute__((aligned(16))) char smem[];   // all of it dynamic: the base stays 16-byte aligned for the float4 reads of qs
    float* qs = (float*)smem;                                     // [RQ_DPAD]
    uint64_t* key = (uint64_t*)(smem + RQ_DPAD * sizeof(float));  // [a.sort_n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.y;
    const int64_t slot = (int64_t)q * a.k + (int)blockIdx.x;
    float* out_s = a.out_scores + slot * a.s;
    int64_t* out_r = a.out_rows + slot * a.s;

    // (a) -- uniform over the workgroup
    const int64_t wrow = a.win_rows[slot], wloc = wrow - a.row_offset;
    const int32_t wg = a.win_groups[slot];
    const bool present = wrow >= 0 && wloc >= 0 && wloc < a.n_rows;
    int64_t begin = 0, cnt = 0;
    if (present && wg < 0) cnt = 1;
    if (present && wg >= 0) {
        int64_t lo = 0, hi = a.gt_groups;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.gt_ids[mid] < wg) lo = mid + 1; else hi = mid;
        }
        if (lo < a.gt_groups && a.gt_ids[lo] == wg) {
            begin = (int64_t)a.gt_off[lo];
            cnt = (int64_t)a.gt_off[lo + 1] - begin;
        }
    }
    const bool overflow = cnt > (int64_t)a.cap || cnt > (int64_t)a.sort_n;
    if (overflow || cnt <= 0) {
        for (int t = tid; t < a.s; t += RQ_GROUP_FILL_THREADS) { out_s[t] = 0.f; out_r[t] = -1; }
        if (tid == 0) {
            a.out_count[slot] = overflow ? -1 : 0;
            a.scored[slot] = 0;
            if (overflow) a.out_status[q] = 1;
        }
        return;
    }
    const int n = (int)cnt;
    int P = RQ_GROUP_FILL_MIN_SORT;
    while (P < n) P <<= 1;   // (n <= sort_n, a power of two: P <= sort_n)

    // (b)
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) qs[pp * 256 + tid] = a.q32[(size_t)q * RQ_DPAD + pp * 256 + tid];
    for (int i = tid; i < P; i += RQ_GROUP_FILL_THREADS) key[i] = 0;
    __syncthreads();
    const double qn = a.qnorm64[q];
    const int sub = lane & 15, rloc = lane >> 4;
    const char* xb = (const char*)a.x;
    const bool single = wg < 0;
    for (int j0 = wave * 8; j0 < n; j0 += RQ_GROUP_FILL_THREADS / 8) {   // uniform over the wave
        rq_half8 xv[2][NP];
        int pos[2];
        int64_t loc[2];
        double rn[2];
        bool member[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pos[u] = j0 + u * 4 + rloc;
            member[u] = pos[u] < n;
            int64_t r = member[u] ? (single ? wloc : (int64_t)a.gt_rows[begin + pos[u]]) : wloc;
            if (r >= a.n_rows) { member[u] = false; r = wloc; }   // (never an address outside the shard)
            if (member[u] && a.fbits) member[u] = (a.fbits[r >> 5] >> (r & 31)) & 1u;
            loc[u] = r;
            rn[u] = a.rownorm64[r];
            const char* p = xb + r * (DP * 2) + sub * 16;
#pragma unroll
            for (int pp = 0; pp < NP; ++pp) xv[u][pp] = *(const rq_half8*)(p + pp * 256);
        }
        double dot[2];
        rq_rowdot16<NP, 2>(xv, qs, sub, dot);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (sub == 0 && member[u]) {
                double sc = dot[u];
                if (a.metric == 0) sc = dot[u] / (qn * rn[u] + 1e-30);
                if (qn == 0.0) sc = 0.0;   // a zero-norm query scores every row 0 (include/rq.h), as rq_score_rows_kernel
                key[pos[u]] = rq_make_key(rq_sanitize((float)sc), (uint32_t)loc[u]);   // (-0.0 becomes +0.0 inside the key)
            }
        }
    }
    __syncthreads();

    // (c)
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += RQ_GROUP_FILL_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const uint64_t ka = key[lo], kb = key[hi];
                const bool desc = (lo & size) == 0;
                if (desc ? ka < kb : ka > kb) { key[lo] = kb; key[hi] = ka; }
            }
            __syncthreads();
        }
    }

    // (d)
    for (int t = tid; t < a.s; t += RQ_GROUP_FILL_THREADS) {
        const uint64_t kk = t < P ? key[t] : 0;
        out_s[t] = kk ? rq_key_score(kk) : 0.f;
        out_r[t] = kk ? a.row_offset + (int64_t)rq_key_index(kk) : (int64_t)-1;
    }
    if (tid == 0) {
        int lo = 0, hi = P;   // the first absent key = the members in play
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key[mid] != 0) lo = mid + 1; else hi = mid;
        }
        a.out_count[slot] = min(lo, a.s);
        a.scored[slot] = lo;
    }
}

static hipError_t rq_group_members_launch(const RqGroupFillArgs& a, int queries, int dp, hipStream_t stream) {
    if (queries < 1 || queries > 65535 || a.k < 1 || a.s < 1 || (int64_t)a.k * a.s > RQ_MAX_K || a.n_rows < 1 || (dp != 384 && dp != RQ_DPAD) || a.cap < 1 || a.cap > a.sort_n ||
        a.sort_n < RQ_GROUP_FILL_MIN_SORT || a.sort_n > RQ_GROUP_FILL_MAX || (a.sort_n & (a.sort_n - 1)) || a.gt_groups < 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.k, (unsigned)queries);
    const size_t lds = RQ_DPAD * sizeof(float) + (size_t)a.sort_n * sizeof(uint64_t);   // (= GroupFillGeometry::lds_bytes)
    if (dp == 384) hipLaunchKernelGGL(rq_group_members_kernel<384>, grid, dim3(RQ_GROUP_FILL_THREADS), lds, stream, a);
    else hipLaunchKernelGGL(rq_group_members_kernel<RQ_DPAD>, grid, dim3(RQ_GROUP_FILL_THREADS), lds, stream, a);
    return hipGetLastError();
}

// ---- the member table ---------------------------------------------------------------------------------
void drop_group_table(rq_index* idx) {
    free_dev(idx->gt_ids, idx->gt_off, idx->gt_rows);
    idx->gt_groups = 0; idx->gt_largest = 0; idx->gt_valid = false;
}

// Built by the first fill after rq_index_set_groups (blocking: host sort, three uploads).  Without a group set there is no table:
// every row is a group of its own and no slot looks anything up.
static int ensure_group_table(rq_index* idx) {
    if (idx->gt_valid || idx->h_groups.empty()) return RQ_OK;
    GroupTable t;
    group_table_build(idx->h_groups.data(), (int64_t)idx->h_groups.size(), t);
    drop_group_table(idx);
    if (hipMalloc((void**)&idx->gt_ids, std::max<size_t>(t.ids.size(), 1) * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&idx->gt_off, t.off.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&idx->gt_rows, std::max<size_t>(t.rows.size(), 1) * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        drop_group_table(idx);
        return set_err(RQ_ENOMEM, "hipMalloc of the member table of %zu rows in %zu groups failed", t.rows.size(), t.ids.size());
    }
    if (!t.ids.empty()) HIPCHK(hipMemcpy(idx->gt_ids, t.ids.data(), t.ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(idx->gt_off, t.off.data(), t.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!t.rows.empty()) HIPCHK(hipMemcpy(idx->gt_rows, t.rows.data(), t.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    idx->gt_groups = (int64_t)t.ids.size(); idx->gt_largest = t.largest; idx->gt_valid = true;
    idx->group_table_builds++;
    return RQ_OK;
}

// ---- the fill ---------------------------------------------------------------------------------------------
struct MembersOut {   // a call's device outputs
    float* scores; int64_t* rows; int32_t* count; int* status;
};

// Enqueues the fill of B x k slots; the caller has completed what the stream defers and set the status words (the kernel only
// raises them).  The queries are prepared in groups, as rq_score_rows_device prepares them.
static int group_fill(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int s, int metric, const int64_t* d_win_rows, const int32_t* d_win_groups,
                      const MembersOut& out, hipStream_t st) {
    idx->group_fill_calls++;
    const size_t slots = (size_t)B * (size_t)k;
    if (idx->n == 0) {   // every slot is absent
        idx->gm_scored_slots = 0;
        if (int r = mark_no_scan(idx, st)) return r;
        HIPCHK(hipMemsetAsync(out.scores, 0, slots * (size_t)s * sizeof(float), st));
        HIPCHK(hipMemsetAsync(out.rows, 0xff, slots * (size_t)s * sizeof(int64_t), st));
        HIPCHK(hipMemsetAsync(out.count, 0, slots * sizeof(int32_t), st));
        return RQ_OK;
    }
    if (int r = ensure_group_table(idx)) return r;
    if ((int64_t)slots > idx->gm_scored_cap) {   // (hipFree waits for the device: no earlier fill still writes the old array)
        free_dev(idx->gm_scored);
        idx->gm_scored_cap = 0; idx->gm_scored_slots = 0;
        if (hipMalloc((void**)&idx->gm_scored, slots * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            idx->gm_scored = nullptr;
            return set_err(RQ_ENOMEM, "hipMalloc of %zu slot counters failed", slots);
        }
        idx->gm_scored_cap = (int64_t)slots;
    }
    idx->gm_scored_slots = (int64_t)slots;
    const ScoreGroups g = score_groups(B);
    const QuerySet* qs = nullptr;
    if (int r = scanless_workspace(idx, st, g.slots, 0, &qs, nullptr)) return r;
    const int cap = group_fill_cap(idx->group_fill_cap);
    for (int i = 0; i < g.count; ++i) {
        const int off = i * g.group, nq = std::min(g.group, B - off);
        const RqPrepArgs pa = prep_args(*qs, d_q + (size_t)off * idx->dim, idx->dim, nq, (nq + 63) / 64 * 64, false);
        const GroupFillGeometry geo = group_fill_geometry(nq, k, idx->gt_largest, cap);
        const size_t so = (size_t)off * (size_t)k;
        RqGroupFillArgs a;
        a.x = idx->x; a.rownorm64 = idx->rownorm64; a.n_rows = idx->n; a.row_offset = idx->row_offset;
        a.q32 = qs->q32; a.qnorm64 = qs->qn; a.fbits = f ? f->d_bits : nullptr;
        a.gt_ids = idx->gt_ids; a.gt_off = idx->gt_off; a.gt_rows = idx->gt_rows; a.gt_groups = idx->gt_valid ? idx->gt_groups : 0;
        a.win_rows = d_win_rows + so; a.win_groups = d_win_groups + so;
        a.k = k; a.s = s; a.metric = metric; a.cap = std::min(cap, geo.sort_n); a.sort_n = geo.sort_n;
        a.out_scores = out.scores + so * (size_t)s; a.out_rows = out.rows + so * (size_t)s; a.out_count = out.count + so; a.out_status = out.status + off;
        a.scored = idx->gm_scored + so;
        HIPCHK(rq_prep_queries_launch(pa, st));
        HIPCHK(rq_group_members_launch(a, nq, idx->dpad, st));
    }
    return RQ_OK;
}

// The grouped search with its winners in the stream's workspace ([B][k] scores and rows; the ids go to the caller's d_groups and
// the grouped stage's status to the caller's d_status), then the fill.  Nothing waits (the first call after rq_index_set_groups
// builds the member table).
static int search_group_members_device(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int s, int metric, int32_t* d_groups, const MembersOut& out,
                                       hipStream_t st) {
    if (int r = flush_tails(idx, st)) return r;
    if (int r = ensure_group_table(idx)) return r;
    if (int r = mark_no_scan(idx, st)) return r;   // (enters the stream as every call does)
    {
        StreamCtx& cx = idx->ctx[st];
        const size_t elems = (size_t)B * (size_t)k;
        if (elems > cx.gm_elems) {   // (hipFree waits for the device: no earlier call still reads the old buffers)
            free_dev(cx.gm_scores, cx.gm_rows);
            cx.gm_elems = 0;
            if (hipMalloc((void**)&cx.gm_scores, elems * sizeof(float)) != hipSuccess || hipMalloc((void**)&cx.gm_rows, elems * sizeof(int64_t)) != hipSuccess) {
                (void)hipGetLastError();
                free_dev(cx.gm_scores, cx.gm_rows);
                return set_err(RQ_ENOMEM, "hipMalloc of %zu group winners failed", elems);
            }
            cx.gm_elems = elems;
        }
    }
    float* ws = idx->ctx[st].gm_scores; int64_t* wr = idx->ctx[st].gm_rows;   // (the search may add stream contexts: no reference is kept across it)
    if (int r = search_grouped_device(idx, f, d_q, B, k, metric, {ws, wr, d_groups, nullptr, out.status}, st)) return r;
    if (int r = flush_tails(idx, st)) return r;
    return group_fill(idx, f, d_q, B, k, s, metric, wr, d_groups, out, st);
}

// One overflowed slot of a repaired query, exactly: the rows in play of group g become a temporary filter (host copy of the ids and
// the caller's filter); the query is searched filtered for s rows into the slot's own outputs and repaired by the usual ladder.
static int group_members_exact_slot(rq_index* idx, const rq_filter* f, const float* d_q1, int32_t g, int s, int metric, float* d_scores, int64_t* d_rows, int* d_status1,
                                    int32_t* count, hipStream_t st) {
    const int64_t n = idx->n;
    std::vector<uint32_t> bits((size_t)((n + 31) / 32), 0u);
    for (int64_t r = 0; r < n && r < (int64_t)idx->h_groups.size(); ++r)
        if (idx->h_groups[(size_t)r] == g && (!f || ((f->bits[(size_t)(r >> 5)] >> (r & 31)) & 1u))) bits[(size_t)(r >> 5)] |= 1u << (r & 31);
    rq_filter* only = rq_filter_create(idx, bits.data(), n);
    if (!only) return RQ_EHIP;   // (the message is rq_filter_create's)
    *count = (int32_t)std::min<int64_t>(s, only->na);
    int rc = RQ_OK;
    if (only->na > 0) {
        rc = search_filtered_device(idx, only, d_q1, 1, s, metric, {d_scores, d_rows, nullptr, d_status1}, st);
        if (rc == RQ_OK) { const int fr = fixup_ladder(idx, only, d_q1, 1, s, metric, d_scores, d_rows, nullptr, d_status1, st); rc = fr < 0 ? fr : RQ_OK; }
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == RQ_OK) rc = set_err(RQ_EHIP, "the exact route of a group's members failed");
    rq_filter_destroy(only);
    return rc;
}

// Synchronises `st` and repairs the flagged queries: their winners are searched again and repaired (rq_group.hip: rung 1, then
// rungs 2 and 3 of grouped_fixup), the fill runs again over the proven winners, and every slot that still overflows takes the exact
// route.  Returns how many queries it repaired.
static int group_members_fixup(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int s, int metric, int32_t* d_groups, const MembersOut& out, hipStream_t st) {
    if (int r = flush_tails(idx, st)) return r;
    Stage fx(st);
    RepairList bad;
    if (int r = repair_flagged(fx, out.status, B, bad)) return r;
    if (bad.empty()) return 0;
    const int nb = (int)bad.size();
    const GroupMembersStaging z = group_members_staging(idx->dim, nb, k, s);
    const size_t bytes[9] = {z.q, z.win_scores, z.win_rows, z.groups, z.status, z.scores, z.rows, z.count, z.status};
    if (int r = fx.alloc(bytes, 9, "the repair of a group-members search")) return r;
    fx.launched();   // (kernels write these buffers from here on: a failed step waits for the stream before they are freed)
    float* fq = fx.at<float>(0);
    const GroupOut win{fx.at<float>(1), fx.at<int64_t>(2), fx.at<int32_t>(3), nullptr, fx.at<int>(4)};
    const MembersOut fo{fx.at<float>(5), fx.at<int64_t>(6), fx.at<int32_t>(7), fx.at<int>(8)};
    if (int r = repair_pack(fx, bad, {repair_col(d_q, fq, (size_t)idx->dim)})) return r;
    if (int r = search_grouped_device(idx, f, fq, nb, k, metric, win, st)) return r;
    if (int r = grouped_fixup(idx, f, fq, nb, k, metric, win, st); r < 0) return r;
    if (int r = flush_tails(idx, st)) return r;
    if (int r = fx.zero(fo.status, z.status)) return r;
    if (int r = group_fill(idx, f, fq, nb, k, s, metric, win.rows, win.groups, fo, st)) return r;
    const size_t slots = (size_t)nb * (size_t)k;
    std::vector<int32_t> h_count(slots), h_groups(slots);
    fx.down(h_count.data(), fo.count, z.count);
    fx.down(h_groups.data(), win.groups, z.groups);
    if (int r = fx.finish()) return r;
    fx.launched();   // (the exact route's searches read the packed queries and write the packed outputs)
    for (int i = 0; i < nb; ++i)   // "group_fill_repaired": the queries that hold a slot the kernel could not fill
        if (std::find(h_count.begin() + (size_t)i * (size_t)k, h_count.begin() + (size_t)(i + 1) * (size_t)k, -1) != h_count.begin() + (size_t)(i + 1) * (size_t)k) idx->group_fill_repaired++;
    for (size_t i = 0; i < slots; ++i) {
        if (h_count[i] != -1) continue;
        int32_t count = 0;
        if (int r = group_members_exact_slot(idx, f, fq + (i / (size_t)k) * (size_t)idx->dim, h_groups[i], s, metric, fo.scores + i * (size_t)s, fo.rows + i * (size_t)s,
                                             win.status + i / (size_t)k, &count, st)) return r;
        HIPCHK(hipMemcpy(fo.count + i, &count, sizeof(count), hipMemcpyHostToDevice));   // (blocking, from a local)
    }
    const size_t ks = (size_t)k * (size_t)s;
    if (int r = repair_unpack(fx, bad, {repair_col(out.scores, fo.scores, ks), repair_col(out.rows, fo.rows, ks), repair_col(d_groups, win.groups, (size_t)k),
                                        repair_col(out.count, fo.count, (size_t)k)})) return r;
    if (int r = repair_unpack(fx, bad, {}, out.status)) return r;   // (the status words after every copy)
    if (int r = fx.finish()) return r;
    return nb;
}

// ---- entry points -------------------------------------------------------------------------------
static int check_members_call(const rq_index* idx, const rq_filter* f, const void* q, int B, int k, int s, int metric, const void* a0, const void* a1, const void* a2,
                              const void* a3, const void* a4) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_group_members_args(idx, q, B, k, s, metric, a0, a1, a2, a3, a4)) return r;
    if (f)
        if (int r = check_filter(idx, f)) return r;
    return RQ_OK;
}

extern "C" int rq_group_fill_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, const int64_t* d_win_rows,
                                    const int32_t* d_win_groups, float* d_scores, int64_t* d_rows, int32_t* d_count, int* d_status, void* stream) {
    if (int r = check_members_call(idx, f, d_queries, B, k, s, metric, d_win_rows, d_win_groups, d_scores, d_rows, d_count)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    hipStream_t st = (hipStream_t)stream;
    // like a "pipeline" = 0 call: whatever the stream still defers is completed first (the prepared-query slots are the stream's)
    if (int r = flush_tails(idx, st)) return r;
    HIPCHK(hipMemsetAsync(d_status, 0, (size_t)B * sizeof(int), st));
    return group_fill(idx, f, d_queries, B, k, s, metric, d_win_rows, d_win_groups, {d_scores, d_rows, d_count, d_status}, st);
}

extern "C" int rq_search_group_members_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, float* d_scores,
                                              int64_t* d_rows, int32_t* d_groups, int32_t* d_count, int* d_status, void* stream) {
    if (int r = check_members_call(idx, f, d_queries, B, k, s, metric, d_scores, d_rows, d_groups, d_count, d_status)) return r;
    RQ_ON_DEVICE(idx);
    return search_group_members_device(idx, f, d_queries, B, k, s, metric, d_groups, {d_scores, d_rows, d_count, d_status}, (hipStream_t)stream);
}

extern "C" int rq_search_group_members_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int s, int metric, float* d_scores,
                                                    int64_t* d_rows, int32_t* d_groups, int32_t* d_count, int* d_status, void* stream) {
    if (int r = check_members_call(idx, f, d_queries, B, k, s, metric, d_scores, d_rows, d_groups, d_count, d_status)) return r;
    RQ_ON_DEVICE(idx);
    return group_members_fixup(idx, f, d_queries, B, k, s, metric, d_groups, {d_scores, d_rows, d_count, d_status}, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h), repair included.
extern "C" int rq_search_group_members(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int s, int metric, float* out_scores, int64_t* out_rows,
                                       int32_t* out_groups, int32_t* out_count) {
    if (int r = check_members_call(idx, f, queries, B, k, s, metric, out_scores, out_rows, out_groups, out_count, out_count)) return r;
    RQ_ON_DEVICE(idx);
    const GroupMembersStaging z = group_members_staging(idx->dim, B, k, s);
    const size_t bytes[6] = {z.q, z.scores, z.rows, z.groups, z.count, z.status};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 6, "a group-members search")) return r;
    float* d_q = st.at<float>(0);
    int32_t* d_groups = st.at<int32_t>(3);
    const MembersOut o{st.at<float>(1), st.at<int64_t>(2), st.at<int32_t>(4), st.at<int>(5)};
    if (int r = st.up(d_q, queries, z.q)) return r;
    if (int r = search_group_members_device(idx, f, d_q, B, k, s, metric, d_groups, o, st.s)) return r;
    if (int r = group_members_fixup(idx, f, d_q, B, k, s, metric, d_groups, o, st.s); r < 0) return r;
    st.down(out_scores, o.scores, z.scores);
    st.down(out_rows, o.rows, z.rows);
    st.down(out_groups, d_groups, z.groups);
    st.down(out_count, o.count, z.count);
    return st.finish();
}
