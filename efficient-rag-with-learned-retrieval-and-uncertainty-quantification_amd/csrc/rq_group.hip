// rq_group.hip -- grouped searches (include/rq.h rq_index_set_groups, rq_group_collapse_device, rq_search_grouped*): the best row
// of each of the k best groups -- "field collapsing" of a chunked corpus, one passage per article -- next to the rows.
//
// Every stored row carries an int32 group id (RQ_GROUP_NONE = a group of its own).  A grouped search is the exact search for m
// rows followed by a collapse: one workgroup per query sorts the m candidate keys (score, local row) in LDS, a candidate is its
// group's winner iff no better candidate carries the same id, and the k best winners leave in key order.  The list was the exact
// top m rows, so its d winners are the exact top d groups: with d >= k the answer is proven, otherwise the query is flagged and
// rq_search_grouped_fixup_device widens the list and finally excludes the groups already found with a temporary rq_filter -- no
// new scan kernel.  The collapse reads 4 bytes per candidate from the group array and never a stored row, so there is one kernel
// for both row layouts.  What a call fetches is decided by rq_group_plan.h.  Replaces the over-fetch / collapse-on-the-host loop
// around the collection.query of reference rag_uq/streaming_index.py:355-359.
#include "rq_group_plan.h"
#include "rq_repair.h"

// ---- kernel -------------------------------------------------------------------------------------
struct RqGroupArgs {
    const int64_t* cand_rows;     // [B][m] global rows, any order; -1 / outside the shard = absent
    const float* cand_scores;     // [B][m]; NaN = absent
    const int32_t* cand_groups;   // [B][m] or null: look the id up in `groups`
    const int32_t* groups;        // [n_rows] the index's group ids, null = every row RQ_GROUP_NONE
    const int* search_status;     // [B] or null: the certificate of the search that produced the candidates
    int64_t n_rows, row_offset;
    int m, k, sort_n;
    int complete;                 // the candidates are every row in play: fewer than k groups is then the whole answer
    float* out_scores; int64_t* out_rows; int32_t* out_groups; uint64_t* out_keys;   // [B][k]; keys may be null
    int* out_status;              // [B]
};

// One workgroup per query.  (a) keys and ids into LDS, absent candidates as key 0; (b) bitonic sort, keys descending -- present
// keys are distinct (they carry their row), so the order is the canonical one and nothing depends on the schedule; (c) position p is
// a winner iff it is present and ungrouped, or no position before it carries its id; (d) the winners' ranks by ballot and prefix
// over the waves, the first k are written; (e) padding and the status.
__global__ __launch_bounds__(RQ_GROUP_THREADS) void rq_group_collapse_kernel(RqGroupArgs a) {
    constexpr int NW = RQ_GROUP_THREADS / 64;
    __shared__ uint64_t key[RQ_MAX_K];
    __shared__ int32_t grp[RQ_MAX_K];
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x, m = a.m, k = a.k, P = a.sort_n;   // (m <= P <= RQ_MAX_K: the launcher)
    const int64_t* crow = a.cand_rows + (int64_t)q * m;
    const float* cscore = a.cand_scores + (int64_t)q * m;
    const int32_t* cgrp = a.cand_groups ? a.cand_groups + (int64_t)q * m : nullptr;

    for (int i = tid; i < P; i += RQ_GROUP_THREADS) {
        uint64_t kk = 0;
        int32_t g = RQ_GROUP_NONE;
        if (i < m) {
            const int64_t row = crow[i], loc = row - a.row_offset;
            const float s = cscore[i];
            if (row >= 0 && loc >= 0 && loc < a.n_rows && s == s) {   // an absent candidate's group is never looked up
                kk = rq_make_key(s, (uint32_t)loc);
                g = cgrp ? cgrp[i] : (a.groups ? a.groups[loc] : RQ_GROUP_NONE);
                if (g < 0) g = RQ_GROUP_NONE;
            }
        }
        key[i] = kk;
        grp[i] = g;
    }
    __syncthreads();

    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += RQ_GROUP_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const uint64_t ka = key[lo], kb = key[hi];
                const bool desc = (lo & size) == 0;
                if (desc ? ka < kb : ka > kb) {
                    const int32_t ga = grp[lo], gb = grp[hi];
                    key[lo] = kb; key[hi] = ka;
                    grp[lo] = gb; grp[hi] = ga;
                }
            }
            __syncthreads();
        }
    }

    float* out_s = a.out_scores + (int64_t)q * k;
    int64_t* out_r = a.out_rows + (int64_t)q * k;
    int32_t* out_g = a.out_groups + (int64_t)q * k;
    uint64_t* out_k = a.out_keys ? a.out_keys + (int64_t)q * k : nullptr;
    int distinct = 0;
    for (int p0 = 0; p0 < P; p0 += RQ_GROUP_THREADS) {   // (uniform over the workgroup)
        const int p = p0 + tid;
        bool win = false;
        uint64_t kk = 0;
        int32_t g = RQ_GROUP_NONE;
        if (p < P) {
            kk = key[p];
            g = grp[p];
            win = kk != 0;
            if (win && g >= 0)
                for (int j = 0; j < p; ++j)
                    if (grp[j] == g) { win = false; break; }   // (positions before p are present: absent keys sort last)
        }
        const unsigned long long bal = __ballot(win);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int slot = distinct + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            slot += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        if (win && slot < k) {
            const float s = rq_key_score(kk);
            const int64_t grow = a.row_offset + (int64_t)rq_key_index(kk);
            out_s[slot] = s;
            out_r[slot] = grow;
            out_g[slot] = g;
            if (out_k) out_k[slot] = rq_make_key(s, (uint32_t)grow);
        }
        distinct += total;
        __syncthreads();   // (wsum is written again by the next round)
    }
    for (int t = min(k, distinct) + tid; t < k; t += RQ_GROUP_THREADS) {
        out_s[t] = 0.f;
        out_r[t] = -1;
        out_g[t] = RQ_GROUP_NONE;
        if (out_k) out_k[t] = 0;
    }
    if (tid == 0) {
        const bool searched = !a.search_status || a.search_status[q] == 0;
        a.out_status[q] = (searched && (distinct >= k || a.complete)) ? 0 : 1;
    }
}

static hipError_t rq_group_collapse_launch(const RqGroupArgs& a, int B, hipStream_t stream) {
    if (B < 1 || B > 65535 || a.m < 1 || a.m > RQ_MAX_K || a.k < 1 || a.k > a.m || a.sort_n < a.m || a.sort_n > RQ_MAX_K || (a.sort_n & (a.sort_n - 1)) || a.n_rows < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_group_collapse_kernel, dim3(B), dim3(RQ_GROUP_THREADS), 0, stream, a);
    return hipGetLastError();
}

// ---- group storage --------------------------------------------------------------------------------
extern "C" int rq_index_set_groups(rq_index* idx, int64_t row_begin, int64_t n_rows, const int32_t* groups) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_group_range(idx, row_begin, n_rows, groups)) return r;
    if (int r = check_group_ids(groups, n_rows)) return r;
    if (n_rows == 0) return RQ_OK;
    RQ_ON_DEVICE(idx);
    // as an append: searches in flight on any stream may still read the ids
    if (int r = flush_all(idx)) return r;
    HIPCHK(hipDeviceSynchronize());
    drop_group_table(idx);   // the member table follows the ids: the next fill builds it again (rq_group_members.hip)
    if (!idx->d_groups) {
        int32_t* fresh = nullptr;
        if (hipMalloc((void**)&fresh, (size_t)idx->cap * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(RQ_ENOMEM, "hipMalloc of the group ids of %lld rows failed", (long long)idx->cap);
        }
        if (hipMemset(fresh, 0xff, (size_t)idx->cap * sizeof(int32_t)) != hipSuccess) {   // RQ_GROUP_NONE everywhere
            (void)hipFree(fresh);
            return set_err(RQ_EHIP, "clearing the group ids failed");
        }
        idx->d_groups = fresh;
        idx->h_groups.assign((size_t)idx->n, RQ_GROUP_NONE);
    }
    HIPCHK(hipMemcpy(idx->d_groups + row_begin, groups, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    std::copy(groups, groups + n_rows, idx->h_groups.begin() + row_begin);
    return RQ_OK;
}

extern "C" int rq_index_get_groups(const rq_index* idx, int64_t row_begin, int64_t n_rows, int32_t* out) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_group_range(idx, row_begin, n_rows, out)) return r;
    if (n_rows == 0) return RQ_OK;
    if (!idx->d_groups) {
        std::fill(out, out + n_rows, (int32_t)RQ_GROUP_NONE);
        return RQ_OK;
    }
    RQ_ON_DEVICE(idx);
    HIPCHK(hipMemcpy(out, idx->d_groups + row_begin, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));   // the copy the kernel reads
    return RQ_OK;
}

// ---- the collapse -----------------------------------------------------------------------------------
static int group_collapse(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_scores, const int32_t* d_cand_groups, const int* d_search_status,
                          int B, int m, int k, bool complete, const GroupOut& out, hipStream_t s) {
    const GroupGeometry g = group_geometry(B, m);
    RqGroupArgs a;
    a.cand_rows = d_cand_rows; a.cand_scores = d_cand_scores; a.cand_groups = d_cand_groups; a.groups = idx->d_groups;
    a.search_status = d_search_status; a.n_rows = idx->n; a.row_offset = idx->row_offset;
    a.m = m; a.k = k; a.sort_n = g.sort_n; a.complete = complete ? 1 : 0;
    a.out_scores = out.scores; a.out_rows = out.rows; a.out_groups = out.groups; a.out_keys = out.keys; a.out_status = out.status;
    HIPCHK(rq_group_collapse_launch(a, (int)g.grid, s));
    idx->group_calls++;
    return RQ_OK;
}

extern "C" int rq_group_collapse_device(rq_index* idx, const int64_t* d_cand_rows, const float* d_cand_scores, const int32_t* d_cand_groups, int B, int m, int k,
                                        float* d_scores, int64_t* d_rows, int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_group_collapse_args(idx, d_cand_rows, d_cand_scores, B, m, k, d_scores, d_rows, d_groups, d_status)) return r;
    RQ_ON_DEVICE(idx);
    return group_collapse(idx, d_cand_rows, d_cand_scores, d_cand_groups, nullptr, B, m, k, false, {d_scores, d_rows, d_groups, d_keys, d_status}, (hipStream_t)stream);
}

// ---- searches -----------------------------------------------------------------------------------------
static int64_t rows_in_play(const rq_index* idx, const rq_filter* f) { return f ? f->na : idx->n; }

// The exact-search half of a rung: the top m rows of B queries (over the filter's rows when f is given), enqueued, not repaired.
static int group_fetch_rows(rq_index* idx, const rq_filter* f, const float* d_q, int B, int m, int metric, const SearchOut& cand, hipStream_t s) {
    if (f) return search_filtered_device(idx, f, d_q, B, m, metric, cand, s);
    idx->t.searches++;
    idx->t.queries += B;
    return run_pipeline(idx, d_q, B, m, metric, nb_default(idx, m), cand, s, CALL_ALLOW8 | CALL_FETCH);
}

static int group_fill_empty(int B, int k, const GroupOut& out, hipStream_t s) {
    HIPCHK(hipMemsetAsync(out.scores, 0, (size_t)B * k * sizeof(float), s));
    HIPCHK(hipMemsetAsync(out.rows, 0xff, (size_t)B * k * sizeof(int64_t), s));
    HIPCHK(hipMemsetAsync(out.groups, 0xff, (size_t)B * k * sizeof(int32_t), s));
    if (out.keys) HIPCHK(hipMemsetAsync(out.keys, 0, (size_t)B * k * sizeof(uint64_t), s));
    HIPCHK(hipMemsetAsync(out.status, 0, (size_t)B * sizeof(int), s));
    return RQ_OK;
}

// Rung 1: the exact search for m1 = "group_fetch" x k rows into the stream's candidate buffers, then the collapse.  Nothing waits.
int search_grouped_device(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int metric, const GroupOut& out, hipStream_t s) {
    // like a "pipeline" = 0 call: whatever the stream still defers (fused tail, scanned-ahead pair, hint) is completed first
    if (int r = flush_tails(idx, s)) return r;
    const int64_t play = rows_in_play(idx, f);
    if (play == 0) {   // no row to return: padding, proven
        idx->t.searches++;
        idx->t.queries += B;
        if (int r = mark_no_scan(idx, s)) return r;
        return group_fill_empty(B, k, out, s);
    }
    const int m1 = group_fetch(k, idx->group_fetch, idx->group_fetch_cap, play);
    if (int r = mark_no_scan(idx, s)) return r;   // (enters the stream as every call does: beyond the remembered streams the idle ones are dropped first)
    StreamCtx& cx = idx->ctx[s];
    const size_t elems = (size_t)B * (size_t)m1;
    if (elems > cx.grp_elems || B > cx.grp_bcap) {   // (hipFree waits for the device: no earlier call still reads the old buffers)
        const size_t ne = std::max(elems, cx.grp_elems);
        const int nb = std::max(B, cx.grp_bcap);
        free_dev(cx.grp_scores, cx.grp_rows, cx.grp_status);
        cx.grp_elems = 0; cx.grp_bcap = 0;
        if (hipMalloc((void**)&cx.grp_scores, ne * sizeof(float)) != hipSuccess || hipMalloc((void**)&cx.grp_rows, ne * sizeof(int64_t)) != hipSuccess ||
            hipMalloc((void**)&cx.grp_status, (size_t)nb * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            free_dev(cx.grp_scores, cx.grp_rows, cx.grp_status);
            return set_err(RQ_ENOMEM, "hipMalloc of %zu candidate rows for a grouped search failed", ne);
        }
        cx.grp_elems = ne; cx.grp_bcap = nb;
    }
    float* cs = cx.grp_scores; int64_t* cr = cx.grp_rows; int* cst = cx.grp_status;   // (run_pipeline may add stream contexts: no reference is kept across it)
    if (int r = group_fetch_rows(idx, f, d_q, B, m1, metric, {cs, cr, nullptr, cst}, s)) return r;
    return group_collapse(idx, cr, cs, nullptr, cst, B, m1, k, (int64_t)m1 >= play, out, s);
}

// One query's answer on the host while the exclusion loop extends it.
struct GroupAnswer {
    std::vector<float> scores; std::vector<int64_t> rows; std::vector<int32_t> groups;
    int found = 0;
};

// Rung 3 for ONE query that holds `ans.found` < k winners -- the exact top groups, because its list was the exact top rows: the
// rows in play that belong to none of them become a temporary filter; that query is searched filtered, collapsed, and the new
// winners are appended; until k winners are found or no row is left.  Every round adds at least one group.
static int group_exclusion_loop(rq_index* idx, const rq_filter* f, const float* d_q1, int k, int metric, GroupAnswer& ans, int64_t* rounds, hipStream_t s) {
    const int64_t n = idx->n;
    const size_t words = (size_t)((n + 31) / 32);
    std::vector<uint32_t> bits(words, 0xffffffffu);
    if (f) bits = f->bits;
    else if (n & 31) bits[words - 1] = (1u << (n & 31)) - 1u;
    const bool grouped = !idx->h_groups.empty();
    int done_from = 0;   // winners already taken out of the bitmap
    while (ans.found < k) {
        std::vector<int32_t> gone;
        for (int i = done_from; i < ans.found; ++i) {
            const int64_t loc = ans.rows[(size_t)i] - idx->row_offset;
            bits[(size_t)(loc >> 5)] &= ~(1u << (loc & 31));
            if (ans.groups[(size_t)i] >= 0) gone.push_back(ans.groups[(size_t)i]);
        }
        done_from = ans.found;
        if (grouped && !gone.empty()) {
            std::sort(gone.begin(), gone.end());
            for (int64_t r = 0; r < n; ++r) {
                const int32_t g = idx->h_groups[(size_t)r];
                if (g >= 0 && std::binary_search(gone.begin(), gone.end(), g)) bits[(size_t)(r >> 5)] &= ~(1u << (r & 31));
            }
        }
        rq_filter* rest = rq_filter_create(idx, bits.data(), n);
        if (!rest) return RQ_EHIP;   // (the message is rq_filter_create's)
        const int64_t left = rest->na;
        if (left == 0) { rq_filter_destroy(rest); break; }
        const int want = k - ans.found;
        const int m = group_max_fetch(want, idx->group_fetch_cap, left);
        const GroupStaging sz = group_staging(idx->dim, 1, m, want);
        const size_t bytes[7] = {sz.cand_scores, sz.cand_rows, sz.cand_status, sz.out_scores, sz.out_rows, sz.out_groups, sz.status};
        int rc = RQ_OK;
        {
            Stage st(s);
            rc = st.alloc(bytes, 7, "the exclusion round of a grouped search");
            st.launched();   // (kernels write these buffers from here on: whichever step fails, the stream is waited for before they are freed)
            float* cs = st.at<float>(0); int64_t* cr = st.at<int64_t>(1); int* cst = st.at<int>(2);
            const GroupOut o{st.at<float>(3), st.at<int64_t>(4), st.at<int32_t>(5), nullptr, st.at<int>(6)};
            if (rc == RQ_OK) rc = search_filtered_device(idx, rest, d_q1, 1, m, metric, {cs, cr, nullptr, cst}, s);
            if (rc == RQ_OK) { const int fr = fixup_ladder(idx, rest, d_q1, 1, m, metric, cs, cr, nullptr, cst, s); rc = fr < 0 ? fr : RQ_OK; }
            if (rc == RQ_OK) rc = group_collapse(idx, cr, cs, nullptr, nullptr, 1, m, want, (int64_t)m >= left, o, s);
            if (rc == RQ_OK) {
                st.down(ans.scores.data() + ans.found, o.scores, sz.out_scores);
                st.down(ans.rows.data() + ans.found, o.rows, sz.out_rows);
                st.down(ans.groups.data() + ans.found, o.groups, sz.out_groups);
                rc = st.finish();
            }
        }
        rq_filter_destroy(rest);
        if (rc != RQ_OK) return rc;
        ++*rounds;
        int added = 0;
        while (ans.found + added < k && ans.rows[(size_t)(ans.found + added)] >= 0) ++added;
        if (added == 0) return set_err(RQ_EHIP, "internal: an exclusion round over %lld rows found no group", (long long)left);
        ans.found += added;
    }
    return RQ_OK;
}

// Synchronises `s`, repairs the flagged queries: rung 2 = the widest list a rung may ask for, repaired by the usual ladder and
// collapsed; rung 3 = the exclusion loop for the queries still short of k groups.  Returns how many queries it repaired.
int grouped_fixup(rq_index* idx, const rq_filter* f, const float* d_q, int B, int k, int metric, const GroupOut& out, hipStream_t s) {
    if (int r = flush_tails(idx, s)) return r;
    Stage fx(s);
    RepairList bad;
    if (int r = repair_flagged(fx, out.status, B, bad)) return r;
    if (bad.empty()) return 0;
    const int nb = (int)bad.size();
    idx->group_repaired += nb;
    idx->group_rounds_last = 0;
    const int64_t play = rows_in_play(idx, f);
    const int m2 = group_max_fetch(k, idx->group_fetch_cap, play);
    const GroupStaging sz = group_staging(idx->dim, nb, m2, k);
    const size_t bytes[9] = {sz.q, sz.cand_scores, sz.cand_rows, sz.cand_status, sz.out_scores, sz.out_rows, sz.out_groups, sz.out_keys, sz.status};
    if (int r = fx.alloc(bytes, 9, "the repair of a grouped search")) return r;
    fx.launched();   // (kernels write these buffers from here on: a failed step waits for the stream before they are freed)
    float* fq = fx.at<float>(0); float* cs = fx.at<float>(1); int64_t* cr = fx.at<int64_t>(2); int* cst = fx.at<int>(3);
    const GroupOut fo{fx.at<float>(4), fx.at<int64_t>(5), fx.at<int32_t>(6), fx.at<uint64_t>(7), fx.at<int>(8)};
    if (int r = repair_pack(fx, bad, {repair_col(d_q, fq, (size_t)idx->dim)})) return r;
    // rung 2
    if (int r = group_fetch_rows(idx, f, fq, nb, m2, metric, {cs, cr, nullptr, cst}, s)) return r;
    if (int r = fixup_ladder(idx, f, fq, nb, m2, metric, cs, cr, nullptr, cst, s); r < 0) return r;
    if (int r = group_collapse(idx, cr, cs, nullptr, nullptr, nb, m2, k, (int64_t)m2 >= play, fo, s)) return r;
    const size_t kk = (size_t)k;
    std::vector<float> h_scores((size_t)nb * kk);
    std::vector<int64_t> h_rows((size_t)nb * kk);
    std::vector<int32_t> h_groups((size_t)nb * kk);
    std::vector<int> h_status((size_t)nb);
    fx.down(h_scores.data(), fo.scores, sz.out_scores);
    fx.down(h_rows.data(), fo.rows, sz.out_rows);
    fx.down(h_groups.data(), fo.groups, sz.out_groups);
    fx.down(h_status.data(), fo.status, sz.status);
    if (int r = fx.finish()) return r;
    // rung 3, query by query; the extended answers go back into the repair's buffers
    fx.launched();   // (its searches read the packed queries)
    for (int i = 0; i < nb; ++i) {
        if (h_status[(size_t)i] == 0) continue;
        GroupAnswer ans;
        ans.scores.assign(h_scores.begin() + (size_t)i * kk, h_scores.begin() + (size_t)(i + 1) * kk);
        ans.rows.assign(h_rows.begin() + (size_t)i * kk, h_rows.begin() + (size_t)(i + 1) * kk);
        ans.groups.assign(h_groups.begin() + (size_t)i * kk, h_groups.begin() + (size_t)(i + 1) * kk);
        while (ans.found < k && ans.rows[(size_t)ans.found] >= 0) ++ans.found;
        if (int r = group_exclusion_loop(idx, f, fq + (size_t)i * idx->dim, k, metric, ans, &idx->group_rounds_last, s)) return r;
        std::vector<uint64_t> keys(kk, 0);
        for (int j = 0; j < k; ++j) {
            if (j >= ans.found) { ans.scores[(size_t)j] = 0.f; ans.rows[(size_t)j] = -1; ans.groups[(size_t)j] = RQ_GROUP_NONE; }
            else keys[(size_t)j] = rq_make_key(ans.scores[(size_t)j], (uint32_t)ans.rows[(size_t)j]);
        }
        // (blocking copies from pageable memory: the vectors die with this iteration)
        HIPCHK(hipMemcpy(fo.scores + (size_t)i * kk, ans.scores.data(), kk * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(fo.rows + (size_t)i * kk, ans.rows.data(), kk * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(fo.groups + (size_t)i * kk, ans.groups.data(), kk * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(fo.keys + (size_t)i * kk, keys.data(), kk * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    if (int r = repair_unpack(fx, bad, {repair_col(out.scores, fo.scores, kk), repair_col(out.rows, fo.rows, kk), repair_col(out.groups, fo.groups, kk),
                                        repair_col(out.keys, fo.keys, kk)})) return r;
    if (int r = repair_unpack(fx, bad, {}, out.status)) return r;   // (the status words after every copy)
    if (int r = fx.finish()) return r;
    return nb;
}

// ---- entry points -------------------------------------------------------------------------------
static int check_grouped_call(const rq_index* idx, const rq_filter* f, const void* q, int B, int k, int metric, const void* scores, const void* rows, const void* groups) {
    if (!idx && rq_device_count() <= 0) return err_no_device();
    if (int r = check_group_search_args(idx, q, B, k, metric, scores, rows, groups)) return r;
    if (f)
        if (int r = check_filter(idx, f)) return r;
    return RQ_OK;
}

extern "C" int rq_search_grouped_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                                        int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_grouped_call(idx, f, d_queries, B, k, metric, d_scores, d_rows, d_groups)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return search_grouped_device(idx, f, d_queries, B, k, metric, {d_scores, d_rows, d_groups, d_keys, d_status}, (hipStream_t)stream);
}

extern "C" int rq_search_grouped_fixup_device(rq_index* idx, const rq_filter* f, const float* d_queries, int B, int k, int metric, float* d_scores, int64_t* d_rows,
                                              int32_t* d_groups, uint64_t* d_keys, int* d_status, void* stream) {
    if (int r = check_grouped_call(idx, f, d_queries, B, k, metric, d_scores, d_rows, d_groups)) return r;
    if (!d_status) return set_err(RQ_EINVAL, "d_status is required");
    RQ_ON_DEVICE(idx);
    return grouped_fixup(idx, f, d_queries, B, k, metric, {d_scores, d_rows, d_groups, d_keys, d_status}, (hipStream_t)stream);
}

// The blocking host-buffer form, on the index's own stream (rq_stage.h), repair included.
extern "C" int rq_search_grouped(rq_index* idx, const rq_filter* f, const float* queries, int B, int k, int metric, float* out_scores, int64_t* out_rows,
                                 int32_t* out_groups) {
    if (int r = check_grouped_call(idx, f, queries, B, k, metric, out_scores, out_rows, out_groups)) return r;
    RQ_ON_DEVICE(idx);
    const GroupStaging sz = group_staging(idx->dim, B, k, k);
    const size_t bytes[5] = {sz.q, sz.out_scores, sz.out_rows, sz.out_groups, sz.status};
    Stage st(idx->own_stream);
    if (int r = st.alloc(bytes, 5, "a grouped search")) return r;
    float* d_q = st.at<float>(0);
    const GroupOut o{st.at<float>(1), st.at<int64_t>(2), st.at<int32_t>(3), nullptr, st.at<int>(4)};
    if (int r = st.up(d_q, queries, sz.q)) return r;
    if (int r = search_grouped_device(idx, f, d_q, B, k, metric, o, st.s)) return r;
    if (int r = grouped_fixup(idx, f, d_q, B, k, metric, o, st.s); r < 0) return r;
    st.down(out_scores, o.scores, sz.out_scores);
    st.down(out_rows, o.rows, sz.out_rows);
    st.down(out_groups, o.groups, sz.out_groups);
    return st.finish();
}
