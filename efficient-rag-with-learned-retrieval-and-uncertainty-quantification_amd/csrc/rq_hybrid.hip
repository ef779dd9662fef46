// rq_hybrid.hip -- hybrid fusion on the device (include/rq.h rq_hybrid_*, rq_sparse_score_rows*): the arithmetic of
// HybridRetriever._fuse_batch_rows for a whole batch, with the same bits.
//
// rq_hybrid_kernel<P, FUSE>, one workgroup per query, P = the candidate count padded to a power of two, everything in LDS:
//   1. every candidate position i gets its key (a sparse row, or dense_key[dense row]; absent: all ones), b, d and a flag byte;
//   2. the (key, position) pairs -- one uint64 each, unique because the position is part of it -- are sorted (bitonic); a key that
//      follows itself, first from the sparse pool and then from the dense pool, is a document in both: the sparse position takes
//      the dense position's d, the dense position loses its valid flag.  A sparse position is the first of at most one such pair
//      and a dense position the second of at most one, so no two threads touch the same slot, whatever the pools hold;
//   FUSE = false (rq_hybrid_missing_device) writes the miss lists from the flags and leaves.
//   3. extra scores replace the 0.0 of the missing side; max_b, max_d and the number of valid candidates are reduced with a NaN flag
//      each (wave shuffles, then one slot per wave); a maximum that is 0, NaN or infinite becomes 1.0;
//   4. h = (b / max_b + d / max_d) / 2 in float64 (IEEE division, no contraction: -ffp-contract=off); the composite key
//      (inverted sortable bits of h with NaN as -inf and -0.0 as +0.0, then the position) is unique, so the second bitonic sort
//      gives one order whatever the thread order: h descending, ties by ascending position, invalid slots last;
//   5. the first min(valid, top_k) are written, h recomputed from the same operands, then the padding.
// Every index into LDS is a position below P and every global read is at (query, position): a repeated row cannot leave the arrays.
//
// rq_sparse_score_rows_kernel, one thread per (query, row) pair: for the query's tokens IN QUERY ORDER a binary search over the
// token's strictly ascending rows, and the posting's contribution is added where the row is found -- 0.0 + c_1 + c_2 + ... in float64,
// the additions that a full score vector makes for that row (csrc/rq_sparse.hip), hence its bits.
#include "rq_hybrid_plan.h"
#include "rq_sparse_handle.h"
#include "rq_stage.h"

#define HY_ABSENT 0xFFFFFFFFu
#define HY_VALID 1u     // present and known, and not the dense twin of a sparse position
#define HY_BOTH 2u      // a sparse position whose document is in the dense pool too

struct HybridArgs {
    const int32_t* dense_key;    // [n_dense]
    const uint8_t* known;        // [n_keys]
    const int32_t* dense_row;    // [n_keys]
    int64_t nb, n_dense;
    const int32_t* sp_rows;      // [B][K1]
    const double* sp_scores;
    const int64_t* de_rows;      // [B][K2]
    const float* de_scores;
    int K1, K2;
    const int64_t* miss_dense;   // fuse: inputs, may be NULL
    const float* extra_dense;
    const int32_t* miss_sparse;
    const double* extra_sparse;
    int64_t* out_miss_dense;     // missing: outputs
    int32_t* out_miss_sparse;
    int top_k;
    int32_t* keys;               // [B][top_k]
    double* b;
    double* d;
    double* h;
    int32_t* pos;                // may be NULL
    int32_t* count;              // [B]
    const int32_t* key_group;    // [n_keys], grouped fusion only (rq_hybrid_kernel<P, true, true>): -1 = a group of its own
};

// the key of a VALID position (its row was range-checked when the flags were set)
__device__ __forceinline__ int32_t hybrid_key_of(const HybridArgs& a, int q, int p) {
    if (p < a.K1) return a.sp_rows[(size_t)q * (size_t)a.K1 + (size_t)p];
    return a.dense_key[a.de_rows[(size_t)q * (size_t)a.K2 + (size_t)(p - a.K1)]];
}

template <int P, bool FUSE, bool GROUPED = false>
__global__ __launch_bounds__(P / 2 < 64 ? 64 : (P / 2 > RQ_HYBRID_MAX_THREADS ? RQ_HYBRID_MAX_THREADS : P / 2)) void rq_hybrid_kernel(HybridArgs a) {
    constexpr int T = P / 2 < 64 ? 64 : (P / 2 > RQ_HYBRID_MAX_THREADS ? RQ_HYBRID_MAX_THREADS : P / 2);
    constexpr int W = T / 64;
    __shared__ uint64_t s_a[P];
    __shared__ uint8_t s_f[P];
    __shared__ double s_b[FUSE ? P : 1], s_d[FUSE ? P : 1];
    __shared__ int32_t s_pos[FUSE ? P : 1];
    __shared__ double s_max[2 * W];
    __shared__ int s_cnt[3 * W];
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x;
    const int K1 = a.K1, N = a.K1 + a.K2;
    // ---- 1. keys, scores, flags ----
    for (int i = tid; i < P; i += T) {
        uint32_t key = HY_ABSENT;
        double b = 0.0, d = 0.0;
        if (i < K1) {
            const size_t o = (size_t)q * (size_t)K1 + (size_t)i;
            const int32_t r = a.sp_rows[o];
            if (r >= 0 && (int64_t)r < a.nb) {
                key = (uint32_t)r;
                if (FUSE) b = a.sp_scores[o];
            }
        } else if (i < N) {
            const size_t o = (size_t)q * (size_t)a.K2 + (size_t)(i - K1);
            const int64_t r = a.de_rows[o];
            if (r >= 0 && r < a.n_dense) {
                key = (uint32_t)a.dense_key[r];
                if (FUSE) d = (double)a.de_scores[o];
            }
        }
        s_a[i] = ((uint64_t)key << 32) | (uint32_t)i;
        s_f[i] = (key != HY_ABSENT && a.known[key]) ? HY_VALID : 0u;
        if (FUSE) { s_b[i] = b; s_d[i] = d; }
    }
    __syncthreads();
    // ---- 2. documents in both pools: ascending bitonic sort of the (key, position) pairs ----
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t x = s_a[i], y = s_a[j];
                if ((x > y) == ((i & size) == 0)) { s_a[i] = y; s_a[j] = x; }
            }
            __syncthreads();
        }
    for (int t = tid; t < P - 1; t += T) {
        const uint64_t x = s_a[t], y = s_a[t + 1];
        const uint32_t kx = (uint32_t)(x >> 32);
        const int px = (int)(uint32_t)x, py = (int)(uint32_t)y;
        if (kx == HY_ABSENT || kx != (uint32_t)(y >> 32) || px >= K1 || py < K1) continue;
        if (FUSE) s_d[px] = s_d[py];
        s_f[px] |= HY_BOTH;
        s_f[py] = 0u;
    }
    __syncthreads();
    if (!FUSE) {
        for (int i = tid; i < N; i += T) {
            const unsigned f = s_f[i];
            if (i < K1) {
                a.out_miss_dense[(size_t)q * (size_t)K1 + (size_t)i] = (f & HY_VALID) && !(f & HY_BOTH) ? (int64_t)a.dense_row[hybrid_key_of(a, q, i)] : (int64_t)-1;
            } else {
                const int32_t key = (f & HY_VALID) ? hybrid_key_of(a, q, i) : -1;
                a.out_miss_sparse[(size_t)q * (size_t)a.K2 + (size_t)(i - K1)] = (int64_t)key < a.nb ? key : -1;
            }
        }
        return;
    }
    // ---- 3. extra scores, the maxima with their NaN flags, the number of valid candidates ----
    double mb = -INFINITY, md = -INFINITY;
    int nan_b = 0, nan_d = 0, cnt = 0;
    for (int i = tid; i < N; i += T) {
        const unsigned f = s_f[i];
        if (!(f & HY_VALID)) continue;
        if (i < K1) {
            const size_t o = (size_t)q * (size_t)K1 + (size_t)i;
            if (!(f & HY_BOTH) && a.extra_dense && a.miss_dense[o] >= 0) s_d[i] = (double)a.extra_dense[o];
        } else {
            const size_t o = (size_t)q * (size_t)a.K2 + (size_t)(i - K1);
            if (a.extra_sparse && a.miss_sparse[o] >= 0) s_b[i] = a.extra_sparse[o];
        }
        const double vb = s_b[i], vd = s_d[i];
        if (vb != vb) nan_b = 1;
        else if (vb > mb) mb = vb;
        if (vd != vd) nan_d = 1;
        else if (vd > md) md = vd;
        ++cnt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(mb, o), od = __shfl_xor(md, o);
        mb = ob > mb ? ob : mb;
        md = od > md ? od : md;
        nan_b |= __shfl_xor(nan_b, o);
        nan_d |= __shfl_xor(nan_d, o);
        cnt += __shfl_xor(cnt, o);
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        s_max[2 * w] = mb; s_max[2 * w + 1] = md;
        s_cnt[3 * w] = nan_b; s_cnt[3 * w + 1] = nan_d; s_cnt[3 * w + 2] = cnt;
    }
    __syncthreads();
    mb = s_max[0]; md = s_max[1]; nan_b = s_cnt[0]; nan_d = s_cnt[1]; cnt = s_cnt[2];
    for (int w = 1; w < W; ++w) {
        mb = s_max[2 * w] > mb ? s_max[2 * w] : mb;
        md = s_max[2 * w + 1] > md ? s_max[2 * w + 1] : md;
        nan_b |= s_cnt[3 * w]; nan_d |= s_cnt[3 * w + 1]; cnt += s_cnt[3 * w + 2];
    }
    const double max_b = (nan_b || mb == 0.0 || isinf(mb)) ? 1.0 : mb;   // (no valid candidate: -inf)
    const double max_d = (nan_d || md == 0.0 || isinf(md)) ? 1.0 : md;
    // ---- 4. the hybrid score and the sort on (inverted sortable bits of h, position) ----
    for (int i = tid; i < P; i += T) {
        uint64_t inv = ~0ull;                                            // invalid and padding: behind every candidate
        if (i < N && (s_f[i] & HY_VALID)) {
            double h = (s_b[i] / max_b + s_d[i] / max_d) / 2.0;
            if (h != h) h = -INFINITY;
            if (h == 0.0) h = 0.0;                                       // -0.0 ranks as +0.0
            const uint64_t u = (uint64_t)__double_as_longlong(h);
            inv = (u >> 63) ? u : ~(u | 0x8000000000000000ull);          // ~(sortable bits): ascending = h descending
        }
        s_a[i] = inv;
        s_pos[i] = i;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t x = s_a[i], y = s_a[j];
                const int32_t px = s_pos[i], py = s_pos[j];
                const bool gt = x > y || (x == y && px > py);
                if (gt == ((i & size) == 0)) { s_a[i] = y; s_a[j] = x; s_pos[i] = py; s_pos[j] = px; }
            }
            __syncthreads();
        }
    const size_t base = (size_t)q * (size_t)a.top_k;
    if constexpr (GROUPED) {
        // ---- 5g. one ordered pass over the full ranking: the first candidate of every group stays (include/rq.h rq_hybrid_fuse_grouped*) ----
        // Ranks 0 .. cnt-1 hold the valid candidates in order.  The (group, rank) pairs -- unique: the rank is part of them -- are
        // sorted; a pair whose predecessor has another group is its group's first rank.  Group -1 is a group of its own and never
        // enters the sort.  s_a (the sort keys are spent) holds the pairs, s_f (the flags are spent) the keep flag of every RANK.
        for (int r = tid; r < P; r += T) {
            uint64_t pair = ~0ull;
            uint8_t keep = 0;
            if (r < cnt) {
                const int32_t g = a.key_group[hybrid_key_of(a, q, s_pos[r])];
                if (g < 0) keep = 1;
                else pair = ((uint64_t)(uint32_t)g << 32) | (uint32_t)r;
            }
            s_a[r] = pair;
            s_f[r] = keep;
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < P / 2; t += T) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const uint64_t x = s_a[i], y = s_a[j];
                    if ((x > y) == ((i & size) == 0)) { s_a[i] = y; s_a[j] = x; }
                }
                __syncthreads();
            }
        for (int t = tid; t < P; t += T) {
            const uint64_t x = s_a[t];
            if (x == ~0ull) continue;
            if (t == 0 || (uint32_t)(s_a[t - 1] >> 32) != (uint32_t)(x >> 32)) s_f[(uint32_t)x] = 1;   // (one writer per rank)
        }
        __syncthreads();
        // thread t owns ranks C x t .. C x t + C - 1: the exclusive prefix sum of the keep flags is the output position
        constexpr int C = P / T;
        int own = 0;
        for (int j = 0; j < C; ++j) own += s_f[C * tid + j];
        int inc = own;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if ((tid & 63) >= o) inc += v;
        }
        if ((tid & 63) == 63) s_cnt[tid >> 6] = inc;   // (the reduction's slots were read before the sort's barriers)
        __syncthreads();
        int at = inc - own, kept = 0;
        for (int w = 0; w < W; ++w) {
            if (w < (tid >> 6)) at += s_cnt[w];
            kept += s_cnt[w];
        }
        const int want = kept < a.top_k ? kept : a.top_k;
        for (int j = 0; j < C; ++j) {
            const int r = C * tid + j;
            if (!s_f[r]) continue;
            if (at < a.top_k) {
                const int p = s_pos[r];
                const double b = s_b[p], d = s_d[p];
                a.keys[base + at] = hybrid_key_of(a, q, p);
                a.b[base + at] = b;
                a.d[base + at] = d;
                a.h[base + at] = (b / max_b + d / max_d) / 2.0;
                if (a.pos) a.pos[base + at] = p;
            }
            ++at;
        }
        for (int i = want + tid; i < a.top_k; i += T) {
            a.keys[base + i] = -1;
            a.b[base + i] = 0.0;
            a.d[base + i] = 0.0;
            a.h[base + i] = 0.0;
            if (a.pos) a.pos[base + i] = -1;
        }
        if (tid == 0) a.count[q] = want;
        return;
    }
    // ---- 5. output ----
    const int want = cnt < a.top_k ? cnt : a.top_k;
    for (int i = tid; i < a.top_k; i += T) {
        int32_t key = -1, p = -1;
        double b = 0.0, d = 0.0, h = 0.0;
        if (i < want) {
            p = s_pos[i];
            key = hybrid_key_of(a, q, p);
            b = s_b[p];
            d = s_d[p];
            h = (b / max_b + d / max_d) / 2.0;
        }
        a.keys[base + i] = key;
        a.b[base + i] = b;
        a.d[base + i] = d;
        a.h[base + i] = h;
        if (a.pos) a.pos[base + i] = p;
    }
    if (tid == 0) a.count[q] = want;
}

__global__ __launch_bounds__(RQ_HYBRID_SCORE_THREADS) void rq_sparse_score_rows_kernel(const int64_t* indptr, const int32_t* rows, const double* contrib, int64_t n_tokens,
                                                                                     int64_t n_docs, const int64_t* q_indptr, const int32_t* q_tokens, int64_t n_q_tokens,
                                                                                     int B, int m, const int32_t* want, double* out) {
    const int64_t idx = (int64_t)blockIdx.x * RQ_HYBRID_SCORE_THREADS + threadIdx.x;
    if (idx >= (int64_t)B * m) return;
    const int q = (int)(idx / m);
    const int64_t r = want[idx];
    double s = 0.0;
    if (r >= 0 && r < n_docs) {
        // the arrays may be the caller's device memory, which no host check has seen: stay inside [0, n_q_tokens)
        int64_t t0 = q_indptr[q], t1 = q_indptr[q + 1];
        t0 = t0 < 0 ? 0 : (t0 > n_q_tokens ? n_q_tokens : t0);
        t1 = t1 < t0 ? t0 : (t1 > n_q_tokens ? n_q_tokens : t1);
        for (int64_t t = t0; t < t1; ++t) {
            const int64_t tok = q_tokens[t];
            if (tok < 0 || tok >= n_tokens) continue;   // an id outside the index is an empty posting list
            int64_t lo = indptr[tok];
            const int64_t e = indptr[tok + 1];
            int64_t hi = e;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if ((int64_t)rows[mid] < r) lo = mid + 1;
                else hi = mid;
            }
            if (lo < e && (int64_t)rows[lo] == r) s += contrib[lo];
        }
    }
    out[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct rq_hybrid {
    int device = 0;
    int64_t nb = 0, n_dense = 0, n_keys = 0;
    int32_t* d_dense_key = nullptr;
    uint8_t* d_known = nullptr;
    int32_t* d_dense_row = nullptr;
    hipStream_t own = nullptr;
    int64_t calls = 0, fuse_calls = 0, missing_calls = 0;
    int32_t* d_key_group = nullptr;   // [n_keys], rq_hybrid_set_groups (null: no table)
    int64_t grouped_calls = 0;        // rq_hybrid_fuse_grouped* (counted in calls and fuse_calls too)
};

static void hybrid_free(rq_hybrid* h) {
    if (h->own) (void)hipStreamDestroy(h->own);
    free_dev(h->d_dense_key, h->d_known, h->d_dense_row, h->d_key_group);
    delete h;
}

extern "C" rq_hybrid* rq_hybrid_create(int device_id, int64_t nb, int64_t n_dense, const int64_t* dense_key, const uint8_t* known, int64_t n_keys) {
    std::vector<int32_t> dense_row;
    if (hybrid_check_create(nb, n_dense, dense_key, known, n_keys, dense_row) != RQ_OK) return nullptr;
    const int ndev = rq_device_count();
    if (ndev <= 0) { err_no_device(); return nullptr; }
    if (device_id < 0 || device_id >= ndev) { set_err(RQ_EINVAL, "device %d outside 0..%d", device_id, ndev - 1); return nullptr; }
    DeviceGuard dg_(device_id);
    hipDeviceProp_t prop;
    if (!dg_.ok || hipGetDeviceProperties(&prop, device_id) != hipSuccess) { set_err(RQ_EHIP, "cannot open device %d", device_id); return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(RQ_ENODEVICE, "device %d is %s; this library holds gfx950 code only", device_id, prop.gcnArchName);
        return nullptr;
    }
    std::vector<int32_t> key32((size_t)n_dense);
    for (int64_t j = 0; j < n_dense; ++j) key32[(size_t)j] = (int32_t)dense_key[j];
    rq_hybrid* h = new rq_hybrid();
    h->device = device_id;
    h->nb = nb;
    h->n_dense = n_dense;
    h->n_keys = n_keys;
    const size_t nd = (size_t)n_dense, nk = (size_t)n_keys;   // (empty tables: the kernels still get valid pointers)
    if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess || hipMalloc((void**)&h->d_dense_key, (nd ? nd : 1) * 4) != hipSuccess ||
        hipMalloc((void**)&h->d_known, nk ? nk : 1) != hipSuccess || hipMalloc((void**)&h->d_dense_row, (nk ? nk : 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        set_err(RQ_ENOMEM, "no room for %zu dense rows and %zu keys on device %d", nd, nk, device_id);
        hybrid_free(h);
        return nullptr;
    }
    if ((nd && hipMemcpy(h->d_dense_key, key32.data(), nd * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        (nk && (hipMemcpy(h->d_known, known, nk, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_dense_row, dense_row.data(), nk * 4, hipMemcpyHostToDevice) != hipSuccess))) {
        set_err(RQ_EHIP, "upload of the key space to device %d failed", device_id);
        hybrid_free(h);
        return nullptr;
    }
    return h;
}

extern "C" void rq_hybrid_destroy(rq_hybrid* h) {
    if (!h) return;
    DeviceGuard dg_(h->device);
    (void)hipDeviceSynchronize();
    hybrid_free(h);
}

extern "C" double rq_hybrid_get_option(const rq_hybrid* h, const char* name) {
    if (!h || !name) { set_err(RQ_EINVAL, "null argument"); return -1.0; }
    if (!strcmp(name, "calls")) return (double)h->calls;
    if (!strcmp(name, "fuse_calls")) return (double)h->fuse_calls;
    if (!strcmp(name, "missing_calls")) return (double)h->missing_calls;
    if (!strcmp(name, "grouped_calls")) return (double)h->grouped_calls;
    if (!strcmp(name, "grouped")) return h->d_key_group ? 1.0 : 0.0;
    if (!strcmp(name, "nb")) return (double)h->nb;
    if (!strcmp(name, "n_dense")) return (double)h->n_dense;
    if (!strcmp(name, "n_keys")) return (double)h->n_keys;
    set_err(RQ_EINVAL, "unknown hybrid option '%s'", name);
    return -1.0;
}

template <bool FUSE>
static void hybrid_launch(const HybridArgs& a, int B, hipStream_t s) {
    const int pad = hybrid_pad(a.K1 + a.K2);
    const dim3 grid((unsigned)B), block((unsigned)hybrid_threads(pad));
    switch (pad) {
    case 64: hipLaunchKernelGGL((rq_hybrid_kernel<64, FUSE>), grid, block, 0, s, a); break;
    case 128: hipLaunchKernelGGL((rq_hybrid_kernel<128, FUSE>), grid, block, 0, s, a); break;
    case 256: hipLaunchKernelGGL((rq_hybrid_kernel<256, FUSE>), grid, block, 0, s, a); break;
    case 512: hipLaunchKernelGGL((rq_hybrid_kernel<512, FUSE>), grid, block, 0, s, a); break;
    case 1024: hipLaunchKernelGGL((rq_hybrid_kernel<1024, FUSE>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((rq_hybrid_kernel<RQ_HYBRID_MAX_CAND, FUSE>), grid, block, 0, s, a); break;
    }
}

static void hybrid_launch_grouped(const HybridArgs& a, int B, hipStream_t s) {
    const int pad = hybrid_pad(a.K1 + a.K2);
    const dim3 grid((unsigned)B), block((unsigned)hybrid_threads(pad));
    switch (pad) {
    case 64: hipLaunchKernelGGL((rq_hybrid_kernel<64, true, true>), grid, block, 0, s, a); break;
    case 128: hipLaunchKernelGGL((rq_hybrid_kernel<128, true, true>), grid, block, 0, s, a); break;
    case 256: hipLaunchKernelGGL((rq_hybrid_kernel<256, true, true>), grid, block, 0, s, a); break;
    case 512: hipLaunchKernelGGL((rq_hybrid_kernel<512, true, true>), grid, block, 0, s, a); break;
    case 1024: hipLaunchKernelGGL((rq_hybrid_kernel<1024, true, true>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((rq_hybrid_kernel<RQ_HYBRID_MAX_CAND, true, true>), grid, block, 0, s, a); break;
    }
}

static HybridArgs hybrid_args(const rq_hybrid* h, const int32_t* sp_rows, const double* sp_scores, const int64_t* de_rows, const float* de_scores, int K1, int K2) {
    HybridArgs a = {};
    a.dense_key = h->d_dense_key; a.known = h->d_known; a.dense_row = h->d_dense_row;
    a.nb = h->nb; a.n_dense = h->n_dense;
    a.sp_rows = sp_rows; a.sp_scores = sp_scores; a.de_rows = de_rows; a.de_scores = de_scores;
    a.K1 = K1; a.K2 = K2;
    return a;
}

extern "C" int rq_hybrid_missing_device(rq_hybrid* h, const int32_t* d_sp_rows, const int64_t* d_de_rows, int B, int K1, int K2, int64_t* d_miss_dense,
                                        int32_t* d_miss_sparse, void* stream) {
    if (int rc = hybrid_check_missing(h, d_sp_rows, d_de_rows, B, K1, K2, d_miss_dense, d_miss_sparse)) return rc;
    RQ_ON_DEVICE(h);
    HybridArgs a = hybrid_args(h, d_sp_rows, nullptr, d_de_rows, nullptr, K1, K2);
    a.out_miss_dense = d_miss_dense;
    a.out_miss_sparse = d_miss_sparse;
    hybrid_launch<false>(a, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    h->calls++;
    h->missing_calls++;
    return RQ_OK;
}

extern "C" int rq_hybrid_fuse_device(rq_hybrid* h, const int32_t* d_sp_rows, const double* d_sp_scores, const int64_t* d_de_rows, const float* d_de_scores, int B,
                                     int K1, int K2, const int64_t* d_miss_dense, const float* d_extra_dense, const int32_t* d_miss_sparse,
                                     const double* d_extra_sparse, int top_k, int32_t* d_keys, double* d_b, double* d_d, double* d_h, int32_t* d_pos,
                                     int32_t* d_count, void* stream) {
    if (int rc = hybrid_check_fuse(h, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, B, K1, K2, d_miss_dense, d_extra_dense, d_miss_sparse, d_extra_sparse, top_k,
                                   d_keys, d_b, d_d, d_h, d_count))
        return rc;
    RQ_ON_DEVICE(h);
    HybridArgs a = hybrid_args(h, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, K1, K2);
    a.miss_dense = d_miss_dense; a.extra_dense = K1 > 0 ? d_extra_dense : nullptr;
    a.miss_sparse = d_miss_sparse; a.extra_sparse = K2 > 0 ? d_extra_sparse : nullptr;
    a.top_k = top_k;
    a.keys = d_keys; a.b = d_b; a.d = d_d; a.h = d_h; a.pos = d_pos; a.count = d_count;
    hybrid_launch<true>(a, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    h->calls++;
    h->fuse_calls++;
    return RQ_OK;
}

extern "C" int rq_hybrid_set_groups(rq_hybrid* h, const int32_t* key_group, int64_t n_keys) {
    if (int rc = hybrid_check_groups(h, key_group, n_keys, h ? h->n_keys : 0)) return rc;
    RQ_ON_DEVICE(h);
    int32_t* fresh = nullptr;
    if (hipMalloc((void**)&fresh, (size_t)(n_keys ? n_keys : 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(RQ_ENOMEM, "no room for a group table of %lld keys on device %d", (long long)n_keys, h->device);
    }
    if (n_keys && hipMemcpy(fresh, key_group, (size_t)n_keys * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(fresh);
        return set_err(RQ_EHIP, "upload of the group table to device %d failed", h->device);
    }
    if (h->d_key_group) {        // an earlier call may still read the table it replaces
        HIPCHK(hipDeviceSynchronize());
        free_dev(h->d_key_group);
    }
    h->d_key_group = fresh;
    return RQ_OK;
}

extern "C" int rq_hybrid_fuse_grouped_device(rq_hybrid* h, const int32_t* d_sp_rows, const double* d_sp_scores, const int64_t* d_de_rows, const float* d_de_scores,
                                             int B, int K1, int K2, int top_k, int32_t* d_keys, double* d_b, double* d_d, double* d_h, int32_t* d_pos,
                                             int32_t* d_count, void* stream) {
    if (int rc = hybrid_check_fuse(h, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, B, K1, K2, nullptr, nullptr, nullptr, nullptr, top_k, d_keys, d_b, d_d, d_h, d_count))
        return rc;
    if (!h->d_key_group) return set_err(RQ_EINVAL, "no group table: call rq_hybrid_set_groups first");
    RQ_ON_DEVICE(h);
    HybridArgs a = hybrid_args(h, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, K1, K2);
    a.top_k = top_k;
    a.keys = d_keys; a.b = d_b; a.d = d_d; a.h = d_h; a.pos = d_pos; a.count = d_count;
    a.key_group = h->d_key_group;
    hybrid_launch_grouped(a, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    h->calls++;
    h->fuse_calls++;
    h->grouped_calls++;
    return RQ_OK;
}

extern "C" int rq_hybrid_missing(rq_hybrid* h, const int32_t* sp_rows, const int64_t* de_rows, int B, int K1, int K2, int64_t* miss_dense, int32_t* miss_sparse) {
    if (int rc = hybrid_check_missing(h, sp_rows, de_rows, B, K1, K2, miss_dense, miss_sparse)) return rc;
    RQ_ON_DEVICE(h);
    const size_t n1 = (size_t)B * (size_t)K1, n2 = (size_t)B * (size_t)K2;
    const size_t bytes[4] = {(n1 ? n1 : 1) * 4, (n2 ? n2 : 1) * 8, (n1 ? n1 : 1) * 8, (n2 ? n2 : 1) * 4};
    Stage st(h->own);
    if (st.alloc(bytes, 4, "rq_hybrid_missing") != RQ_OK) return st.code();
    if (n1) st.up(st.at<void>(0), sp_rows, n1 * 4);
    if (n2) st.up(st.at<void>(1), de_rows, n2 * 8);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_hybrid_missing_device(h, st.at<int32_t>(0), st.at<int64_t>(1), B, K1, K2, st.at<int64_t>(2), st.at<int32_t>(3), (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    if (n1) st.down(miss_dense, st.at<void>(2), n1 * 8);
    if (n2) st.down(miss_sparse, st.at<void>(3), n2 * 4);
    return st.finish();
}

extern "C" int rq_hybrid_fuse(rq_hybrid* h, const int32_t* sp_rows, const double* sp_scores, const int64_t* de_rows, const float* de_scores, int B, int K1, int K2,
                              const int64_t* miss_dense, const float* extra_dense, const int32_t* miss_sparse, const double* extra_sparse, int top_k,
                              int32_t* out_keys, double* out_b, double* out_d, double* out_h, int32_t* out_pos, int32_t* out_count) {
    if (int rc = hybrid_check_fuse(h, sp_rows, sp_scores, de_rows, de_scores, B, K1, K2, miss_dense, extra_dense, miss_sparse, extra_sparse, top_k, out_keys, out_b,
                                   out_d, out_h, out_count))
        return rc;
    RQ_ON_DEVICE(h);
    const size_t n1 = (size_t)B * (size_t)K1, n2 = (size_t)B * (size_t)K2, no = (size_t)B * (size_t)top_k;
    // one block for the inputs (8-byte arrays first: every offset stays aligned), one for the outputs
    const bool md = n1 && miss_dense, ed = n1 && extra_dense, ms = n2 && miss_sparse, es = n2 && extra_sparse;
    const size_t in_sizes[8] = {n1 * 8, n2 * 8, md ? n1 * 8 : 0, es ? n2 * 8 : 0, n1 * 4, n2 * 4, ed ? n1 * 4 : 0, ms ? n2 * 4 : 0};
    const void* in_src[8] = {sp_scores, de_rows, miss_dense, extra_sparse, sp_rows, de_scores, extra_dense, miss_sparse};
    size_t in_off[8], in_total = 0;
    for (int i = 0; i < 8; ++i) { in_off[i] = in_total; in_total += (in_sizes[i] + 7) / 8 * 8; }
    const size_t bytes[2] = {in_total ? in_total : 8, no * 32 + (size_t)B * 4};   // b, d, h | keys, pos | count
    Stage st(h->own);
    if (st.alloc(bytes, 2, "rq_hybrid_fuse") != RQ_OK) return st.code();
    char* in = st.at<char>(0);
    char* out = st.at<char>(1);
    for (int i = 0; i < 8; ++i)
        if (in_sizes[i]) st.up(in + in_off[i], in_src[i], in_sizes[i]);
    if (st.code() != RQ_OK) return st.code();
    auto at = [&](int i) -> const void* { return in_sizes[i] ? (const void*)(in + in_off[i]) : nullptr; };
    double* ob = (double*)out;
    int32_t* ok = (int32_t*)(out + no * 24);
    int32_t* oc = (int32_t*)(out + no * 32);
    const int rc = rq_hybrid_fuse_device(h, (const int32_t*)at(4), (const double*)at(0), (const int64_t*)at(1), (const float*)at(5), B, K1, K2, (const int64_t*)at(2),
                                         (const float*)at(6), (const int32_t*)at(7), (const double*)at(3), top_k, ok, ob, ob + no, ob + 2 * no, ok + no, oc, (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_b, ob, no * 8);
    st.down(out_d, ob + no, no * 8);
    st.down(out_h, ob + 2 * no, no * 8);
    st.down(out_keys, ok, no * 4);
    if (out_pos) st.down(out_pos, ok + no, no * 4);
    st.down(out_count, oc, (size_t)B * 4);
    return st.finish();
}

extern "C" int rq_hybrid_fuse_grouped(rq_hybrid* h, const int32_t* sp_rows, const double* sp_scores, const int64_t* de_rows, const float* de_scores, int B, int K1,
                                      int K2, int top_k, int32_t* out_keys, double* out_b, double* out_d, double* out_h, int32_t* out_pos, int32_t* out_count) {
    if (int rc = hybrid_check_fuse(h, sp_rows, sp_scores, de_rows, de_scores, B, K1, K2, nullptr, nullptr, nullptr, nullptr, top_k, out_keys, out_b, out_d, out_h,
                                   out_count))
        return rc;
    if (!h->d_key_group) return set_err(RQ_EINVAL, "no group table: call rq_hybrid_set_groups first");
    RQ_ON_DEVICE(h);
    const size_t n1 = (size_t)B * (size_t)K1, n2 = (size_t)B * (size_t)K2, no = (size_t)B * (size_t)top_k;
    // sp_scores, de_rows (8-byte elements first: every offset stays aligned), sp_rows, de_scores | b, d, h, keys, pos, count
    const size_t bytes[5] = {(n1 ? n1 : 1) * 8, (n2 ? n2 : 1) * 8, (n1 ? n1 : 1) * 4, (n2 ? n2 : 1) * 4, no * 32 + (size_t)B * 4};
    Stage st(h->own);
    if (st.alloc(bytes, 5, "rq_hybrid_fuse_grouped") != RQ_OK) return st.code();
    if (n1) { st.up(st.at<void>(0), sp_scores, n1 * 8); st.up(st.at<void>(2), sp_rows, n1 * 4); }
    if (n2) { st.up(st.at<void>(1), de_rows, n2 * 8); st.up(st.at<void>(3), de_scores, n2 * 4); }
    if (st.code() != RQ_OK) return st.code();
    char* out = st.at<char>(4);
    double* ob = (double*)out;
    int32_t* ok = (int32_t*)(out + no * 24);
    int32_t* oc = (int32_t*)(out + no * 32);
    const int rc = rq_hybrid_fuse_grouped_device(h, n1 ? st.at<int32_t>(2) : nullptr, n1 ? st.at<double>(0) : nullptr, n2 ? st.at<int64_t>(1) : nullptr,
                                                 n2 ? st.at<float>(3) : nullptr, B, K1, K2, top_k, ok, ob, ob + no, ob + 2 * no, ok + no, oc, (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_b, ob, no * 8);
    st.down(out_d, ob + no, no * 8);
    st.down(out_h, ob + 2 * no, no * 8);
    st.down(out_keys, ok, no * 4);
    if (out_pos) st.down(out_pos, ok + no, no * 4);
    st.down(out_count, oc, (size_t)B * 4);
    return st.finish();
}

// ---- rq_sparse_score_rows* ---------------------------------------------------------------------------------------------------------
extern "C" int rq_sparse_score_rows_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, const int32_t* d_rows,
                                           int m, double* d_scores, void* stream) {
    if (int rc = hybrid_check_score_rows(h, d_q_indptr, B, d_rows, m, d_scores)) return rc;
    if (n_q_tokens < 0 || (n_q_tokens > 0 && !d_q_tokens)) return set_err(RQ_EINVAL, "n_q_tokens %lld negative, or tokens without an array", (long long)n_q_tokens);
    RQ_ON_DEVICE(h);
    hipLaunchKernelGGL(rq_sparse_score_rows_kernel, dim3(hybrid_score_blocks(B, m)), dim3(RQ_HYBRID_SCORE_THREADS), 0, (hipStream_t)stream, h->d_indptr, h->d_rows,
                       h->d_contrib, h->n_tokens, h->n_docs, d_q_indptr, d_q_tokens, n_q_tokens, B, m, d_rows, d_scores);
    HIPCHK(hipGetLastError());
    h->score_calls++;
    return RQ_OK;
}

extern "C" int rq_sparse_score_rows(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, const int32_t* rows, int m, double* out_scores) {
    if (int rc = hybrid_check_score_rows(h, q_indptr, B, rows, m, out_scores)) return rc;
    if (int rc = sparse_check_queries(q_indptr, q_tokens, B, h->n_tokens)) return rc;
    RQ_ON_DEVICE(h);
    const int64_t nq = q_indptr[B];
    const size_t n = (size_t)B * (size_t)m;
    const size_t bytes[4] = {(size_t)(B + 1) * 8, (size_t)(nq ? nq : 1) * 4, n * 4, n * 8};
    Stage st(h->own);
    if (st.alloc(bytes, 4, "rq_sparse_score_rows") != RQ_OK) return st.code();
    st.up(st.at<void>(0), q_indptr, bytes[0]);
    if (nq) st.up(st.at<void>(1), q_tokens, (size_t)nq * 4);
    st.up(st.at<void>(2), rows, bytes[2]);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_sparse_score_rows_device(h, st.at<int64_t>(0), st.at<int32_t>(1), B, nq, st.at<int32_t>(2), m, st.at<double>(3), (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_scores, st.at<void>(3), bytes[3]);
    return st.finish();
}
