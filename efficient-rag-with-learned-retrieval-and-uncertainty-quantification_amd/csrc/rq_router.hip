// rq_router.hip -- the router gate and the rerank of the fused pool on the device (include/rq.h rq_router_*): the
// arithmetic of tests/router_gate_oracle.py for a whole batch, where rq_hybrid_fuse_device left the pool.
//
// rq_router_kernel<P2, RANK>, one workgroup per query, P2 = the column length P padded to a power of two, everything in LDS:
//   0. the weight table (5 doubles per hidden unit) is copied to LDS once; in the gate every lane reads the same address: a broadcast;
//   1. b and d of every position are loaded; slots at and beyond P hold +0.0;
//   2. RQ_ROUTER_NORM_QUERY: the tree sum S of both columns at once (a[i] += a[i + n/2] over n = the next power of two of P, a
//      barrier per level: the additions and their order are those of the definition whatever the thread count), the means, then the
//      same tree over the squared deviations, the scales.  RQ_ROUTER_NORM_STATS: the four statistics arrive by value;
//   3. router_gate, ONE device function, gives w of every position below P: the j loop of the definition, then exp;
//   RANK = false (rq_router_gate_device) writes w and leaves.
//   4. h = w*d + (1.0 - w)*b; the composite key (inverted sortable bits of h with NaN as -inf and -0.0 as +0.0, then the position) is
//      unique, so the bitonic sort gives one order whatever the thread order: h descending, ties by ascending position; a position
//      at or beyond count, or with a negative key, sorts behind every candidate (all ones: no candidate's key, a NaN being -inf);
//   5. the first min(candidates, top_r) are written, h recomputed from the same operands, then the padding; the slot that ends the
//      candidates writes the count.
// Every index into LDS is a position below P2 and every global access is at (query, position below P or top_r).
// LDS at P2 = 1 024, RANK: b, d 16 KiB; the two tree arrays, reused as sort keys and weights, 16 KiB; positions 4 KiB; the weight
// table 10 KiB: 46 KiB and a few scalars, about 47 KiB, under the 64 KiB of a static allocation (router_lds_bytes).
#include "rq_router_plan.h"
#include "rq_stage.h"

struct RouterArgs {
    const double* table;         // [hidden][RQ_ROUTER_ROW], or w1[0..2] for one layer
    int hidden, layers;
    double b1;
    int P, tree, mode;
    double mean_b, std_b, mean_d, std_d;   // RQ_ROUTER_NORM_STATS
    const int32_t* keys;         // [B][P]   (rank form)
    const double* b;
    const double* d;
    const int32_t* count;        // [B]      (rank form)
    double* w;                   // [B][P]   (gate form)
    int top_r;
    int32_t* out_keys;           // [B][top_r]
    double* out_b;
    double* out_d;
    double* out_w;
    double* out_h;
    int32_t* out_pos;
    int32_t* out_count;          // [B]
};

// The gate of the definition for one position: `t` is the weight table in LDS.  Both kernels call it, so both report the same bits.
__device__ __forceinline__ double router_gate(const double* t, int hidden, int layers, double b1, double nb, double nd) {
    const double df = nd - nb;
    double z;
    if (layers == 1) {
        z = ((t[0] * nb + t[1] * nd) + t[2] * df) + b1;
    } else {
        z = 0.0;
        for (int j = 0; j < hidden; ++j) {
            const double* row = t + j * RQ_ROUTER_ROW;
            const double a = ((row[0] * nb + row[1] * nd) + row[2] * df) + row[3];
            const double r = a > 0.0 ? a : 0.0;
            z = z + row[4] * r;
        }
        z = z + b1;
    }
    return 1.0 / (1.0 + exp(-z));
}

template <int P2, bool RANK>
__global__ __launch_bounds__(P2 / 2 < 64 ? 64 : (P2 / 2 > RQ_ROUTER_MAX_THREADS ? RQ_ROUTER_MAX_THREADS : P2 / 2)) void rq_router_kernel(RouterArgs a) {
    constexpr int T = P2 / 2 < 64 ? 64 : (P2 / 2 > RQ_ROUTER_MAX_THREADS ? RQ_ROUTER_MAX_THREADS : P2 / 2);
    __shared__ double s_t[RQ_ROUTER_MAX_HIDDEN * RQ_ROUTER_ROW];
    __shared__ double s_b[P2], s_d[P2];
    __shared__ double s_x[P2], s_y[P2];          // the two tree sums; afterwards s_y holds w, and s_x's bytes the sort keys
    __shared__ int32_t s_pos[RANK ? P2 : 1];
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x;
    const int P = a.P;
    const size_t base = (size_t)q * (size_t)P;
    // ---- 0. / 1. the weight table and the columns ----
    const int n_table = a.layers == 1 ? 3 : a.hidden * RQ_ROUTER_ROW;
    for (int i = tid; i < n_table; i += T) s_t[i] = a.table[i];
    for (int i = tid; i < P2; i += T) {
        const double b = i < P ? a.b[base + i] : 0.0, d = i < P ? a.d[base + i] : 0.0;
        s_b[i] = b; s_d[i] = d;
        s_x[i] = b; s_y[i] = d;
    }
    __syncthreads();
    // ---- 2. normalisation ----
    double mean_b = a.mean_b, mean_d = a.mean_d, scale_b = a.std_b + 1e-6, scale_d = a.std_d + 1e-6;
    if (a.mode == RQ_ROUTER_NORM_QUERY) {
        for (int half = a.tree >> 1; half > 0; half >>= 1) {
            for (int i = tid; i < half; i += T) { s_x[i] = s_x[i] + s_x[i + half]; s_y[i] = s_y[i] + s_y[i + half]; }
            __syncthreads();
        }
        mean_b = s_x[0] / (double)P;
        mean_d = s_y[0] / (double)P;
        __syncthreads();
        for (int i = tid; i < P2; i += T) {
            const double eb = s_b[i] - mean_b, ed = s_d[i] - mean_d;
            s_x[i] = i < P ? eb * eb : 0.0;
            s_y[i] = i < P ? ed * ed : 0.0;
        }
        __syncthreads();
        for (int half = a.tree >> 1; half > 0; half >>= 1) {
            for (int i = tid; i < half; i += T) { s_x[i] = s_x[i] + s_x[i + half]; s_y[i] = s_y[i] + s_y[i + half]; }
            __syncthreads();
        }
        scale_b = sqrt(s_x[0] / (double)(P - 1)) + 1e-6;
        scale_d = sqrt(s_y[0] / (double)(P - 1)) + 1e-6;
        __syncthreads();
    }
    // ---- 3. the gate ----
    for (int i = tid; i < P; i += T) {
        const double w = router_gate(s_t, a.hidden, a.layers, a.b1, (s_b[i] - mean_b) / scale_b, (s_d[i] - mean_d) / scale_d);
        if (RANK) s_y[i] = w;
        else a.w[base + i] = w;
    }
    if (!RANK) return;
    // ---- 4. the hybrid score and the sort on (inverted sortable bits of h, position) ----
    uint64_t* s_a = reinterpret_cast<uint64_t*>(s_x);
    int cnt = a.count[q];
    cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
    for (int i = tid; i < P2; i += T) {
        uint64_t inv = ~0ull;                                            // no candidate and padding: behind every candidate
        if (i < cnt && a.keys[base + i] >= 0) {
            const double w = s_y[i];
            double h = w * s_d[i] + (1.0 - w) * s_b[i];
            if (h != h) h = -INFINITY;
            if (h == 0.0) h = 0.0;                                       // -0.0 ranks as +0.0
            const uint64_t u = (uint64_t)__double_as_longlong(h);
            inv = (u >> 63) ? u : ~(u | 0x8000000000000000ull);          // ~(sortable bits): ascending = h descending
        }
        s_a[i] = inv;
        s_pos[i] = i;
    }
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P2 / 2; t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t x = s_a[i], y = s_a[j];
                const int32_t px = s_pos[i], py = s_pos[j];
                const bool gt = x > y || (x == y && px > py);
                if (gt == ((i & size) == 0)) { s_a[i] = y; s_a[j] = x; s_pos[i] = py; s_pos[j] = px; }
            }
            __syncthreads();
        }
    // ---- 5. output: the candidates are a prefix of the sorted slots ----
    const size_t obase = (size_t)q * (size_t)a.top_r;
    for (int i = tid; i < a.top_r; i += T) {       // top_r <= P <= P2
        const bool live = s_a[i] != ~0ull;
        int32_t key = -1, p = -1;
        double b = 0.0, d = 0.0, w = 0.0, h = 0.0;
        if (live) {
            p = s_pos[i];
            key = a.keys[base + p];
            b = s_b[p];
            d = s_d[p];
            w = s_y[p];
            h = w * d + (1.0 - w) * b;
            if (i + 1 == a.top_r || s_a[i + 1] == ~0ull) a.out_count[q] = i + 1;
        } else if (i == 0) {
            a.out_count[q] = 0;
        }
        a.out_keys[obase + i] = key;
        a.out_b[obase + i] = b;
        a.out_d[obase + i] = d;
        a.out_w[obase + i] = w;
        a.out_h[obase + i] = h;
        a.out_pos[obase + i] = p;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct rq_router {
    int device = 0;
    int hidden = 0, layers = 0;
    double b1 = 0.0;
    double* d_table = nullptr;
    hipStream_t own = nullptr;
    int64_t calls = 0, gate_calls = 0, rerank_calls = 0;
};

static void router_free(rq_router* r) {
    if (r->own) (void)hipStreamDestroy(r->own);
    free_dev(r->d_table);
    delete r;
}

extern "C" rq_router* rq_router_create(int device_id, int num_layers, int hidden, int use_batch_norm, const float* w0, const float* b0, const float* w1, float b1) {
    std::vector<double> table;
    if (router_check_create(num_layers, hidden, use_batch_norm, w0, b0, w1, table) != RQ_OK) return nullptr;
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
    rq_router* r = new rq_router();
    r->device = device_id;
    r->layers = num_layers;
    r->hidden = num_layers == 1 ? 0 : hidden;
    r->b1 = (double)b1;
    const size_t bytes = table.size() * 8;
    if (hipStreamCreateWithFlags(&r->own, hipStreamNonBlocking) != hipSuccess || hipMalloc((void**)&r->d_table, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_err(RQ_ENOMEM, "no room for %zu bytes of router weights on device %d", bytes, device_id);
        router_free(r);
        return nullptr;
    }
    if (hipMemcpy(r->d_table, table.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_err(RQ_EHIP, "upload of the router weights to device %d failed", device_id);
        router_free(r);
        return nullptr;
    }
    return r;
}

extern "C" void rq_router_destroy(rq_router* r) {
    if (!r) return;
    DeviceGuard dg_(r->device);
    (void)hipDeviceSynchronize();
    router_free(r);
}

extern "C" double rq_router_get_option(const rq_router* r, const char* name) {
    if (!r || !name) { set_err(RQ_EINVAL, "null argument"); return -1.0; }
    if (!strcmp(name, "calls")) return (double)r->calls;
    if (!strcmp(name, "gate_calls")) return (double)r->gate_calls;
    if (!strcmp(name, "rerank_calls")) return (double)r->rerank_calls;
    if (!strcmp(name, "hidden")) return (double)r->hidden;
    if (!strcmp(name, "layers")) return (double)r->layers;
    set_err(RQ_EINVAL, "unknown router option '%s'", name);
    return -1.0;
}

template <bool RANK>
static void router_launch(const RouterArgs& a, int B, hipStream_t s) {
    const int pad = router_pad(a.P);
    const dim3 grid((unsigned)B), block((unsigned)router_threads(pad));
    switch (pad) {
    case 64: hipLaunchKernelGGL((rq_router_kernel<64, RANK>), grid, block, 0, s, a); break;
    case 128: hipLaunchKernelGGL((rq_router_kernel<128, RANK>), grid, block, 0, s, a); break;
    case 256: hipLaunchKernelGGL((rq_router_kernel<256, RANK>), grid, block, 0, s, a); break;
    case 512: hipLaunchKernelGGL((rq_router_kernel<512, RANK>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((rq_router_kernel<1024, RANK>), grid, block, 0, s, a); break;
    }
}

static RouterArgs router_args(const rq_router* r, const double* b, const double* d, int P, int mode, const double* stats) {
    RouterArgs a = {};
    a.table = r->d_table; a.hidden = r->hidden; a.layers = r->layers; a.b1 = r->b1;
    a.P = P; a.tree = router_tree(P); a.mode = mode;
    if (mode == RQ_ROUTER_NORM_STATS) { a.mean_b = stats[0]; a.std_b = stats[1]; a.mean_d = stats[2]; a.std_d = stats[3]; }
    a.b = b; a.d = d;
    return a;
}

extern "C" int rq_router_gate_device(rq_router* r, const double* d_b, const double* d_d, int B, int P, int mode, const double* stats, double* d_w, void* stream) {
    if (int rc = router_check_gate(r, d_b, d_d, B, P, mode, stats, d_w)) return rc;
    RQ_ON_DEVICE(r);
    RouterArgs a = router_args(r, d_b, d_d, P, mode, stats);
    a.w = d_w;
    router_launch<false>(a, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    r->calls++;
    r->gate_calls++;
    return RQ_OK;
}

extern "C" int rq_router_rerank_device(rq_router* r, const int32_t* d_keys, const double* d_b, const double* d_d, const int32_t* d_count, int B, int P, int mode,
                                       const double* stats, int top_r, int32_t* d_out_keys, double* d_out_b, double* d_out_d, double* d_out_w, double* d_out_h,
                                       int32_t* d_out_pos, int32_t* d_out_count, void* stream) {
    if (int rc = router_check_rerank(r, d_keys, d_b, d_d, d_count, B, P, mode, stats, top_r, d_out_keys, d_out_b, d_out_d, d_out_w, d_out_h, d_out_pos, d_out_count))
        return rc;
    RQ_ON_DEVICE(r);
    RouterArgs a = router_args(r, d_b, d_d, P, mode, stats);
    a.keys = d_keys; a.count = d_count; a.top_r = top_r;
    a.out_keys = d_out_keys; a.out_b = d_out_b; a.out_d = d_out_d; a.out_w = d_out_w; a.out_h = d_out_h; a.out_pos = d_out_pos; a.out_count = d_out_count;
    router_launch<true>(a, B, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    r->calls++;
    r->rerank_calls++;
    return RQ_OK;
}

extern "C" int rq_router_gate(rq_router* r, const double* b, const double* d, int B, int P, int mode, const double* stats, double* out_w) {
    if (int rc = router_check_gate(r, b, d, B, P, mode, stats, out_w)) return rc;
    RQ_ON_DEVICE(r);
    const size_t n = (size_t)B * (size_t)P;
    const size_t bytes[3] = {n * 8, n * 8, n * 8};
    Stage st(r->own);
    if (st.alloc(bytes, 3, "rq_router_gate") != RQ_OK) return st.code();
    st.up(st.at<void>(0), b, n * 8);
    st.up(st.at<void>(1), d, n * 8);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_router_gate_device(r, st.at<double>(0), st.at<double>(1), B, P, mode, stats, st.at<double>(2), (void*)r->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_w, st.at<void>(2), n * 8);
    return st.finish();
}

extern "C" int rq_router_rerank(rq_router* r, const int32_t* keys, const double* b, const double* d, const int32_t* count, int B, int P, int mode, const double* stats,
                                int top_r, int32_t* out_keys, double* out_b, double* out_d, double* out_w, double* out_h, int32_t* out_pos, int32_t* out_count) {
    if (int rc = router_check_rerank(r, keys, b, d, count, B, P, mode, stats, top_r, out_keys, out_b, out_d, out_w, out_h, out_pos, out_count)) return rc;
    RQ_ON_DEVICE(r);
    const size_t n = (size_t)B * (size_t)P, no = (size_t)B * (size_t)top_r;
    // one block for the inputs (b, d | keys | count), one for the outputs (b, d, w, h | keys, pos | count): 8-byte arrays first
    const size_t bytes[2] = {n * 20 + (size_t)B * 4, no * 40 + (size_t)B * 4};
    Stage st(r->own);
    if (st.alloc(bytes, 2, "rq_router_rerank") != RQ_OK) return st.code();
    double* ib = st.at<double>(0);
    int32_t* ik = (int32_t*)(ib + 2 * n);
    st.up(ib, b, n * 8);
    st.up(ib + n, d, n * 8);
    st.up(ik, keys, n * 4);
    st.up(ik + n, count, (size_t)B * 4);
    if (st.code() != RQ_OK) return st.code();
    double* ob = st.at<double>(1);
    int32_t* ok = (int32_t*)(ob + 4 * no);
    const int rc = rq_router_rerank_device(r, ik, ib, ib + n, ik + n, B, P, mode, stats, top_r, ok, ob, ob + no, ob + 2 * no, ob + 3 * no, ok + no, ok + 2 * no,
                                           (void*)r->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_b, ob, no * 8);
    st.down(out_d, ob + no, no * 8);
    st.down(out_w, ob + 2 * no, no * 8);
    st.down(out_h, ob + 3 * no, no * 8);
    st.down(out_keys, ok, no * 4);
    st.down(out_pos, ok + no, no * 4);
    st.down(out_count, ok + 2 * no, (size_t)B * 4);
    return st.finish();
}
