// rq_api.hip -- the C ABI of include/rq.h: shard storage in HBM, options, debug hooks, timing, persistence.
//
// One rq_index = one row shard resident on one MI355X.  Layout in HBM:
//   x          [cap][dpad] fp16 (dpad = 768, or 384 for dim <= 384: option "row_pad"), cap % 64 == 0, rows >= n are zero   (the only large array)
//   rownorm64  [cap]      fp64 L2 norm of the stored row               (exact re-score)
//   inv_norm   [cap]      fp32 2^-12 / norm, 0 for zero rows, NaN for pad rows (scan, cosine; the queries carry 2^12)
//   ones       [cap]      fp32 2^-12 for rows < n, NaN beyond                  (scan, inner product; lazy)
// plus one workspace per stream (query fragments, per-bin scan records, bin keys, candidate keys).
// Internal definitions: rq_index.h; searches: rq_search.hip (what a call does: rq_plan.h); the int8 image: rq_scan8.hip; filtered
// searches: rq_filter.hip; the multi-device parent (n_devices > 1): rq_multi.hip.
#include "rq_group_members_plan.h"

hipError_t rq_rowscale_launch(const double* norm64, int64_t row_begin, int64_t row_end, float* inv_norm, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* rq_err_text() { return g_err; }
int err_no_device() { return set_err(RQ_ENODEVICE, "RQ_ENODEVICE: no HIP device visible: the gfx950 backend has no CPU fallback"); }

extern "C" int rq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" const char* rq_last_error(void) { return rq_err_text(); }
extern "C" const char* rq_version(void) { return "rq-hip 0.1 (gfx950)"; }

static int grow(rq_index* idx, int64_t want_rows) {
    if (want_rows <= idx->cap) return RQ_OK;
    int64_t cap = std::max<int64_t>(idx->cap * 2, 4096);
    while (cap < want_rows) cap *= 2;
    if (want_rows > (int64_t)1 << 27 && cap > want_rows + want_rows / 8) cap = want_rows + want_rows / 8;   // big shards: 12% headroom
    cap = (cap + 63) / 64 * 64;
    if (int r = flush_all(idx)) return r;
    HIPCHK(hipDeviceSynchronize());   // searches in flight on any stream still read the old buffers
    char* nx = nullptr; double* nn = nullptr; float* ni = nullptr;
    const size_t rowb = idx->rowb();
    hipError_t e = hipMalloc((void**)&nx, (size_t)cap * rowb);
    if (e != hipSuccess) return set_err(RQ_ENOMEM, "hipMalloc of %lld corpus rows failed: %s", (long long)cap, hipGetErrorString(e));
    if ((e = hipMalloc((void**)&nn, (size_t)cap * sizeof(double))) != hipSuccess || (e = hipMalloc((void**)&ni, (size_t)cap * sizeof(float))) != hipSuccess) {
        (void)hipFree(nx);
        if (nn) (void)hipFree(nn);
        return set_err(RQ_ENOMEM, "hipMalloc of the row statistics of %lld rows failed: %s", (long long)cap, hipGetErrorString(e));
    }
    const int64_t keep = idx->n;
    if (keep > 0) {
        HIPCHK(hipMemcpyAsync(nx, idx->x, (size_t)keep * rowb, hipMemcpyDeviceToDevice, idx->own_stream));
        HIPCHK(hipMemcpyAsync(nn, idx->rownorm64, (size_t)keep * sizeof(double), hipMemcpyDeviceToDevice, idx->own_stream));
        HIPCHK(hipMemcpyAsync(ni, idx->inv_norm, (size_t)keep * sizeof(float), hipMemcpyDeviceToDevice, idx->own_stream));
    }
    HIPCHK(hipMemsetAsync(nx + (size_t)keep * rowb, 0, (size_t)(cap - keep) * rowb, idx->own_stream));
    HIPCHK(hipMemsetAsync(nn + keep, 0, (size_t)(cap - keep) * sizeof(double), idx->own_stream));
    // row scales of the pad rows are NaN (0xffffffff): their scan scores sort last without a per-score row test
    // (rq_scan_wide.hip); rq_scan.hip masks rows >= n on its own
    HIPCHK(hipMemsetAsync(ni + keep, 0xff, (size_t)(cap - keep) * sizeof(float), idx->own_stream));
    int32_t* ng = nullptr;   // the group ids follow the rows once a group has been set (rq_group.hip); rows beyond `keep` are RQ_GROUP_NONE (0xffffffff)
    if (idx->d_groups) {
        if (hipMalloc((void**)&ng, (size_t)cap * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            free_dev(nx, nn, ni);
            return set_err(RQ_ENOMEM, "hipMalloc of the group ids of %lld rows failed", (long long)cap);
        }
        if (keep > 0) HIPCHK(hipMemcpyAsync(ng, idx->d_groups, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToDevice, idx->own_stream));
        HIPCHK(hipMemsetAsync(ng + keep, 0xff, (size_t)(cap - keep) * sizeof(int32_t), idx->own_stream));
    }
    HIPCHK(hipStreamSynchronize(idx->own_stream));
    if (ng) { (void)hipFree(idx->d_groups); idx->d_groups = ng; }
    if (idx->x) (void)hipFree(idx->x);
    if (idx->rownorm64) (void)hipFree(idx->rownorm64);
    if (idx->inv_norm) (void)hipFree(idx->inv_norm);
    if (idx->ones) { (void)hipFree(idx->ones); idx->ones = nullptr; idx->ones_valid = 0; }
    drop_x8(idx);   // the int8 image is rebuilt for the new capacity by the next search that wants it
    idx->x = nx; idx->rownorm64 = nn; idx->inv_norm = ni; idx->cap = cap;
    return RQ_OK;
}

extern "C" rq_index* rq_index_create(int dim, int n_devices, const int* device_ids) {
    if (dim < 1 || dim > RQ_MAX_DIM) { set_err(RQ_EINVAL, "dim %d outside 1..%d", dim, RQ_MAX_DIM); return nullptr; }
    if (n_devices < 1 || n_devices > 64 || !device_ids) { set_err(RQ_EINVAL, "n_devices %d outside 1..64 or no device list", n_devices); return nullptr; }
    if (n_devices > 1) return rq_multi_create(dim, n_devices, device_ids);
    const int ndev = rq_device_count();
    if (ndev <= 0) { set_err(RQ_ENODEVICE, "no HIP device visible: the gfx950 backend has no CPU fallback"); return nullptr; }
    if (device_ids[0] < 0 || device_ids[0] >= ndev) { set_err(RQ_EINVAL, "device %d outside 0..%d", device_ids[0], ndev - 1); return nullptr; }
    rq_index* idx = new rq_index();
    idx->dim = dim;
    idx->dpad = dim <= 384 ? 384 : RQ_DPAD;   // the rule of "row_pad"
    idx->device = device_ids[0];
    DeviceGuard dg_(idx->device);
    hipDeviceProp_t prop;
    if (!dg_.ok || hipGetDeviceProperties(&prop, idx->device) != hipSuccess) {
        set_err(RQ_EHIP, "cannot open device %d", idx->device);
        delete idx;
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(RQ_ENODEVICE, "device %d is %s; this library holds gfx950 code only", idx->device, prop.gcnArchName);
        delete idx;
        return nullptr;
    }
    idx->cu_count = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&idx->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&idx->d_maxnorm, 3 * sizeof(double)) != hipSuccess ||
        hipMemset(idx->d_maxnorm, 0, 3 * sizeof(double)) != hipSuccess) {
        set_err(RQ_EHIP, "device setup failed on device %d", idx->device);
        delete idx;
        return nullptr;
    }
    return idx;
}

extern "C" void rq_index_destroy(rq_index* idx) {
    if (!idx) return;
    if (!idx->shards.empty()) {
        for (rq_index* c : idx->shards) rq_index_destroy(c);
        delete idx;
        return;
    }
    DeviceGuard dg_(idx->device);
    (void)flush_all(idx);   // calls gathered in an open bundle are scanned and finished: their results were promised
    (void)hipDeviceSynchronize();
    for (auto& kv : idx->ctx) free_ctx(kv.second);
    free_filters(idx);   // the filters nobody destroyed (include/rq.h rq_filter_destroy)
    free_dev(idx->range_bins, idx->d_groups, idx->gm_scored);
    drop_group_table(idx);
    for (auto& ev : idx->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (idx->hs_pin) (void)hipHostFree(idx->hs_pin);
    if (idx->hs_pin_q) (void)hipHostFree(idx->hs_pin_q);
    free_dev(idx->add_stage, idx->x, idx->rownorm64, idx->inv_norm, idx->ones, idx->x8, idx->scale8_cos, idx->scale8_ip, idx->binerr8, idx->d_stat8, idx->d_maxnorm,
             idx->h_dq, idx->h_dscores, idx->h_drows, idx->h_dstatus, idx->hs_dev, idx->dbg_stamps);
    if (idx->own_stream) (void)hipStreamDestroy(idx->own_stream);
    delete idx;
}

extern "C" int rq_index_dim(const rq_index* idx) { return idx ? idx->dim : RQ_EINVAL; }
extern "C" int64_t rq_index_size(const rq_index* idx) { return idx ? idx->n : RQ_EINVAL; }
extern "C" int rq_index_set_row_offset(rq_index* idx, int64_t off) {
    if (!idx || off < 0) return set_err(RQ_EINVAL, "bad row offset");
    // keys carry the global row as a 32-bit field (0xffffffff is reserved): the whole shard must stay below it
    if ((uint64_t)off + (uint64_t)idx->n >= 0xffffffffull) return set_err(RQ_EUNSUPPORTED, "row_offset %lld + %lld rows reaches 2^32-1: row ids are 32-bit inside keys", (long long)off, (long long)idx->n);
    if (idx->shards.empty() && bundles_open(idx)) {   // gathered calls return the row ids of the offset they were made under
        RQ_ON_DEVICE(idx);
        if (int r = flush_all(idx)) return r;
    }
    idx->row_offset = off;
    return RQ_OK;
}
extern "C" int rq_index_reserve(rq_index* idx, int64_t n_rows) {
    if (!idx || n_rows < 0) return set_err(RQ_EINVAL, "bad reserve");
    if (!idx->shards.empty()) return rq_multi_reserve(idx, n_rows);
    RQ_ON_DEVICE(idx);
    return grow(idx, n_rows);
}

// ---- append ----------------------------------------------------------------------------------
static int finish_add(rq_index* idx, int64_t n_new) {
    hipStream_t s = idx->own_stream;
    const int64_t b = idx->n, e = idx->n + n_new;
    HIPCHK(rq_rownorm_launch(idx->x, idx->dpad, b, e, idx->rownorm64, (unsigned long long*)idx->d_maxnorm, s));
    HIPCHK(rq_rowscale_launch(idx->rownorm64, b, e, idx->inv_norm, s));
    double st[3] = {0.0, 0.0, 0.0};
    HIPCHK(hipMemcpyAsync(st, idx->d_maxnorm, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    idx->max_row_norm = st[0]; idx->max_sub_rel = st[1]; idx->max_sub_abs = st[2];
    idx->n = e;
    if (idx->d_groups) idx->h_groups.resize((size_t)e, RQ_GROUP_NONE);   // appended rows are groups of their own (the device side: grow)
    return RQ_OK;
}

static int add_device_common(rq_index* idx, const void* d_rows, int64_t n_rows, bool is_f32, int normalize) {
    if (!idx || (!d_rows && n_rows > 0) || n_rows < 0) return set_err(RQ_EINVAL, "bad add arguments");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "device-pointer appends on a multi-device index: use rq_index_add_f16 / _f32 (host rows)");
    if (n_rows == 0) return RQ_OK;
    if ((uint64_t)idx->row_offset + (uint64_t)idx->n + (uint64_t)n_rows >= 0xffffffffull)   // checked BEFORE anything is appended
        return set_err(RQ_EUNSUPPORTED, "row ids beyond 2^32-1 are not supported (row_offset %lld + %lld rows)", (long long)idx->row_offset, (long long)(idx->n + n_rows));
    RQ_ON_DEVICE(idx);
    // The rows may have been produced on any stream of the caller (e.g. torch's): wait for all of it.
    // Appending is not a hot path; searches in flight on other streams are drained too, which also
    // makes it safe to reallocate the shard below.
    if (int r = flush_all(idx)) return r;
    HIPCHK(hipDeviceSynchronize());
    if (int r = grow(idx, idx->n + n_rows)) return r;
    char* dst = idx->x + (size_t)idx->n * idx->rowb();
    if (is_f32) HIPCHK(rq_convert_f32_launch((const float*)d_rows, idx->dim, n_rows, normalize, dst, idx->dpad, idx->own_stream));
    else if (idx->dim == idx->dpad) HIPCHK(hipMemcpyAsync(dst, d_rows, (size_t)n_rows * idx->rowb(), hipMemcpyDeviceToDevice, idx->own_stream));
    else HIPCHK(rq_pad_f16_launch(d_rows, idx->dim, n_rows, dst, idx->dpad, idx->own_stream));
    return finish_add(idx, n_rows);
}
extern "C" int rq_index_add_f16_device(rq_index* idx, const void* d_rows, int64_t n_rows) { return add_device_common(idx, d_rows, n_rows, false, 0); }
extern "C" int rq_index_add_f32_device(rq_index* idx, const float* d_rows, int64_t n_rows, int normalize) {
    return add_device_common(idx, d_rows, n_rows, true, normalize);
}

int rq_add_host_common(rq_index* idx, const void* rows, int64_t n_rows, bool is_f32, int normalize) {
    if (!idx || (!rows && n_rows > 0) || n_rows < 0) return set_err(RQ_EINVAL, "bad add arguments");
    if (n_rows == 0) return RQ_OK;
    if (!idx->shards.empty()) return rq_multi_add(idx, rows, n_rows, is_f32, normalize);
    RQ_ON_DEVICE(idx);
    if (int r = grow(idx, idx->n + n_rows)) return r;
    // stream the host rows through a bounded device staging buffer, kept between calls (an indexing run appends
    // 100 documents at a time: no hipMalloc / hipFree per batch); a buffer beyond 16 MiB is given back after the call
    const size_t esz = is_f32 ? 4 : 2;
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)(idx->dim * esz));
    const size_t need = (size_t)std::min(chunk, n_rows) * idx->dim * esz;
    if (need > idx->add_stage_bytes) {
        if (idx->add_stage) (void)hipFree(idx->add_stage);
        idx->add_stage = nullptr; idx->add_stage_bytes = 0;
        HIPCHK(hipMalloc(&idx->add_stage, need));
        idx->add_stage_bytes = need;
    }
    int rc = RQ_OK;
    for (int64_t off = 0; off < n_rows && rc == RQ_OK; off += chunk) {
        const int64_t m = std::min(chunk, n_rows - off);
        hipError_t e = hipMemcpy(idx->add_stage, (const char*)rows + (size_t)off * idx->dim * esz, (size_t)m * idx->dim * esz, hipMemcpyHostToDevice);
        if (e != hipSuccess) { rc = set_err(RQ_EHIP, "H2D copy failed: %s", hipGetErrorString(e)); break; }
        rc = add_device_common(idx, idx->add_stage, m, is_f32, normalize);
    }
    if (idx->add_stage_bytes > ((size_t)16 << 20)) { (void)hipFree(idx->add_stage); idx->add_stage = nullptr; idx->add_stage_bytes = 0; }
    return rc;
}
extern "C" int rq_index_add_f16(rq_index* idx, const uint16_t* rows, int64_t n_rows) { return rq_add_host_common(idx, rows, n_rows, false, 0); }
extern "C" int rq_index_add_f32(rq_index* idx, const float* rows, int64_t n_rows, int normalize) {
    return rq_add_host_common(idx, rows, n_rows, true, normalize);
}

extern "C" int rq_index_get_rows_f16(const rq_index* idx, int64_t row_begin, int64_t n_rows, uint16_t* out) {
    if (!idx || !out || row_begin < 0 || n_rows < 0 || row_begin + n_rows > idx->n) return set_err(RQ_EINVAL, "row range outside the index");
    if (n_rows == 0) return RQ_OK;
    if (!idx->shards.empty()) return rq_multi_get_rows(idx, row_begin, n_rows, out);
    RQ_ON_DEVICE(idx);
    HIPCHK(hipMemcpy2D(out, (size_t)idx->dim * 2, idx->x + (size_t)row_begin * idx->rowb(), idx->rowb(), (size_t)idx->dim * 2,
                       (size_t)n_rows, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- options ---------------------------------------------------------------------------------
extern "C" int rq_set_option(rq_index* idx, const char* name, double v) {
    if (!idx || !name) return set_err(RQ_EINVAL, "bad option call");
    if (!idx->shards.empty()) {
        if (std::string(name) == "stripe_rows") {   // multi-device parent: rows per stripe (rq_multi.hip), before the first append only
            if (idx->n != 0) return set_err(RQ_EINVAL, "stripe_rows can only be set on an empty multi-device index");
            if (v < 64 || v > (double)(1 << 30) || (int64_t)v % 64 != 0) return set_err(RQ_EINVAL, "stripe_rows must be a multiple of 64 in 64..2^30");
            idx->stripe = (int64_t)v;
            return RQ_OK;
        }
        // (the children take the same row length, before the first append: a child that is still empty later must not be given another)
        if (std::string(name) == "row_pad" && idx->n != 0) return set_err(RQ_EINVAL, "row_pad can only be set on an empty index");
        for (rq_index* c : idx->shards)
            if (int r = rq_set_option(c, name, v)) return r;
        return RQ_OK;
    }
    const std::string s(name);
    // Calls gathered in an open bundle (rq_bundle_plan.h) are scanned late, by a plan made then: they are completed under the
    // options they were made with before any option changes.
    if (bundles_open(idx)) {
        RQ_ON_DEVICE(idx);
        if (int r = flush_all(idx)) return r;
    }
    if (s == "row_pad") {   // stored row length: 384 (dim <= 384 only) or 768, while no row is stored
        if (v != 384 && v != RQ_DPAD) return set_err(RQ_EINVAL, "row_pad must be 384 or %d", RQ_DPAD);
        if (v == 384 && idx->dim > 384) return set_err(RQ_EINVAL, "row_pad 384 needs dim <= 384 (dim is %d)", idx->dim);
        if (idx->n != 0) return set_err(RQ_EINVAL, "row_pad can only be set on an empty index");
        if ((int)v != idx->dpad) {
            RQ_ON_DEVICE(idx);
            const int64_t reserved = idx->cap;   // a reservation is made again with the new row length
            if (int r = flush_all(idx)) return r;
            HIPCHK(hipDeviceSynchronize());
            free_dev(idx->x, idx->rownorm64, idx->inv_norm, idx->ones);
            idx->ones_valid = 0; idx->cap = 0;
            drop_x8(idx);
            idx->dpad = (int)v;
            if (reserved > 0) return grow(idx, reserved);
        }
    }
    else if (s == "ring") { if (v < 2 || v > 6) return set_err(RQ_EINVAL, "ring must be 2..6"); idx->ring = (int)v; }
    else if (s == "wide_batch") { if (v < 0 || v > 3) return set_err(RQ_EINVAL, "wide_batch must be 0..3"); idx->wide_batch = (int)v; }
    // (8 and 11, the fp16 forms with asm fragment reads and counted LDS waits, are withdrawn: csrc/rq_scan_wide.hip)
    else if (s == "wide128") { if (v < 0 || v > 99 || v == 8) return set_err(RQ_EINVAL, "wide128: a 128-query variant of csrc/rq_scan_wide.hip (8 is withdrawn)"); idx->wide128 = (int)v; }
    else if (s == "wide256") { if (v < 0 || v > 92 || v == 11) return set_err(RQ_EINVAL, "wide256: a 256-query variant of csrc/rq_scan_wide.hip (11 is withdrawn)"); idx->wide256 = (int)v; }
    else if (s == "kstage") { if (v != 1 && v != 2) return set_err(RQ_EINVAL, "kstage must be 1 or 2"); idx->kstage = (int)v; }
    else if (s == "prefetch") { if (v != 1 && v != 4 && v != 6 && v != 12) return set_err(RQ_EINVAL, "prefetch must be 1, 4, 6 or 12"); idx->prefetch = (int)v; }
    else if (s == "wg_per_cu") { if (v < 0 || v > 8) return set_err(RQ_EINVAL, "wg_per_cu must be 1..8 (0: back to the library's rule)"); idx->wg_auto = v == 0; idx->wg_per_cu = v == 0 ? 2 : (int)v; }
    else if (s == "nt") idx->nt = (int)v;
    else if (s == "cu_count") { if (v < 1 || v > 1024) return set_err(RQ_EINVAL, "cu_count must be 1..1024"); idx->cu_count = (int)v; }   // test hook: shrinks the scan grid
    else if (s == "slack_bins") idx->slack_bins = (int)v;
    else if (s == "eps") idx->eps = v;
    else if (s == "profile") idx->profile = (int)v;
    else if (s == "scan_nostore") idx->scan_nostore = (int)v;   // timing experiments only: 1 = the scan writes nothing (results invalid)
    else if (s == "profile_stride") { if (v < 1) return set_err(RQ_EINVAL, "profile_stride must be >= 1"); idx->profile_stride = (int)v; }
    else if (s == "fast_tail") idx->fast_tail = (int)v;
    else if (s == "pipeline") { if (v != 0 && v != 1 && v != 2) return set_err(RQ_EINVAL, "pipeline must be 0, 1 or 2"); if (int r = flush_all(idx)) return r; idx->pipeline = (int)v; }
    else if (s == "tail_stop") idx->tail_stop = (int)v;
    else if (s == "epi" || s == "fused_epi") idx->epi = (int)v != 0;   // selection form of the 64-query scan (default variant and fused launch): 1 = positions inside the scores, 0 = compare / select
    else if (s == "profile_legacy") idx->profile_legacy = (int)v != 0;   // time scans with hipEventRecord around the launch (round 1) instead of dispatch-attached events
    else if (s == "scan8") { if (v < 0 || v > 2) return set_err(RQ_EINVAL, "scan8 must be 0, 1 or 2"); idx->scan8 = (int)v; scan8_reset_levels(idx); }   // see rq_plan.h scan8_wanted
    else if (s == "wide256_8") { if (v != 0 && v != 22 && v != 25 && !(v >= 30 && v <= 33)) return set_err(RQ_EINVAL, "wide256_8: 0 (off) or a 256-query int8 variant of csrc/rq_scan_wide.hip (22, 25, 30..33)"); idx->wide256_8 = (int)v; }
    else if (s == "wide8") idx->wide8 = (int)v != 0;   // calls of more than 64 queries may use 128-query passes over the int8 image
    else if (s == "scan8_split") { if (v < -1 || v > 1) return set_err(RQ_EINVAL, "scan8_split must be -1, 0 or 1"); idx->scan8_split = (int)v; scan8_reset_levels(idx); }   // see rq_plan.h plan_call
    else if (s == "thr_mult8") { if (!(v >= 1.05 && v <= 2.25)) return set_err(RQ_EINVAL, "thr_mult8 %g outside 1.05..2.25", v); idx->thr_mult8 = v; }
    else if (s == "exact_mfma") idx->exact_mfma = (int)v != 0;   // A/B: 0 = the exact scan of a whole shard re-scores bin by bin and query by query (rq_rescore_kernel, rounds 1-2)
    else if (s == "fused_nv") idx->fused_nv = (int)v;   // development: bins per riding tail workgroup (0 = the launcher's rule, 1 / 4 / 8 x 512)
    else if (s == "bin_bound") idx->bin_bound = (int)v != 0;     // A/B: 0 = every bin is tested with the shard's worst row error (round 2)
    else if (s == "tail_local") idx->tail_local = (int)v != 0;   // A/B: 0 = every re-scored row's key goes to the query's global list
    else if (s == "use_hint") idx->use_hint = (int)v != 0;   // 0: rq_search_hint_next_device is ignored (A/B of the folded query preparation)
    else if (s == "scan_ahead") idx->scan_ahead = (int)v != 0;   // 0: a hinted batch is never scanned together with the call before it (A/B)
    // bundles of scanned-ahead calls: 2 = pairs only, 4 = up to four calls per 256-query pass once a loop is steady
    else if (s == "scan_bundle") { if (v != 2 && v != 4) return set_err(RQ_EINVAL, "scan_bundle must be 2 or 4"); if (int r = flush_all(idx)) return r; idx->scan_bundle = (int)v; }
    else if (s == "filter_route") { if (v != -1 && v != 1 && v != 2 && v != 3) return set_err(RQ_EINVAL, "filter_route must be -1 (rule), 1 (gather), 2 (scan) or 3 (exact)"); idx->filter_route = (int)v; }   // rq_filter_plan.h
    else if (s == "filter_each_key_cap") { if (!(v >= 0 && v <= (double)((int64_t)1 << 40))) return set_err(RQ_EINVAL, "filter_each_key_cap must be 0 (default) .. 2^40"); idx->each_key_cap = (int64_t)v; }   // test hook (rq_filter_each_plan.h: keys per ragged round)
    else if (s == "range_route") { if (v != -1 && v != 1 && v != 2 && v != 3) return set_err(RQ_EINVAL, "range_route must be -1 (rule), 1 (scan), 2 (gather) or 3 (exact)"); idx->range_route = (int)v; }   // rq_range_plan.h
    else if (s == "range_cand_cap") { if (v < 0 || v > (1 << 20)) return set_err(RQ_EINVAL, "range_cand_cap must be 0 (default) .. 1048576"); idx->range_cand_cap = (int)v; }   // test hook (never below a call's cap)
    else if (s == "group_fetch") { if (!(v >= 1 && v <= RQ_MAX_K)) return set_err(RQ_EINVAL, "group_fetch must be 1..%d", RQ_MAX_K); idx->group_fetch = (int)v; }   // rq_group_plan.h group_fetch
    else if (s == "group_fill_cap") { if (!(v >= 0 && v <= RQ_GROUP_FILL_MAX)) return set_err(RQ_EINVAL, "group_fill_cap must be 0 (default) .. %d", RQ_GROUP_FILL_MAX); idx->group_fill_cap = (int)v; }   // test hook (rq_group_members_plan.h group_fill_cap)
    else if (s == "group_fetch_cap") { if (!(v >= 0 && v <= RQ_MAX_K)) return set_err(RQ_EINVAL, "group_fetch_cap must be 0 (default) .. %d", RQ_MAX_K); idx->group_fetch_cap = (int)v; }   // test hook (never below a call's k)
    else if (s == "poison_cand") idx->poison_cand = (int)v;   // test hook: candidate lists are filled with 0xff..ff keys before every tail
    else if (s == "poison_bins") idx->poison_bins = (int)v;   // test hook: the query slots a call's passes cover are filled with 0xff bytes before its scan
    else return set_err(RQ_EINVAL, "unknown option '%s'", name);
    return RQ_OK;
}
extern "C" double rq_get_option(const rq_index* idx, const char* name) {
    if (!idx || !name) return NAN;
    if (!idx->shards.empty()) {   // the statistics are shard maxima, everything else is the same on every child
        const std::string o(name);
        if (o == "stripe_rows") return (double)idx->stripe;
        double v = rq_get_option(idx->shards[0], name);
        if (o.rfind("max_", 0) == 0 || o.rfind("eps_", 0) == 0 || o == "scan8_row_err" || o == "scan8_suspended")
            for (rq_index* c : idx->shards) v = std::max(v, rq_get_option(c, name));
        if (o == "scan8_used" || o == "hints_used" || o == "bundles4") {   // counters: summed
            v = 0;
            for (rq_index* c : idx->shards) v += rq_get_option(c, name);
        }
        return v;
    }
    const std::string s(name);
    if (s == "row_pad") return idx->dpad;
    if (s == "ring") return idx->ring;
    if (s == "prefetch") return idx->prefetch;
    if (s == "kstage") return idx->kstage;
    if (s == "wide_batch") return idx->wide_batch;
    if (s == "wg_per_cu") return idx->wg_per_cu;
    if (s == "nt") return idx->nt;
    if (s == "slack_bins") return idx->slack_bins;
    if (s == "eps") return idx->eps < 0 ? RQ_EPS_DEFAULT : idx->eps;   // the base bound; "eps_cosine" / "eps_ip": with the shard's flush term
    if (s == "profile") return idx->profile;
    if (s == "fast_tail") return idx->fast_tail;
    if (s == "scan_ahead") return idx->scan_ahead;
    if (s == "scan_bundle") return idx->scan_bundle;
    if (s == "bundles4") return (double)idx->bundles4;   // 256-query passes of bundles of three or four calls
    if (s == "pipeline") return idx->pipeline;
    if (s == "profile_stride") return idx->profile_stride;
    if (s == "cu_count") return idx->cu_count;
    if (s == "max_row_norm") return idx->max_row_norm;
    if (s == "scan8") return idx->scan8;
    if (s == "thr_mult8") return idx->thr_mult8;
    if (s == "scan8_split") return idx->scan8_split;
    if (s == "wide8") return idx->wide8;
    if (s == "wide256_8") return idx->wide256_8;
    if (s == "scan8_row_err") return idx->x8_valid == idx->n && idx->x8 ? idx->max_e8 : -1.0;   // worst row's relative int8 error (-1: image not built)
    if (s == "scan8_suspended") return (idx->scan8_level[0] == 2 ? 1.0 : 0.0) + (idx->scan8_level[1] == 2 ? 2.0 : 0.0);   // bit 0: k <= 32, bit 1: larger k
    if (s == "scan8_wide_one_image") {   // per class (units: k <= 32, tens: larger k): 1 = its calls of more than 64 queries scan ONE int8 image per query now
        double r = 0;
        for (int c = 0; c < 2; ++c) {
            const int lvl = idx->scan8_level[c];
            const bool on = idx->scan8 && idx->wide8 && (lvl == 0 || (lvl == 1 && idx->scan8_split < 0 && !idx->wide1_off[c] && (idx->scan8 == 2 || idx->wide1_ok[c])));
            r += (c ? 10.0 : 1.0) * (on ? 1 : 0);
        }
        return r;
    }
    if (s == "scan8_level") return idx->scan8_level[0] + 10.0 * idx->scan8_level[1];   // per class: 0 one image, 1 two images, 2 fp16 scan   // too many repairs behind the int8 scan (rq_search_fixup_device)
    if (s == "scan8_calibrated_rows") return (double)idx->calib_rows;   // rows of the shard when the int8 ladder's start was last measured (0: never)
    // "scan8_calib_ms_<class><rung>" / "scan8_calib_unc_<class><rung>" (class 0: k <= 32, 1: larger; rung 0 one image, 1 two images,
    // 2 fp16 rows): milliseconds and uncertified queries of the 64-query sample search the calibration measured for that rung
    for (int unc = 0; unc < 2; ++unc) {
        const std::string pre = unc ? "scan8_calib_unc_" : "scan8_calib_ms_";
        if (s.rfind(pre, 0) == 0 && s.size() == pre.size() + 2) {
            const int c = s[pre.size()] - '0', l = s[pre.size() + 1] - '0';
            if (c >= 0 && c < 2 && l >= 0 && l < 3) return unc ? (double)idx->calib_unc[c][l] : (double)idx->calib_ms[c][l];
        }
    }
    if (s == "filter_route") return idx->filter_route;
    if (s == "filter_route_last") return idx->filter_route_last;   // the route the last filtered call took (0: no row allowed; -1: none yet)
    if (s == "filter_repaired") return (double)idx->filter_repaired;   // queries of filtered calls that were repaired
    if (s == "filter_each_calls") return (double)idx->each_calls;               // searches with one filter per query so far (rq_filter_each.hip)
    if (s == "filter_each_groups_last") return (double)idx->each_groups_last;   // distinct filters of the last one (NULL counts as one)
    if (s == "filter_each_ragged_last") return (double)idx->each_ragged_last;   // queries its ragged launches answered
    if (s == "filter_each_rounds_last") return (double)idx->each_rounds_last;   // ragged rounds it ran
    if (s == "filter_each_shared_exact_last") return (double)idx->each_shared_last;   // queries its shared exact route answered
    if (s == "filter_each_routes_last") return (double)idx->each_routes_last;   // bit r: some group took route r (4: the unrestricted group)
    if (s == "filter_each_key_cap") return (double)idx->each_key_cap;
    if (s == "mmr_calls") return (double)idx->mmr_calls;  // MMR selections launched (rq_mmr_select_device, rq_search_mmr)
    if (s == "score_calls") return (double)idx->score_calls;   // scoring calls (rq_score_rows_device, rq_score_rows)
    if (s == "score_pairs") return (double)idx->score_pairs;   // ... and the (query, row) pairs they were given: B x m each
    if (s == "range_route") return idx->range_route;
    if (s == "range_route_last") return idx->range_route_last;   // the route the last range call took (0: no row to return; -1: none yet)
    if (s == "range_calls") return (double)idx->range_calls;     // range calls (rq_search_range_device, rq_search_range)
    if (s == "range_repaired") return (double)idx->range_repaired;   // queries the range fixup re-ran on the exact route
    if (s == "range_cand_cap") return idx->range_cand_cap;
    if (s == "range_bins_last") {   // bins the last range call's tail re-scored, all queries (-1: it did not take the scan route); waits for the device
        if (!idx->range_bins_valid || !idx->range_bins) return -1.0;
        DeviceGuard dg_(idx->device);
        unsigned long long v = 0;
        if (!dg_.ok || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, idx->range_bins, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return NAN;
        return (double)v;
    }
    if (s == "group_fetch") return idx->group_fetch;
    if (s == "group_fetch_cap") return idx->group_fetch_cap;
    if (s == "group_calls") return (double)idx->group_calls;         // collapses launched (rq_group_collapse_device, rq_search_grouped*)
    if (s == "group_repaired") return (double)idx->group_repaired;   // queries the grouped fixup repaired
    if (s == "group_rounds_last") return (double)idx->group_rounds_last;   // exclusion rounds of the last grouped fixup, all its queries
    if (s == "group_fill_cap") return idx->group_fill_cap;
    if (s == "group_table_builds") return (double)idx->group_table_builds;   // member tables built (rq_group_members.hip)
    if (s == "group_fill_calls") return (double)idx->group_fill_calls;       // fill launches (every entry point, the repair's included)
    if (s == "group_fill_repaired") return (double)idx->group_fill_repaired; // queries the member fixup filled by the exact route
    if (s == "group_fill_rows_last") {   // members the last fill scored, all its slots (-1: no fill yet); waits for the device
        if (!idx->gm_scored || idx->gm_scored_slots <= 0) return idx->group_fill_calls > 0 ? 0.0 : -1.0;
        DeviceGuard dg_(idx->device);
        std::vector<int> h((size_t)idx->gm_scored_slots);
        if (!dg_.ok || hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), idx->gm_scored, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return NAN;
        double v = 0;
        for (int x : h) v += x;
        return v;
    }
    if (s == "repaired_queries") return (double)idx->repaired_total;   // queries rq_search_fixup_device (or the blocking rq_search) had to repair so far
    if (s == "scan8_used") return (double)idx->scan8_used;   // searches that scanned the int8 image
    if (s == "hints_used") return (double)idx->hints_used;   // searches that found their queries prepared by the launch before them
    if (s == "max_sub_rel") return idx->max_sub_rel;   // largest share of a row's norm that sits in fp16-subnormal elements
    if (s == "max_sub_abs") return idx->max_sub_abs;
    if (s == "eps_cosine") return scan_eps(idx, RQ_METRIC_COSINE);
    if (s == "eps_ip") return scan_eps(idx, RQ_METRIC_IP);
    return NAN;
}

// ---- development hook: wall-clock (start, end) stamps of every workgroup of the LAST fused launch ------------
extern "C" int rq_debug_stamps(rq_index* idx, int enable, unsigned long long* out, int max_wgs) {
    if (!idx) return set_err(RQ_EINVAL, "null index");
    if (!idx->shards.empty()) return set_err(RQ_EUNSUPPORTED, "debug hooks work on single-device indexes");
    RQ_ON_DEVICE(idx);
    HIPCHK(hipDeviceSynchronize());
    if (enable && !idx->dbg_stamps) { HIPCHK(hipMalloc((void**)&idx->dbg_stamps, 4 * 8192 * sizeof(unsigned long long))); HIPCHK(hipMemset(idx->dbg_stamps, 0, 4 * 8192 * sizeof(unsigned long long))); }
    if (out && idx->dbg_stamps) HIPCHK(hipMemcpy(out, idx->dbg_stamps, (size_t)4 * std::min(max_wgs, 8192) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (!enable && idx->dbg_stamps) { (void)hipFree(idx->dbg_stamps); idx->dbg_stamps = nullptr; }
    return RQ_OK;
}

// ---- measurement hook: plain streaming read of the shard (see rq_read_probe_kernel) ------------------------
extern "C" double rq_debug_read_bandwidth(rq_index* idx, int iters, int nt, int wg_per_cu) {
    if (!idx || iters < 1 || iters > 1000 || wg_per_cu < 1 || wg_per_cu > 32 || !idx->shards.empty()) { set_err(RQ_EINVAL, "bad arguments"); return -1.0; }
    DeviceGuard dg_(idx->device);
    if (!dg_.ok) { set_err(RQ_EHIP, "cannot select device %d", idx->device); return -1.0; }
    if (idx->n == 0) { set_err(RQ_EINVAL, "empty index"); return -1.0; }
    if (flush_all(idx)) return -1.0;
    const int64_t bytes = idx->n * (int64_t)idx->rowb();
    const bool use_nt = nt < 0 ? bytes > ((int64_t)208 << 20) : nt != 0;
    uint32_t* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double gbs = -1.0;
    hipStream_t s = idx->own_stream;
    do {
        if (hipMalloc((void**)&sink, 64) != hipSuccess) break;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) break;
        const int grid = idx->cu_count * wg_per_cu;
        if (rq_read_probe_launch(idx->x, bytes, use_nt, grid, sink, s) != hipSuccess) break;   // warm-up
        if (hipEventRecord(e0, s) != hipSuccess) break;
        bool ok = true;
        for (int i = 0; i < iters && ok; ++i) ok = rq_read_probe_launch(idx->x, bytes, use_nt, grid, sink, s) == hipSuccess;
        if (!ok || hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.f) break;
        gbs = (double)bytes * iters / (ms * 1e-3) / 1e9;
    } while (0);
    if (gbs < 0) set_err(RQ_EHIP, "read probe failed: %s", hipGetErrorString(hipGetLastError()));
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (sink) (void)hipFree(sink);
    return gbs;
}

// ---- test hook: the scan's per-bin maxima of the last search on `stream` ---------------------------------
extern "C" int64_t rq_debug_pooled(rq_index* idx, void* stream, int query, float* out, int64_t max_bins) {
    if (!idx || !out || query < 0 || !idx->shards.empty()) return set_err(RQ_EINVAL, "bad arguments");
    RQ_ON_DEVICE(idx);
    auto it = idx->ctx.find((hipStream_t)stream);
    if (it == idx->ctx.end() || !it->second.rec_bins) return set_err(RQ_EINVAL, "the last search on this stream ran no approximate scan");
    const StreamCtx& c = it->second;
    if (query >= c.rec_slots) return set_err(RQ_EINVAL, "query %d beyond the %d slots the last search's passes covered", query, c.rec_slots);
    const int64_t n = std::min({(idx->n + 63) / 64, max_bins, c.rec_stride});   // (rows appended since: their bins have no record)
    HIPCHK(hipDeviceSynchronize());
    // field x of every 8-byte record: the bin's largest approximate score (26 bits, rounded up) | its row
    std::vector<uint32_t> raw((size_t)n);
    HIPCHK(hipMemcpy2D(raw.data(), sizeof(uint32_t), c.rec_bins + (size_t)query * c.rec_stride, sizeof(uint2), sizeof(uint32_t), (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) out[i] = rq_rec_m1(raw[(size_t)i]);
    return n;
}

// ---- test hook: the raw bin records (rq_device.h) of query slots q0 .. q0 + nq of the last search on `stream` ----------
extern "C" int64_t rq_debug_bin_records(rq_index* idx, void* stream, int q0, int nq, uint32_t* out, int64_t max_bins) {
    if (!idx || !out || q0 < 0 || nq < 1 || max_bins < 0 || !idx->shards.empty()) return set_err(RQ_EINVAL, "bad arguments");
    RQ_ON_DEVICE(idx);
    auto it = idx->ctx.find((hipStream_t)stream);
    if (it == idx->ctx.end() || !it->second.rec_bins) return set_err(RQ_EINVAL, "the last search on this stream ran no approximate scan");
    const StreamCtx& c = it->second;
    if ((int64_t)q0 + nq > c.rec_slots) return set_err(RQ_EINVAL, "slots %d..%d beyond the %d the last search's passes covered", q0, q0 + nq - 1, c.rec_slots);
    const int64_t n = std::min({(idx->n + 63) / 64, max_bins, c.rec_stride});
    HIPCHK(hipDeviceSynchronize());
    if (n > 0)
        HIPCHK(hipMemcpy2D(out, (size_t)n * sizeof(uint2), c.rec_bins + (size_t)q0 * c.rec_stride, (size_t)c.rec_stride * sizeof(uint2), (size_t)n * sizeof(uint2),
                           (size_t)nq, hipMemcpyDeviceToHost));
    return n;
}

// ---- test hook: the int8 image's worst row error per bin (what the tail lifts its threshold by) -------------
extern "C" int64_t rq_debug_bin_err(rq_index* idx, float* out, int64_t max_bins) {
    if (!idx || !out || !idx->shards.empty()) return set_err(RQ_EINVAL, "bad arguments");
    RQ_ON_DEVICE(idx);
    if (!idx->x8 || !idx->binerr8 || idx->x8_valid != idx->n) return set_err(RQ_EINVAL, "the int8 image is not built (run a search with the int8 scan first)");
    const int64_t n = std::min((idx->n + 63) / 64, max_bins);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, idx->binerr8, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

// ---- timing ----------------------------------------------------------------------------------
extern "C" int rq_get_timing(rq_index* idx, rq_timing* out) {
    if (!idx || !out) return set_err(RQ_EINVAL, "null argument");
    if (!idx->shards.empty()) {   // kernel figures summed over the children, call counts of the parent
        rq_timing sum = idx->t;
        for (rq_index* c : idx->shards) {
            rq_timing t;
            if (int r = rq_get_timing(c, &t)) return r;
            sum.scan_ms += t.scan_ms; sum.scan_launches += t.scan_launches; sum.scan_bytes += t.scan_bytes;
            sum.widened += t.widened; sum.exact_scans += t.exact_scans;
        }
        *out = sum;
        return RQ_OK;
    }
    RQ_ON_DEVICE(idx);
    HIPCHK(hipDeviceSynchronize());
    double ms = 0.0;
    for (size_t i = 0; i < idx->ev_used; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, idx->events[i].first, idx->events[i].second));
        ms += t;
    }
    idx->t.scan_ms = ms;
    idx->t.scan_launches = (int64_t)idx->ev_used;
    idx->t.scan_bytes = idx->ev_bytes;
    *out = idx->t;
    return RQ_OK;
}
extern "C" int rq_reset_timing(rq_index* idx) {
    if (!idx) return set_err(RQ_EINVAL, "null argument");
    if (!idx->shards.empty()) {
        idx->t = rq_timing{};
        for (rq_index* c : idx->shards)
            if (int r = rq_reset_timing(c)) return r;
        return RQ_OK;
    }
    RQ_ON_DEVICE(idx);
    HIPCHK(hipDeviceSynchronize());
    idx->ev_used = 0; idx->ev_bytes = 0;
    idx->t = rq_timing{};
    return RQ_OK;
}

// ---- persistence -----------------------------------------------------------------------------
extern "C" int rq_save(const rq_index* idx, const char* path) {
    if (!idx || !path) return set_err(RQ_EINVAL, "null argument");
    RQ_ON_DEVICE(idx);
    if (idx->shards.empty())   // (open bundles are completed first, as before every call that touches the rows)
        if (int r = flush_all(const_cast<rq_index*>(idx))) return r;
    const std::string meta = std::string(path) + ".meta", data = std::string(path) + ".f16";
    FILE* f = fopen(data.c_str(), "wb");
    if (!f) return set_err(RQ_EIO, "cannot write %s", data.c_str());
    const int64_t chunk = 65536;
    std::vector<uint16_t> buf((size_t)chunk * idx->dim);
    for (int64_t off = 0; off < idx->n; off += chunk) {
        const int64_t m = std::min(chunk, idx->n - off);
        if (int r = rq_index_get_rows_f16(idx, off, m, buf.data())) { fclose(f); return r; }
        if (fwrite(buf.data(), (size_t)idx->dim * 2, (size_t)m, f) != (size_t)m) { fclose(f); return set_err(RQ_EIO, "short write to %s", data.c_str()); }
    }
    fclose(f);
    f = fopen(meta.c_str(), "w");
    if (!f) return set_err(RQ_EIO, "cannot write %s", meta.c_str());
    fprintf(f, "rq-index 1\ndim %d\nrows %lld\ndtype f16\n", idx->dim, (long long)idx->n);
    fclose(f);
    return RQ_OK;
}

extern "C" rq_index* rq_load(const char* path, int n_devices, const int* device_ids) {
    if (!path) { set_err(RQ_EINVAL, "null path"); return nullptr; }
    const std::string meta = std::string(path) + ".meta", data = std::string(path) + ".f16";
    FILE* f = fopen(meta.c_str(), "r");
    if (!f) { set_err(RQ_EIO, "cannot read %s", meta.c_str()); return nullptr; }
    int ver = 0, dim = 0;
    long long rows = -1;
    char dtype[16] = "";
    const int got = fscanf(f, "rq-index %d dim %d rows %lld dtype %15s", &ver, &dim, &rows, dtype);
    fclose(f);
    if (got != 4 || ver != 1 || rows < 0 || strcmp(dtype, "f16") != 0) { set_err(RQ_EIO, "%s is not an rq-index v1 meta file", meta.c_str()); return nullptr; }
    rq_index* idx = rq_index_create(dim, n_devices, device_ids);
    if (!idx) return nullptr;
    f = fopen(data.c_str(), "rb");
    if (!f) { set_err(RQ_EIO, "cannot read %s", data.c_str()); rq_index_destroy(idx); return nullptr; }
    if (!idx->shards.empty()) {   // multi-device: stripes no longer than an even share, so that a small collection still uses every device
        const int64_t g = (int64_t)idx->shards.size(), share = ((rows + g - 1) / g + 63) / 64 * 64;
        idx->stripe = std::min<int64_t>(idx->stripe, std::max<int64_t>(share, 4096));
    }
    if (rows > 0 && rq_index_reserve(idx, rows) != RQ_OK) { fclose(f); rq_index_destroy(idx); return nullptr; }
    const int64_t chunk = 65536;
    std::vector<uint16_t> buf((size_t)chunk * dim);
    for (int64_t off = 0; off < rows; off += chunk) {
        const int64_t m = std::min<int64_t>(chunk, rows - off);
        if (fread(buf.data(), (size_t)dim * 2, (size_t)m, f) != (size_t)m) { fclose(f); set_err(RQ_EIO, "short read from %s", data.c_str()); rq_index_destroy(idx); return nullptr; }
        if (rq_index_add_f16(idx, buf.data(), m) != RQ_OK) { fclose(f); rq_index_destroy(idx); return nullptr; }
    }
    fclose(f);
    return idx;
}
