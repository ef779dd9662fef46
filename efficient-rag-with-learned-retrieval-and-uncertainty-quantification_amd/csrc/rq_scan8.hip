// rq_scan8.hip -- the int8 image of a shard (option "scan8"): building it, measuring where its ladder one image -> two
// images -> fp16 scan starts, and moving a class of k along that ladder when its searches need too many repairs.
// Whether a call scans the image: rq_plan.h scan8_wanted / scan8_usable.
#include "rq_plan.h"

void drop_x8(rq_index* idx) {
    free_dev(idx->x8, idx->scale8_cos, idx->scale8_ip, idx->binerr8);
    idx->x8_valid = 0; idx->max_e8 = 0.0;
}

// int8 scan, per class of k (<= 32 / larger): where the adaptive ladder one image -> two images -> fp16 scan starts
void scan8_reset_levels(rq_index* idx) {
    for (int c = 0; c < 2; ++c) {
        idx->scan8_level[c] = idx->scan8_split < 0 ? c : (idx->scan8_split ? 1 : 0);
        idx->scan8_checked[c] = idx->scan8_repaired[c] = 0;
        idx->wide1_ok[c] = idx->wide1_off[c] = false;
        idx->wide1_checked[c] = idx->wide1_repaired[c] = 0;
    }
    idx->calib_rows = 0;   // "scan8" = 1: the next search that brings the image up to date calibrates again
}

// Where the int8 ladder STARTS on this shard ("scan8" = 1, the automatic rule), decided when the image is built instead of
// after slow batches (round 2 started every shard at one image / two images and let rq_search_fixup_device escalate: a
// clustered 1M-row corpus paid 4-8 batches of 0.5-0.7 ms, and a document-structured 125k-row shard kept an int8 scan that
// was twice as slow as the fp16 one).  64 STORED rows, evenly spread, are searched as queries -- on-topic queries are the
// hard case: their neighbourhoods are where the quantisation bound collects candidates -- through every rung (one image,
// two images, fp16 rows) for each class of k (k = 10 for k <= 32, k = 100 beyond), timed with HIP events (prep + scan + tail,
// plain sequential form, best of three).  A rung is eligible when at most 1 in 16 sample queries came back uncertified (the
// ladder's own rule); the LOWEST eligible rung wins unless a higher one is 8 % faster, the fp16 rows being always eligible.  Costs ~20 scans of the shard,
// once per image build (and again when the shard has doubled).  "scan8" = 2 (always) skips this and starts as round 2 did.
static int scan8_calibrate(rq_index* idx, hipStream_t s) {
    if (idx->scan8 != 1 || idx->calibrating || !idx->x8 || idx->n < 64 * 64) return RQ_OK;
    idx->calibrating = true;
    struct Done { rq_index* i; ~Done() { i->calibrating = false; } } done{idx};
    const int S = 64, KMAX = 100;
    std::vector<uint16_t> h16((size_t)S * RQ_DPAD);
    std::vector<float> h32((size_t)S * idx->dim);
    for (int i = 0; i < S; ++i) {
        const int64_t row = (int64_t)((double)i + 0.5) * idx->n / S;
        HIPCHK(hipMemcpy(h16.data() + (size_t)i * RQ_DPAD, idx->x + (size_t)std::min(row, idx->n - 1) * idx->rowb(), idx->rowb(), hipMemcpyDeviceToHost));
        for (int j = 0; j < idx->dim; ++j) {
            _Float16 v; __builtin_memcpy(&v, &h16[(size_t)i * RQ_DPAD + j], 2);
            h32[(size_t)i * idx->dim + j] = (float)v;
        }
    }
    float* d_q = nullptr; float* d_sc = nullptr; int64_t* d_rw = nullptr; int* d_st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = RQ_OK;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_q, h32.size() * sizeof(float)));
        HIPCHK(hipMalloc((void**)&d_sc, (size_t)S * KMAX * sizeof(float)));
        HIPCHK(hipMalloc((void**)&d_rw, (size_t)S * KMAX * sizeof(int64_t)));
        HIPCHK(hipMalloc((void**)&d_st, (size_t)S * sizeof(int)));
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipMemcpy(d_q, h32.data(), h32.size() * sizeof(float), hipMemcpyHostToDevice));
        const int64_t used0 = idx->scan8_used;
        for (int c = 0; c < 2; ++c) {
            const int k = c == 0 ? 10 : KMAX;
            if ((int64_t)k * 2 * 64 > idx->n) { idx->scan8_level[c] = 2; continue; }
            float ms_of[3] = {0.f, 0.f, 0.f};
            int unc_of[3] = {0, 0, 0};
            for (int level = 2; level >= 0; --level) {          // fp16 first: always eligible
                idx->scan8_level[c] = level;
                float ms = 1e30f;
                int unc = 0;
                for (int rep = 0; rep < 4; ++rep) {             // (the first run warms the workspace of this shape)
                    HIPCHK(hipEventRecord(e0, s));
                    if (int r = run_pipeline(idx, d_q, S, k, RQ_METRIC_COSINE, nb_default(idx, k), {d_sc, d_rw, nullptr, d_st}, s, level < 2 ? CALL_ALLOW8 : 0)) return r;
                    HIPCHK(hipEventRecord(e1, s));
                    HIPCHK(hipEventSynchronize(e1));
                    float t = 0.f;
                    HIPCHK(hipEventElapsedTime(&t, e0, e1));
                    if (rep > 0) ms = std::min(ms, t);
                }
                int st[64];
                HIPCHK(hipMemcpy(st, d_st, sizeof st, hipMemcpyDeviceToHost));
                for (int i = 0; i < S; ++i) unc += st[i] != 0;
                ms_of[level] = ms; unc_of[level] = unc;
            }
            // the lowest eligible rung, unless a higher one is clearly (8 %) faster: one image per query is also the only form with
            // wide int8 passes, and two rungs within the boxes' run-to-run noise must not flip the choice between processes
            int best = 2;
            for (int level = 1; level >= 0; --level)
                if (unc_of[level] * 16 <= S) best = level;
            for (int level = best + 1; level < 3; ++level)
                if ((level == 2 || unc_of[level] * 16 <= S) && ms_of[level] < 0.92f * ms_of[best]) best = level;
            idx->scan8_level[c] = best;
            idx->scan8_checked[c] = idx->scan8_repaired[c] = 0;
            idx->wide1_ok[c] = unc_of[0] * 16 <= S;      // one image is eligible on the sample (whichever rung 64-query calls were given)
            idx->wide1_off[c] = false;
            idx->wide1_checked[c] = idx->wide1_repaired[c] = 0;
            for (int l = 0; l < 3; ++l) { idx->calib_ms[c][l] = ms_of[l]; idx->calib_unc[c][l] = unc_of[l]; }
        }
        idx->scan8_used = used0;      // (the calibration's own scans are not the caller's searches)
        idx->calib_rows = idx->n;
        return RQ_OK;
    };
    const int level_before[2] = {idx->scan8_level[0], idx->scan8_level[1]};
    rc = body();
    if (rc != RQ_OK) { idx->scan8_level[0] = level_before[0]; idx->scan8_level[1] = level_before[1]; }   // (a failed measurement leaves no trial rung behind)
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    free_dev(d_q, d_sc, d_rw, d_st);
    return rc;
}

// int8 scan ("scan8"): bring the int8 image of the shard up to date (rows appended since the last search that used it) and
// read back the worst row's relative quantisation error.  One blocking 8-byte copy per append, nothing when up to date.
int ensure_x8(rq_index* idx, hipStream_t s) {
    if (idx->x8 && idx->x8_valid == idx->n) {
        if (idx->scan8 == 1 && idx->calib_rows == 0 && !idx->calibrating && idx->max_e8 <= RQ_SCAN8_MAX_ROW_ERR) return scan8_calibrate(idx, s);
        return RQ_OK;
    }
    if (!idx->x8) {
        hipError_t e = hipMalloc((void**)&idx->x8, (size_t)idx->cap * RQ_DPAD);
        if (e == hipSuccess) e = hipMalloc((void**)&idx->scale8_cos, (size_t)idx->cap * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&idx->scale8_ip, (size_t)idx->cap * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&idx->binerr8, (size_t)(idx->cap / 64 + 64) * sizeof(float));   // (+64: the tail reads whole record strides)
        if (e == hipSuccess && !idx->d_stat8) e = hipMalloc((void**)&idx->d_stat8, sizeof(unsigned long long));
        if (e != hipSuccess) {   // no room for the image (+50 % of the shard): not an error, the fp16 rows remain the scan operand
            drop_x8(idx);
            (void)hipGetLastError();
            idx->scan8_level[0] = idx->scan8_level[1] = 2;
            return RQ_OK;
        }
        HIPCHK(hipMemsetAsync(idx->x8, 0, (size_t)idx->cap * RQ_DPAD, s));
        HIPCHK(hipMemsetAsync(idx->scale8_cos, 0xff, (size_t)idx->cap * sizeof(float), s));   // pad rows: NaN (see grow)
        HIPCHK(hipMemsetAsync(idx->scale8_ip, 0xff, (size_t)idx->cap * sizeof(float), s));
        HIPCHK(hipMemsetAsync(idx->d_stat8, 0, sizeof(unsigned long long), s));
        HIPCHK(hipMemsetAsync(idx->binerr8, 0, (size_t)(idx->cap / 64 + 64) * sizeof(float), s));
        idx->x8_valid = 0; idx->max_e8 = 0.0;
    }
    HIPCHK(rq_quant_rows_launch(idx->x, idx->rownorm64, idx->x8_valid, idx->n, idx->x8, idx->scale8_cos, idx->scale8_ip, idx->d_stat8, idx->binerr8, s));
    unsigned long long bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, idx->d_stat8, sizeof bits, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    __builtin_memcpy(&idx->max_e8, &bits, sizeof bits);
    idx->x8_valid = idx->n;
    if (idx->scan8 == 1 && idx->max_e8 <= RQ_SCAN8_MAX_ROW_ERR && (idx->calib_rows == 0 || idx->n >= 2 * idx->calib_rows))
        return scan8_calibrate(idx, s);
    return RQ_OK;
}

// The int8 scan bets that real errors stay well below its worst-case bound (threshold multiplier thr_mult8 < 2) and that few
// rows sit within that bound of the k-th score.  A shard / query mix on which either fails shows up as repairs: beyond 1 in 16
// CHECKED queries (windows of 256) the class of k moves one step along one image -> two images -> fp16 scan, until "scan8" /
// "scan8_split" is set again.  Every checked query counts, the clean ones too (rq_search_end's clean branch reports them: a
// server answering one query per call must not see only its failures), whatever the size of the call.
void scan8_account(rq_index* idx, int k, int checked, int repaired) {
    if (!idx->last_use8 || !idx->x8 || !idx->scan8) return;
    const int kclass = scan8_kclass(k);
    if (idx->scan8_level[kclass] >= 2) return;
    if (idx->last_wide1) {       // a wide call on one image in a two-image class: its repairs decide about the wide calls only
        idx->wide1_checked[kclass] += checked; idx->wide1_repaired[kclass] += repaired;
        if (idx->wide1_checked[kclass] >= 256) {
            if (idx->wide1_repaired[kclass] * 16 > idx->wide1_checked[kclass]) idx->wide1_off[kclass] = true;
            idx->wide1_checked[kclass] = idx->wide1_repaired[kclass] = 0;
        }
        return;
    }
    idx->scan8_checked[kclass] += checked; idx->scan8_repaired[kclass] += repaired;
    if (idx->scan8_checked[kclass] >= 256) {
        if (idx->scan8_repaired[kclass] * 16 > idx->scan8_checked[kclass]) idx->scan8_level[kclass]++;
        idx->scan8_checked[kclass] = idx->scan8_repaired[kclass] = 0;
    }
}
