// rq_stage.h -- the staging buffers of ONE blocking host-buffer call on one stream (rq_search_filtered, rq_search_mmr, rq_score_rows, rq_search_range and its repair):
// alloc, up, the device form, down, finish.  The first failure sticks: every later step returns it and issues nothing.  A call that
// leaves with work enqueued that finish() has not waited for -- whichever step failed, the device form's included -- waits for the
// stream before anything is freed: no copy is in flight on freed buffers or into the caller's memory when it returns.
// Host only; tests/native/stage_check.cpp runs it against stand-ins for the five HIP calls below.
#pragma once
#include "rq_index.h"

struct Stage {
    hipStream_t s;
    void* buf[8] = {};
    int n = 0, rc = RQ_OK;
    bool in_flight = false;   // something was enqueued on s that finish() has not waited for
    explicit Stage(hipStream_t stream) : s(stream) {}
    Stage(const Stage&) = delete;
    ~Stage() {
        if (in_flight) (void)hipStreamSynchronize(s);
        for (int i = 0; i < n; ++i) (void)hipFree(buf[i]);
    }
    // count (<= 8) buffers of bytes[i] each, all or none (a failed call's are freed with the object); at<T>(i) is the i-th
    int alloc(const size_t* bytes, int count, const char* what) {
        size_t total = 0;
        for (int i = 0; i < count; ++i) total += bytes[i];
        for (n = 0; n < count; ++n) {
            if (hipMalloc(&buf[n], bytes[n]) == hipSuccess) continue;
            (void)hipGetLastError();   // (a failed hipMalloc stays the runtime's last error otherwise)
            return rc = set_err(RQ_ENOMEM, "staging of %zu bytes for %s", total, what);
        }
        return RQ_OK;
    }
    template <class T> T* at(int i) const { return (T*)buf[i]; }
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* text) {
        if (rc != RQ_OK) return rc;
        in_flight = true;
        if (hipMemcpyAsync(dst, src, bytes, kind, s) != hipSuccess) rc = set_err(RQ_EHIP, "%s", text);
        return rc;
    }
    int up(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice, "H2D copy failed"); }
    int down(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost, "D2H copy failed"); }
    int finish() {
        if (rc == RQ_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_err(RQ_EHIP, "D2H copy failed");
        in_flight = in_flight && rc != RQ_OK;
        return rc;
    }
};
