// rq_stage.h -- the staging of ONE blocking call on one stream: the host-buffer forms (rq_search_filtered, rq_search_filtered_each, rq_search_mmr, rq_score_rows,
// rq_search_range, rq_search_grouped, rq_search_group_members: alloc, up, the device form, down, finish) and the repairs (fixup_ladder,
// range_fixup, grouped_fixup and its exclusion rounds, group_members_fixup, through rq_repair.h: d2d, zero, launched).  The first failure sticks: every later step
// returns it and issues nothing.  A call that leaves with work enqueued that finish() has not waited for -- whichever step failed, the
// device form's included -- waits for the stream before anything is freed: no copy is in flight on freed buffers or into the caller's
// memory when it returns.
// Host only; tests/native/stage_check.cpp runs it against stand-ins for the six HIP calls below.
#pragma once
#include "rq_index.h"

struct Stage {
    hipStream_t s;
    void* buf[9] = {};
    int n = 0, rc = RQ_OK;    // (callers read code() and say launched(): rc and in_flight are this header's)
    bool in_flight = false;   // something was enqueued on s that finish() has not waited for
    explicit Stage(hipStream_t stream) : s(stream) {}
    Stage(const Stage&) = delete;
    ~Stage() {
        if (in_flight) (void)hipStreamSynchronize(s);
        for (int i = 0; i < n; ++i) (void)hipFree(buf[i]);
    }
    // count (<= 9) buffers of bytes[i] each, all or none (a failed call's are freed with the object); at<T>(i) is the i-th
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
    int code() const { return rc; }
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* text) {   // (no src: zeroes)
        if (rc != RQ_OK) return rc;
        in_flight = true;
        if ((src ? hipMemcpyAsync(dst, src, bytes, kind, s) : hipMemsetAsync(dst, 0, bytes, s)) != hipSuccess) rc = set_err(RQ_EHIP, "%s", text);
        return rc;
    }
    int up(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice, "H2D copy failed"); }
    int down(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost, "D2H copy failed"); }
    int d2d(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToDevice, "D2D copy failed"); }
    int zero(void* dst, size_t bytes) { return copy(dst, nullptr, bytes, hipMemcpyDefault, "memset failed"); }
    // the caller enqueues kernels on s that use the buffers: whichever step fails from here on, the stream is waited for before they are freed
    void launched() { in_flight = in_flight || rc == RQ_OK; }
    int finish() {
        if (rc == RQ_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_err(RQ_EHIP, "D2H copy failed");
        in_flight = in_flight && rc != RQ_OK;
        return rc;
    }
};
