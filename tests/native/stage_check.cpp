// Host-side check of csrc/rq_stage.h, the staging of the blocking host-buffer calls (rq_search_filtered, rq_search_mmr,
// rq_score_rows).  The five HIP calls the helper makes -- allocate, free, asynchronous copy, stream synchronisation, last error --
// are STAND-INS defined here, at link time: they keep a log, can be told to fail at a given call, and work on real host memory of
// the requested size, so that -fsanitize=address,undefined sees every copy, a double free and a leak.  The calls are driven in
// the order the three entry points use, with the sizes of their own pure sizing functions.  The stand-ins are test scaffolding:
// nothing in the product links them.
//   hipcc -O1 -g -std=c++17 --offload-host-only -fsanitize=address,undefined -I <csrc> tests/native/stage_check.cpp -o stage_check
#include "rq_stage.h"
#include "rq_mmr_plan.h"
#include "rq_score_plan.h"

#include <cstdlib>
#include <set>

static thread_local char g_err[512] = "";
int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* rq_err_text() { return g_err; }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

// ---- the stand-ins ----------------------------------------------------------------------------------------------------------
// log: M allocate, F free, U copy to the device, D copy to the host, S synchronise, E last error read, K the device form ran
static std::string g_log;
static std::set<void*> g_live;
static int g_bad_free = 0, g_mallocs = 0, g_copies = 0, g_syncs = 0;
static int g_fail_malloc = -1, g_fail_copy = -1, g_fail_sync = -1;   // the call (counted from 0) that fails; -1: none
static int g_stream_tag = 0;
static hipStream_t const g_stream = (hipStream_t)(void*)&g_stream_tag;

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    g_log += 'M';
    if (g_mallocs++ == g_fail_malloc) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    g_log += 'F';
    if (!g_live.erase(p)) { ++g_bad_free; return hipErrorInvalidValue; }   // never allocated, or freed before
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    g_log += kind == hipMemcpyHostToDevice ? 'U' : (kind == hipMemcpyDeviceToHost ? 'D' : '?');
    if (s != g_stream) g_log += '!';
    if (g_copies++ == g_fail_copy) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t s) {
    g_log += 'S';
    if (s != g_stream) g_log += '!';
    return g_syncs++ == g_fail_sync ? hipErrorUnknown : hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) {
    g_log += 'E';
    return hipSuccess;
}

// ---- one blocking call, as the entry points write it ---------------------------------------------------------------------------
struct Copy { int buf; size_t bytes; };
struct Shape {
    const char* name;
    std::vector<size_t> bytes;       // the staging buffers, in allocation order
    std::vector<Copy> ups, downs;    // the copies, in order
    const char* want;                // the log of a call that succeeds
};
static std::vector<char> g_host;     // the caller's memory: large enough for every copy of every shape

static int run_call(const Shape& sh, int device_rc) {
    Stage st(g_stream);
    if (int r = st.alloc(sh.bytes.data(), (int)sh.bytes.size(), sh.name)) return r;
    for (const Copy& c : sh.ups) st.up(st.at<char>(c.buf), g_host.data(), c.bytes);
    if (st.rc != RQ_OK) return st.rc;
    g_log += 'K';
    if (device_rc != RQ_OK) return device_rc;
    for (const Copy& c : sh.downs) st.down(g_host.data(), st.at<char>(c.buf), c.bytes);
    return st.finish();
}
static int run(const Shape& sh, int fail_malloc, int fail_copy, int fail_sync, int device_rc = RQ_OK) {
    g_log.clear();
    g_bad_free = g_mallocs = g_copies = g_syncs = 0;
    g_fail_malloc = fail_malloc; g_fail_copy = fail_copy; g_fail_sync = fail_sync;
    g_err[0] = 0;
    const int rc = run_call(sh, device_rc);
    CHECK(g_live.empty() && g_bad_free == 0, "%s [%s]: %zu buffers left, %d bad frees", sh.name, g_log.c_str(), g_live.size(), g_bad_free);
    CHECK(g_log.find('!') == std::string::npos && g_log.find('?') == std::string::npos, "%s [%s]: another stream or copy kind", sh.name, g_log.c_str());
    return rc;
}
static int count(char c) { return (int)std::count(g_log.begin(), g_log.end(), c); }
// every buffer allocated was freed once (run() has checked the pointers), after a wait if anything had been enqueued, and nothing
// was enqueued after the failure at log position `at`
static void check_failed_call(const Shape& sh, int allocated, size_t at) {
    CHECK(count('F') == allocated, "%s [%s]: %d frees of %d buffers", sh.name, g_log.c_str(), count('F'), allocated);
    const size_t first_free = g_log.find('F'), first_copy = g_log.find_first_of("UD");
    if (first_copy != std::string::npos && first_free != std::string::npos) {
        const size_t last_sync = g_log.rfind('S', first_free);
        CHECK(last_sync != std::string::npos && last_sync > at, "%s [%s]: no wait between the failure and the first free", sh.name, g_log.c_str());
    }
    CHECK(g_log.find_first_of("UDK", at + 1) == std::string::npos, "%s [%s]: work issued after the failure", sh.name, g_log.c_str());
}

int main() {
    const int dim = 33, B = 3, k = 5, m = 20;
    const SearchStaging fs = search_staging(dim, B, k);
    const MmrStaging ms = mmr_staging(dim, B, m, k);
    const ScoreStaging ss = score_staging(dim, B, m);
    CHECK(fs.q == 396 && fs.scores == 60 && fs.rows == 120 && fs.status == 12, "search_staging(33, 3, 5)");
    CHECK(search_staging(768, 65535, 1024).rows == (size_t)65535 * 1024 * 8 && search_staging(1, 32768, 65536).scores == ((size_t)1 << 33), "64-bit sizes");
    CHECK(ms.q == fs.q && ms.status == fs.status && ms.cand_scores == 240 && ms.cand_rows == 480 && ms.out_scores == 60 && ms.out_rows == 120 && ms.out_mmr == 60, "mmr_staging");
    g_host.assign(std::max({fs.q, ms.cand_rows, ss.rows}), 1);
    const Shape shapes[] = {
        {"a filtered search", {fs.q, fs.scores, fs.rows, fs.status}, {{0, fs.q}}, {{1, fs.scores}, {2, fs.rows}}, "MMMMUKDDSFFFF"},
        {"an MMR search", {ms.q, ms.cand_scores, ms.cand_rows, ms.status, ms.out_scores, ms.out_rows}, {{0, ms.q}}, {{4, ms.out_scores}, {5, ms.out_rows}}, "MMMMMMUKDDSFFFFFF"},
        {"an MMR search with its values", {ms.q, ms.cand_scores, ms.cand_rows, ms.status, ms.out_scores, ms.out_rows, ms.out_mmr}, {{0, ms.q}},
         {{4, ms.out_scores}, {5, ms.out_rows}, {6, ms.out_mmr}}, "MMMMMMMUKDDDSFFFFFFF"},
        {"scoring given rows", {ss.q, ss.rows, ss.scores}, {{0, ss.q}, {1, ss.rows}}, {{2, ss.scores}}, "MMMUUKDSFFF"},
    };
    for (const Shape& sh : shapes) {
        const int nbuf = (int)sh.bytes.size(), nup = (int)sh.ups.size(), ncopy = nup + (int)sh.downs.size();
        size_t total = 0;
        for (size_t b : sh.bytes) total += b;
        // ---- success: the exact sequence of calls, one wait, at the end of the copies
        CHECK(run(sh, -1, -1, -1) == RQ_OK && g_log == sh.want, "%s: [%s], expected [%s]", sh.name, g_log.c_str(), sh.want);
        // ---- every allocation fails in turn: RQ_ENOMEM with the total in the message, the earlier buffers freed, the runtime's
        // error read (cleared), nothing enqueued and nothing waited for
        for (int i = 0; i < nbuf; ++i) {
            CHECK(run(sh, i, -1, -1) == RQ_ENOMEM, "%s, allocation %d: [%s]", sh.name, i, g_log.c_str());
            CHECK(std::strstr(g_err, std::to_string(total).c_str()) && std::strstr(g_err, sh.name), "%s, allocation %d: message '%s'", sh.name, i, g_err);
            CHECK(g_log == std::string((size_t)i + 1, 'M') + "E" + std::string((size_t)i, 'F'), "%s, allocation %d: [%s]", sh.name, i, g_log.c_str());
        }
        // ---- every copy fails in turn: RQ_EHIP, it is the last thing enqueued, the stream is waited for before the first free
        for (int j = 0; j < ncopy; ++j) {
            CHECK(run(sh, -1, j, -1) == RQ_EHIP, "%s, copy %d: [%s]", sh.name, j, g_log.c_str());
            CHECK(count('U') + count('D') == j + 1 && count('K') == (j >= nup ? 1 : 0), "%s, copy %d: [%s]", sh.name, j, g_log.c_str());
            check_failed_call(sh, nbuf, g_log.find_last_of("UD"));
            CHECK(std::strstr(g_err, j < nup ? "H2D" : "D2H"), "%s, copy %d: message '%s'", sh.name, j, g_err);
        }
        // ---- the device form fails (its own code comes back), with the upward copies enqueued before it
        for (int code : {RQ_EHIP, RQ_ENOMEM, RQ_EINVAL}) {
            CHECK(run(sh, -1, -1, -1, code) == code && count('D') == 0, "%s, device form %d: [%s]", sh.name, code, g_log.c_str());
            check_failed_call(sh, nbuf, g_log.find('K'));
        }
        // ---- the final wait fails: RQ_EHIP, and the stream is waited for once more before anything is freed
        CHECK(run(sh, -1, -1, 0) == RQ_EHIP && count('S') == 2, "%s, failed wait: [%s]", sh.name, g_log.c_str());
        check_failed_call(sh, nbuf, g_log.find('S'));
    }
    {   // ---- a call that allocates and leaves before it enqueues anything waits for nothing
        g_log.clear();
        g_mallocs = 0; g_fail_malloc = -1;
        { Stage st(g_stream); const size_t b[2] = {8, 16}; CHECK(st.alloc(b, 2, "nothing") == RQ_OK && st.at<char>(1) && !st.at<char>(2), "two buffers"); }
        CHECK(g_log == "MMFF" && g_live.empty(), "[%s]", g_log.c_str());
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
