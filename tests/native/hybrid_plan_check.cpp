// Host-side check of csrc/rq_hybrid_plan.h: the validation of the key space at create time and the inverse map it yields, the checks
// of a call's arguments, the instantiation of the fuse kernel by candidate count with its threads and LDS bytes, and the grid of the
// row-scoring kernel -- plain arithmetic, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/hybrid_plan_check.cpp -o hybrid_plan_check
#include "rq_hybrid_plan.h"

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

int main() {
    {   // ---- the key space at create time and the inverse map -------------------------------------------------------------------
        std::vector<int32_t> inv;
        const int64_t dk[] = {2, 5, 0, 6};            // nb = 4: dense rows 0 and 2 are sparse rows 2 and 0, rows 1 and 3 are dense only
        const uint8_t known[] = {1, 1, 0, 1, 1, 1, 0};
        CHECK(hybrid_check_create(4, 4, dk, known, 7, inv) == RQ_OK, "a good key space: %s", g_err);
        const int32_t want[] = {2, -1, 0, -1, -1, 1, 3};
        CHECK(inv.size() == 7 && std::equal(inv.begin(), inv.end(), want), "the inverse map");
        CHECK(hybrid_check_create(4, 0, nullptr, known, 7, inv) == RQ_OK && inv.size() == 7 && *std::max_element(inv.begin(), inv.end()) == -1, "no dense rows: no inverse");
        CHECK(hybrid_check_create(0, 0, nullptr, nullptr, 0, inv) == RQ_OK && inv.empty(), "an empty key space");
        CHECK(hybrid_check_create(0, 4, dk, known, 7, inv) == RQ_OK, "no sparse rows");
        const int64_t twice[] = {2, 5, 2, 6};
        CHECK(hybrid_check_create(4, 4, twice, known, 7, inv) == RQ_EINVAL && std::strstr(g_err, "injective") && std::strstr(g_err, "rows 0 and 2"), "a key held twice: %s", g_err);
        const int64_t beyond[] = {2, 5, 0, 7};
        CHECK(hybrid_check_create(4, 4, beyond, known, 7, inv) == RQ_EINVAL && std::strstr(g_err, "outside"), "a key = n_keys: %s", g_err);
        const int64_t negative[] = {2, -1, 0, 6};
        CHECK(hybrid_check_create(4, 4, negative, known, 7, inv) == RQ_EINVAL && std::strstr(g_err, "outside"), "a negative key");
        CHECK(hybrid_check_create(8, 4, dk, known, 7, inv) == RQ_EINVAL && std::strstr(g_err, "nb "), "nb beyond n_keys");
        CHECK(hybrid_check_create(-1, 4, dk, known, 7, inv) == RQ_EINVAL && hybrid_check_create(4, -1, dk, known, 7, inv) == RQ_EINVAL &&
              hybrid_check_create(4, 4, dk, known, -7, inv) == RQ_EINVAL, "negative sizes");
        CHECK(hybrid_check_create(4, 4, nullptr, known, 7, inv) == RQ_EINVAL && hybrid_check_create(4, 4, dk, nullptr, 7, inv) == RQ_EINVAL, "null tables");
        CHECK(hybrid_check_create(4, 4, dk, known, (int64_t)1 << 31, inv) == RQ_EINVAL && std::strstr(g_err, "2^31"), "n_keys = 2^31 is refused before anything is allocated");
        CHECK(hybrid_check_create(4, (int64_t)1 << 31, dk, known, 7, inv) == RQ_EINVAL && std::strstr(g_err, "2^31"), "n_dense = 2^31");
    }
    {   // ---- the instantiation by candidate count ---------------------------------------------------------------------------------
        struct { int n, pad, threads; } want[] = {{1, 64, 64}, {2, 64, 64}, {63, 64, 64}, {64, 64, 64}, {65, 128, 64}, {128, 128, 64}, {129, 256, 128}, {200, 256, 128},
                                                  {255, 256, 128}, {256, 256, 128}, {257, 512, 256}, {512, 512, 256}, {513, 1024, 256}, {1024, 1024, 256},
                                                  {1025, 2048, 256}, {2047, 2048, 256}, {2048, 2048, 256}};
        for (const auto& w : want) {
            const int pad = hybrid_pad(w.n);
            CHECK(pad == w.pad && hybrid_threads(pad) == w.threads, "%d candidates: pad %d, %d threads", w.n, pad, hybrid_threads(pad));
            CHECK(pad >= w.n && (pad & (pad - 1)) == 0 && hybrid_threads(pad) % 64 == 0 && hybrid_threads(pad) <= pad, "whole waves, a comparator or a slot per thread");
        }
        CHECK(RQ_HYBRID_MAX_CAND == RQ_SPARSE_MAX_K + RQ_MAX_K && hybrid_pad(RQ_HYBRID_MAX_CAND) == RQ_HYBRID_MAX_CAND, "the largest call is the largest instantiation");
        CHECK(hybrid_lds_bytes(2048, true) == 2048 * 29 + 4 * 32 && hybrid_lds_bytes(2048, true) < 65536, "fuse, 2 048 candidates: %zu bytes of LDS", hybrid_lds_bytes(2048, true));
        CHECK(hybrid_lds_bytes(64, true) == 64 * 29 + 32 && hybrid_lds_bytes(256, true) == 256 * 29 + 2 * 32, "the small pools do not pay for 2 048");
        CHECK(hybrid_lds_bytes(2048, false) == 2048 * 9 && hybrid_lds_bytes(64, false) == 64 * 9, "missing: the sort array and the flags");
    }
    {   // ---- a call's arguments ----------------------------------------------------------------------------------------------------
        int dummy = 0;
        const void* p = &dummy;
        CHECK(hybrid_check_pools(p, p, p, 1, 1, 1) == RQ_OK && hybrid_check_pools(p, p, p, 65535, 1024, 1024) == RQ_OK, "the limits");
        CHECK(hybrid_check_pools(p, nullptr, p, 1, 0, 1) == RQ_OK && hybrid_check_pools(p, p, nullptr, 1, 1, 0) == RQ_OK, "a pool of width 0 needs no array");
        CHECK(hybrid_check_pools(p, nullptr, nullptr, 1, 0, 0) == RQ_EINVAL && std::strstr(g_err, "no candidates"), "K1 + K2 = 0");
        CHECK(hybrid_check_pools(p, nullptr, p, 1, 1, 1) == RQ_EINVAL && hybrid_check_pools(p, p, nullptr, 1, 1, 1) == RQ_EINVAL && hybrid_check_pools(nullptr, p, p, 1, 1, 1) == RQ_EINVAL, "null pointers");
        for (int B : {0, -1, 65536}) CHECK(hybrid_check_pools(p, p, p, B, 1, 1) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        for (int K : {-1, 1025}) {
            CHECK(hybrid_check_pools(p, p, p, 1, K, 1) == RQ_EINVAL && std::strstr(g_err, "K1 "), "K1 = %d", K);
            CHECK(hybrid_check_pools(p, p, p, 1, 1, K) == RQ_EINVAL && std::strstr(g_err, "K2 "), "K2 = %d", K);
        }
        CHECK(hybrid_check_missing(p, p, p, 3, 4, 5, p, p) == RQ_OK && hybrid_check_missing(p, p, p, 3, 4, 5, nullptr, p) == RQ_EINVAL &&
              hybrid_check_missing(p, p, p, 3, 4, 5, p, nullptr) == RQ_EINVAL && hybrid_check_missing(p, p, nullptr, 3, 4, 0, p, nullptr) == RQ_OK, "miss arrays");
        CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, 10, p, p, p, p, p) == RQ_OK, "no extras: %s", g_err);
        CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, p, p, p, p, 1024, p, p, p, p, p) == RQ_OK && hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, p, nullptr, p, nullptr, 1, p, p, p, p, p) == RQ_OK,
              "all extras; miss arrays alone");
        CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, p, nullptr, nullptr, 10, p, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "without its miss"), "extra_dense alone");
        CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, nullptr, nullptr, p, 10, p, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "without its miss"), "extra_sparse alone");
        for (int k : {0, -1, 1025}) CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, k, p, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "top_k"), "top_k = %d", k);
        CHECK(hybrid_check_fuse(p, p, nullptr, p, p, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, 10, p, p, p, p, p) == RQ_EINVAL &&
              hybrid_check_fuse(p, p, p, p, nullptr, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, 10, p, p, p, p, p) == RQ_EINVAL, "null scores");
        CHECK(hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, 10, nullptr, p, p, p, p) == RQ_EINVAL &&
              hybrid_check_fuse(p, p, p, p, p, 3, 4, 5, nullptr, nullptr, nullptr, nullptr, 10, p, p, p, p, nullptr) == RQ_EINVAL, "null outputs");
        CHECK(hybrid_check_score_rows(p, p, 1, p, 1, p) == RQ_OK && hybrid_check_score_rows(p, p, 65535, p, RQ_MAX_SCORE_ROWS, p) == RQ_OK, "row scoring: the limits");
        for (int m : {0, -1, RQ_MAX_SCORE_ROWS + 1}) CHECK(hybrid_check_score_rows(p, p, 1, p, m, p) == RQ_EINVAL && std::strstr(g_err, "m "), "m = %d", m);
        for (int B : {0, 65536}) CHECK(hybrid_check_score_rows(p, p, B, p, 1, p) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        CHECK(hybrid_check_score_rows(nullptr, p, 1, p, 1, p) == RQ_EINVAL && hybrid_check_score_rows(p, nullptr, 1, p, 1, p) == RQ_EINVAL &&
              hybrid_check_score_rows(p, p, 1, nullptr, 1, p) == RQ_EINVAL && hybrid_check_score_rows(p, p, 1, p, 1, nullptr) == RQ_EINVAL, "row scoring: null pointers");
        CHECK(hybrid_score_blocks(1, 1) == 1u && hybrid_score_blocks(1, 256) == 1u && hybrid_score_blocks(1, 257) == 2u && hybrid_score_blocks(500, 100) == 196u, "one thread per pair");
        CHECK(hybrid_score_blocks(65535, RQ_MAX_SCORE_ROWS) == 16776960u, "the largest call: B x m beyond 2^31 pairs in 64 bits");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
