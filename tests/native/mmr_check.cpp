// Host-side check of csrc/rq_mmr_plan.h: the argument checks of rq_mmr_select_device and rq_search_mmr, the number of candidates a
// search fetches, the launch geometry and the staged bytes (64-bit arithmetic at the limits) -- plain arithmetic on a
// default-constructed rq_index, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/mmr_check.cpp -o mmr_check
#include "rq_mmr_plan.h"

#include <limits>

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
    rq_index idx;
    idx.dim = 768; idx.dpad = 768; idx.n = idx.cap = 4101;
    const rq_index snapshot = idx;
    int dummy = 0;
    const void* p = &dummy;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {   // ---- rq_mmr_select_device -----------------------------------------------------------------------------------------
        CHECK(check_mmr_select_args(&idx, p, p, 64, 100, 10, 0.5, 0, p, p) == RQ_OK, "the plain call");
        CHECK(check_mmr_select_args(&idx, p, p, 1, 1, 1, 0.0, 1, p, p) == RQ_OK && check_mmr_select_args(&idx, p, p, 65535, RQ_MAX_K, RQ_MAX_K, 1.0, 0, p, p) == RQ_OK, "the limits");
        CHECK(check_mmr_select_args(nullptr, p, p, 1, 1, 1, 0.5, 0, p, p) == RQ_EINVAL && std::strstr(g_err, "null"), "null index");
        CHECK(check_mmr_select_args(&idx, nullptr, p, 1, 1, 1, 0.5, 0, p, p) == RQ_EINVAL && check_mmr_select_args(&idx, p, nullptr, 1, 1, 1, 0.5, 0, p, p) == RQ_EINVAL &&
              check_mmr_select_args(&idx, p, p, 1, 1, 1, 0.5, 0, nullptr, p) == RQ_EINVAL && check_mmr_select_args(&idx, p, p, 1, 1, 1, 0.5, 0, p, nullptr) == RQ_EINVAL, "null pointers");
        for (int B : {0, -1, 65536}) CHECK(check_mmr_select_args(&idx, p, p, B, 10, 5, 0.5, 0, p, p) == RQ_EINVAL, "B = %d", B);
        for (int m : {0, -3, RQ_MAX_K + 1}) CHECK(check_mmr_select_args(&idx, p, p, 1, m, 1, 0.5, 0, p, p) == RQ_EINVAL, "m = %d", m);
        for (int k : {0, -1, 11}) CHECK(check_mmr_select_args(&idx, p, p, 1, 10, k, 0.5, 0, p, p) == RQ_EINVAL, "k = %d of m = 10", k);
        for (double l : {-1e-9, 1.0 + 1e-9, nan, inf, -inf}) CHECK(check_mmr_select_args(&idx, p, p, 1, 10, 5, l, 0, p, p) == RQ_EINVAL && std::strstr(g_err, "lambda"), "lambda = %g", l);
        for (int metric : {-1, 2}) CHECK(check_mmr_select_args(&idx, p, p, 1, 10, 5, 0.5, metric, p, p) == RQ_EINVAL, "metric %d", metric);
        rq_index multi;
        multi.shards.push_back(&idx);
        CHECK(check_mmr_select_args(&multi, p, p, 1, 10, 5, 0.5, 0, p, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED"), "multi-device");
        CHECK(check_mmr_select_args(&multi, p, p, 1, 10, 50, 0.5, 0, p, p) == RQ_EINVAL, "argument errors come first");
    }
    {   // ---- rq_search_mmr ------------------------------------------------------------------------------------------------
        CHECK(check_mmr_search_args(&idx, p, 64, 10, 100, 0.5, 0, p, p) == RQ_OK && check_mmr_search_args(&idx, p, 1, 1, 1, 1.0, 1, p, p) == RQ_OK &&
              check_mmr_search_args(&idx, p, 65535, RQ_MAX_K, RQ_MAX_K, 0.0, 0, p, p) == RQ_OK, "plain calls and the limits");
        CHECK(check_mmr_search_args(nullptr, p, 1, 1, 1, 0.5, 0, p, p) == RQ_EINVAL && check_mmr_search_args(&idx, nullptr, 1, 1, 1, 0.5, 0, p, p) == RQ_EINVAL &&
              check_mmr_search_args(&idx, p, 1, 1, 1, 0.5, 0, nullptr, p) == RQ_EINVAL && check_mmr_search_args(&idx, p, 1, 1, 1, 0.5, 0, p, nullptr) == RQ_EINVAL, "null arguments");
        CHECK(check_mmr_search_args(&idx, p, 1, 11, 10, 0.5, 0, p, p) == RQ_EINVAL && std::strstr(g_err, "fetch_k"), "k > fetch_k");
        CHECK(check_mmr_search_args(&idx, p, 1, 10, RQ_MAX_K + 1, 0.5, 0, p, p) == RQ_EINVAL, "fetch_k > RQ_MAX_K");
        CHECK(check_mmr_search_args(&idx, p, 1, 0, 10, 0.5, 0, p, p) == RQ_EINVAL && check_mmr_search_args(&idx, p, 0, 1, 10, 0.5, 0, p, p) == RQ_EINVAL, "k = 0, B = 0");
        for (double l : {-0.5, 1.5, nan}) CHECK(check_mmr_search_args(&idx, p, 1, 5, 10, l, 0, p, p) == RQ_EINVAL, "lambda = %g", l);
        CHECK(check_mmr_search_args(&idx, p, 1, 5, 10, 0.5, 7, p, p) == RQ_EINVAL, "metric");
        rq_index multi;
        multi.shards.push_back(&idx);
        CHECK(check_mmr_search_args(&multi, p, 1, 5, 10, 0.5, 0, p, p) == RQ_EUNSUPPORTED, "multi-device");
    }
    {   // ---- candidates fetched: min(fetch_k, rows in play), never fewer than k -------------------------------------------
        CHECK(mmr_fetch(10, 100, 4101) == 100 && mmr_fetch(10, 100, 100) == 100 && mmr_fetch(10, 100, 99) == 99, "clamped to the rows");
        CHECK(mmr_fetch(10, 100, 5) == 10 && mmr_fetch(10, 100, 0) == 10 && mmr_fetch(10, 10, 4101) == 10, "never below k");
        CHECK(mmr_fetch(1, RQ_MAX_K, (int64_t)1 << 40) == RQ_MAX_K, "rows beyond 32 bits");
    }
    {   // ---- geometry ------------------------------------------------------------------------------------------------------
        CHECK(RQ_MMR_THREADS % 64 == 0 && RQ_MMR_THREADS <= 1024 && RQ_MMR_ROWS_PER_ROUND == RQ_MMR_THREADS / 8, "constants");
        for (int m : {1, 63, 64, 65, 100, 257, RQ_MAX_K}) {
            const MmrGeometry g = mmr_geometry(&idx, 70, m);
            CHECK(g.grid == 70u && g.block == (unsigned)RQ_MMR_THREADS && g.dp == 768, "m = %d", m);
            CHECK((int64_t)g.rounds * RQ_MMR_ROWS_PER_ROUND >= m && (int64_t)(g.rounds - 1) * RQ_MMR_ROWS_PER_ROUND < m, "rounds %d cover m = %d exactly", g.rounds, m);
        }
        rq_index narrow;
        narrow.dim = 33; narrow.dpad = 384;
        CHECK(mmr_geometry(&narrow, 65535, 1).dp == 384 && mmr_geometry(&narrow, 65535, 1).grid == 65535u, "narrow layout, largest batch");
    }
    {   // ---- staging: B x m x 8 in 64 bits -------------------------------------------------------------------------------
        const MmrStaging s = mmr_staging(768, 65535, RQ_MAX_K, RQ_MAX_K);
        CHECK(s.cand_rows == (size_t)65535 * 1024 * 8 && s.cand_rows == 536862720ull, "B x m x 8 = %zu", s.cand_rows);
        CHECK(s.cand_scores == s.cand_rows / 2 && s.out_rows == s.cand_rows && s.out_scores == s.out_mmr && s.out_mmr == s.cand_scores, "the other arrays");
        CHECK(s.q == (size_t)65535 * 768 * 4 && s.status == (size_t)65535 * 4, "queries and status");
        const MmrStaging t = mmr_staging(33, 1, 1, 1);
        CHECK(t.q == 132 && t.cand_rows == 8 && t.cand_scores == 4 && t.status == 4 && t.out_rows == 8 && t.out_scores == 4 && t.out_mmr == 4, "the smallest call");
        // the same product formed in int arithmetic from a larger batch would wrap: B x m x 8 is taken in size_t from the first factor on
        CHECK(mmr_staging(768, 65535, RQ_MAX_K, RQ_MAX_K).cand_rows * 8 == (size_t)4294901760ull, "eight such arrays");
    }
    CHECK(idx.n == snapshot.n && idx.mmr_calls == snapshot.mmr_calls && idx.ctx.empty() && idx.filters.empty(), "the plan wrote to the index");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
