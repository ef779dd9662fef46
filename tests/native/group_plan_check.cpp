// Host-side check of csrc/rq_group_plan.h: the argument checks of rq_index_set_groups, rq_group_collapse_device and
// rq_search_grouped*, the rows each rung fetches at its clamps, the launch geometry and the staged bytes (64-bit arithmetic at the
// limits) -- plain arithmetic on a default-constructed rq_index, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/group_plan_check.cpp -o group_plan_check
#include "rq_group_plan.h"

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
    rq_index multi;
    multi.shards.push_back(&idx);
    {   // ---- rq_index_set_groups / rq_index_get_groups ----------------------------------------------------------------------
        CHECK(check_group_range(&idx, 0, 4101, p) == RQ_OK && check_group_range(&idx, 4100, 1, p) == RQ_OK && check_group_range(&idx, 4101, 0, p) == RQ_OK, "whole range, last row, empty tail");
        CHECK(check_group_range(&idx, 0, 0, nullptr) == RQ_OK, "nothing to write needs no array");
        CHECK(check_group_range(nullptr, 0, 1, p) == RQ_EINVAL && check_group_range(&idx, 0, 1, nullptr) == RQ_EINVAL && std::strstr(g_err, "null"), "null arguments");
        CHECK(check_group_range(&idx, -1, 1, p) == RQ_EINVAL && check_group_range(&idx, 0, -1, p) == RQ_EINVAL, "negative begin / count");
        CHECK(check_group_range(&idx, 4100, 2, p) == RQ_EINVAL && check_group_range(&idx, 4102, 0, p) == RQ_EINVAL && check_group_range(&idx, 0, 4102, p) == RQ_EINVAL, "beyond the stored rows");
        const int64_t big = std::numeric_limits<int64_t>::max();
        CHECK(check_group_range(&idx, 1, big, p) == RQ_EINVAL && check_group_range(&idx, big, 1, p) == RQ_EINVAL && check_group_range(&idx, big, big, p) == RQ_EINVAL, "no overflow in begin + count");
        CHECK(check_group_range(&multi, 0, 1, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED"), "multi-device");
        const int32_t good[5] = {0, RQ_GROUP_NONE, 7, std::numeric_limits<int32_t>::max(), 7};
        const int32_t bad[3] = {0, -2, 1};
        CHECK(check_group_ids(good, 5) == RQ_OK && check_group_ids(good, 0) == RQ_OK, "ids 0, 2^31 - 1 and RQ_GROUP_NONE");
        CHECK(check_group_ids(bad, 3) == RQ_EINVAL && std::strstr(g_err, "row 1") && check_group_ids(bad, 1) == RQ_OK, "an id below RQ_GROUP_NONE names its row");
    }
    {   // ---- rq_group_collapse_device ------------------------------------------------------------------------------------------
        CHECK(check_group_collapse_args(&idx, p, p, 64, 100, 10, p, p, p, p) == RQ_OK, "the plain call");
        CHECK(check_group_collapse_args(&idx, p, p, 1, 1, 1, p, p, p, p) == RQ_OK && check_group_collapse_args(&idx, p, p, 65535, RQ_MAX_K, RQ_MAX_K, p, p, p, p) == RQ_OK, "the limits");
        CHECK(check_group_collapse_args(nullptr, p, p, 1, 1, 1, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "null"), "null index");
        CHECK(check_group_collapse_args(&idx, nullptr, p, 1, 1, 1, p, p, p, p) == RQ_EINVAL && check_group_collapse_args(&idx, p, nullptr, 1, 1, 1, p, p, p, p) == RQ_EINVAL &&
              check_group_collapse_args(&idx, p, p, 1, 1, 1, nullptr, p, p, p) == RQ_EINVAL && check_group_collapse_args(&idx, p, p, 1, 1, 1, p, nullptr, p, p) == RQ_EINVAL &&
              check_group_collapse_args(&idx, p, p, 1, 1, 1, p, p, nullptr, p) == RQ_EINVAL && check_group_collapse_args(&idx, p, p, 1, 1, 1, p, p, p, nullptr) == RQ_EINVAL, "null pointers");
        for (int B : {0, -1, 65536}) CHECK(check_group_collapse_args(&idx, p, p, B, 10, 5, p, p, p, p) == RQ_EINVAL, "B = %d", B);
        for (int m : {0, -3, RQ_MAX_K + 1}) CHECK(check_group_collapse_args(&idx, p, p, 1, m, 1, p, p, p, p) == RQ_EINVAL, "m = %d", m);
        for (int k : {0, -1, 11}) CHECK(check_group_collapse_args(&idx, p, p, 1, 10, k, p, p, p, p) == RQ_EINVAL, "k = %d of m = 10", k);
        CHECK(check_group_collapse_args(&multi, p, p, 1, 10, 5, p, p, p, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED"), "multi-device");
        CHECK(check_group_collapse_args(&multi, p, p, 1, 10, 50, p, p, p, p) == RQ_EINVAL, "argument errors come first");
    }
    {   // ---- rq_search_grouped* -----------------------------------------------------------------------------------------------
        CHECK(check_group_search_args(&idx, p, 64, 10, 0, p, p, p) == RQ_OK && check_group_search_args(&idx, p, 1, 1, 1, p, p, p) == RQ_OK &&
              check_group_search_args(&idx, p, 65535, RQ_MAX_K, 0, p, p, p) == RQ_OK, "plain calls and the limits");
        CHECK(check_group_search_args(nullptr, p, 1, 1, 0, p, p, p) == RQ_EINVAL && check_group_search_args(&idx, nullptr, 1, 1, 0, p, p, p) == RQ_EINVAL &&
              check_group_search_args(&idx, p, 1, 1, 0, nullptr, p, p) == RQ_EINVAL && check_group_search_args(&idx, p, 1, 1, 0, p, nullptr, p) == RQ_EINVAL &&
              check_group_search_args(&idx, p, 1, 1, 0, p, p, nullptr) == RQ_EINVAL, "null arguments");
        for (int k : {0, -1, RQ_MAX_K + 1}) CHECK(check_group_search_args(&idx, p, 1, k, 0, p, p, p) == RQ_EINVAL, "k = %d", k);
        for (int B : {0, 65536}) CHECK(check_group_search_args(&idx, p, B, 1, 0, p, p, p) == RQ_EINVAL, "B = %d", B);
        for (int metric : {-1, 2, 7}) CHECK(check_group_search_args(&idx, p, 1, 5, metric, p, p, p) == RQ_EINVAL, "metric %d", metric);
        CHECK(check_group_search_args(&multi, p, 1, 5, 0, p, p, p) == RQ_EUNSUPPORTED, "multi-device");
    }
    {   // ---- the fetch rule: "group_fetch" x k within [k, min(rows in play, "group_fetch_cap" or RQ_MAX_K)] --------------------
        CHECK(group_fetch(10, 4, 0, 4101) == 40 && group_fetch(10, 1, 0, 4101) == 10 && group_fetch(10, 8, 0, 4101) == 80, "the multiple");
        CHECK(group_fetch(10, 4, 0, 39) == 39 && group_fetch(10, 4, 0, 40) == 40 && group_fetch(10, 4, 0, 10) == 10, "clamped to the rows in play");
        CHECK(group_fetch(10, 4, 0, 5) == 10 && group_fetch(10, 4, 0, 0) == 10 && group_fetch(10, 0, 0, 4101) == 10 && group_fetch(10, -3, 0, 4101) == 10, "never below k");
        CHECK(group_fetch(300, 4, 0, 1 << 20) == RQ_MAX_K && group_fetch(RQ_MAX_K, RQ_MAX_K, 0, (int64_t)1 << 40) == RQ_MAX_K, "clamped to RQ_MAX_K, the product in 64 bits");
        CHECK(group_fetch(5, 4, 64, 4101) == 20 && group_fetch(20, 4, 64, 4101) == 64 && group_fetch(100, 4, 64, 4101) == 100, "the cap, which never goes below k");
        CHECK(group_fetch(5, 4, 5000, 4101) == 20 && group_max_fetch(5, 5000, 1 << 20) == RQ_MAX_K, "a cap beyond RQ_MAX_K is RQ_MAX_K");
        CHECK(group_max_fetch(5, 0, 4101) == RQ_MAX_K && group_max_fetch(5, 0, 1000) == 1000 && group_max_fetch(5, 64, 4101) == 64 && group_max_fetch(5, 64, 3) == 5 &&
              group_max_fetch(100, 64, 4101) == 100 && group_max_fetch(1, 0, (int64_t)1 << 40) == RQ_MAX_K, "the widest rung");
    }
    {   // ---- geometry ------------------------------------------------------------------------------------------------------------
        CHECK(RQ_GROUP_THREADS % 64 == 0 && RQ_GROUP_THREADS <= 1024 && RQ_GROUP_THREADS * 2 >= RQ_MAX_K && (RQ_GROUP_MIN_SORT & (RQ_GROUP_MIN_SORT - 1)) == 0, "constants");
        const int ms[7] = {1, 63, 64, 65, 257, 1000, RQ_MAX_K}, want[7] = {64, 64, 64, 128, 512, 1024, 1024};
        for (int i = 0; i < 7; ++i) {
            const GroupGeometry g = group_geometry(70, ms[i]);
            CHECK(g.grid == 70u && g.block == (unsigned)RQ_GROUP_THREADS && g.sort_n == want[i], "m = %d sorts %d slots", ms[i], g.sort_n);
            CHECK(g.sort_n >= ms[i] && g.sort_n <= RQ_MAX_K && g.lds_bytes == (size_t)g.sort_n * 12 && g.lds_bytes <= 64 * 1024, "LDS of m = %d", ms[i]);
        }
        CHECK(group_geometry(65535, 1).grid == 65535u, "largest batch");
    }
    {   // ---- staging: B x m x 8 in 64 bits -------------------------------------------------------------------------------------
        const GroupStaging s = group_staging(768, 65535, RQ_MAX_K, RQ_MAX_K);
        CHECK(s.cand_rows == (size_t)65535 * 1024 * 8 && s.cand_rows == 536862720ull, "B x m x 8 = %zu", s.cand_rows);
        CHECK(s.cand_scores == s.cand_rows / 2 && s.out_rows == s.cand_rows && s.out_keys == s.cand_rows && s.out_scores == s.cand_scores && s.out_groups == s.cand_scores, "the other arrays");
        CHECK(s.q == (size_t)65535 * 768 * 4 && s.status == (size_t)65535 * 4 && s.cand_status == s.status, "queries and status");
        const GroupStaging t = group_staging(33, 1, 4, 1);
        CHECK(t.q == 132 && t.cand_rows == 32 && t.cand_scores == 16 && t.cand_status == 4 && t.out_rows == 8 && t.out_scores == 4 && t.out_groups == 4 && t.out_keys == 8 && t.status == 4, "a small call");
        CHECK(s.cand_rows * 8 == (size_t)4294901760ull, "eight such arrays pass 2^32");
    }
    CHECK(idx.n == snapshot.n && idx.group_calls == snapshot.group_calls && idx.group_fetch == 8 && idx.group_fetch_cap == 0 && idx.h_groups.empty() && !idx.d_groups &&
          idx.ctx.empty() && idx.filters.empty(), "the plan wrote to the index");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
