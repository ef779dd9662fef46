// Host-side check of csrc/rq_range_plan.h: the argument checks of rq_search_range*, the route of a call, the groups of queries it is
// cut into, the candidate capacity of a query and the staged bytes (64-bit arithmetic at the limits) -- plain arithmetic on a
// default-constructed rq_index, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/range_plan_check.cpp -o range_plan_check
#include "rq_range_plan.h"

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
    idx.dim = 768; idx.dpad = 768; idx.n = idx.cap = 4101; idx.max_row_norm = 1.0;
    const rq_index snapshot = idx;
    int dummy = 0;
    const void* p = &dummy;
    {   // ---- argument checks ------------------------------------------------------------------------------------------------
        const float fine[3] = {0.5f, -1.0f, 0.f};
        CHECK(check_range_args(&idx, p, 3, fine, fine, 10, 0, p, p, p) == RQ_OK, "the plain call");
        CHECK(check_range_args(&idx, p, 1, p, nullptr, 1, 1, p, p, p) == RQ_OK && check_range_args(&idx, p, 65535, p, nullptr, RQ_MAX_K, 0, p, p, p) == RQ_OK, "the limits");
        CHECK(check_range_args(nullptr, p, 1, p, nullptr, 1, 0, p, p, p) == RQ_EINVAL && std::strstr(g_err, "null"), "null index");
        CHECK(check_range_args(&idx, nullptr, 1, p, nullptr, 1, 0, p, p, p) == RQ_EINVAL && check_range_args(&idx, p, 1, nullptr, nullptr, 1, 0, p, p, p) == RQ_EINVAL &&
              check_range_args(&idx, p, 1, p, nullptr, 1, 0, nullptr, p, p) == RQ_EINVAL && check_range_args(&idx, p, 1, p, nullptr, 1, 0, p, nullptr, p) == RQ_EINVAL &&
              check_range_args(&idx, p, 1, p, nullptr, 1, 0, p, p, nullptr) == RQ_EINVAL, "null pointers");
        for (int B : {0, -1, 65536}) CHECK(check_range_args(&idx, p, B, p, nullptr, 10, 0, p, p, p) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        for (int cap : {0, -3, RQ_MAX_K + 1}) CHECK(check_range_args(&idx, p, 1, p, nullptr, cap, 0, p, p, p) == RQ_EINVAL && std::strstr(g_err, "cap "), "cap = %d", cap);
        for (int metric : {-1, 2, 7}) CHECK(check_range_args(&idx, p, 1, p, nullptr, 10, metric, p, p, p) == RQ_EINVAL && std::strstr(g_err, "metric"), "metric %d", metric);
        const float inf = std::numeric_limits<float>::infinity();
        for (float bad : {std::numeric_limits<float>::quiet_NaN(), inf, -inf}) {
            const float thr[3] = {0.5f, 0.25f, bad};
            CHECK(check_range_args(&idx, p, 3, thr, thr, 10, 0, p, p, p) == RQ_EINVAL && std::strstr(g_err, "threshold 2"), "a non-finite host threshold");
            CHECK(check_range_args(&idx, p, 2, thr, thr, 10, 0, p, p, p) == RQ_OK, "... beyond B is not read");
            CHECK(check_range_args(&idx, p, 3, thr, nullptr, 10, 0, p, p, p) == RQ_OK, "device thresholds are not read on the host");
        }
        const float big[1] = {std::numeric_limits<float>::max()};
        CHECK(check_range_args(&idx, p, 1, big, big, 10, 0, p, p, p) == RQ_OK, "FLT_MAX is finite");
        rq_index multi;
        multi.shards.push_back(&idx);
        CHECK(check_range_args(&multi, p, 1, p, nullptr, 10, 0, p, p, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED") && std::strstr(g_err, "multi-device"), "multi-device");
        CHECK(check_range_args(&multi, p, 1, p, nullptr, 0, 0, p, p, p) == RQ_EINVAL, "argument errors come first");
    }
    {   // ---- candidate capacity: the default, the hook, never below cap ------------------------------------------------------
        CHECK(RQ_RANGE_CAND_CAP == 4096 && RQ_RANGE_CAND_CAP >= RQ_MAX_K, "the default holds the largest cap");
        CHECK(range_cand_capacity(10, 0) == 4096 && range_cand_capacity(1024, 0) == 4096, "default");
        CHECK(range_cand_capacity(10, 10) == 10 && range_cand_capacity(10, 3) == 10 && range_cand_capacity(100, 64) == 100, "never below cap");
        CHECK(range_cand_capacity(10, 100000) == 100000 && range_cand_capacity(10, -5) == 4096, "the hook; a negative value is the default");
    }
    {   // ---- routes ------------------------------------------------------------------------------------------------------------
        CHECK(RROUTE_EMPTY == 0 && RROUTE_SCAN == 1 && RROUTE_GATHER == 2 && RROUTE_EXACT == 3, "the documented numbers");
        rq_index empty;
        empty.dim = 33; empty.dpad = 384;
        for (int forced : {-1, 1, 2, 3}) CHECK(plan_range(&empty, nullptr, 3, 0, forced) == RROUTE_EMPTY, "an empty index, forced %d", forced);
        for (int B : {1, 64, 130, 65535})
            for (int metric : {0, 1}) {
                CallPlan cp;
                CHECK(plan_range(&idx, nullptr, B, metric, -1, &cp) == RROUTE_SCAN, "the rule, B = %d", B);
                CHECK(!cp.exact && !cp.use8 && cp.nbins == 65 && cp.bpad >= std::min(B, RQ_RANGE_GROUP) && cp.bpad % 64 == 0, "the scan route's call plan, B = %d", B);
                CHECK(plan_range(&idx, nullptr, B, metric, 1) == RROUTE_SCAN && plan_range(&idx, nullptr, B, metric, 3) == RROUTE_EXACT, "forced, B = %d", B);
                CHECK(plan_range(&idx, nullptr, B, metric, 2) == RROUTE_SCAN, "an unfiltered call has no list to gather");
            }
        // 70 rows: two bins.  A top-k would scan exactly (fewer than two bins per wanted bin); a range search wants no bin
        rq_index small = idx;
        small.n = small.cap = 70;
        CHECK(plan_range(&small, nullptr, 3, 0, -1) == RROUTE_SCAN, "a tiny shard is still scanned");
        // a shard whose scan scores say nothing (fp16-subnormal rows): the exact route, also when the scan is forced
        rq_index sub = idx;
        sub.max_sub_rel = 0.2;
        CHECK(plan_range(&sub, nullptr, 3, 0, -1) == RROUTE_EXACT && plan_range(&sub, nullptr, 3, 0, 1) == RROUTE_EXACT, "eps beyond use");
        CHECK(plan_range(&sub, nullptr, 3, 1, -1) == RROUTE_SCAN, "... for the metric it concerns only");
        sub.eps = 0.01;
        CHECK(plan_range(&sub, nullptr, 3, 0, -1) == RROUTE_SCAN, "an explicit eps is taken at its word");
        // filters: occupancy is not needed, only n and na
        auto shape = [&](int64_t na) { FilterShape f; f.n = 4101; f.na = na; return f; };
        const FilterShape none = shape(0), sparse = shape(30), quarter = shape(1025), over = shape(1026), most = shape(4000), edge = shape(64);
        for (int forced : {-1, 1, 2, 3}) CHECK(plan_range(&idx, &none, 3, 0, forced) == RROUTE_EMPTY, "no row allowed, forced %d", forced);
        CHECK(plan_range(&idx, &sparse, 64, 0, -1) == RROUTE_GATHER, "64 x 30 <= 4101");
        CHECK(plan_range(&idx, &sparse, 130, 0, -1) == RROUTE_GATHER && plan_range(&idx, &sparse, 137, 0, -1) == RROUTE_SCAN, "B x na against n: 3900, 4110");
        CHECK(plan_range(&idx, &edge, 64, 0, -1) == RROUTE_GATHER && plan_range(&idx, &edge, 65, 0, -1) == RROUTE_SCAN, "64 x 64 = 4096 <= 4101 < 65 x 64");
        CHECK(plan_range(&idx, &quarter, 1, 0, -1) == RROUTE_GATHER && plan_range(&idx, &over, 1, 0, -1) == RROUTE_SCAN, "the list fits up to a quarter of the rows");
        CHECK(plan_range(&idx, &most, 1, 0, -1) == RROUTE_SCAN, "most rows allowed");
        for (const FilterShape* f : {&sparse, &quarter, &most})
            CHECK(plan_range(&idx, f, 3, 0, 1) == RROUTE_SCAN && plan_range(&idx, f, 3, 0, 2) == RROUTE_GATHER && plan_range(&idx, f, 3, 0, 3) == RROUTE_EXACT, "forced routes");
        CHECK(plan_range(&sub, &most, 3, 0, -1) == RROUTE_SCAN && plan_range(&sub, &sparse, 3, 0, -1) == RROUTE_GATHER, "(sub.eps is explicit now)");
        sub.eps = -1;
        CHECK(plan_range(&sub, &most, 3, 0, -1) == RROUTE_EXACT && plan_range(&sub, &sparse, 3, 0, -1) == RROUTE_GATHER, "gather needs no scan scores");
    }
    {   // ---- groups ------------------------------------------------------------------------------------------------------------
        CHECK(RQ_RANGE_GROUP == 1024, "the documented group");
        struct { int route, B; int64_t per; int group, count; } want[] = {
            {RROUTE_SCAN, 1, 0, 1, 1}, {RROUTE_SCAN, 130, 0, 130, 1}, {RROUTE_SCAN, 1024, 0, 1024, 1}, {RROUTE_SCAN, 1025, 0, 1024, 2}, {RROUTE_SCAN, 65535, 0, 1024, 64},
            {RROUTE_EXACT, 64, 4160, 64, 1}, {RROUTE_EXACT, 65535, 4160, 1024, 64}, {RROUTE_EXACT, 64, 1000000, 64, 1}, {RROUTE_EXACT, 500, 1000000, 134, 4},
            {RROUTE_EXACT, 3, (int64_t)1 << 28, 1, 3}, {RROUTE_GATHER, 64, 30, 64, 1}, {RROUTE_GATHER, 2000, 1 << 20, 128, 16}};
        for (const auto& w : want) {
            const RangeGroups g = range_groups(w.route, w.B, w.per);
            CHECK(g.group == w.group && g.count == w.count, "route %d B %d per %lld: group %d count %d", w.route, w.B, (long long)w.per, g.group, g.count);
            CHECK(g.group >= 1 && g.group <= RQ_RANGE_GROUP && (int64_t)g.group * g.count >= w.B && (int64_t)g.group * (g.count - 1) < w.B, "the groups cover B = %d exactly", w.B);
            if (w.route != RROUTE_SCAN && g.group > 1) CHECK((int64_t)g.group * w.per * 8 <= ((int64_t)1 << 30), "keys within 1 GiB");
        }
        CHECK(RQ_RANGE_CHUNK == 2048 && range_chunks(1) == 1u && range_chunks(2048) == 1u && range_chunks(2049) == 2u && range_chunks(15625) == 8u, "chunks of the tail");
        CHECK(range_chunks(((int64_t)1 << 32) / 64) == 32768u, "the largest shard stays within a grid's y");
    }
    {   // ---- staging: B x (dim x 4 + 4 + cap x 12 + 12) in 64 bits -----------------------------------------------------------
        const RangeStaging s = range_staging(768, 65535, RQ_MAX_K);
        CHECK(s.q == (size_t)65535 * 768 * 4 && s.thr == (size_t)65535 * 4 && s.scores == (size_t)65535 * 1024 * 4 && s.rows == (size_t)65535 * 1024 * 8 &&
              s.count == (size_t)65535 * 8 && s.status == (size_t)65535 * 4, "the largest call");
        CHECK(s.total() == (size_t)65535 * (768 * 4 + 1024 * 12 + 16), "total %zu", s.total());
        const RangeStaging t = range_staging(33, 1, 1);
        CHECK(t.q == 132 && t.thr == 4 && t.scores == 4 && t.rows == 8 && t.count == 8 && t.status == 4 && t.total() == 160, "the smallest call");
        CHECK(range_staging(1, 65535, 1024).rows == (size_t)536862720, "B x cap x 8 = %zu", range_staging(1, 65535, 1024).rows);
    }
    CHECK(idx.n == snapshot.n && idx.range_route == snapshot.range_route && idx.range_route_last == snapshot.range_route_last && idx.range_calls == snapshot.range_calls &&
          idx.range_cand_cap == snapshot.range_cand_cap && idx.ctx.empty() && idx.filters.empty(), "the plan wrote to the index");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
