// Host-side check of csrc/rq_score_plan.h: the argument checks of rq_score_rows_device and rq_score_rows, the groups of queries a
// call is cut into, the launch geometry and the staged bytes (64-bit arithmetic at the limits) -- plain arithmetic on a
// default-constructed rq_index, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/score_plan_check.cpp -o score_plan_check
#include "rq_score_plan.h"

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
    {   // ---- argument checks ------------------------------------------------------------------------------------------------
        CHECK(RQ_MAX_SCORE_ROWS == 65536, "the documented limit");
        CHECK(check_score_args(&idx, p, 64, p, 100, 0, p) == RQ_OK, "the plain call");
        CHECK(check_score_args(&idx, p, 1, p, 1, 1, p) == RQ_OK && check_score_args(&idx, p, 65535, p, RQ_MAX_SCORE_ROWS, 0, p) == RQ_OK, "the limits");
        CHECK(check_score_args(nullptr, p, 1, p, 1, 0, p) == RQ_EINVAL && std::strstr(g_err, "null"), "null index");
        CHECK(check_score_args(&idx, nullptr, 1, p, 1, 0, p) == RQ_EINVAL && check_score_args(&idx, p, 1, nullptr, 1, 0, p) == RQ_EINVAL &&
              check_score_args(&idx, p, 1, p, 1, 0, nullptr) == RQ_EINVAL, "null pointers");
        for (int B : {0, -1, 65536}) CHECK(check_score_args(&idx, p, B, p, 10, 0, p) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        for (int m : {0, -3, RQ_MAX_SCORE_ROWS + 1}) CHECK(check_score_args(&idx, p, 1, p, m, 0, p) == RQ_EINVAL && std::strstr(g_err, "m "), "m = %d", m);
        for (int metric : {-1, 2, 7}) CHECK(check_score_args(&idx, p, 1, p, 10, metric, p) == RQ_EINVAL && std::strstr(g_err, "metric"), "metric %d", metric);
        rq_index empty;
        empty.dim = 33; empty.dpad = 384;
        CHECK(check_score_args(&empty, p, 3, p, 7, 0, p) == RQ_OK, "an empty index is scored (every entry absent)");
        rq_index multi;
        multi.shards.push_back(&idx);
        CHECK(check_score_args(&multi, p, 1, p, 10, 0, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED") && std::strstr(g_err, "multi-device"), "multi-device");
        CHECK(check_score_args(&multi, p, 1, p, 0, 0, p) == RQ_EINVAL, "argument errors come first");
    }
    {   // ---- groups of at most 1 024 queries, slots a multiple of 64 ----------------------------------------------------------
        CHECK(RQ_SCORE_GROUP == 1024, "the documented group");
        struct { int B, group, count, slots; } want[] = {{1, 1, 1, 64}, {63, 63, 1, 64}, {64, 64, 1, 64}, {65, 65, 1, 128}, {70, 70, 1, 128},
                                                         {1024, 1024, 1, 1024}, {1025, 1024, 2, 1024}, {2048, 1024, 2, 1024}, {65535, 1024, 64, 1024}};
        for (const auto& w : want) {
            const ScoreGroups g = score_groups(w.B);
            CHECK(g.group == w.group && g.count == w.count && g.slots == w.slots, "B = %d: group %d count %d slots %d", w.B, g.group, g.count, g.slots);
            CHECK(g.slots % 64 == 0 && g.slots >= g.group && g.slots <= RQ_SCORE_GROUP, "B = %d: slots", w.B);
            // the groups cover the queries exactly, the last one may be short
            int covered = 0, last = 0;
            for (int i = 0; i < g.count; ++i) { last = std::min(g.group, w.B - i * g.group); CHECK(last >= 1, "B = %d: empty group %d", w.B, i); covered += last; }
            CHECK(covered == w.B, "B = %d: %d queries covered", w.B, covered);
        }
        CHECK(65535 - 63 * 1024 == 1023, "the last group of the largest batch holds 1 023 queries");
    }
    {   // ---- geometry: (queries, tiles of the list) x 256 threads ----------------------------------------------------------
        CHECK(RQ_SCORE_THREADS == 256 && RQ_SCORE_TILE % 32 == 0 && RQ_SCORE_TILE >= 32, "4 waves x 8 positions per round, whole rounds per tile");
        for (int m : {1, 63, 64, 65, 100, 1500, RQ_MAX_SCORE_ROWS}) {
            const ScoreGeometry g = score_geometry(&idx, 70, m);
            CHECK(g.grid_x == 70u && g.block == 256u && g.dp == 768, "m = %d", m);
            CHECK((int64_t)g.grid_y * RQ_SCORE_TILE >= m && (int64_t)(g.grid_y - 1) * RQ_SCORE_TILE < m, "%u tiles cover m = %d exactly", g.grid_y, m);
            CHECK(g.grid_y >= 1 && g.grid_y <= 65535u, "grid y %u within the launch limit", g.grid_y);
        }
        CHECK(score_geometry(&idx, 1, 1).grid_y == 1u && score_geometry(&idx, 1, 64).grid_y == (unsigned)(64 / RQ_SCORE_TILE) &&
              score_geometry(&idx, 1, 65).grid_y == (unsigned)((65 + RQ_SCORE_TILE - 1) / RQ_SCORE_TILE) &&
              score_geometry(&idx, 1, 65536).grid_y == (unsigned)(65536 / RQ_SCORE_TILE), "m = 1, 64, 65, 65 536");
        rq_index narrow;
        narrow.dim = 33; narrow.dpad = 384;
        CHECK(score_geometry(&narrow, 1024, 1).dp == 384 && score_geometry(&narrow, 1024, 1).grid_x == 1024u, "narrow layout, a whole group");
    }
    {   // ---- staging: B x dim x 4 + B x m x 12 in 64 bits -----------------------------------------------------------------
        const ScoreStaging s = score_staging(768, 65535, RQ_MAX_SCORE_ROWS);
        CHECK(s.rows == (size_t)65535 * 65536 * 8 && s.rows == 34359214080ull, "B x m x 8 = %zu", s.rows);     // beyond 2^32, beyond 2^35 - 2^19
        CHECK(s.scores == s.rows / 2 && s.q == (size_t)65535 * 768 * 4, "scores and queries");
        CHECK(s.total() == (size_t)65535 * 768 * 4 + (size_t)65535 * 65536 * 12, "total %zu", s.total());
        const ScoreStaging t = score_staging(33, 1, 1);
        CHECK(t.q == 132 && t.rows == 8 && t.scores == 4 && t.total() == 144, "the smallest call");
        const ScoreStaging u = score_staging(768, 500, 100);
        CHECK(u.total() == (size_t)500 * 768 * 4 + (size_t)500 * 100 * 12, "the hybrid batch: %zu bytes", u.total());
        // the same product formed in int arithmetic would wrap: 32 768 x 65 536 x 4 = 2^33
        CHECK(score_staging(1, 32768, 65536).scores == ((size_t)1 << 33), "B x m x 4 past 32 bits");
    }
    CHECK(idx.n == snapshot.n && idx.score_calls == snapshot.score_calls && idx.score_pairs == snapshot.score_pairs && idx.ctx.empty() && idx.filters.empty(),
          "the plan wrote to the index");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
