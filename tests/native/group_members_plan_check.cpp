// Host-side check of csrc/rq_group_members_plan.h: the argument checks of rq_group_fill_device and rq_search_group_members*, the
// launch geometry of the fill kernel (sort sizes at the powers of two and one either side), the staged bytes (64-bit arithmetic at
// the limits) and the group member table against brute force -- plain arithmetic on a default-constructed rq_index, so it runs
// without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/group_members_plan_check.cpp -o group_members_plan_check
#include "rq_group_members_plan.h"

#include <limits>
#include <random>

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

// The table of `groups` against brute force: every id's rows are exactly the rows carrying it, ascending; the ids are the distinct
// ids >= 0, ascending; every lookup finds its id and no other.
static void check_table(const std::vector<int32_t>& groups, const char* what) {
    GroupTable t;
    group_table_build(groups.data(), (int64_t)groups.size(), t);
    std::map<int32_t, std::vector<uint32_t>> brute;
    for (size_t r = 0; r < groups.size(); ++r)
        if (groups[r] >= 0) brute[groups[r]].push_back((uint32_t)r);
    size_t grouped = 0, largest = 0;
    for (const auto& kv : brute) { grouped += kv.second.size(); largest = std::max(largest, kv.second.size()); }
    CHECK(t.ids.size() == brute.size() && t.off.size() == brute.size() + 1 && t.rows.size() == grouped && t.largest == (int64_t)largest, "%s: sizes", what);
    CHECK(t.off.front() == 0 && t.off.back() == grouped, "%s: the offsets span the rows", what);
    size_t i = 0;
    for (const auto& kv : brute) {
        if (i >= t.ids.size()) break;
        CHECK(t.ids[i] == kv.first, "%s: id %zu", what, i);
        const std::vector<uint32_t> mine(t.rows.begin() + t.off[i], t.rows.begin() + t.off[i + 1]);
        CHECK(mine == kv.second, "%s: the rows of id %d", what, (int)kv.first);
        CHECK(group_table_find(t.ids.data(), (int64_t)t.ids.size(), kv.first) == (int64_t)i, "%s: the lookup of id %d", what, (int)kv.first);
        ++i;
    }
    for (int32_t g : {0, 1, 7, 1000003, std::numeric_limits<int32_t>::max() - 1, std::numeric_limits<int32_t>::max()})
        if (!brute.count(g)) CHECK(group_table_find(t.ids.data(), (int64_t)t.ids.size(), g) == -1, "%s: id %d is carried by no row", what, (int)g);
}

int main() {
    rq_index idx;
    idx.dim = 768; idx.dpad = 768; idx.n = idx.cap = 4101;
    const rq_index snapshot = idx;
    int dummy = 0;
    const void* p = &dummy;
    rq_index multi;
    multi.shards.push_back(&idx);
    {   // ---- the argument checks ---------------------------------------------------------------------------------------------
        CHECK(check_group_members_args(&idx, p, 64, 10, 3, 0, p, p, p, p, p) == RQ_OK && check_group_members_args(&idx, p, 1, 1, 1, 1, p, p, p, p, p) == RQ_OK, "plain calls");
        CHECK(check_group_members_args(&idx, p, 65535, 128, 8, 0, p, p, p, p, p) == RQ_OK && check_group_members_args(&idx, p, 1, RQ_MAX_K, 1, 0, p, p, p, p, p) == RQ_OK &&
              check_group_members_args(&idx, p, 1, 1, RQ_MAX_K, 0, p, p, p, p, p) == RQ_OK, "k x s = RQ_MAX_K exactly");
        CHECK(check_group_members_args(&idx, p, 1, 1025, 1, 0, p, p, p, p, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 205, 5, 0, p, p, p, p, p) == RQ_EINVAL &&
              check_group_members_args(&idx, p, 1, 1, 1025, 0, p, p, p, p, p) == RQ_EINVAL, "k x s = 1025");
        const int big = std::numeric_limits<int>::max();
        CHECK(check_group_members_args(&idx, p, 1, big, big, 0, p, p, p, p, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 65536, 65536, 0, p, p, p, p, p) == RQ_EINVAL,
              "the product in 64 bits (65536 x 65536 wraps to 0 in 32)");
        for (int v : {0, -1}) CHECK(check_group_members_args(&idx, p, 1, v, 2, 0, p, p, p, p, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 2, v, 0, p, p, p, p, p) == RQ_EINVAL, "k / s = %d", v);
        for (int B : {0, -1, 65536}) CHECK(check_group_members_args(&idx, p, B, 2, 2, 0, p, p, p, p, p) == RQ_EINVAL, "B = %d", B);
        for (int metric : {-1, 2, 7}) CHECK(check_group_members_args(&idx, p, 1, 2, 2, metric, p, p, p, p, p) == RQ_EINVAL, "metric %d", metric);
        CHECK(check_group_members_args(nullptr, p, 1, 2, 2, 0, p, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "null"), "null index");
        CHECK(check_group_members_args(&idx, nullptr, 1, 2, 2, 0, p, p, p, p, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 2, 2, 0, nullptr, p, p, p, p) == RQ_EINVAL &&
              check_group_members_args(&idx, p, 1, 2, 2, 0, p, nullptr, p, p, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 2, 2, 0, p, p, nullptr, p, p) == RQ_EINVAL &&
              check_group_members_args(&idx, p, 1, 2, 2, 0, p, p, p, nullptr, p) == RQ_EINVAL && check_group_members_args(&idx, p, 1, 2, 2, 0, p, p, p, p, nullptr) == RQ_EINVAL, "null pointers");
        CHECK(check_group_members_args(&multi, p, 1, 2, 2, 0, p, p, p, p, p) == RQ_EUNSUPPORTED && std::strstr(g_err, "RQ_EUNSUPPORTED"), "multi-device");
        CHECK(check_group_members_args(&multi, p, 1, 2, 1000, 0, p, p, p, p, p) == RQ_EINVAL, "argument errors come first");
    }
    {   // ---- the cap and the geometry ------------------------------------------------------------------------------------------
        CHECK(RQ_GROUP_FILL_THREADS % 64 == 0 && (RQ_GROUP_FILL_MAX & (RQ_GROUP_FILL_MAX - 1)) == 0 && (RQ_GROUP_FILL_MIN_SORT & (RQ_GROUP_FILL_MIN_SORT - 1)) == 0 &&
              RQ_GROUP_FILL_MAX * sizeof(uint64_t) == 32 * 1024, "constants");
        CHECK(group_fill_cap(0) == RQ_GROUP_FILL_MAX && group_fill_cap(-5) == RQ_GROUP_FILL_MAX && group_fill_cap(16) == 16 && group_fill_cap(1) == 1 &&
              group_fill_cap(RQ_GROUP_FILL_MAX) == RQ_GROUP_FILL_MAX && group_fill_cap(RQ_GROUP_FILL_MAX + 1) == RQ_GROUP_FILL_MAX && group_fill_cap(1 << 30) == RQ_GROUP_FILL_MAX,
              "the option can only lower the maximum");
        const int64_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, (int64_t)1 << 40};
        const int want[] = {64, 64, 64, 64, 128, 128, 128, 256, 256, 256, 512, 512, 512, 1024, 1024, 1024, 2048, 2048, 2048, 4096, 4096, 4096, 4096, 4096};
        for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
            const GroupFillGeometry g = group_fill_geometry(70, 10, sizes[i], 0);
            CHECK(g.grid_x == 10u && g.grid_y == 70u && g.block == (unsigned)RQ_GROUP_FILL_THREADS && g.sort_n == want[i], "largest group %lld sorts %d slots", (long long)sizes[i], g.sort_n);
            CHECK((g.sort_n & (g.sort_n - 1)) == 0 && g.sort_n <= RQ_GROUP_FILL_MAX && (g.sort_n >= sizes[i] || g.sort_n == RQ_GROUP_FILL_MAX) && g.lds_bytes == 3072 + (size_t)g.sort_n * 8 &&
                  g.lds_bytes <= 35 * 1024 && g.lds_bytes % 16 == 0, "LDS of a largest group of %lld", (long long)sizes[i]);
        }
        CHECK(group_fill_geometry(1, 1, 5000, 16).sort_n == 64 && group_fill_geometry(1, 1, 5000, 65).sort_n == 128 && group_fill_geometry(1, 1, 40, 1000).sort_n == 64 &&
              group_fill_geometry(1, 1, 5000, 1000).sort_n == 1024, "the cap bounds the sort");
        const GroupFillGeometry lim = group_fill_geometry(65535, RQ_MAX_K, 1, 0);
        CHECK(lim.grid_x == 1024u && lim.grid_y == 65535u, "largest grid");
    }
    {   // ---- staging: B x k x s x 8 in 64 bits --------------------------------------------------------------------------------
        const GroupMembersStaging z = group_members_staging(768, 65535, 128, 8);
        CHECK(z.rows == (size_t)65535 * 1024 * 8 && z.rows == 536862720ull && z.scores == z.rows / 2, "B x k x s x 8 = %zu", z.rows);
        CHECK(z.groups == (size_t)65535 * 128 * 4 && z.count == z.groups && z.win_scores == z.groups && z.win_rows == 2 * z.groups, "the per-slot arrays");
        CHECK(z.q == (size_t)65535 * 768 * 4 && z.status == (size_t)65535 * 4, "queries and status");
        CHECK(z.rows * 8 == (size_t)4294901760ull, "eight such arrays pass 2^32");
        const GroupMembersStaging t = group_members_staging(33, 1, 2, 3);
        CHECK(t.q == 132 && t.scores == 24 && t.rows == 48 && t.groups == 8 && t.count == 8 && t.status == 4 && t.win_scores == 8 && t.win_rows == 16, "a small call");
    }
    {   // ---- the member table against brute force -------------------------------------------------------------------------------
        const int32_t top = std::numeric_limits<int32_t>::max();
        check_table({}, "an empty index");
        check_table(std::vector<int32_t>(100, RQ_GROUP_NONE), "every row RQ_GROUP_NONE");
        check_table(std::vector<int32_t>(100, 5), "every row in one group");
        check_table(std::vector<int32_t>(70, top), "every row in group 2^31 - 1");
        check_table({0, top, RQ_GROUP_NONE, 0, top, 7, RQ_GROUP_NONE, 0}, "ids 0 and 2^31 - 1");
        check_table({top}, "one row");
        check_table({RQ_GROUP_NONE}, "one ungrouped row");
        std::mt19937 rng(11);
        std::vector<int32_t> sparse(5000), runs(4101), dense(3000);
        for (auto& g : sparse) { const uint32_t v = rng(); g = v % 10 == 0 ? RQ_GROUP_NONE : (int32_t)((v % 600) * 3571427u % (uint32_t)top); }   // sparse ids over the whole range
        sparse[0] = 0; sparse[1] = top; sparse[4999] = top;
        for (size_t r = 0; r < runs.size(); ++r) runs[r] = (int32_t)(r / 8);
        for (auto& g : dense) g = (int32_t)(rng() % 40) - 1;
        check_table(sparse, "sparse ids");
        check_table(runs, "runs of 8");
        check_table(dense, "few large groups");
        GroupTable t;
        group_table_build(runs.data(), (int64_t)runs.size(), t);
        CHECK(t.ids.size() == 513 && t.largest == 8 && t.off[512] == 4096 && t.off[513] == 4101, "runs of 8 over 4101 rows: 512 full groups and one of 5");
        group_table_build(runs.data(), 0, t);   // (a table is rebuilt in place)
        CHECK(t.ids.empty() && t.rows.empty() && t.off.size() == 1 && t.off[0] == 0 && t.largest == 0, "rebuilt over no rows");
        CHECK(group_table_find(nullptr, 0, 3) == -1, "a lookup in an empty table");
    }
    CHECK(idx.n == snapshot.n && idx.group_fill_calls == 0 && idx.group_table_builds == 0 && idx.group_fill_cap == 0 && !idx.gt_valid && !idx.gt_ids && idx.h_groups.empty() &&
          idx.ctx.empty() && idx.filters.empty(), "the plan wrote to the index");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
