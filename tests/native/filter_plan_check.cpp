// Host-side check of the route rule of filtered searches (csrc/rq_filter_plan.h): plain arithmetic on the index's fields, the
// call's arguments and the filter's recorded occupancy, so it runs here on a default-constructed rq_index without a GPU and can
// be built under the host sanitizers.  Expectations are worked out by hand from the rule the header states; the
// sweep at the end recounts the occupied partitions of every scan decision from the definition (bin -> scan workgroup ->
// partition) instead of plan_filter's own loop.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/filter_plan_check.cpp -o filter_plan_check
#include "rq_filter_plan.h"

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

static void fp16_index(rq_index& idx, int64_t n) { idx.dim = 768; idx.dpad = 768; idx.n = idx.cap = n; }

// A filter's recorded shape from the list of bins that hold allowed rows and how many each holds.
struct Filt {
    std::vector<int32_t> prefix;
    FilterShape shape;
    std::vector<char> occ;
    Filt(int64_t n, const std::vector<std::pair<int64_t, int>>& bins) {   // (bin, allowed rows in it)
        const int64_t nbins = (n + 63) / 64;
        occ.assign((size_t)nbins, 0);
        int64_t na = 0;
        for (auto& b : bins) { occ[(size_t)b.first] = b.second > 0; na += b.second; }
        prefix.assign((size_t)nbins + 1, 0);
        for (int64_t b = 0; b < nbins; ++b) prefix[(size_t)b + 1] = prefix[(size_t)b] + occ[(size_t)b];
        shape.n = n; shape.na = na; shape.occ_prefix = prefix.data();
    }
};
static std::vector<std::pair<int64_t, int>> run(int64_t first_bin, int64_t count, int rows_each, int64_t stride = 1) {
    std::vector<std::pair<int64_t, int>> v;
    for (int64_t i = 0; i < count; ++i) v.push_back({first_bin + i * stride, rows_each});
    return v;
}
// partitions that hold an allowed row, from the definition: every occupied bin -> the scan workgroup that owns it -> its partition
static int partitions_by_definition(const Filt& f, int nquads, int G, int m) {
    const int NP = m <= 8 ? 64 : (m <= 64 ? 256 : 512);
    std::set<int> parts;
    int g = 0;
    for (int b = 0; b < nquads; ++b) {
        while ((int)((int64_t)(g + 1) * nquads / G) <= b) ++g;   // workgroup g owns bins [g nquads / G, (g + 1) nquads / G)
        if (f.occ[(size_t)b]) parts.insert(g % NP);
    }
    return (int)parts.size();
}

int main() {
    const int64_t BIG = (int64_t)1 << 20;   // 16384 bins; grids: 256 workgroups (wide passes), 512 (64-query passes)
    rq_index idx;
    fp16_index(idx, BIG);
    CHECK(idx.cu_count == 256 && idx.wg_per_cu == 2 && idx.filter_route == -1, "defaults moved");
    {   // ---- empty and forced routes -------------------------------------------------------------------------------
        Filt none(BIG, {});
        for (int forced : {-1, 1, 2, 3}) CHECK(plan_filter(&idx, none.shape, 64, 10, 0, forced) == FROUTE_EMPTY, "na = 0, forced %d", forced);
        Filt half(BIG, run(0, 8192, 64, 2));
        CHECK(plan_filter(&idx, half.shape, 64, 10, 0, 1) == FROUTE_GATHER && plan_filter(&idx, half.shape, 64, 10, 0, 3) == FROUTE_EXACT, "forced");
        CHECK(plan_filter(&idx, half.shape, 64, 10, 0, 2) == FROUTE_SCAN, "forced scan");
        rq_index tiny;
        fp16_index(tiny, 1000);   // 16 bins: 2 nb >= bins, the scan's plan is exact
        Filt t(1000, run(0, 16, 30));
        CHECK(plan_filter(&tiny, t.shape, 64, 10, 0, 2) == FROUTE_EXACT, "forced scan on a shard whose plan is exact");
        CHECK(plan_filter(&tiny, t.shape, 64, 10, 0, -1) == FROUTE_GATHER, "tiny shard: fewer than two bins per wanted bin");
    }
    {   // ---- gather by rows re-scored: B x na <= N and 4 na <= N ---------------------------------------------------------------
        Filt at(BIG, run(0, 16384, 1));                      // 16384 rows, one in every bin: 64 x 16384 = N
        auto more = run(0, 16383, 1); more.push_back({16383, 2});
        Filt over(BIG, more);                                // 16385 rows, every workgroup occupied
        CHECK(at.shape.na == 16384 && over.shape.na == 16385, "shapes");
        CHECK(plan_filter(&idx, at.shape, 64, 10, 0, -1) == FROUTE_GATHER, "64 x 16384 = N");
        CHECK(plan_filter(&idx, over.shape, 64, 10, 0, -1) == FROUTE_SCAN, "64 x 16385 > N, every partition occupied");
        CHECK(plan_filter(&idx, over.shape, 1, 10, 0, -1) == FROUTE_GATHER, "B = 1: 16385 <= N");
        CHECK(plan_filter(&idx, at.shape, 256, 10, 0, -1) == FROUTE_SCAN, "B = 256: 256 x 16384 > N");
        // one query: the list must fit as well (a quarter of the rows)
        Filt quarter(BIG, run(0, 4096, 64));
        auto q1 = run(0, 4096, 64); q1.push_back({4096, 1});
        Filt quarter1(BIG, q1);
        CHECK(quarter.shape.na * 4 == BIG && plan_filter(&idx, quarter.shape, 1, 10, 0, -1) == FROUTE_GATHER, "B = 1, na = N / 4");
        CHECK(plan_filter(&idx, quarter1.shape, 1, 10, 0, -1) == FROUTE_SCAN, "B = 1, na = N / 4 + 1: 129 partitions >= 10");
    }
    {   // ---- gather by bins: 2 nb >= bins that hold an allowed row (k = 10: nb = 18); B = 512 so that B x na > N ----------------
        Filt b36(BIG, run(100, 36, 64)), b37(BIG, run(100, 37, 64));
        CHECK(512 * b36.shape.na > BIG && plan_filter(&idx, b36.shape, 512, 10, 0, -1) == FROUTE_GATHER, "36 occupied bins");
        // 37 bins in a row sit in one or two scan workgroups: the threshold cannot narrow, the list fits -> gather all the same
        CHECK(plan_filter(&idx, b37.shape, 512, 10, 0, -1) == FROUTE_GATHER, "37 contiguous bins");
        Filt s37(BIG, run(0, 37, 64, 400));      // 37 full bins far apart: 37 workgroups of the wide grid, 37 partitions >= 10
        CHECK(plan_filter(&idx, s37.shape, 512, 10, 0, -1) == FROUTE_SCAN, "37 scattered bins");
    }
    {   // ---- the partition condition and what follows when it fails -----------------------------------------------------------
        Filt half(BIG, run(0, 8192, 64));        // the first half of the shard: workgroups 0..255 of 512
        CHECK(plan_filter(&idx, half.shape, 64, 10, 0, -1) == FROUTE_SCAN, "k = 10: 256 partitions of 256");
        CHECK(plan_filter(&idx, half.shape, 64, 100, 0, -1) == FROUTE_SCAN, "k = 100: 256 partitions of 512 >= 100");
        CHECK(plan_filter(&idx, half.shape, 64, 320, 0, -1) == FROUTE_EXACT, "k = 320: 256 partitions < 320, half the rows: exact");
        Filt fifth(BIG, run(0, 3277, 64));       // 20 % in one run: 103 workgroups
        CHECK(plan_filter(&idx, fifth.shape, 64, 320, 0, -1) == FROUTE_GATHER, "k = 320: 103 partitions < 320, a fifth of the rows: gather");
        CHECK(plan_filter(&idx, fifth.shape, 64, 100, 0, -1) == FROUTE_SCAN, "k = 100: 103 partitions >= 100");
        Filt tenth(BIG, run(4096, 1638, 64));    // 10 %: 52 workgroups
        CHECK(plan_filter(&idx, tenth.shape, 64, 100, 0, -1) == FROUTE_GATHER, "a contiguous tenth at k = 100 is not scanned");
        CHECK(plan_filter(&idx, tenth.shape, 64, 10, 0, -1) == FROUTE_SCAN, "... but at k = 10 it is (52 partitions >= 10)");
        // the generic tail has no partition threshold: k beyond the fast tail scans whatever the occupancy
        CHECK(plan_filter(&idx, half.shape, 64, 400, 0, -1) == FROUTE_SCAN, "k = 400: generic tail");
        // a wide call uses the 256-workgroup grid for its 256-query pass and the 512-workgroup grid for the rest: both must hold
        Filt q(BIG, run(0, 4096, 64));           // the first quarter: 64 of 256 wide workgroups, 128 of 512
        CHECK(plan_filter(&idx, q.shape, 300, 100, 0, -1) == FROUTE_GATHER, "B = 300, k = 100: 64 partitions of the wide grid < 100");
        CHECK(plan_filter(&idx, q.shape, 64, 100, 0, -1) == FROUTE_SCAN, "B = 64, k = 100: 128 partitions >= 100");
        // fewer allowed rows than k: m = na
        Filt five(BIG, {{3, 1}, {900, 2}, {5000, 1}, {16383, 1}});
        CHECK(five.shape.na == 5 && plan_filter(&idx, five.shape, 64, 10, 0, -1) == FROUTE_GATHER, "na = 5");
    }
    {   // ---- a shard whose scan scores say nothing (rq_plan.h RQ_EPS_USELESS) ------------------------------------------------
        rq_index sub;
        fp16_index(sub, BIG);
        sub.max_sub_rel = 0.2;
        Filt half(BIG, run(0, 8192, 64, 2)), fifth(BIG, run(0, 3277, 64, 5));
        CHECK(plan_filter(&sub, half.shape, 64, 10, 0, -1) == FROUTE_EXACT && plan_filter(&sub, fifth.shape, 64, 10, 0, -1) == FROUTE_GATHER, "useless eps");
    }
    {   // ---- sweep: the scan route is never chosen with fewer than min(k, na) occupied partitions; nothing is written ------------
        int scans = 0, others = 0;
        for (int64_t n : {(int64_t)4101, (int64_t)70000, BIG}) {
            rq_index ix;
            fp16_index(ix, n);
            const rq_index snapshot = ix;
            const int64_t nbins = (n + 63) / 64;
            for (int k : {1, 8, 9, 10, 64, 65, 100, 320})
                for (int B : {1, 64, 100, 256, 300})
                    for (int64_t count : {(int64_t)1, (int64_t)5, nbins / 20 + 1, nbins / 3 + 1, nbins})
                        for (int64_t stride : {(int64_t)1, (int64_t)3, (int64_t)17}) {
                            if ((count - 1) * stride >= nbins) continue;
                            Filt f(n, run(0, count, 1 + (int)(count % 3), stride));
                            CallPlan p;
                            const int route = plan_filter(&ix, f.shape, B, k, 0, -1, &p);
                            if (route != FROUTE_SCAN) { ++others; continue; }
                            ++scans;
                            CHECK(!p.exact, "scan route with an exact plan");
                            if (!p.fast) continue;
                            const int m = (int)std::min<int64_t>(k, f.shape.na);
                            const int gn = scan_grid(&ix, p.nquads, ix.wg_per_cu);
                            if (p.nwg_split > 0) CHECK(partitions_by_definition(f, p.nquads, p.grid_wide, m) >= m, "n=%lld k=%d B=%d count=%lld stride=%lld (wide grid)", (long long)n, k, B, (long long)count, (long long)stride);
                            if (p.nwg_split < p.bpad) CHECK(partitions_by_definition(f, p.nquads, gn, m) >= m, "n=%lld k=%d B=%d count=%lld stride=%lld (narrow grid)", (long long)n, k, B, (long long)count, (long long)stride);
                        }
            CHECK(ix.n == snapshot.n && ix.filter_route == snapshot.filter_route && ix.filter_route_last == snapshot.filter_route_last &&
                  ix.filter_repaired == snapshot.filter_repaired && ix.scan8_used == snapshot.scan8_used && ix.last_use8 == snapshot.last_use8 && ix.ctx.empty(),
                  "plan_filter wrote to the index");
        }
        CHECK(scans > 50 && others > 50, "the sweep reached %d scan and %d other decisions", scans, others);
        std::printf("sweep: %d scan decisions, %d others\n", scans, others);
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
