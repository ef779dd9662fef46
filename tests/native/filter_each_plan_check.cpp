// Host-side check of the plan of a search with one filter per query (csrc/rq_filter_each_plan.h): plain arithmetic on the index's
// fields, the call's arguments and what each filter recorded, so it runs here on a default-constructed rq_index and hand-made
// rq_filter records without a GPU and can be built under the host sanitizers.  Expectations are worked out by hand from the rules
// the header states and from the boundaries of plan_filter that tests/native/filter_plan_check.cpp pins.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/filter_each_plan_check.cpp -o filter_each_plan_check
#include "rq_filter_each_plan.h"

#include <memory>

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

// A filter's host record: `count` occupied bins from first_bin on, `stride` bins apart, rows_each allowed rows in each.
static std::unique_ptr<rq_filter> filt(rq_index* idx, int64_t first_bin, int64_t count, int rows_each, int64_t stride = 1) {
    std::unique_ptr<rq_filter> f(new rq_filter());
    const int64_t nbins = (idx->n + 63) / 64;
    std::vector<char> occ((size_t)nbins, 0);
    for (int64_t i = 0; i < count; ++i) occ[(size_t)(first_bin + i * stride)] = rows_each > 0;
    f->idx = idx; f->n = idx->n; f->na = count * rows_each;
    f->occ_prefix.assign((size_t)nbins + 1, 0);
    for (int64_t b = 0; b < nbins; ++b) f->occ_prefix[(size_t)b + 1] = f->occ_prefix[(size_t)b] + occ[(size_t)b];
    return f;
}
static bool same(const std::vector<int>& a, std::initializer_list<int> b) { return a == std::vector<int>(b); }
static int plan(const rq_index& idx, const std::vector<const rq_filter*>& fl, int k, int forced, int64_t cap, EachPlan& p) {
    return plan_filter_each(&idx, fl.data(), (int)fl.size(), k, 0, forced, cap, &p);
}

int main() {
    const int64_t BIG = (int64_t)1 << 20;   // 16384 bins
    rq_index idx;
    fp16_index(idx, BIG);
    CHECK(RQ_FILTER_EACH_EXACT_GROUPS == 12 && RQ_FILTER_EACH_KEY_CAP == ((int64_t)1 << 27), "constants moved");
    // tenants: 300 rows in 300 bins each (gather at any B_g here); broad: half of every bin (scan at k = 10); at: 16384 rows, one per bin
    auto A = filt(&idx, 0, 300, 1), Bf = filt(&idx, 1000, 300, 1), Cf = filt(&idx, 2000, 300, 1), none = filt(&idx, 0, 0, 0);
    auto at = filt(&idx, 0, 16384, 1), at2 = filt(&idx, 0, 16384, 1);
    std::vector<std::unique_ptr<rq_filter>> broad;
    for (int i = 0; i < 64; ++i) broad.push_back(filt(&idx, 0, 16384, 32));
    const rq_index snapshot = idx;
    EachPlan p;
    {   // ---- grouping: first appearance, interleaved and repeated entries, NULL, contiguity -------------------------------------
        std::vector<const rq_filter*> fl = {A.get(), Bf.get(), A.get(), nullptr, Bf.get(), Cf.get(), nullptr, A.get()};
        CHECK(plan(idx, fl, 10, -1, 0, p) == RQ_OK, "plan");
        CHECK(p.groups.size() == 4, "%zu groups", p.groups.size());
        CHECK(p.groups[0].f == A.get() && p.groups[1].f == Bf.get() && p.groups[2].f == nullptr && p.groups[3].f == Cf.get(), "first appearance order");
        CHECK(same(p.groups[0].q, {0, 2, 7}) && same(p.groups[1].q, {1, 4}) && same(p.groups[2].q, {3, 6}) && same(p.groups[3].q, {5}), "members");
        CHECK(!p.groups[0].contiguous && !p.groups[1].contiguous && !p.groups[2].contiguous && p.groups[3].contiguous, "contiguity");
        CHECK(p.groups[2].kind == EACH_PASS && p.groups[2].route == EACH_ROUTE_NULL, "the NULL group is a pass group of its own");
        CHECK(p.groups[0].kind == EACH_RAGGED && p.groups[1].kind == EACH_RAGGED && p.groups[3].kind == EACH_RAGGED, "tenants gather");
        // the ragged set in launch order: group by group
        CHECK(same(p.ragged_q, {0, 2, 7, 1, 4, 5}) && same(p.ragged_g, {0, 0, 0, 1, 1, 3}), "ragged order");
        CHECK(p.rounds.size() == 1 && p.rounds[0].first == 0 && p.rounds[0].count == 6 && p.rounds[0].keys == 6 * 300, "one round");
        CHECK(p.routes == ((1 << FROUTE_GATHER) | (1 << EACH_ROUTE_NULL)) && p.last_route == FROUTE_GATHER && p.pass_groups == 0 && p.shared_q.empty(), "routes");
        // arranged by filter: every group is one run
        fl = {A.get(), A.get(), nullptr, nullptr, Bf.get(), Bf.get(), Bf.get()};
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.groups.size() == 3 && p.groups[0].contiguous && p.groups[1].contiguous && p.groups[2].contiguous && same(p.groups[2].q, {4, 5, 6}), "runs");
        CHECK(p.last_route == FROUTE_GATHER, "last route");
        // one filter, and NULL alone
        fl.assign(5, A.get());
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.groups.size() == 1 && p.groups[0].contiguous && p.groups[0].q.size() == 5, "one group");
        fl.assign(5, nullptr);
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.groups.size() == 1 && p.groups[0].kind == EACH_PASS && p.ragged_q.empty() && p.rounds.empty() && p.last_route == EACH_ROUTE_NULL, "NULL alone");
    }
    {   // ---- every group is routed by its OWN number of queries: B_g x na <= N (filter_plan_check.cpp: 64 x 16384 = N) --------------
        std::vector<const rq_filter*> fl;
        for (int i = 0; i < 64; ++i) { fl.push_back(at.get()); fl.push_back(at2.get()); }   // 128 queries, 64 per filter
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.groups.size() == 2 && p.groups[0].route == FROUTE_GATHER && p.groups[1].route == FROUTE_GATHER && p.ragged_q.size() == 128, "64 queries each: gather");
        CHECK(plan_filter(&idx, each_shape(at.get()), 128, 10, 0, -1) == FROUTE_SCAN, "(the batch as one call would scan)");
        fl.push_back(at.get());                                                               // 65 queries of `at`
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.groups[0].route == FROUTE_SCAN && p.groups[0].kind == EACH_PASS && p.groups[1].kind == EACH_RAGGED && p.ragged_q.size() == 64 && p.pass_groups == 1, "65 x 16384 > N: a pass group");
        CHECK(!p.groups[0].contiguous && p.groups[0].q.back() == 128, "its queries");
        // no row allowed: padding, whatever is forced
        for (int forced : {-1, 1, 2, 3}) {
            fl = {none.get(), A.get(), none.get()};
            plan(idx, fl, 10, forced, 0, p);
            CHECK(p.groups[0].kind == EACH_EMPTY && p.groups[0].route == FROUTE_EMPTY && (p.routes & 1), "empty group, forced %d", forced);
        }
    }
    {   // ---- rule 4: G_p > 12 x ceil(S / 64) ---------------------------------------------------------------------------------
        for (int nf : {12, 13}) {
            std::vector<const rq_filter*> fl;
            for (int i = 0; i < 64; ++i) fl.push_back(broad[(size_t)(i % nf)].get());
            plan(idx, fl, 10, -1, 0, p);
            CHECK((int)p.groups.size() == nf && p.groups[0].route == (nf == 13 ? FROUTE_EXACT : FROUTE_SCAN), "%d broad filters: route %d", nf, p.groups[0].route);
            if (nf == 12) CHECK(p.shared_q.empty() && p.pass_groups == 12 && p.groups[11].kind == EACH_PASS, "12 over 64 queries: one pass each");
            else CHECK(p.shared_q.size() == 64 && p.pass_groups == 0 && p.groups[12].kind == EACH_SHARED && p.routes == (1 << FROUTE_EXACT), "13 over 64 queries: shared");
        }
        for (int nf : {24, 25}) {   // 128 queries: two scans' worth
            std::vector<const rq_filter*> fl;
            for (int i = 0; i < 128; ++i) fl.push_back(broad[(size_t)(i % nf)].get());
            plan(idx, fl, 10, -1, 0, p);
            CHECK((p.shared_q.size() == 128) == (nf == 25), "%d broad filters over 128 queries", nf);
        }
        {   // 65 queries already count as two scans; the ragged and NULL groups do not count
            std::vector<const rq_filter*> fl;
            for (int i = 0; i < 65; ++i) fl.push_back(broad[(size_t)(i % 13)].get());
            fl.push_back(A.get()); fl.push_back(nullptr);
            plan(idx, fl, 10, -1, 0, p);
            CHECK(p.shared_q.empty() && p.pass_groups == 13 && p.ragged_q.size() == 1, "13 over 65 queries: 13 <= 24");
            fl.resize(64); fl.push_back(A.get()); fl.push_back(nullptr);
            plan(idx, fl, 10, -1, 0, p);
            CHECK(p.shared_q.size() == 64 && p.ragged_q.size() == 1 && p.groups.back().kind == EACH_PASS && p.last_route == EACH_ROUTE_NULL, "13 over 64 of 66 queries");
            // shared order: group by group, positions ascending within a group
            CHECK(p.shared_q[0] == 0 && p.shared_q[1] == 13 && p.shared_g[0] == 0 && p.shared_g[5] == 1 && p.shared_q[5] == 1, "shared order");
        }
    }
    {   // ---- forced routes ---------------------------------------------------------------------------------------------------
        std::vector<const rq_filter*> fl = {A.get(), broad[0].get(), nullptr, none.get(), broad[1].get(), A.get()};
        plan(idx, fl, 10, FROUTE_GATHER, 0, p);
        CHECK(p.ragged_q.size() == 4 && p.shared_q.empty() && p.pass_groups == 0 && p.groups[2].kind == EACH_PASS && p.groups[3].kind == EACH_EMPTY, "forced 1: the ragged set");
        CHECK(p.rounds.size() == 1 && p.rounds[0].keys == 2 * 300 + 2 * (BIG / 2), "forced 1: keys");
        plan(idx, fl, 10, FROUTE_SCAN, 0, p);
        CHECK(p.ragged_q.empty() && p.shared_q.empty() && p.pass_groups == 3 && p.groups[0].route == FROUTE_SCAN, "forced 2: one pass per group");
        plan(idx, fl, 10, FROUTE_EXACT, 0, p);
        CHECK(p.ragged_q.empty() && p.shared_q.size() == 4 && p.pass_groups == 0 && p.groups[0].kind == EACH_SHARED && p.groups[2].kind == EACH_PASS && p.groups[3].kind == EACH_EMPTY, "forced 3: shared");
        std::vector<const rq_filter*> many;
        for (int i = 0; i < 64; ++i) many.push_back(broad[(size_t)i].get());
        plan(idx, many, 10, FROUTE_SCAN, 0, p);
        CHECK(p.shared_q.empty() && p.pass_groups == 64, "forced 2 keeps 64 broad filters apart");
    }
    {   // ---- rounds: cut at query boundaries once the keys pass the cap; a query beyond the cap gets a round of its own --------------
        std::vector<const rq_filter*> fl = {A.get(), Bf.get(), Cf.get(), A.get(), at.get()};   // 300, 300, 300, 300 (A again: launch order A A B C), 16384
        plan(idx, fl, 10, -1, 600, p);
        CHECK(same(p.ragged_q, {0, 3, 1, 2, 4}), "launch order");
        CHECK(p.rounds.size() == 3 && p.rounds[0].count == 2 && p.rounds[0].keys == 600 && p.rounds[1].first == 2 && p.rounds[1].count == 2 && p.rounds[2].first == 4 &&
              p.rounds[2].count == 1 && p.rounds[2].keys == 16384, "cap 600: %zu rounds", p.rounds.size());
        plan(idx, fl, 10, -1, 601, p);
        CHECK(p.rounds.size() == 3 && p.rounds[0].count == 2, "cap 601");
        plan(idx, fl, 10, -1, 299, p);
        CHECK(p.rounds.size() == 5 && p.rounds[3].first == 3 && p.rounds[4].keys == 16384, "cap 299: every query alone");
        plan(idx, fl, 10, -1, 0, p);
        CHECK(p.rounds.size() == 1 && p.rounds[0].count == 5 && p.rounds[0].keys == 4 * 300 + 16384, "default cap");
        int64_t total = 0; int covered = 0;
        plan(idx, fl, 10, -1, 900, p);
        for (const EachRound& r : p.rounds) { CHECK(r.first == covered, "rounds are consecutive"); covered += r.count; total += r.keys; }
        CHECK(covered == 5 && total == 4 * 300 + 16384, "rounds cover the set");
    }
    // ---- nothing written ---------------------------------------------------------------------------------------------------
    CHECK(idx.n == snapshot.n && idx.filter_route == snapshot.filter_route && idx.filter_route_last == snapshot.filter_route_last && idx.each_calls == 0 &&
          idx.each_groups_last == 0 && idx.each_key_cap == 0 && idx.filter_repaired == snapshot.filter_repaired && idx.t.searches == 0 && idx.ctx.empty() && idx.filters.empty(),
          "plan_filter_each wrote to the index");
    CHECK(A->na == 300 && A->n == BIG && !A->d_list && !A->d_bits && !A->scale[0] && A->occ_prefix.back() == 300 && broad[0]->na == BIG / 2 && !broad[0]->scale[0],
          "plan_filter_each wrote to a filter");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
