// rq_filter_each_plan.h -- what a search with one filter per query will do (include/rq.h rq_search_filtered_each), decided like
// the route of one filter in rq_filter_plan.h: plain arithmetic on the index's fields, the call's arguments and what each filter
// recorded at creation.  No HIP runtime call, nothing is written to the index or to the filters
// (tests/native/filter_each_plan_check.cpp runs it on the host).  Results never depend on the plan: query q's answer is that of
// rq_search_filtered with filters[q] for that query alone.
//   1. the queries are grouped by filter pointer, in order of first appearance; NULL (unrestricted) is a group of its own;
//   2. every group is routed by plan_filter with its OWN number of queries and the "filter_route" option;
//   3. EMPTY groups are padding; all GATHER groups together are the RAGGED SET (one prepare, one ragged gather and one final launch
//      per round, rq_filter_each.hip); the others (SCAN, EXACT, NULL) are PASS groups: one existing call each;
//   4. unless enough filtered pass groups share the batch: then ONE exact fp64 scan of the shard answers all of them, each query's
//      keys masked by its own bitmap (the SHARED exact route);
//   5. the ragged set's candidate keys live in the stream's workspace: beyond the key cap it is cut into rounds at query boundaries.
#pragma once
#include "rq_filter_plan.h"

#include <map>

// Rule 4: with G_p filtered pass groups of S queries in all, the shared exact route is taken when
// G_p > RQ_FILTER_EACH_EXACT_GROUPS * ceil(S / 64).  12 is DERIVED, from two measured figures of rq_filter_plan.h (1M x 768, B = 64):
// a filtered scan call costs 285 us, one exact fp64 scan of the shard answers 64 queries in 3.45 ms whatever their filters allow
// (3.45 ms / 285 us = 12.1); when the constant was chosen the combined route had not been measured.
// MEASURED since (tools/gpu_filter_each.py shape D, profiles/filter_each.json; 1M x 768, 64 queries, half-allowing masks
// dealt interleaved, each call with its repair step): one pass per group costs 247 us per group inside the each-call (2.02 ms at 8
// groups, 3.00 at 12, 3.98 at 16, 7.90 at 32, 15.47 at 64), the shared exact route 3.50 - 3.53 ms whatever the number of groups: they
// cross at 14.2 groups.  The derived 12 stays: at 13 and 14 groups the shared route gives away 0.29 and 0.04 ms (9 % and 1 %), from
// 15 on it wins, and a filter whose masked scale has not been built yet (4 N bytes and a synchronisation per filter, which the
// shared route never needs) moves the crossover down, not up.
#define RQ_FILTER_EACH_EXACT_GROUPS 12
// Rule 5: candidate keys of one ragged round, 1 GiB of them as queries_per_gib bounds the other routes ("filter_each_key_cap": test hook).
#define RQ_FILTER_EACH_KEY_CAP (((int64_t)1 << 30) / (int64_t)sizeof(uint64_t))

enum EachKind {
    EACH_EMPTY = 0,    // no row allowed: padding
    EACH_RAGGED = 1,   // member of the ragged set
    EACH_PASS = 2,     // one existing call for the group (scan route, exact route, or the unfiltered search of the NULL group)
    EACH_SHARED = 3,   // answered by the shared exact scan
};
#define EACH_ROUTE_NULL 4   // EachGroup::route of the NULL group (FilterRoute has 0..3); also its bit in "filter_each_routes_last"

struct EachGroup {
    const rq_filter* f = nullptr;   // null: the unrestricted queries
    std::vector<int> q;             // positions in the batch, ascending
    bool contiguous = true;         // q is one run q[0], q[0] + 1, ...: served through pointer offsets, no copy
    int route = FROUTE_EMPTY;       // plan_filter's answer for the group's own B_g (EACH_ROUTE_NULL for the NULL group)
    int kind = EACH_EMPTY;
};
struct EachRound { int first = 0, count = 0; int64_t keys = 0; };   // ragged queries [first, first + count) and their keys

struct EachPlan {
    std::vector<EachGroup> groups;     // in order of first appearance
    std::vector<int> ragged_q;         // the ragged set in launch order (group by group): position in the batch ...
    std::vector<int> ragged_g;         // ... and group of each
    std::vector<EachRound> rounds;
    std::vector<int> shared_q, shared_g;   // the queries of the shared exact route, group by group
    int pass_groups = 0;               // filtered groups that keep a pass of their own
    int routes = 0;                    // bit r: some group took route r (EACH_ROUTE_NULL: the NULL group)
    int last_route = -1;               // the last group's route
};

static inline FilterShape each_shape(const rq_filter* f) { return FilterShape{f->n, f->na, f->occ_prefix.data()}; }

// forced: option "filter_route" (-1 = the rules).  key_cap: option "filter_each_key_cap" (<= 0: RQ_FILTER_EACH_KEY_CAP).
static inline int plan_filter_each(const rq_index* idx, const rq_filter* const* filters, int B, int k, int metric, int forced, int64_t key_cap, EachPlan* plan) {
    EachPlan& p = *plan;
    p = EachPlan();
    // 1. groups by pointer, first appearance first
    std::map<const rq_filter*, int> seen;
    for (int q = 0; q < B; ++q) {
        auto it = seen.find(filters[q]);
        if (it == seen.end()) {
            it = seen.emplace(filters[q], (int)p.groups.size()).first;
            p.groups.emplace_back();
            p.groups.back().f = filters[q];
        }
        EachGroup& g = p.groups[(size_t)it->second];
        if (!g.q.empty() && g.q.back() + 1 != q) g.contiguous = false;
        g.q.push_back(q);
    }
    // 2. + 3. the route of every group by its own B_g
    int gp = 0;
    int64_t sq = 0;
    for (EachGroup& g : p.groups) {
        if (!g.f) { g.route = EACH_ROUTE_NULL; g.kind = EACH_PASS; continue; }
        g.route = plan_filter(idx, each_shape(g.f), (int)g.q.size(), k, metric, forced);
        g.kind = g.route == FROUTE_EMPTY ? EACH_EMPTY : (g.route == FROUTE_GATHER ? EACH_RAGGED : EACH_PASS);
        if (g.kind == EACH_PASS) { ++gp; sq += (int64_t)g.q.size(); }
    }
    // 4. the shared exact route (forced 3: every group that has a row to return; forced 1 left no pass group; forced 2 keeps them)
    const bool shared = forced == FROUTE_EXACT ? gp > 0 : (forced < 0 && (int64_t)gp > (int64_t)RQ_FILTER_EACH_EXACT_GROUPS * ((sq + 63) / 64));
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        EachGroup& g = p.groups[gi];
        if (g.f && g.kind == EACH_PASS && shared) { g.kind = EACH_SHARED; g.route = FROUTE_EXACT; }
        if (g.f && g.kind == EACH_PASS) ++p.pass_groups;
        for (int q : g.q) {
            if (g.kind == EACH_RAGGED) { p.ragged_q.push_back(q); p.ragged_g.push_back((int)gi); }
            if (g.kind == EACH_SHARED) { p.shared_q.push_back(q); p.shared_g.push_back((int)gi); }
        }
        p.routes |= 1 << g.route;
        p.last_route = g.route;
    }
    // 5. rounds of the ragged set: cut at query boundaries; a query beyond the cap gets a round of its own
    const int64_t cap = key_cap > 0 ? key_cap : RQ_FILTER_EACH_KEY_CAP;
    EachRound cur;
    for (size_t i = 0; i < p.ragged_q.size(); ++i) {
        const int64_t na = p.groups[(size_t)p.ragged_g[i]].f->na;
        if (cur.count > 0 && cur.keys + na > cap) { p.rounds.push_back(cur); cur = EachRound(); cur.first = (int)i; }
        cur.count++;
        cur.keys += na;
    }
    if (cur.count > 0) p.rounds.push_back(cur);
    return RQ_OK;
}
