// bundle_plan_check.cpp -- csrc/rq_bundle_plan.h on the host: every sequence of up to 12 events of one stream is run through
// the plan, and a model of what rq_search.hip does with each step (preparations, passes, tail launches, the ring slots they
// write and read) is checked:
//   * every call is scanned exactly once, or was scanned ahead and claimed;
//   * every call's tail is issued exactly once, after its pass;
//   * no ring slot is rewritten while a pass or a tail that reads it is outstanding, and every pass and tail finds the queries
//     of its own call in the slot it reads;
//   * no bundle of four opens before RQ_BUNDLE_STREAK matched pairs have completed back to back;
//   * a hinted loop of n calls makes 3 + ceil((n - 6) / 4) passes (n >= 6; ceil(n / 2) below, and always with scan_bundle = 2).
// Events: A = a matching call that announces the next batch, N = a matching call that announces nothing, M = a call that brings
// another batch than the announced one (and announces one itself), F = a flush.  Stand-alone: no HIP, no Python.
#include <cstdio>
#include <cstring>

#include "rq_bundle_plan.h"

static long failures = 0, sequences = 0;
static const char* cur_seq = "";
#define CHECK(cond, what)                                                                  \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            if (failures++ < 20) std::printf("FAIL [%s] %s (line %d)\n", cur_seq, what, __LINE__); \
        }                                                                                  \
    } while (0)

static const int MAXC = 48;

struct Model {
    BundleState st;
    int limit = 4;
    // calls made so far
    int ncalls = 0;
    int scanned[MAXC], tails[MAXC], slot_of[MAXC];
    // batches are tokens: a call brings one; an announcement names the next one
    int next_tok = 0;
    int hint_tok = -1;                       // announced, not yet acted on
    int await_tok = -1;                      // the batch the open bundle awaits
    int prepped_tok = -1, prepped_slot = -1;
    int holds[RQ_RING_SLOTS];                // token whose prepared queries a slot holds
    int readers[RQ_RING_SLOTS];              // passes / tails still to be issued that read the slot
    int member[RQ_BUNDLE_MAX];               // calls of the open bundle
    int ahead_slot = -1;                     // slot of the batch a pass has scanned ahead
    int pending = -1;                        // the call whose tail waits for the stream's next fused launch
    int launches = 0, bundles4 = 0;
    int pairs_done = 0;                      // matched pairs completed back to back, as the model saw them
    Model() {
        std::memset(scanned, 0, sizeof scanned); std::memset(tails, 0, sizeof tails); std::memset(slot_of, -1, sizeof slot_of);
        for (int i = 0; i < RQ_RING_SLOTS; ++i) { holds[i] = -1; readers[i] = 0; }
        for (int& m : member) m = -1;
    }
    int tok_of[MAXC];

    void write(int slot, int tok) {
        CHECK(slot >= 0 && slot < RQ_RING_SLOTS, "preparation into a slot outside the ring");
        if (slot < 0 || slot >= RQ_RING_SLOTS) return;
        CHECK(readers[slot] == 0, "a ring slot is rewritten while a pass or tail that reads it is outstanding");
        holds[slot] = tok;
    }
    void take(int id, int slot) { slot_of[id] = slot; readers[slot]++; }
    void scan(int id) {
        CHECK(holds[slot_of[id]] == tok_of[id], "a pass reads a slot that does not hold its call's queries");
        scanned[id]++;
    }
    void tail(int id) {
        CHECK(scanned[id] == 1, "a tail is issued before its call was scanned");
        CHECK(holds[slot_of[id]] == tok_of[id], "a tail reads a slot that does not hold its call's queries");
        tails[id]++;
        readers[slot_of[id]]--;
    }
    void drop_ahead() { if (ahead_slot >= 0) readers[ahead_slot]--; ahead_slot = -1; }
    void run_pending() { if (pending >= 0) tail(pending); pending = -1; }

    // one pass over the first n members (+ the awaited batch in slot `ahead`, -1 none)
    void pass(int n, int base, int ahead) {
        launches++;
        const int width = n + (ahead >= 0);
        if (width >= 3) { bundles4++; CHECK(base % RQ_BUNDLE_MAX == 0, "a 256-query pass over slots that are not an aligned quarter"); }
        for (int j = 0; j < n; ++j) {
            CHECK(slot_of[member[j]] == (base + j) % RQ_RING_SLOTS, "member not in its slot");
            scan(member[j]);
        }
        if (ahead >= 0) {
            CHECK(ahead == (base + n) % RQ_RING_SLOTS, "the batch scanned ahead is not in the slot behind the members");
            CHECK(holds[ahead] == await_tok, "the pass scans a slot ahead that does not hold the awaited batch");
            ahead_slot = ahead; readers[ahead]++;
        }
    }
    // tails of the first n members in one launch, which also prepares `tok` into `slot` (-1: nothing)
    void tails_launch(int n, int slot, int tok) {
        if (slot >= 0) write(slot, tok);   // (checked while the launch's own tails still count as readers)
        for (int j = 0; j < n; ++j) tail(member[j]);
    }
    void do_break(const BundleStep& s) {
        if (s.brk == BREAK_NONE) return;
        await_tok = -1;
        pairs_done = 0;
        if (s.brk == BREAK_SCAN) { run_pending(); pass(s.brk_n, s.brk_base, -1); }
        else drop_ahead();
        if (s.brk_n == 1) pending = member[0];
        else tails_launch(s.brk_n, -1, -1);
    }
    void flush() {
        hint_tok = -1;
        do_break(bundle_end(st));
        pairs_done = 0;
        run_pending();
        for (int i = 0; i < ncalls; ++i) {
            CHECK(scanned[i] == 1, "after a flush: a call was not scanned exactly once");
            CHECK(tails[i] == 1, "after a flush: a call's tail was not issued exactly once");
        }
        for (int i = 0; i < RQ_RING_SLOTS; ++i) CHECK(readers[i] == 0, "after a flush: a ring slot still has readers");
    }
    // matching: the call brings the announced batch (any batch if none was announced); announces: it announces the next one
    void call(bool matching, bool announces) {
        const int id = ncalls++;
        const int announced = await_tok >= 0 ? await_tok : (prepped_tok >= 0 ? prepped_tok : -1);
        const int tok = matching && announced >= 0 ? announced : next_tok++;
        tok_of[id] = tok;
        hint_tok = announces ? next_tok++ : -1;
        BundleCall c;
        c.fused = c.eligible = c.full = true;
        c.next_full = announces;
        c.announces = announces;
        c.matches = await_tok >= 0 && tok == await_tok;
        c.prepped_slot = prepped_tok == tok ? prepped_slot : -1;
        c.other = announced >= 0 && tok != announced;
        if (c.other) pairs_done = 0;
        const int phase0 = st.phase;
        const BundleStep s = bundle_call(st, c, limit);
        do_break(s);
        CHECK(s.role != ROLE_OTHER, "a fused call got no role");
        CHECK(s.slot >= 0 && s.slot < RQ_RING_SLOTS, "slot outside the ring");
        if (s.role == ROLE_CLAIM) {
            CHECK(phase0 == BUNDLE_AHEAD && s.slot == ahead_slot, "claim of a batch no pass has scanned ahead");
            slot_of[id] = s.slot; ahead_slot = -1;   // (the reader of the slot goes from the pass to this call's tail)
            CHECK(holds[s.slot] == tok, "claimed slot holds another batch");
            scanned[id]++;
        } else {
            CHECK(s.prep_self == (c.prepped_slot != s.slot), "prep_self does not say whether the call's queries are in its slot");
            if (s.prep_self) write(s.slot, tok);
            take(id, s.slot);
        }
        prepped_tok = -1;
        const int j = (s.slot - s.base + RQ_RING_SLOTS) % RQ_RING_SLOTS;
        switch (s.role) {
        case ROLE_SINGLE:
            pairs_done = 0;
            launches++;
            if (s.next_slot >= 0) write(s.next_slot, hint_tok);   // (same launch as the scan and the riding tail: both still readers)
            scan(id);
            run_pending();
            pending = id;
            break;
        case ROLE_PAIR_FIRST:
            CHECK(announces && s.next_slot >= 0, "pair without an announced batch");
            write(s.next_slot, hint_tok);
            run_pending();
            member[0] = id; await_tok = hint_tok;
            pass(1, s.slot, s.next_slot);
            break;
        case ROLE_OPEN:
            CHECK(limit == RQ_BUNDLE_MAX, "a bundle of four with scan_bundle = 2");
            CHECK(pairs_done >= RQ_BUNDLE_STREAK, "a bundle of four opens before three matched pairs in a row");
            CHECK(s.slot % RQ_BUNDLE_MAX == 0, "a bundle of four does not start an aligned quarter");
            CHECK(pending < 0, "a bundle of four opens while a tail still waits");
            CHECK(s.next_slot < 0, "the opening call prepares nothing ahead");
            member[0] = id; await_tok = hint_tok;
            break;
        case ROLE_JOIN:
            CHECK(j == 1 && s.next_slot == bundle_slot_after(s.slot), "join");
            write(s.next_slot, hint_tok);
            member[j] = id; await_tok = hint_tok;
            break;
        case ROLE_JOIN_PASS:
            CHECK(j == 2 && s.n == RQ_BUNDLE_MAX && s.next_slot == bundle_slot_after(s.slot), "join + pass");
            write(s.next_slot, hint_tok);
            member[j] = id; await_tok = hint_tok;
            run_pending();
            pass(3, s.base, s.next_slot);
            break;
        case ROLE_CLOSE:
            CHECK(j == s.n - 1 && s.n >= 2 && s.n <= 3, "close");
            member[j] = id; await_tok = -1;
            run_pending();
            pass(s.n, s.base, -1);
            tails_launch(s.n, s.next_slot, hint_tok);
            pairs_done += s.n / 2;
            break;
        case ROLE_CLAIM:
            CHECK(j == s.n - 1 && (s.n == 2 || s.n == RQ_BUNDLE_MAX), "claim");
            member[j] = id; await_tok = -1;
            readers[s.slot]--; take(id, s.slot);   // pass -> tail
            tails_launch(s.n, s.next_slot, hint_tok);
            pairs_done += s.n / 2;
            break;
        default: break;
        }
        if (s.next_slot >= 0) { prepped_tok = hint_tok; prepped_slot = s.next_slot; CHECK(announces, "a slot for a batch nobody announced"); }
        CHECK(st.streak == pairs_done, "the plan's streak is not the pairs the model saw complete");
        hint_tok = -1;
    }
};

static char seq[16];
static void dfs(const Model& m, int depth, int maxdepth) {
    static const char ev[4] = {'A', 'N', 'M', 'F'};
    for (int e = 0; e < 4; ++e) {
        Model n = m;
        seq[depth] = ev[e]; seq[depth + 1] = 0;
        cur_seq = seq;
        if (e == 0) n.call(true, true);
        else if (e == 1) n.call(true, false);
        else if (e == 2) n.call(false, true);
        else n.flush();
        if (depth + 1 < maxdepth) dfs(n, depth + 1, maxdepth);
        else { n.flush(); sequences++; }
    }
}

int main() {
    for (int limit : {2, 4}) {
        Model m; m.limit = limit;
        dfs(m, 0, limit == 4 ? 12 : 9);
    }
    // hinted loops: n calls, all but the last announce, then a flush
    static char name[32];
    for (int limit : {2, 4})
        for (int n = 1; n <= 40; ++n) {
            std::snprintf(name, sizeof name, "loop n=%d limit=%d", n, limit);
            cur_seq = name;
            Model m; m.limit = limit;
            for (int i = 0; i < n; ++i) m.call(true, i + 1 < n);
            m.flush();
            const int want = limit == 4 && n >= 6 ? 3 + (n - 6 + 3) / 4 : (n + 1) / 2;
            CHECK(m.launches == want, "launch count of a hinted loop");
            const int want4 = limit == 4 && n >= 6 ? (n - 6) / 4 + ((n - 6) % 4 == 3) : 0;
            CHECK(m.bundles4 == want4, "256-query passes of a hinted loop");
        }
    std::printf("%ld sequences\n%ld failures\n", sequences, failures);
    return failures ? 1 : 0;
}
