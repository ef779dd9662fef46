// rq_bundle_plan.h -- bundles of scanned-ahead calls (options "scan_ahead" / "scan_bundle"): what a fused call of a
// stream does with the calls before it, decided before anything is launched.  A bundle is up to four consecutive 64-query calls
// of one stream that ONE corpus pass scans (128 queries for two members, 256 for three or four) and ONE launch finishes; a pair
// is a bundle of two.  Host only: plain integers, no HIP type, nothing of the index (tests/native/bundle_plan_check.cpp runs
// every event sequence through it).  rq_search.hip executes the steps.
//
// States of a stream:
//   IDLE     nothing waits (a lone fused call's tail may, that is rq_search.hip's fused_pending)
//   GATHER   n = 1..2 members have been accepted and NOT scanned yet; the batch the last one announced is awaited
//   AHEAD    a pass has scanned n = 1 or 3 members and, ahead, the batch the last of them announced; their tails wait for it
// Events: a call (BundleCall) or the end of the loop (flush, release, another route, a mutation of the index: bundle_end).
// A bundle of four may open only after RQ_BUNDLE_STREAK matched pairs back to back: hinted loops of up to six calls keep the
// launches they had when pairs were the only bundles, and a loop has proven itself steady before results are held back longer.
//
// Ring slots: the prepared queries of a stream live in RQ_RING_SLOTS slots of 64 queries, contiguous in memory.  The members of
// a bundle take consecutive slots (a bundle of four an aligned quarter, 0..3 or 4..7, so that its pass reads ONE block of 256
// queries); the batch announced after a bundle is prepared by the bundle's tail launch into a slot none of its tails reads.
#pragma once

static const int RQ_RING_SLOTS = 8;
static const int RQ_BUNDLE_MAX = 4;
static const int RQ_BUNDLE_STREAK = 3;

enum BundlePhase { BUNDLE_IDLE = 0, BUNDLE_GATHER = 1, BUNDLE_AHEAD = 2 };

struct BundleState {
    int phase = BUNDLE_IDLE;
    int n = 0;                       // GATHER: members waiting for their pass; AHEAD: members whose tails wait (the awaited batch is member n)
    int base = 0;                    // ring slot of member 0; member j sits in (base + j) % RQ_RING_SLOTS
    int last = RQ_RING_SLOTS - 1;    // the last ring slot handed out
    int streak = 0;                  // matched pairs completed back to back (a bundle of four counts as two)
};

// What the plan has to know of a call.
struct BundleCall {
    bool fused = false;       // a fused call ("pipeline" = 2, <= 64 queries, fast tail)
    bool eligible = false;    // ... that may be scanned with others: fp16 rows of 768 elements, no filter, shard beyond the size rule, "scan_ahead" on
    bool matches = false;     // ... and brings exactly the batch (pointer, B, metric) the stream's open bundle awaits
    bool announces = false;   // the stream has announced the batch after this one (B <= 64)
    bool full = false;        // B == 64: only the last member of a bundle may be ragged
    bool next_full = false;   // the announced batch has 64 queries
    int prepped_slot = -1;    // ring slot that already holds this call's prepared queries (-1: none)
    bool other = false;       // the stream had announced a batch for this call and it brings another one: an unmatched call
};

enum BundleBreak { BREAK_NONE = 0, BREAK_SCAN, BREAK_TAILS };
enum BundleRole {
    ROLE_OTHER = 0,     // not fused: no ring slot
    ROLE_SINGLE,        // a fused call on its own (its launch carries the tail waiting before it and prepares the announced batch)
    ROLE_PAIR_FIRST,    // scans itself and the announced batch in one 128-query pass                     -> AHEAD, n = 1
    ROLE_OPEN,          // member 0 of a bundle of four: launches no pass                                 -> GATHER, n = 1
    ROLE_JOIN,          // member 1: prepares itself and the announced batch in ONE launch, no pass       -> GATHER, n = 2
    ROLE_JOIN_PASS,     // member 2: prepares the announced batch, then ONE 256-query pass over all four  -> AHEAD, n = 3
    ROLE_CLOSE,         // last member of a bundle cut short (it announces nothing, or is ragged): pass over the n members, their tails in one launch
    ROLE_CLAIM          // the batch scanned ahead has come: no scan, ONE launch with the tails of all n members
};

struct BundleStep {
    // first: what becomes of the bundle this event does not continue
    int brk = BREAK_NONE;   // BREAK_SCAN: brk_n gathered members are scanned now by the narrowest pass (64 / 128 / 256 with 192 valid);
    int brk_n = 0;          // BREAK_TAILS: the brk_n scanned members' tails complete, the batch scanned ahead is discarded.
    int brk_base = 0;       // One waiting tail (brk_n = 1) becomes the stream's pending tail, several run in one launch at once.
    // then: the call itself
    int role = ROLE_OTHER;
    int slot = -1;          // ring slot of the call's own queries
    bool prep_self = false; // ... which this call has to prepare
    int next_slot = -1;     // ring slot the announced batch is prepared into by work of this call (-1: none)
    int n = 0, base = 0;    // ROLE_JOIN_PASS / ROLE_CLOSE / ROLE_CLAIM: members of the pass or tail launch (this call included), slot of member 0
};

static inline int bundle_slot_after(int slot) { return (slot + 1) % RQ_RING_SLOTS; }
static inline int bundle_quarter_after(int slot) { return ((slot / RQ_BUNDLE_MAX + 1) * RQ_BUNDLE_MAX) % RQ_RING_SLOTS; }
// The slot of the batch announced behind a call whose own slot is st.last: the start of the other quarter when the next call may
// open a bundle of four (no tail that is still to run reads from there: a bundle's members share the quarter of its last slot, a
// pair's first member sits at most one slot back), else the next slot.
static inline int bundle_next_slot(const BundleState& st, int limit) {
    return limit >= RQ_BUNDLE_MAX && st.streak >= RQ_BUNDLE_STREAK ? bundle_quarter_after(st.last) : bundle_slot_after(st.last);
}

// The loop ends here (flush, release, a call of another route, a mutation of the index): only the break fields are set.
static inline BundleStep bundle_end(BundleState& st) {
    BundleStep s;
    if (st.phase == BUNDLE_GATHER) s.brk = BREAK_SCAN;
    if (st.phase == BUNDLE_AHEAD) s.brk = BREAK_TAILS;
    s.brk_n = st.phase == BUNDLE_IDLE ? 0 : st.n;
    s.brk_base = st.base;
    st.phase = BUNDLE_IDLE; st.n = 0; st.streak = 0;
    return s;
}

// limit: option "scan_bundle" (2: pairs only, 4).
static inline BundleStep bundle_call(BundleState& st, const BundleCall& c, int limit) {
    BundleStep s;
    const bool cont = st.phase != BUNDLE_IDLE && c.fused && c.eligible && c.matches;
    if (cont && st.phase == BUNDLE_AHEAD) {
        s.role = ROLE_CLAIM; s.n = st.n + 1; s.base = st.base;
        s.slot = (st.base + st.n) % RQ_RING_SLOTS;
        st.phase = BUNDLE_IDLE; st.n = 0; st.streak += s.n / 2;
        st.last = s.slot;
        if (c.announces) st.last = s.next_slot = bundle_next_slot(st, limit);
        return s;
    }
    if (cont) {   // GATHER
        const int members = st.n + 1;
        s.slot = (st.base + st.n) % RQ_RING_SLOTS;
        s.prep_self = c.prepped_slot != s.slot;
        s.base = st.base;
        st.last = s.slot;
        if (c.full && c.announces && members < RQ_BUNDLE_MAX - 1) {
            s.role = ROLE_JOIN; st.n = members;
            st.last = s.next_slot = bundle_slot_after(s.slot);
        } else if (c.full && c.announces) {
            s.role = ROLE_JOIN_PASS; s.n = RQ_BUNDLE_MAX;
            st.phase = BUNDLE_AHEAD; st.n = members;
            st.last = s.next_slot = bundle_slot_after(s.slot);
        } else {
            s.role = ROLE_CLOSE; s.n = members;
            st.phase = BUNDLE_IDLE; st.n = 0; st.streak += members / 2;
            if (c.announces) st.last = s.next_slot = bundle_next_slot(st, limit);
        }
        return s;
    }
    const int streak0 = st.streak;
    const BundleStep brk = bundle_end(st);   // a call that breaks a bundle, brings another batch than the announced one or runs on its own ends the streak
    const int streak = brk.brk == BREAK_NONE && !c.other ? streak0 : 0;
    s.brk = brk.brk; s.brk_n = brk.brk_n; s.brk_base = brk.brk_base;
    if (!c.fused) return s;   // ROLE_OTHER
    const bool may_open = limit >= RQ_BUNDLE_MAX && brk.brk == BREAK_NONE && streak >= RQ_BUNDLE_STREAK && c.eligible && c.announces && c.full && c.next_full &&
                          (c.prepped_slot < 0 || c.prepped_slot % RQ_BUNDLE_MAX == 0);
    s.slot = c.prepped_slot >= 0 ? c.prepped_slot : (may_open ? bundle_quarter_after(st.last) : bundle_slot_after(st.last));
    s.prep_self = c.prepped_slot < 0;
    s.base = s.slot;
    st.last = s.slot;
    if (may_open) {
        s.role = ROLE_OPEN;
        st.phase = BUNDLE_GATHER; st.n = 1; st.base = s.slot; st.streak = streak;
    } else if (c.eligible && c.announces) {
        s.role = ROLE_PAIR_FIRST; s.n = 2;
        st.phase = BUNDLE_AHEAD; st.n = 1; st.base = s.slot; st.streak = streak;
        st.last = s.next_slot = bundle_slot_after(s.slot);
    } else {
        s.role = ROLE_SINGLE;
        if (c.announces) st.last = s.next_slot = bundle_slot_after(s.slot);
    }
    return s;
}
