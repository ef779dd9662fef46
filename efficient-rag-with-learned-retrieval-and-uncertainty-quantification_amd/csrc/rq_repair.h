// rq_repair.h -- what the repairs of the device forms share (fixup_ladder in rq_search.hip, range_fixup in rq_range.hip, grouped_fixup
// in rq_group.hip, group_members_fixup in rq_group_members.hip; fixup_filtered_each in rq_filter_each.hip packs the flagged queries of a scattered group the same way
// before it hands them to fixup_ladder).  A repair reads the call's d_status and waits, lists the flagged queries, PACKS their inputs into the first slots of
// buffers of its own, runs them again, and UNPACKS the packed outputs over the flagged queries' outputs; the other queries' outputs are
// not touched.  A column is one array of the call ("full", one entry per query) with its packed twin (one entry per slot) and the bytes
// of an entry; a null column (the optional keys) is skipped.  Every copy is one D2D copy on the Stage's stream (rq_stage.h), in the
// order pair by pair, column by column; after a failure nothing more is enqueued and the Stage waits before the caller's buffers die.
// Host only; tests/native/stage_check.cpp runs the column sets of the three repairs against stand-ins for the HIP calls.
#pragma once
#include "rq_stage.h"

struct RepairPair { int slot, q; };   // slot of the packed buffers <-> query of the call
typedef std::vector<RepairPair> RepairList;
struct RepairColumn { char* full; char* packed; size_t bytes; };
template <class T> RepairColumn repair_col(const T* full, const T* packed, size_t per_query) { return {(char*)full, (char*)packed, per_query * sizeof(T)}; }

// d_status[0..n) on the host: copied on the stage's stream and waited for
inline int repair_status(Stage& st, const int* d_status, int n, std::vector<int>& h) {
    h.resize((size_t)n);
    st.down(h.data(), d_status, (size_t)n * sizeof(int));
    return st.finish();
}
// appends the queries of [0, B) whose status is not zero, in query order, in slots 0, 1, ...
inline int repair_flagged(Stage& st, const int* d_status, int B, RepairList& bad) {
    std::vector<int> h;
    const int r = repair_status(st, d_status, B, h);
    for (int q = 0; r == RQ_OK && q < B; ++q) if (h[(size_t)q] != 0) bad.push_back({(int)bad.size(), q});
    return r;
}
// full[q] -> packed[slot] for every pair
inline int repair_pack(Stage& st, const RepairList& list, std::initializer_list<RepairColumn> cols) {
    for (const RepairPair& p : list)
        for (const RepairColumn& c : cols)
            if (c.full) st.d2d(c.packed + (size_t)p.slot * c.bytes, c.full + (size_t)p.q * c.bytes, c.bytes);
    return st.code();
}
// packed[slot] -> full[q] for every pair (any sub-list of the packed one); with `clear`, clear[q] = 0 follows each pair's copies
inline int repair_unpack(Stage& st, const RepairList& list, std::initializer_list<RepairColumn> cols, int* clear = nullptr) {
    for (const RepairPair& p : list) {
        for (const RepairColumn& c : cols)
            if (c.full) st.d2d(c.full + (size_t)p.q * c.bytes, c.packed + (size_t)p.slot * c.bytes, c.bytes);
        if (clear) st.zero(clear + p.q, sizeof(int));
    }
    return st.code();
}
