// Host-side check of csrc/rq_stage.h, the staging of the blocking host-buffer calls (rq_search_filtered, rq_search_mmr,
// rq_score_rows, rq_search_range, rq_search_grouped), and of csrc/rq_repair.h, the packing and unpacking of the three repairs
// (fixup_ladder, range_fixup, grouped_fixup).  The six HIP calls the helpers make -- allocate, free, asynchronous copy, asynchronous
// memset, stream synchronisation, last error -- are STAND-INS defined here, at link time: they keep a log, can be told to fail at a
// given call, and work on real host memory of the requested size, so that -fsanitize=address,undefined sees every copy, a double
// free and a leak.  The calls are driven in the order the entry points and the repairs use, with the sizes of their own pure sizing
// functions.  The stand-ins are test scaffolding: nothing in the product links them.
//   hipcc -O1 -g -std=c++17 --offload-host-only -fsanitize=address,undefined -I <csrc> tests/native/stage_check.cpp -o stage_check
#include "rq_repair.h"
#include "rq_mmr_plan.h"
#include "rq_score_plan.h"
#include "rq_range_plan.h"
#include "rq_group_plan.h"

#include <cstdlib>
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

// ---- the stand-ins ----------------------------------------------------------------------------------------------------------
// log: M allocate, F free, U copy to the device, D copy to the host, X copy within the device, Z memset, S synchronise, E last error
// read, K the device form ran.  Copies and memsets are counted together: g_fail_copy fails either.
static std::string g_log;
static std::set<void*> g_live;
static int g_bad_free = 0, g_mallocs = 0, g_copies = 0, g_syncs = 0;
static int g_fail_malloc = -1, g_fail_copy = -1, g_fail_sync = -1;   // the call (counted from 0) that fails; -1: none
static int g_stream_tag = 0;
static hipStream_t const g_stream = (hipStream_t)(void*)&g_stream_tag;

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    g_log += 'M';
    if (g_mallocs++ == g_fail_malloc) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    g_log += 'F';
    if (!g_live.erase(p)) { ++g_bad_free; return hipErrorInvalidValue; }   // never allocated, or freed before
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    g_log += kind == hipMemcpyHostToDevice ? 'U' : kind == hipMemcpyDeviceToHost ? 'D' : kind == hipMemcpyDeviceToDevice ? 'X' : '?';
    if (s != g_stream) g_log += '!';
    if (g_copies++ == g_fail_copy) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
    g_log += 'Z';
    if (s != g_stream) g_log += '!';
    if (g_copies++ == g_fail_copy) return hipErrorInvalidValue;
    std::memset(dst, value, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t s) {
    g_log += 'S';
    if (s != g_stream) g_log += '!';
    return g_syncs++ == g_fail_sync ? hipErrorUnknown : hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) {
    g_log += 'E';
    return hipSuccess;
}

// ---- one blocking call, as the entry points write it ---------------------------------------------------------------------------
struct Copy { int buf; size_t bytes; };
struct Shape {
    const char* name;
    std::vector<size_t> bytes;       // the staging buffers, in allocation order
    std::vector<Copy> ups, downs;    // the copies, in order
    const char* want;                // the log of a call that succeeds
};
static std::vector<char> g_host;     // the caller's memory: large enough for every copy of every shape

static int run_call(const Shape& sh, int device_rc) {
    Stage st(g_stream);
    if (int r = st.alloc(sh.bytes.data(), (int)sh.bytes.size(), sh.name)) return r;
    for (const Copy& c : sh.ups) st.up(st.at<char>(c.buf), g_host.data(), c.bytes);
    if (st.code() != RQ_OK) return st.code();
    g_log += 'K';
    if (device_rc != RQ_OK) return device_rc;
    for (const Copy& c : sh.downs) st.down(g_host.data(), st.at<char>(c.buf), c.bytes);
    return st.finish();
}
static void start(int fail_malloc, int fail_copy, int fail_sync) {
    g_log.clear();
    g_bad_free = g_mallocs = g_copies = g_syncs = 0;
    g_fail_malloc = fail_malloc; g_fail_copy = fail_copy; g_fail_sync = fail_sync;
    g_err[0] = 0;
}
static void check_left_clean(const char* name) {
    CHECK(g_live.empty() && g_bad_free == 0, "%s [%s]: %zu buffers left, %d bad frees", name, g_log.c_str(), g_live.size(), g_bad_free);
    CHECK(g_log.find('!') == std::string::npos && g_log.find('?') == std::string::npos, "%s [%s]: another stream or copy kind", name, g_log.c_str());
}
static int run(const Shape& sh, int fail_malloc, int fail_copy, int fail_sync, int device_rc = RQ_OK) {
    start(fail_malloc, fail_copy, fail_sync);
    const int rc = run_call(sh, device_rc);
    check_left_clean(sh.name);
    return rc;
}
static int count(char c) { return (int)std::count(g_log.begin(), g_log.end(), c); }
// every buffer allocated was freed once (run() has checked the pointers), after a wait if anything had been enqueued, and nothing
// was enqueued after the failure at log position `at`
static void check_failed_call(const char* name, int allocated, size_t at) {
    CHECK(count('F') == allocated, "%s [%s]: %d frees of %d buffers", name, g_log.c_str(), count('F'), allocated);
    const size_t first_free = g_log.find('F'), first_copy = g_log.find_first_of("UDXZ");
    if (first_copy != std::string::npos && first_free != std::string::npos) {
        const size_t last_sync = g_log.rfind('S', first_free);
        CHECK(last_sync != std::string::npos && last_sync > at, "%s [%s]: no wait between the failure and the first free", name, g_log.c_str());
    }
    CHECK(g_log.find_first_of("UDXZK", at + 1) == std::string::npos, "%s [%s]: work issued after the failure", name, g_log.c_str());
}
static void check_failed_call(const Shape& sh, int allocated, size_t at) { check_failed_call(sh.name, allocated, at); }

// ---- the repairs (rq_repair.h) --------------------------------------------------------------------------------------------------
// The arrays of a call ("full": one entry per query) and of its repair ("packed": one entry per flagged query), each allocated at
// exactly its size.  Full bytes hold a pattern of (column, query, byte), packed bytes one of (column, slot, byte), and the stand-in for
// the re-run answers slot i with a pattern of (column, the query whose vector it finds in slot i, byte).
enum { LADDER, RANGE, GROUPED };
enum { C_Q, C_THR, C_SCORES, C_ROWS, C_KEYS, C_GROUPS, C_COUNT, C_STATUS, C_N };
enum { FULL, PACKED, ANSWER };
static const int R_DIM = 33, R_K = 5, R_M = 7;   // (R_M: the candidate rows per query of the grouped repair's rung 2)
static const size_t col_bytes[C_N] = {R_DIM * sizeof(float), sizeof(float), R_K * sizeof(float), R_K * sizeof(int64_t), R_K * sizeof(uint64_t),
                                      R_K * sizeof(int32_t), sizeof(int64_t), sizeof(int)};
static const char* const kind_name[3] = {"the ladder", "the range repair", "the grouped repair"};
static bool has_col(int kind, int c) { return c == C_THR || c == C_COUNT ? kind == RANGE : c == C_GROUPS ? kind == GROUPED : true; }
static bool is_answer(int c) { return c != C_Q && c != C_THR && c != C_STATUS; }
static char pat(int side, int c, int idx, size_t b) { return (char)((c + 1) * 37 + idx * 101 + (int)b * 13 + side * 59); }   // (101 is odd: 256 entries differ)

struct Arrays {
    int kind, B;
    std::vector<char> full[C_N], work[C_N];
    char* packed[C_N] = {};
    Arrays(int kind_, int B_, const std::vector<int>& flagged, bool keys) : kind(kind_), B(B_) {
        for (int c = 0; c < C_N; ++c) {
            if (!has_col(kind, c) || (c == C_KEYS && !keys)) continue;
            full[c].resize((size_t)B * col_bytes[c]);
            for (int q = 0; q < B; ++q)
                for (size_t b = 0; b < col_bytes[c]; ++b) full[c][(size_t)q * col_bytes[c] + b] = pat(FULL, c, q, b);
        }
        for (int q = 0; q < B; ++q) d_status()[q] = 0;
        for (int q : flagged) d_status()[q] = 1;
    }
    int* d_status() { return (int*)full[C_STATUS].data(); }
    void fill_packed(int nb) {
        for (int c = 0; c < C_N; ++c)
            for (size_t i = 0; packed[c] && i < (size_t)nb * col_bytes[c]; ++i) packed[c][i] = pat(PACKED, c, (int)(i / col_bytes[c]), i % col_bytes[c]);
    }
    void own_packed(int nb) {   // (the ladder's packed arrays are its workspace's; the other two allocate theirs through the Stage)
        for (int c = 0; c < C_N; ++c) {
            if (full[c].empty() || nb == 0) continue;
            work[c].resize((size_t)nb * col_bytes[c]);
            packed[c] = work[c].data();
        }
        fill_packed(nb);
    }
    RepairColumn col(int c) { return {full[c].empty() ? nullptr : full[c].data(), packed[c], col_bytes[c]}; }
    int pack(Stage& st, const RepairList& l) {
        if (kind == RANGE) return repair_pack(st, l, {col(C_Q), col(C_THR)});
        return repair_pack(st, l, {col(C_Q)});
    }
    int unpack(Stage& st, const RepairList& l) {
        if (kind == LADDER) return repair_unpack(st, l, {col(C_SCORES), col(C_ROWS), col(C_KEYS)}, d_status());
        if (kind == RANGE) return repair_unpack(st, l, {col(C_SCORES), col(C_ROWS), col(C_KEYS), col(C_COUNT), col(C_STATUS)});
        if (int r = repair_unpack(st, l, {col(C_SCORES), col(C_ROWS), col(C_GROUPS), col(C_KEYS)})) return r;
        return repair_unpack(st, l, {}, d_status());
    }
    bool entry_is(int c, int q, int side, int idx) const {
        for (size_t b = 0; b < col_bytes[c]; ++b)
            if (full[c][(size_t)q * col_bytes[c] + b] != pat(side, c, idx, b)) return false;
        return true;
    }
};

// pack, then unpack every second pair: exactly the listed entries change, to the right slot's bytes
static void check_columns(int kind, int B, const std::vector<int>& flagged, bool keys) {
    const char* name = kind_name[kind];
    start(-1, -1, -1);
    Arrays a(kind, B, flagged, keys);
    Stage st(g_stream);
    RepairList l;
    CHECK(repair_flagged(st, a.d_status(), B, l) == RQ_OK && l.size() == flagged.size(), "%s, B %d: %zu flagged", name, B, l.size());
    for (size_t i = 0; i < l.size() && i < flagged.size(); ++i) CHECK(l[i].slot == (int)i && l[i].q == flagged[i], "%s, B %d: pair %zu = (%d, %d)", name, B, i, l[i].slot, l[i].q);
    const int nb = (int)l.size();
    a.own_packed(nb);
    CHECK(a.pack(st, l) == RQ_OK, "%s, B %d: pack", name, B);
    for (int c : {C_Q, C_THR})
        for (const RepairPair& p : l)
            if (a.packed[c]) CHECK(std::memcmp(a.packed[c] + (size_t)p.slot * col_bytes[c], a.full[c].data() + (size_t)p.q * col_bytes[c], col_bytes[c]) == 0, "%s, B %d: column %d of slot %d is not query %d's", name, B, c, p.slot, p.q);
    for (int c = C_SCORES; c < C_N; ++c)
        for (size_t i = 0; a.packed[c] && i < (size_t)nb * col_bytes[c]; ++i) CHECK(a.packed[c][i] == pat(PACKED, c, (int)(i / col_bytes[c]), i % col_bytes[c]), "%s, B %d: pack wrote column %d", name, B, c);
    RepairList sub;
    std::vector<int> slot_of((size_t)B, -1);
    for (int i = 0; i < nb; i += 2) { sub.push_back(l[(size_t)i]); slot_of[(size_t)l[(size_t)i].q] = l[(size_t)i].slot; }
    CHECK(a.unpack(st, sub) == RQ_OK && st.finish() == RQ_OK, "%s, B %d: unpack", name, B);
    for (int c = 0; c < C_N; ++c) {
        if (a.full[c].empty()) continue;
        const bool out = is_answer(c) || (c == C_STATUS && kind == RANGE);
        for (int q = 0; q < B; ++q) {
            const int slot = slot_of[(size_t)q];
            if (c == C_STATUS && !out) CHECK(a.d_status()[q] == (slot >= 0 || !std::count(flagged.begin(), flagged.end(), q) ? 0 : 1), "%s, B %d: status of query %d", name, B, q);
            else if (out && slot >= 0) CHECK(a.entry_is(c, q, PACKED, slot), "%s, B %d: column %d of query %d is not slot %d's", name, B, c, q, slot);
            else if (c != C_STATUS) CHECK(a.entry_is(c, q, FULL, q), "%s, B %d: column %d of query %d changed", name, B, c, q);
            else CHECK(a.d_status()[q] == (std::count(flagged.begin(), flagged.end(), q) ? 1 : 0), "%s, B %d: status of query %d changed", name, B, q);
        }
    }
    check_left_clean(name);
}

// The re-run: slot i is answered from the query vector found there; with `odd_fail` the odd slots stay uncertified.
static void rerun(Arrays& a, int n, bool odd_fail) {
    g_log += 'K';
    for (int i = 0; i < n; ++i) {
        const int tag = (unsigned char)a.packed[C_Q][(size_t)i * col_bytes[C_Q]];
        for (int c = 0; c < C_N; ++c)
            for (size_t b = 0; is_answer(c) && a.packed[c] && b < col_bytes[c]; ++b) a.packed[c][(size_t)i * col_bytes[c] + b] = pat(ANSWER, c, tag, b);
        ((int*)a.packed[C_STATUS])[i] = odd_fail && (i & 1) ? 1 : 0;
    }
}
// One repair as its fixup writes it (rq_search.hip fixup_ladder, rq_range.hip range_fixup, rq_group.hip grouped_fixup without rung 3).
static int repair_call(Arrays& a, bool keys, bool odd_fail) {
    Stage fx(g_stream);
    RepairList bad;
    if (int r = repair_flagged(fx, a.d_status(), a.B, bad)) return r;
    if (bad.empty()) return 0;
    const int nb = (int)bad.size();
    if (a.kind == LADDER) {
        a.own_packed(nb);
        for (int rung = 0; rung < 2 && !bad.empty(); ++rung) {
            const int nbq = (int)bad.size();
            if (int r = a.pack(fx, bad)) return r;
            rerun(a, nbq, odd_fail && rung == 0);
            std::vector<int> st2;
            if (int r = repair_status(fx, (const int*)a.packed[C_STATUS], nbq, st2)) return r;
            RepairList done, still;
            for (const RepairPair& p : bad) {
                if (st2[(size_t)p.slot] == 0) done.push_back(p);
                else still.push_back({(int)still.size(), p.q});
            }
            a.unpack(fx, done);
            if (int r = fx.finish()) return r;
            bad.swap(still);
        }
        return nb;
    }
    if (a.kind == RANGE) {
        const RangeStaging sz = range_staging(R_DIM, nb, R_K);
        const size_t bytes[7] = {sz.q, sz.thr, sz.scores, sz.rows, sz.rows, sz.count, sz.status};
        if (int r = fx.alloc(bytes, 7, kind_name[RANGE])) return r;
        const int at[7] = {C_Q, C_THR, C_SCORES, C_ROWS, C_KEYS, C_COUNT, C_STATUS};
        for (int i = 0; i < 7; ++i) a.packed[at[i]] = at[i] == C_KEYS && !keys ? nullptr : fx.at<char>(i);
        a.fill_packed(nb);
        if (int r = a.pack(fx, bad)) return r;
        rerun(a, nb, false);
        if (int r = a.unpack(fx, bad)) return r;
        if (int r = fx.finish()) return r;
        return nb;
    }
    const GroupStaging sz = group_staging(R_DIM, nb, R_M, R_K);
    const size_t bytes[9] = {sz.q, sz.cand_scores, sz.cand_rows, sz.cand_status, sz.out_scores, sz.out_rows, sz.out_groups, sz.out_keys, sz.status};
    if (int r = fx.alloc(bytes, 9, kind_name[GROUPED])) return r;
    fx.launched();
    a.packed[C_Q] = fx.at<char>(0); a.packed[C_SCORES] = fx.at<char>(4); a.packed[C_ROWS] = fx.at<char>(5); a.packed[C_GROUPS] = fx.at<char>(6);
    a.packed[C_KEYS] = fx.at<char>(7); a.packed[C_STATUS] = fx.at<char>(8);
    a.fill_packed(nb);
    if (int r = a.pack(fx, bad)) return r;
    rerun(a, nb, false);
    std::vector<char> h_scores(sz.out_scores), h_rows(sz.out_rows), h_groups(sz.out_groups), h_status(sz.status);
    fx.down(h_scores.data(), a.packed[C_SCORES], sz.out_scores);
    fx.down(h_rows.data(), a.packed[C_ROWS], sz.out_rows);
    fx.down(h_groups.data(), a.packed[C_GROUPS], sz.out_groups);
    fx.down(h_status.data(), a.packed[C_STATUS], sz.status);
    if (int r = fx.finish()) return r;
    fx.launched();
    if (int r = a.unpack(fx, bad)) return r;
    if (int r = fx.finish()) return r;
    return nb;
}
static std::string times(const char* s, int n) { std::string r; while (n-- > 0) r += s; return r; }
// The log of a repair that succeeds, READ FROM THE CODE BEFORE rq_repair.h EXISTED (the copy loops of the three fixups as they stood
// when each wrote its own), per flagged query:
//   ladder (rq_search.hip:682-752 at that commit, fixup_ladder): the status read and its wait "DS"; per rung one query copy each "X", the re-run, the packed
//     status read and its wait "DS", per certified slot scores, rows, keys if given and the status memset "XXXZ", then the rung's
//     second wait "S".  With odd_fail the even slots certify at the first rung and the others at the second.
//   range (rq_range.hip:312-345, range_fixup): "DS", seven buffers, per query the vector and the threshold "XX", the re-run, per query scores,
//     rows, keys if given, count, status "XXXXX", the wait, seven frees.
//   grouped (rq_group.hip:324-393, grouped_fixup): "DS", nine buffers (then four in one Stage and five in another), one vector copy per query,
//     the re-run (search, ladder, collapse), four copies down and their wait "DDDDS", per query scores, rows, groups, keys if given
//     "XXXX", then one status memset per query, the wait, nine frees.  (The second Stage used to wait once more, on the idle stream
//     between its frees and the first one's: "SFFFFFSFFFF".  That wait belonged to the second object and went with it.)
static std::string repair_log(int kind, int nb, bool keys, bool odd_fail) {
    if (nb == 0) return "DS";
    if (kind == LADDER) {
        const char* slot = keys ? "XXXZ" : "XXZ";
        const int later = odd_fail ? nb / 2 : 0;
        std::string r = "DS" + times("X", nb) + "KDS" + times(slot, nb - later) + "S";
        if (later) r += times("X", later) + "KDS" + times(slot, later) + "S";
        return r;
    }
    if (kind == RANGE) return "DSMMMMMMM" + times("XX", nb) + "K" + times(keys ? "XXXXX" : "XXXX", nb) + "SFFFFFFF";
    return "DSMMMMMMMMM" + times("X", nb) + "KDDDDS" + times(keys ? "XXXX" : "XXX", nb) + times("Z", nb) + "SFFFFFFFFF";
}
static void check_repair(int kind, int B, const std::vector<int>& flagged, bool keys, bool odd_fail) {
    const char* name = kind_name[kind];
    const int nb = (int)flagged.size();
    const std::string want = repair_log(kind, nb, keys, odd_fail);
    {   // ---- success: the sequence of calls, the answers in the flagged queries' places, everything else as it was, every status 0
        start(-1, -1, -1);
        Arrays a(kind, B, flagged, keys);
        CHECK(repair_call(a, keys, odd_fail) == nb && g_log == want, "%s, B %d: [%s], expected [%s]", name, B, g_log.c_str(), want.c_str());
        check_left_clean(name);
        for (int c = 0; c < C_STATUS; ++c)
            for (int q = 0; q < B && !a.full[c].empty(); ++q) {
                const bool fl = std::count(flagged.begin(), flagged.end(), q) != 0;
                if (fl && is_answer(c)) CHECK(a.entry_is(c, q, ANSWER, (unsigned char)pat(FULL, C_Q, q, 0)), "%s, B %d: column %d of query %d is not its answer", name, B, c, q);
                else CHECK(a.entry_is(c, q, FULL, q), "%s, B %d: column %d of query %d changed", name, B, c, q);
            }
        for (int q = 0; q < B; ++q) CHECK(a.d_status()[q] == 0, "%s, B %d: status of query %d", name, B, q);
    }
    // ---- every copy and memset fails in turn: RQ_EHIP, it is the last thing enqueued, the stream is waited for after it and before
    // the first free, every buffer is freed once
    const int ncopy = (int)std::count_if(want.begin(), want.end(), [](char ch) { return ch == 'D' || ch == 'X' || ch == 'Z'; });
    for (int j = 0; j < ncopy; ++j) {
        start(-1, j, -1);
        Arrays a(kind, B, flagged, keys);
        CHECK(repair_call(a, keys, odd_fail) == RQ_EHIP, "%s, B %d, copy %d: [%s]", name, B, j, g_log.c_str());
        check_left_clean(name);
        const size_t at = g_log.find_last_of("DXZ");
        CHECK(count('D') + count('X') + count('Z') == j + 1 && g_log.compare(0, at, want, 0, at) == 0, "%s, B %d, copy %d: [%s]", name, B, j, g_log.c_str());
        CHECK(g_log.find('S', at) != std::string::npos, "%s, B %d, copy %d: [%s] returns without a wait", name, B, j, g_log.c_str());
        check_failed_call(name, count('M'), at);
    }
    // ---- every wait fails in turn: RQ_EHIP, nothing is enqueued after it, and the stream is waited for again before a free
    const int nsync = (int)std::count(want.begin(), want.end(), 'S');
    for (int j = 0; j < nsync; ++j) {
        start(-1, -1, j);
        Arrays a(kind, B, flagged, keys);
        CHECK(repair_call(a, keys, odd_fail) == RQ_EHIP && count('S') == j + 2, "%s, B %d, wait %d: [%s]", name, B, j, g_log.c_str());
        check_left_clean(name);
        size_t at = std::string::npos;
        for (int i = 0; i <= j; ++i) at = g_log.find('S', at + 1);
        check_failed_call(name, count('M'), at);
    }
    // ---- every allocation fails in turn: RQ_ENOMEM, nothing was copied but the status
    for (int i = 0; i < (int)std::count(want.begin(), want.end(), 'M'); ++i) {
        start(i, -1, -1);
        Arrays a(kind, B, flagged, keys);
        CHECK(repair_call(a, keys, odd_fail) == RQ_ENOMEM && g_log == "DS" + std::string((size_t)i + 1, 'M') + "E" + std::string((size_t)i, 'F'), "%s, B %d, allocation %d: [%s]", name, B, i, g_log.c_str());
        check_left_clean(name);
    }
}

int main() {
    const int dim = 33, B = 3, k = 5, m = 20;
    const SearchStaging fs = search_staging(dim, B, k);
    const MmrStaging ms = mmr_staging(dim, B, m, k);
    const ScoreStaging ss = score_staging(dim, B, m);
    CHECK(fs.q == 396 && fs.scores == 60 && fs.rows == 120 && fs.status == 12, "search_staging(33, 3, 5)");
    CHECK(search_staging(768, 65535, 1024).rows == (size_t)65535 * 1024 * 8 && search_staging(1, 32768, 65536).scores == ((size_t)1 << 33), "64-bit sizes");
    CHECK(ms.q == fs.q && ms.status == fs.status && ms.cand_scores == 240 && ms.cand_rows == 480 && ms.out_scores == 60 && ms.out_rows == 120 && ms.out_mmr == 60, "mmr_staging");
    const RangeStaging rs = range_staging(dim, B, k);
    const GroupStaging gs = group_staging(dim, B, k, k);
    CHECK(rs.q == fs.q && rs.thr == 12 && rs.scores == 60 && rs.rows == 120 && rs.count == 24 && rs.status == 12, "range_staging(33, 3, 5)");
    CHECK(gs.q == fs.q && gs.out_scores == 60 && gs.out_rows == 120 && gs.out_groups == 60 && gs.out_keys == 120 && gs.status == 12, "group_staging(33, 3, 5, 5)");
    g_host.assign(std::max({fs.q, ms.cand_rows, ss.rows}), 1);
    const Shape shapes[] = {
        {"a filtered search", {fs.q, fs.scores, fs.rows, fs.status}, {{0, fs.q}}, {{1, fs.scores}, {2, fs.rows}}, "MMMMUKDDSFFFF"},
        {"an MMR search", {ms.q, ms.cand_scores, ms.cand_rows, ms.status, ms.out_scores, ms.out_rows}, {{0, ms.q}}, {{4, ms.out_scores}, {5, ms.out_rows}}, "MMMMMMUKDDSFFFFFF"},
        {"an MMR search with its values", {ms.q, ms.cand_scores, ms.cand_rows, ms.status, ms.out_scores, ms.out_rows, ms.out_mmr}, {{0, ms.q}},
         {{4, ms.out_scores}, {5, ms.out_rows}, {6, ms.out_mmr}}, "MMMMMMMUKDDDSFFFFFFF"},
        {"scoring given rows", {ss.q, ss.rows, ss.scores}, {{0, ss.q}, {1, ss.rows}}, {{2, ss.scores}}, "MMMUUKDSFFF"},
        {"a range search", {rs.q, rs.thr, rs.scores, rs.rows, rs.count, rs.status}, {{0, rs.q}, {1, rs.thr}}, {{2, rs.scores}, {3, rs.rows}, {4, rs.count}},
         "MMMMMMUUKDDDSFFFFFF"},
        {"a grouped search", {gs.q, gs.out_scores, gs.out_rows, gs.out_groups, gs.status}, {{0, gs.q}}, {{1, gs.out_scores}, {2, gs.out_rows}, {3, gs.out_groups}},
         "MMMMMUKDDDSFFFFF"},
    };
    for (const Shape& sh : shapes) {
        const int nbuf = (int)sh.bytes.size(), nup = (int)sh.ups.size(), ncopy = nup + (int)sh.downs.size();
        size_t total = 0;
        for (size_t b : sh.bytes) total += b;
        // ---- success: the exact sequence of calls, one wait, at the end of the copies
        CHECK(run(sh, -1, -1, -1) == RQ_OK && g_log == sh.want, "%s: [%s], expected [%s]", sh.name, g_log.c_str(), sh.want);
        // ---- every allocation fails in turn: RQ_ENOMEM with the total in the message, the earlier buffers freed, the runtime's
        // error read (cleared), nothing enqueued and nothing waited for
        for (int i = 0; i < nbuf; ++i) {
            CHECK(run(sh, i, -1, -1) == RQ_ENOMEM, "%s, allocation %d: [%s]", sh.name, i, g_log.c_str());
            CHECK(std::strstr(g_err, std::to_string(total).c_str()) && std::strstr(g_err, sh.name), "%s, allocation %d: message '%s'", sh.name, i, g_err);
            CHECK(g_log == std::string((size_t)i + 1, 'M') + "E" + std::string((size_t)i, 'F'), "%s, allocation %d: [%s]", sh.name, i, g_log.c_str());
        }
        // ---- every copy fails in turn: RQ_EHIP, it is the last thing enqueued, the stream is waited for before the first free
        for (int j = 0; j < ncopy; ++j) {
            CHECK(run(sh, -1, j, -1) == RQ_EHIP, "%s, copy %d: [%s]", sh.name, j, g_log.c_str());
            CHECK(count('U') + count('D') == j + 1 && count('K') == (j >= nup ? 1 : 0), "%s, copy %d: [%s]", sh.name, j, g_log.c_str());
            check_failed_call(sh, nbuf, g_log.find_last_of("UD"));
            CHECK(std::strstr(g_err, j < nup ? "H2D" : "D2H"), "%s, copy %d: message '%s'", sh.name, j, g_err);
        }
        // ---- the device form fails (its own code comes back), with the upward copies enqueued before it
        for (int code : {RQ_EHIP, RQ_ENOMEM, RQ_EINVAL}) {
            CHECK(run(sh, -1, -1, -1, code) == code && count('D') == 0, "%s, device form %d: [%s]", sh.name, code, g_log.c_str());
            check_failed_call(sh, nbuf, g_log.find('K'));
        }
        // ---- the final wait fails: RQ_EHIP, and the stream is waited for once more before anything is freed
        CHECK(run(sh, -1, -1, 0) == RQ_EHIP && count('S') == 2, "%s, failed wait: [%s]", sh.name, g_log.c_str());
        check_failed_call(sh, nbuf, g_log.find('S'));
    }
    {   // ---- a call that allocates and leaves before it enqueues anything waits for nothing
        g_log.clear();
        g_mallocs = 0; g_fail_malloc = -1;
        { Stage st(g_stream); const size_t b[2] = {8, 16}; CHECK(st.alloc(b, 2, "nothing") == RQ_OK && st.at<char>(1) && !st.at<char>(2), "two buffers"); }
        CHECK(g_log == "MMFF" && g_live.empty(), "[%s]", g_log.c_str());
    }
    {   // ---- ... unless it says that kernels were enqueued on its buffers: then it waits, also after a finish(), but not for buffers it never got
        const size_t b[2] = {8, 16};
        start(-1, -1, -1);
        { Stage st(g_stream); CHECK(st.alloc(b, 2, "kernels") == RQ_OK, "two buffers"); st.launched(); }
        CHECK(g_log == "MMSFF" && g_live.empty(), "[%s]", g_log.c_str());
        start(-1, -1, -1);
        { Stage st(g_stream); CHECK(st.alloc(b, 2, "kernels") == RQ_OK && st.zero(st.at<char>(1), 16) == RQ_OK && st.finish() == RQ_OK, "two buffers"); st.launched(); }
        CHECK(g_log == "MMZSSFF" && g_live.empty(), "[%s]", g_log.c_str());
        start(1, -1, -1);
        { Stage st(g_stream); CHECK(st.alloc(b, 2, "kernels") == RQ_ENOMEM && st.code() == RQ_ENOMEM, "the second buffer fails"); st.launched(); }
        CHECK(g_log == "MMEF" && g_live.empty(), "[%s]", g_log.c_str());
    }
    // ---- the repairs: the helper on the column sets of the three, then each repair's whole sequence of calls
    struct Flagged { int B; std::vector<int> q; };
    const Flagged sets[] = {{1, {0}}, {5, {}}, {5, {0, 3, 4}}, {5, {0, 1, 2, 3, 4}}, {70, {0, 63, 64, 69}}};
    for (int kind : {LADDER, RANGE, GROUPED})
        for (const Flagged& fl : sets)
            for (bool keys : {true, false}) {
                check_columns(kind, fl.B, fl.q, keys);
                check_repair(kind, fl.B, fl.q, keys, false);
                if (kind == LADDER) check_repair(kind, fl.B, fl.q, keys, true);
            }
    // (the same strings once more in full, for B = 5 with queries 0, 3 and 4 flagged and the keys given)
    CHECK(repair_log(LADDER, 3, true, false) == "DSXXXKDSXXXZXXXZXXXZS" && repair_log(LADDER, 3, true, true) == "DSXXXKDSXXXZXXXZSXKDSXXXZS" &&
          repair_log(RANGE, 3, true, false) == "DSMMMMMMMXXXXXXKXXXXXXXXXXXXXXXSFFFFFFF" &&
          repair_log(GROUPED, 3, true, false) == "DSMMMMMMMMMXXXKDDDDSXXXXXXXXXXXXZZZSFFFFFFFFF", "the expected logs");
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
