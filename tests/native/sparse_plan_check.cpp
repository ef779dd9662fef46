// Host-side check of csrc/rq_sparse_plan.h: the validation of the posting arrays and of a call's arguments, the tiles, the launch
// grids, the workspace bytes and the cut of a call into rounds -- plain arithmetic, so it runs without a GPU and can be built under
// the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/sparse_plan_check.cpp -o sparse_plan_check
#include "rq_sparse_plan.h"

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
    {   // ---- tiles at n_docs = 1, tile_docs - 1, tile_docs, tile_docs + 1 (and none for an empty corpus) ------------------------
        for (int t : {64, 256, 8192}) {
            CHECK(sparse_tiles(0, t) == 0 && sparse_tiles(1, t) == 1 && sparse_tiles(t - 1, t) == 1 && sparse_tiles(t, t) == 1 && sparse_tiles(t + 1, t) == 2, "tile_docs %d", t);
            CHECK(sparse_tiles(((int64_t)1 << 31) - 1, t) == (((int64_t)1 << 31) - 1 + t - 1) / t, "the largest corpus, tile_docs %d", t);
        }
        CHECK(sparse_tiles(1000000, 8192) == 123 && sparse_tiles(50000, 8192) == 7, "the two recorded shapes");
        CHECK(RQ_SPARSE_TILE_DEFAULT == 4096 && sparse_tile_ok(RQ_SPARSE_TILE_DEFAULT) && RQ_SPARSE_TILE_MAX * sizeof(double) == 65536, "64 KiB of accumulators at the most");
        for (double v : {64.0, 128.0, 2048.0, 4096.0, 8192.0}) CHECK(sparse_tile_ok(v), "tile_docs %g", v);
        for (double v : {0.0, -64.0, 32.0, 63.0, 65.0, 96.0, 100.0, 8191.0, 16384.0, 64.5, 1e300}) CHECK(!sparse_tile_ok(v), "tile_docs %g", v);
    }
    {   // ---- slots, workspace bytes, grids ----------------------------------------------------------------------------------------
        const SparsePlan p = sparse_plan(1000000, 8192, 500, 100, 0);
        CHECK(p.tiles == 123 && p.slot == 100 && p.query_bytes == 123 * 100 * 12 && p.per_round == 500 && p.rounds == 1, "1M passages, 500 x top-100");
        CHECK(p.cand_elems == (size_t)500 * 123 * 100 && p.count_elems == (size_t)500 * 123, "elements");
        CHECK(p.rows_offset() == p.cand_elems * 8 && p.counts_offset() == p.cand_elems * 12 && p.bytes() == p.cand_elems * 12 + p.count_elems * 4, "layout: bits, rows, counts");
        CHECK(p.rows_offset() % 8 == 0 && p.counts_offset() % 4 == 0, "alignment");
        const SparsePlan s = sparse_plan(200, 64, 3, 1024, 0);
        CHECK(s.tiles == 4 && s.slot == 64 && s.query_bytes == 4 * 64 * 12, "a tile keeps at most tile_docs candidates");
        const SparsePlan e = sparse_plan(0, 8192, 5, 10, 0);
        CHECK(e.tiles == 0 && e.per_round == 5 && e.rounds == 1 && e.bytes() == 0, "an empty corpus");
        const SparseGrid g = sparse_grid(p, 8192, 500);
        CHECK(g.tile_x == 123u && g.tile_y == 500u && g.final_x == 500u && g.block == 256u && g.tile_lds == 65536, "grids");
        CHECK(sparse_grid(s, 64, 3).tile_lds == 512, "LDS of the smallest tile");
        // the limits in 64 bits: 2^31 - 1 documents in tiles of 64, k = 1024, one query
        const SparsePlan big = sparse_plan(((int64_t)1 << 31) - 1, 64, 65535, 1024, 0);
        CHECK(big.tiles == 33554432 && big.query_bytes == (int64_t)33554432 * 64 * 12 && big.per_round == 1 && big.rounds == 65535, "beyond the cap: one query per round");
        CHECK(big.bytes() == (size_t)33554432 * 64 * 12 + (size_t)33554432 * 4, "bytes %zu", big.bytes());
    }
    {   // ---- rounds at and beside the cap; every query in exactly one round -----------------------------------------------------
        const int64_t qb = sparse_plan(2000, 256, 1, 20, 0).query_bytes;
        CHECK(qb == 8 * 20 * 12, "bytes per query %lld", (long long)qb);
        struct { int B; int64_t cap; int per_round, rounds; } want[] = {
            {70, 30 * qb, 30, 3}, {70, 30 * qb - 1, 29, 3}, {70, 30 * qb + qb - 1, 30, 3}, {70, 35 * qb, 35, 2}, {70, 35 * qb - 1, 34, 3}, {70, 70 * qb, 70, 1},
            {70, 70 * qb - 1, 69, 2}, {70, qb, 1, 70}, {70, qb - 1, 1, 70}, {70, 1, 1, 70}, {1, 1, 1, 1}, {65535, 0, 65535, 1}};
        for (const auto& w : want) {
            const SparsePlan p = sparse_plan(2000, 256, w.B, 20, w.cap);
            CHECK(p.per_round == w.per_round && p.rounds == w.rounds, "B %d cap %lld: %d per round, %d rounds", w.B, (long long)w.cap, p.per_round, p.rounds);
            std::vector<int> seen((size_t)w.B, 0);
            for (int r = 0; r < p.rounds; ++r) {
                CHECK(p.round_count(r, w.B) >= 1 && p.round_count(r, w.B) <= p.per_round, "round %d holds %d", r, p.round_count(r, w.B));
                for (int q = p.round_first(r); q < p.round_first(r) + p.round_count(r, w.B); ++q)
                    if (q >= 0 && q < w.B) seen[(size_t)q]++;
                    else CHECK(false, "query %d outside the call", q);
            }
            for (int q = 0; q < w.B; ++q) CHECK(seen[(size_t)q] == 1, "B %d cap %lld: query %d in %d rounds", w.B, (long long)w.cap, q, seen[(size_t)q]);
            CHECK(p.cand_elems == (size_t)p.per_round * 8 * 20 && (w.cap <= 0 || p.per_round == 1 || (int64_t)p.cand_elems * 12 <= w.cap), "a round stays within the cap");
        }
        CHECK(RQ_SPARSE_CAND_CAP == ((int64_t)1 << 30), "the default cap");
        CHECK(sparse_plan(1000000, 8192, 65535, 1024, 0).per_round == (int)(((int64_t)1 << 30) / (123 * 1024 * 12)), "the default cap cuts the largest call");
    }
    {   // ---- the posting arrays ---------------------------------------------------------------------------------------------------
        const int64_t indptr[] = {0, 2, 2, 5};
        const int32_t rows[] = {1, 4, 0, 2, 4};
        const double contrib[] = {1.0, 2.0, 0.5, 0.25, 4.0};
        CHECK(sparse_check_csr(indptr, rows, contrib, 3, 5) == RQ_OK, "a good index: %s", g_err);
        CHECK(sparse_check_csr(indptr, rows, contrib, 0, 5) == RQ_OK && sparse_check_csr(indptr, nullptr, nullptr, 0, 0) == RQ_OK, "no tokens");
        const int32_t desc[] = {4, 1, 0, 2, 4};
        CHECK(sparse_check_csr(indptr, desc, contrib, 3, 5) == RQ_EINVAL && std::strstr(g_err, "ascending"), "a descending pair");
        const int32_t rep[] = {1, 4, 0, 2, 2};
        CHECK(sparse_check_csr(indptr, rep, contrib, 3, 5) == RQ_EINVAL && std::strstr(g_err, "ascending"), "a repeated row");
        const int32_t across[] = {1, 4, 4, 2, 4};   // equal rows in DIFFERENT tokens are fine, but 4 > 2 inside token 2 is not
        CHECK(sparse_check_csr(indptr, across, contrib, 3, 5) == RQ_EINVAL, "descending inside the last token");
        const int32_t restart[] = {1, 4, 0, 1, 4};  // token 2 starts below token 0's last row: allowed
        CHECK(sparse_check_csr(indptr, restart, contrib, 3, 5) == RQ_OK, "every token's rows start afresh");
        CHECK(sparse_check_csr(indptr, rows, contrib, 3, 4) == RQ_EINVAL && std::strstr(g_err, "outside"), "a row = n_docs");
        const int32_t neg[] = {-1, 4, 0, 2, 4};
        CHECK(sparse_check_csr(indptr, neg, contrib, 3, 5) == RQ_EINVAL, "a negative row");
        const int64_t off[] = {1, 2, 2, 5};
        CHECK(sparse_check_csr(off, rows, contrib, 3, 5) == RQ_EINVAL && std::strstr(g_err, "indptr[0]"), "indptr[0] != 0");
        const int64_t dec[] = {0, 3, 2, 5};
        CHECK(sparse_check_csr(dec, rows, contrib, 3, 5) == RQ_EINVAL && std::strstr(g_err, "decreases"), "a decreasing indptr");
        CHECK(sparse_check_csr(nullptr, rows, contrib, 3, 5) == RQ_EINVAL && sparse_check_csr(indptr, nullptr, contrib, 3, 5) == RQ_EINVAL &&
              sparse_check_csr(indptr, rows, nullptr, 3, 5) == RQ_EINVAL, "null arrays");
        CHECK(sparse_check_csr(indptr, rows, contrib, 3, (int64_t)1 << 31) == RQ_EINVAL && std::strstr(g_err, "2^31"), "n_docs = 2^31");
        CHECK(sparse_check_csr(indptr, rows, contrib, 3, ((int64_t)1 << 31) - 1) == RQ_OK, "n_docs = 2^31 - 1");
        CHECK(sparse_check_csr(indptr, rows, contrib, -1, 5) == RQ_EINVAL && sparse_check_csr(indptr, rows, contrib, 3, -1) == RQ_EINVAL, "negative sizes");
    }
    {   // ---- a call's arguments ----------------------------------------------------------------------------------------------------
        int dummy = 0;
        const void* p = &dummy;
        CHECK(RQ_SPARSE_MAX_K == 1024, "the documented limit");
        CHECK(sparse_check_call(p, p, 1, 1, p, p) == RQ_OK && sparse_check_call(p, p, 65535, 1024, p, p) == RQ_OK, "the limits");
        for (int B : {0, -1, 65536}) CHECK(sparse_check_call(p, p, B, 10, p, p) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        for (int k : {0, -1, 1025}) CHECK(sparse_check_call(p, p, 1, k, p, p) == RQ_EINVAL && std::strstr(g_err, "k "), "k = %d", k);
        CHECK(sparse_check_call(nullptr, p, 1, 1, p, p) == RQ_EINVAL && sparse_check_call(p, nullptr, 1, 1, p, p) == RQ_EINVAL &&
              sparse_check_call(p, p, 1, 1, nullptr, p) == RQ_EINVAL && sparse_check_call(p, p, 1, 1, p, nullptr) == RQ_EINVAL, "null pointers");
        const int64_t qi[] = {0, 2, 2, 3};
        const int32_t qt[] = {0, 2, 1};
        CHECK(sparse_check_queries(qi, qt, 3, 3) == RQ_OK, "good queries: %s", g_err);
        CHECK(sparse_check_queries(qi, qt, 3, 2) == RQ_EINVAL && std::strstr(g_err, "token id"), "a token id = n_tokens");
        const int32_t qneg[] = {0, -1, 1};
        CHECK(sparse_check_queries(qi, qneg, 3, 3) == RQ_EINVAL, "a negative token id");
        const int64_t qdec[] = {0, 2, 1, 3};
        CHECK(sparse_check_queries(qdec, qt, 3, 3) == RQ_EINVAL && std::strstr(g_err, "decreases"), "a decreasing q_indptr");
        const int64_t qn[] = {-1, 2, 2, 3};
        CHECK(sparse_check_queries(qn, qt, 3, 3) == RQ_EINVAL, "a negative start");
        const int64_t qe[] = {0, 0, 0, 0};
        CHECK(sparse_check_queries(qe, nullptr, 3, 3) == RQ_OK && sparse_check_queries(qi, nullptr, 3, 3) == RQ_EINVAL, "no tokens needs no array");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
