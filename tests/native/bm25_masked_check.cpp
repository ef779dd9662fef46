// librq_bm25's masked scorer (csrc/rq_bm25.cpp rq_bm25_topk_masked, compiled INTO this program so that -fsanitize=address,undefined
// sees it) against a straightforward per-document reference: scores added as ever, every document outside the query's mask at 0.0
// before the score > 0 selection, ties by descending row, padding.  The corpus ends in the middle of a mask word and the bits of that
// word at or beyond n_docs are SET (they must be ignored, and no word beyond the table is read: the table is allocated exactly);
// masks are shared by queries in a scrambled arrangement with unrestricted queries between them; 1, 3 and 16 threads; refusals.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined tests/native/bm25_masked_check.cpp <csrc>/rq_bm25.cpp -I include -o bm25_masked_check
#include "rq_bm25.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

int main() {
    std::mt19937 g(5);
    const int64_t T = 200, N = 1999;             // 1999 = 62 x 32 + 15: a ragged last word
    const size_t W = (size_t)((N + 31) / 32);
    std::vector<int64_t> ip(T + 1, 0);
    std::vector<int32_t> rows;
    std::vector<double> c;
    for (int64_t t = 0; t < T; ++t) {
        const double p = 0.4 / (1 + t * 0.05);
        for (int64_t d = 0; d < N; ++d)
            if ((g() & 0xffff) < p * 65536) { rows.push_back((int32_t)d); c.push_back(t % 17 == 0 ? -0.25 : 0.5 + (g() & 7) / 8.0); }   // few distinct values: ties
        if (t == 3) { if (rows.empty() || rows.back() != (int32_t)(N - 1)) { rows.push_back((int32_t)(N - 1)); c.push_back(2.0); } }       // the last row has a posting
        ip[t + 1] = (int64_t)rows.size();
    }
    rq_bm25* h = rq_bm25_create(ip.data(), rows.data(), c.data(), T, N);
    CHECK(h != nullptr, "create");
    // masks: 0 = everything, 1 = nothing, 2 = a random half, 3 = the last row alone, 4 = every third row; tail bits set in all of them
    const int M = 5;
    std::vector<uint32_t> masks((size_t)M * W, 0u);
    auto allow = [&](int m, int64_t d) { masks[(size_t)m * W + (size_t)(d >> 5)] |= 1u << (d & 31); };
    for (int64_t d = 0; d < N; ++d) {
        allow(0, d);
        if (g() & 1) allow(2, d);
        if (d % 3 == 0) allow(4, d);
    }
    allow(3, N - 1);
    for (int m = 0; m < M; ++m)
        for (int64_t d = N; d < (int64_t)W * 32; ++d) allow(m, d);
    auto allowed = [&](int m, int64_t d) { return m < 0 || ((masks[(size_t)m * W + (size_t)(d >> 5)] >> (d & 31)) & 1u) != 0; };
    const int B = 80;
    std::vector<int64_t> qp(B + 1, 0);
    std::vector<int32_t> qt, mo(B);
    for (int q = 0; q < B; ++q) {
        const int len = q == 5 ? 0 : 1 + (int)(g() % 9);
        for (int i = 0; i < len; ++i) qt.push_back((int32_t)(g() % (q % 2 ? 30 : T)));
        if (q == 7) { qt.push_back(qt.back()); qt.push_back(qt.back()); }          // a repeated token
        if (q % 10 == 3) qt.push_back(3);                                          // the token that reaches the last row
        qp[q + 1] = (int64_t)qt.size();
        mo[q] = (int32_t)((q * 7) % (M + 1)) - 1;                                  // -1 .. 4, scrambled, every mask many times
    }
    for (int k : {1, 10, 3000}) {
        for (int nt : {1, 3, 16}) {
            std::vector<int32_t> orow((size_t)B * k);
            std::vector<double> osc((size_t)B * k);
            CHECK(rq_bm25_topk_masked(h, qp.data(), qt.data(), B, k, masks.data(), M, mo.data(), orow.data(), osc.data(), nt) == RQ_BM25_OK, "topk_masked");
            for (int q = 0; q < B; ++q) {
                std::vector<double> acc((size_t)N, 0.0);
                for (int64_t t = qp[q]; t < qp[q + 1]; ++t)
                    for (int64_t p = ip[qt[t]]; p < ip[qt[t] + 1]; ++p) acc[(size_t)rows[p]] += c[p];
                for (int64_t d = 0; d < N; ++d)
                    if (!allowed(mo[q], d)) acc[(size_t)d] = 0.0;
                std::vector<int32_t> order;
                for (int32_t d = 0; d < N; ++d) if (acc[(size_t)d] > 0.0) order.push_back(d);
                std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return acc[(size_t)a] > acc[(size_t)b] || (acc[(size_t)a] == acc[(size_t)b] && a > b); });
                if (mo[q] == 1) CHECK(order.empty(), "q %d: the empty mask", q);
                for (int i = 0; i < k; ++i) {
                    const bool v = (size_t)i < order.size();
                    CHECK(orow[(size_t)q * k + i] == (v ? order[(size_t)i] : -1), "k %d nt %d q %d rank %d: row %d", k, nt, q, i, orow[(size_t)q * k + i]);
                    CHECK(osc[(size_t)q * k + i] == (v ? acc[(size_t)order[(size_t)i]] : 0.0), "k %d nt %d q %d rank %d: score", k, nt, q, i);
                }
            }
            // the unmasked call after a masked one: the accumulators were put back, whatever the masks hid
            std::vector<int32_t> urow((size_t)B * k), mrow((size_t)B * k);
            std::vector<double> usc((size_t)B * k), msc((size_t)B * k);
            std::vector<int32_t> none(B, -1);
            CHECK(rq_bm25_topk(h, qp.data(), qt.data(), B, k, urow.data(), usc.data(), nt) == RQ_BM25_OK, "topk");
            CHECK(rq_bm25_topk_masked(h, qp.data(), qt.data(), B, k, nullptr, 0, none.data(), mrow.data(), msc.data(), nt) == RQ_BM25_OK, "all unrestricted, no table");
            CHECK(urow == mrow && usc == msc, "k %d nt %d: every entry -1 is the unmasked call", k, nt);
        }
    }
    // one thread scores a masked query and then an unrestricted one over the same postings: nothing is left in its accumulator
    {
        const int64_t qp2[3] = {0, 1, 2};
        const int32_t qt2[2] = {3, 3}, mo2[2] = {1, -1};
        int32_t r2[2 * 4], r1[4];
        double s2[2 * 4], s1[4];
        CHECK(rq_bm25_topk_masked(h, qp2, qt2, 2, 4, masks.data(), M, mo2, r2, s2, 1) == RQ_BM25_OK, "masked then unrestricted");
        CHECK(rq_bm25_topk(h, qp2, qt2, 1, 4, r1, s1, 1) == RQ_BM25_OK, "plain");
        for (int i = 0; i < 4; ++i) {
            CHECK(r2[i] == -1 && s2[i] == 0.0, "empty mask rank %d", i);
            CHECK(r2[4 + i] == r1[i] && s2[4 + i] == s1[i], "after a masked query rank %d", i);
        }
    }
    std::vector<int32_t> one(4);
    std::vector<double> onesc(4);
    const int64_t qp1[2] = {0, 1};
    const int32_t qt1[1] = {0};
    for (int32_t bad : {-2, M, 1 << 30}) {
        const int32_t mo1[1] = {bad};
        CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, masks.data(), M, mo1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "mask_of %d", bad);
    }
    const int32_t ok1[1] = {0}, free1[1] = {-1};
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, masks.data(), M, nullptr, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "null mask_of");
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, nullptr, M, ok1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "null masks with n_masks > 0");
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, nullptr, 0, ok1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "mask 0 of an empty table");
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, masks.data(), -1, free1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "negative n_masks");
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 0, masks.data(), M, ok1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "k 0");
    CHECK(rq_bm25_topk_masked(nullptr, qp1, qt1, 1, 4, masks.data(), M, ok1, one.data(), onesc.data(), 1) == RQ_BM25_EINVAL, "null handle");
    CHECK(rq_bm25_topk_masked(h, qp1, qt1, 1, 4, nullptr, 0, free1, one.data(), onesc.data(), 1) == RQ_BM25_OK, "no table, every entry -1");
    rq_bm25_destroy(h);
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
