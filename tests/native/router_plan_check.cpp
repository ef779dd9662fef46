// Host-side check of csrc/rq_router_plan.h: what rq_router_create refuses and the widened weight table it builds, the checks of a
// call's arguments, the instantiation of the kernel by column length with its threads, the length of the summation tree and the LDS
// bytes -- plain arithmetic, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/router_plan_check.cpp -o router_plan_check
#include "rq_router_plan.h"

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
    {   // ---- create: refusals and the table ----------------------------------------------------------------------------------------
        std::vector<double> t;
        const float w0[] = {0.1f, -0.2f, 0.3f, 1.5f, 2.5f, -3.5f};
        const float b0[] = {0.25f, -0.75f};
        const float w1[] = {0.7f, -0.9f, 0.11f};
        CHECK(router_check_create(2, 2, 0, w0, b0, w1, t) == RQ_OK, "two layers: %s", g_err);
        const double want[] = {(double)0.1f, (double)-0.2f, (double)0.3f, 0.25, (double)0.7f, 1.5, 2.5, -3.5, -0.75, (double)-0.9f};
        CHECK(t.size() == 2 * RQ_ROUTER_ROW && std::equal(t.begin(), t.end(), want), "rows of W0[j][0..2], b0[j], w1[j], widened exactly");
        CHECK(router_check_create(1, 0, 0, nullptr, nullptr, w1, t) == RQ_OK && t.size() == 3 && t[2] == (double)0.11f, "one layer: w1[0..2], no hidden width needed");
        CHECK(router_check_create(1, 999, 0, nullptr, nullptr, w1, t) == RQ_OK, "one layer ignores hidden");
        std::vector<float> big0(3 * 256, 0.5f), bigb(256, 0.25f), big1(256, -1.0f);
        CHECK(router_check_create(2, 256, 0, big0.data(), bigb.data(), big1.data(), t) == RQ_OK && t.size() == 256 * RQ_ROUTER_ROW && t.back() == -1.0, "the widest router");
        CHECK(router_check_create(2, 1, 0, w0, b0, w1, t) == RQ_OK && t.size() == RQ_ROUTER_ROW, "hidden = 1");
        CHECK(router_check_create(2, 2, 1, w0, b0, w1, t) == RQ_EINVAL && std::strstr(g_err, "use_batch_norm"), "batch norm: %s", g_err);
        for (int layers : {0, -1, 3, 4}) CHECK(router_check_create(layers, 2, 0, w0, b0, w1, t) == RQ_EINVAL && std::strstr(g_err, "num_layers"), "num_layers = %d", layers);
        for (int hidden : {0, -1, 257}) CHECK(router_check_create(2, hidden, 0, big0.data(), bigb.data(), big1.data(), t) == RQ_EINVAL && std::strstr(g_err, "hidden"), "hidden = %d", hidden);
        CHECK(router_check_create(2, 2, 0, nullptr, b0, w1, t) == RQ_EINVAL && router_check_create(2, 2, 0, w0, nullptr, w1, t) == RQ_EINVAL &&
              router_check_create(2, 2, 0, w0, b0, nullptr, t) == RQ_EINVAL && router_check_create(1, 0, 0, nullptr, nullptr, nullptr, t) == RQ_EINVAL, "null weights");
    }
    {   // ---- the instantiation by column length, the tree ---------------------------------------------------------------------------
        struct { int P, pad, threads, tree; } want[] = {{1, 64, 64, 1}, {2, 64, 64, 2}, {3, 64, 64, 4}, {63, 64, 64, 64}, {64, 64, 64, 64}, {65, 128, 64, 128},
                                                        {100, 128, 64, 128}, {128, 128, 64, 128}, {129, 256, 128, 256}, {256, 256, 128, 256}, {257, 512, 256, 512},
                                                        {512, 512, 256, 512}, {513, 1024, 256, 1024}, {1000, 1024, 256, 1024}, {1024, 1024, 256, 1024}};
        for (const auto& w : want) {
            const int pad = router_pad(w.P);
            CHECK(pad == w.pad && router_threads(pad) == w.threads && router_tree(w.P) == w.tree, "P = %d: pad %d, %d threads, tree %d", w.P, pad, router_threads(pad), router_tree(w.P));
            CHECK(pad >= w.P && (pad & (pad - 1)) == 0 && router_threads(pad) % 64 == 0 && router_threads(pad) <= pad, "whole waves, a comparator or a slot per thread");
            CHECK(router_tree(w.P) >= w.P && router_tree(w.P) <= pad && router_tree(w.P) < 2 * w.P, "the tree is the NEXT power of two and fits the instantiation");
        }
        CHECK(router_pad(RQ_MAX_K) == 1024, "the largest call is the largest instantiation");
        CHECK(router_lds_bytes(1024, true) == 1024 * 36 + 10240 && router_lds_bytes(1024, true) < 65536, "rank, 1 024 slots: %zu bytes of LDS", router_lds_bytes(1024, true));
        CHECK(router_lds_bytes(1024, false) == 1024 * 32 + 10240 && router_lds_bytes(64, true) == 64 * 36 + 10240, "the gate form has no positions; small columns do not pay for 1 024");
    }
    {   // ---- a call's arguments ----------------------------------------------------------------------------------------------------
        int dummy = 0;
        const void* p = &dummy;
        CHECK(router_check_gate(p, p, p, 1, 1, RQ_ROUTER_NORM_QUERY, nullptr, p) == RQ_OK && router_check_gate(p, p, p, 65535, 1024, RQ_ROUTER_NORM_STATS, p, p) == RQ_OK, "the limits: %s", g_err);
        CHECK(router_check_gate(p, p, p, 1, 1, RQ_ROUTER_NORM_QUERY, p, p) == RQ_OK, "statistics are ignored per query");
        CHECK(router_check_gate(p, p, p, 1, 1, RQ_ROUTER_NORM_STATS, nullptr, p) == RQ_EINVAL && std::strstr(g_err, "statistics"), "STATS without statistics");
        for (int mode : {-1, 2, 7}) CHECK(router_check_gate(p, p, p, 1, 1, mode, p, p) == RQ_EINVAL && std::strstr(g_err, "mode"), "mode = %d", mode);
        for (int B : {0, -1, 65536}) CHECK(router_check_gate(p, p, p, B, 1, RQ_ROUTER_NORM_QUERY, nullptr, p) == RQ_EINVAL && std::strstr(g_err, "B "), "B = %d", B);
        for (int P : {0, -1, 1025}) CHECK(router_check_gate(p, p, p, 1, P, RQ_ROUTER_NORM_QUERY, nullptr, p) == RQ_EINVAL && std::strstr(g_err, "P "), "P = %d", P);
        CHECK(router_check_gate(nullptr, p, p, 1, 1, 1, nullptr, p) == RQ_EINVAL && router_check_gate(p, nullptr, p, 1, 1, 1, nullptr, p) == RQ_EINVAL &&
              router_check_gate(p, p, nullptr, 1, 1, 1, nullptr, p) == RQ_EINVAL && router_check_gate(p, p, p, 1, 1, 1, nullptr, nullptr) == RQ_EINVAL, "gate: null pointers");
        CHECK(router_check_rerank(p, p, p, p, p, 3, 20, RQ_ROUTER_NORM_QUERY, nullptr, 10, p, p, p, p, p, p, p) == RQ_OK, "rerank: %s", g_err);
        CHECK(router_check_rerank(p, p, p, p, p, 3, 20, RQ_ROUTER_NORM_QUERY, nullptr, 1, p, p, p, p, p, p, p) == RQ_OK &&
              router_check_rerank(p, p, p, p, p, 3, 20, RQ_ROUTER_NORM_QUERY, nullptr, 20, p, p, p, p, p, p, p) == RQ_OK, "top_r at both ends");
        for (int r : {0, -1, 21}) CHECK(router_check_rerank(p, p, p, p, p, 3, 20, RQ_ROUTER_NORM_QUERY, nullptr, r, p, p, p, p, p, p, p) == RQ_EINVAL && std::strstr(g_err, "top_r"), "top_r = %d", r);
        CHECK(router_check_rerank(p, nullptr, p, p, p, 3, 20, 1, nullptr, 10, p, p, p, p, p, p, p) == RQ_EINVAL && router_check_rerank(p, p, p, p, nullptr, 3, 20, 1, nullptr, 10, p, p, p, p, p, p, p) == RQ_EINVAL,
              "rerank: null keys or count");
        for (int miss = 0; miss < 7; ++miss) {
            const void* o[7] = {p, p, p, p, p, p, p};
            o[miss] = nullptr;
            CHECK(router_check_rerank(p, p, p, p, p, 3, 20, 1, nullptr, 10, o[0], o[1], o[2], o[3], o[4], o[5], o[6]) == RQ_EINVAL && std::strstr(g_err, "null output"), "output %d null", miss);
        }
        CHECK(router_check_rerank(p, p, p, p, p, 0, 20, 1, nullptr, 10, p, p, p, p, p, p, p) == RQ_EINVAL && router_check_rerank(p, p, p, p, p, 3, 1025, 1, nullptr, 10, p, p, p, p, p, p, p) == RQ_EINVAL &&
              router_check_rerank(p, p, p, p, p, 3, 20, 5, nullptr, 10, p, p, p, p, p, p, p) == RQ_EINVAL, "rerank inherits the column checks");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
