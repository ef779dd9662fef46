// Host-side check of the grouped part of csrc/rq_sparse_plan.h (rq_sparse_set_groups, rq_sparse_topk_grouped*): the tile clamp, the
// LDS bytes of both grouped kernels, the grids, the checks of the group table and of a call's arguments, and the slot hash -- plain
// arithmetic, so it runs without a GPU and can be built under the host sanitizers.
//   hipcc -O1 -g -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -I <csrc> tests/native/sparse_grouped_plan_check.cpp -o sparse_grouped_plan_check
#include "rq_sparse_plan.h"

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

int main() {
    {   // ---- the tile clamp and the LDS budget ----------------------------------------------------------------------------------
        CHECK(RQ_SPARSE_GROUPED_TILE_MAX == 4096 && sparse_tile_ok(RQ_SPARSE_GROUPED_TILE_MAX), "the clamp is a legal tile");
        for (int t : {64, 128, 1024, 4096}) CHECK(sparse_grouped_tile(t) == t, "tile_docs %d stays", t);
        CHECK(sparse_grouped_tile(8192) == 4096, "8 192 is clamped");
        for (int t : {64, 256, 4096}) {
            CHECK(sparse_grouped_slots(t) == 2 * t && (sparse_grouped_slots(t) & (sparse_grouped_slots(t) - 1)) == 0, "2 x tile slots, a power of two (%d)", t);
            CHECK(sparse_grouped_tile_lds(t) == (size_t)t * 8 + (size_t)t * 16, "accumulators + 8 B per slot (%d)", t);
        }
        CHECK(sparse_grouped_tile_lds(4096) == 96 * 1024, "96 KiB at the most: %zu", sparse_grouped_tile_lds(4096));
        // with the tile kernel's static LDS (two int64 per token of a chunk, the selection histogram) a workgroup stays under 160 KiB
        CHECK(sparse_grouped_tile_lds(4096) + 2 * RQ_SPARSE_CHUNK * 8 + 2048 <= 160 * 1024, "one workgroup fits a CU's LDS");
        CHECK(RQ_SPARSE_GROUPED_CHUNK == RQ_SPARSE_MAX_K && RQ_SPARSE_GROUPED_CHUNK % RQ_SPARSE_THREADS == 0, "a chunk: at most RQ_SPARSE_MAX_K candidates");
        CHECK(RQ_SPARSE_GROUPED_SET == 4096 && 2 * (RQ_SPARSE_MAX_K - 1 + RQ_SPARSE_GROUPED_CHUNK) <= RQ_SPARSE_GROUPED_SET, "the group set is at most half full");
        CHECK(sparse_grouped_final_lds() == 1024 * 16 + 4096 * 8 && sparse_grouped_final_lds() + 2048 <= 64 * 1024, "static LDS of the final kernel: %zu", sparse_grouped_final_lds());
    }
    {   // ---- plans and grids: those of the ungrouped call over the clamped tile ---------------------------------------------------
        const int tile = sparse_grouped_tile(8192);
        const SparsePlan p = sparse_plan(1000000, tile, 500, 100, 0);
        CHECK(p.tiles == 245 && p.slot == 100 && p.rounds == 1 && p.per_round == 500, "1M passages, 500 x top-100 in tiles of 4 096");
        const SparseGrid g = sparse_grouped_grid(p, tile, 500);
        CHECK(g.tile_x == 245u && g.tile_y == 500u && g.final_x == 500u && g.block == 256u && g.tile_lds == 96 * 1024, "grids");
        const SparsePlan s = sparse_plan(300, sparse_grouped_tile(64), 2, 1024, 0);
        CHECK(s.tiles == 5 && s.slot == 64 && sparse_grouped_grid(s, 64, 2).tile_lds == 64 * 24, "the smallest tile");
        CHECK(sparse_grid(p, tile, 500).tile_lds == (size_t)tile * 8, "the ungrouped grid is untouched");
    }
    {   // ---- the group table ------------------------------------------------------------------------------------------------------
        int dummy = 0;
        const void* h = &dummy;
        const int32_t good[] = {-1, 0, 7, 2147483647, 8192, -1};
        CHECK(sparse_check_groups(h, good, 6, 6) == RQ_OK, "a good table: %s", g_err);
        CHECK(sparse_check_groups(h, nullptr, 0, 0) == RQ_OK, "an empty corpus needs no array");
        const int32_t bad[] = {0, -2, 3};
        CHECK(sparse_check_groups(h, bad, 3, 3) == RQ_EINVAL && std::strstr(g_err, "groups[1]"), "a negative id other than -1");
        const int32_t worst[] = {(-2147483647 - 1)};
        CHECK(sparse_check_groups(h, worst, 1, 1) == RQ_EINVAL, "INT32_MIN");
        CHECK(sparse_check_groups(h, good, 5, 6) == RQ_EINVAL && std::strstr(g_err, "n_docs"), "n_docs below the handle's");
        CHECK(sparse_check_groups(h, good, 6, 5) == RQ_EINVAL, "n_docs above the handle's");
        CHECK(sparse_check_groups(h, nullptr, 6, 6) == RQ_EINVAL && sparse_check_groups(nullptr, good, 6, 6) == RQ_EINVAL, "null arguments");
    }
    {   // ---- a call's arguments ----------------------------------------------------------------------------------------------------
        int dummy = 0;
        const void* p = &dummy;
        CHECK(sparse_check_grouped(true, nullptr, 0, nullptr, p) == RQ_OK, "unrestricted: no masks, no mask_of");
        CHECK(sparse_check_grouped(true, nullptr, 0, p, p) == RQ_OK && sparse_check_grouped(true, p, 3, p, p) == RQ_OK, "masked");
        CHECK(sparse_check_grouped(false, p, 3, p, p) == RQ_EINVAL && std::strstr(g_err, "no group table"), "no table");
        CHECK(sparse_check_grouped(true, p, 3, p, nullptr) == RQ_EINVAL && std::strstr(g_err, "out_count"), "null out_count");
        CHECK(sparse_check_grouped(true, nullptr, 2, p, p) == RQ_EINVAL && sparse_check_grouped(true, p, -1, p, p) == RQ_EINVAL, "masks without an array, negative n_masks");
        CHECK(sparse_check_grouped(true, p, 2, nullptr, p) == RQ_EINVAL && std::strstr(g_err, "without mask_of"), "masks without mask_of");
    }
    {   // ---- the slot hash: inside the table, and adverse ids spread ----------------------------------------------------------------
        for (unsigned lg : {7u, 12u, 13u}) {
            const unsigned slots = 1u << lg;
            std::set<unsigned> mult, high;
            for (uint32_t m = 0; m < 512; ++m) {
                const unsigned a = sparse_group_hash(m * 8192u, lg), b = sparse_group_hash(2147483647u - m, lg);
                CHECK(a < slots && b < slots, "slot inside the table (%u)", lg);
                mult.insert(a);
                high.insert(b);
            }
            const size_t least = std::min<size_t>(512, slots) / 2;
            CHECK(mult.size() >= least && high.size() >= least, "%u slots: %zu and %zu distinct slots of 512 ids", slots, mult.size(), high.size());
        }
        CHECK(sparse_group_hash(0u, 7) == 0 && sparse_group_hash(0xFFFFFFFEu, 13) < 8192, "the ends of the id range");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
