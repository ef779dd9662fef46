// rq_sparse_plan.h -- the host side of a sparse (BM25) top-k call (include/rq.h rq_sparse_create, rq_sparse_topk*, rq_sparse_topk_masked*)
// that needs no device: the validation of the posting arrays and of a call's arguments, the tiles of the corpus, the launch grids, the
// workspace bytes and the cut of a call into rounds of queries.  Plain arithmetic in the manner of rq_score_plan.h and
// rq_filter_each_plan.h: no HIP runtime call, nothing is written anywhere (tests/native/sparse_plan_check.cpp runs it on the host).
// Results never depend on the plan: every (tile_docs, cand_cap) gives the same rows and the same score bits.
#pragma once
#include "rq_index.h"

#define RQ_SPARSE_THREADS 256                     // 4 waves per workgroup, both kernels
#define RQ_SPARSE_CHUNK 256                       // query tokens whose posting sub-ranges are searched at once, one thread each
#define RQ_SPARSE_TILE_MIN 64
#define RQ_SPARSE_TILE_MAX 8192                   // 64 KiB of float64 accumulators in LDS: two workgroups per CU
#define RQ_SPARSE_TILE_DEFAULT 4096               // 32 KiB: four workgroups per CU; measured best at 1M passages
#define RQ_SPARSE_CAND_BYTES 12                   // one candidate: the score's 8 bytes + an int32 row
// candidate bytes of one round, 1 GiB as rq_filter_each_plan.h bounds its ragged rounds ("cand_cap": test hook)
#define RQ_SPARSE_CAND_CAP ((int64_t)1 << 30)

// What rq_sparse_create refuses: what rq_bm25_create refuses, and rows of a token that are not STRICTLY ascending (the kernel
// binary-searches them; a repeated row would also be a race inside one token), and n_docs >= 2^31 (rows are int32).
static inline int sparse_check_csr(const int64_t* indptr, const int32_t* rows, const double* contrib, int64_t n_tokens, int64_t n_docs) {
    if (!indptr) return set_err(RQ_EINVAL, "null indptr");
    if (n_tokens < 0 || n_docs < 0) return set_err(RQ_EINVAL, "negative n_tokens or n_docs");
    if (n_docs >= ((int64_t)1 << 31)) return set_err(RQ_EINVAL, "n_docs %lld is 2^31 or more", (long long)n_docs);
    if (indptr[0] != 0) return set_err(RQ_EINVAL, "indptr[0] is %lld, not 0", (long long)indptr[0]);
    for (int64_t t = 0; t < n_tokens; ++t)
        if (indptr[t] > indptr[t + 1]) return set_err(RQ_EINVAL, "indptr decreases at token %lld", (long long)t);
    const int64_t nnz = indptr[n_tokens];
    if (nnz > 0 && (!rows || !contrib)) return set_err(RQ_EINVAL, "null rows or contrib with %lld postings", (long long)nnz);
    for (int64_t t = 0; t < n_tokens; ++t)
        for (int64_t p = indptr[t]; p < indptr[t + 1]; ++p) {
            if (rows[p] < 0 || (int64_t)rows[p] >= n_docs) return set_err(RQ_EINVAL, "row %d of token %lld outside 0..%lld", rows[p], (long long)t, (long long)n_docs - 1);
            if (p > indptr[t] && rows[p] <= rows[p - 1]) return set_err(RQ_EINVAL, "rows of token %lld are not strictly ascending (%d after %d)", (long long)t, rows[p], rows[p - 1]);
        }
    return RQ_OK;
}

// Both entry points (pointers are only tested for null).
static inline int sparse_check_call(const void* h, const void* q_indptr, int B, int k, const void* out_rows, const void* out_scores) {
    if (!h || !q_indptr || !out_rows || !out_scores) return set_err(RQ_EINVAL, "null argument");
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (k < 1 || k > RQ_SPARSE_MAX_K) return set_err(RQ_EINVAL, "k %d outside 1..%d", k, RQ_SPARSE_MAX_K);
    return RQ_OK;
}

// The host form sees the queries: q_indptr starts at 0 or above and never decreases, every token id is in [0, n_tokens).
static inline int sparse_check_queries(const int64_t* q_indptr, const int32_t* q_tokens, int B, int64_t n_tokens) {
    if (q_indptr[0] < 0) return set_err(RQ_EINVAL, "q_indptr[0] is negative");
    for (int q = 0; q < B; ++q)
        if (q_indptr[q] > q_indptr[q + 1]) return set_err(RQ_EINVAL, "q_indptr decreases at query %d", q);
    if (q_indptr[B] > 0 && !q_tokens) return set_err(RQ_EINVAL, "null q_tokens");
    for (int64_t t = q_indptr[0]; t < q_indptr[B]; ++t)
        if (q_tokens[t] < 0 || (int64_t)q_tokens[t] >= n_tokens) return set_err(RQ_EINVAL, "token id %d outside 0..%lld", q_tokens[t], (long long)n_tokens - 1);
    return RQ_OK;
}

// Masks of the masked calls (rq_sparse_topk_masked*): [n_masks][sparse_mask_words(n_docs)] uint32, bit r % 32 of word r / 32 = row r
// is allowed (the layout of rq_filter_create's bitmap).  Both forms: no table is legal when every query is unrestricted.
static inline int64_t sparse_mask_words(int64_t n_docs) { return (n_docs + 31) / 32; }
static inline int sparse_check_masks(const void* masks, int n_masks, const void* mask_of) {
    if (!mask_of) return set_err(RQ_EINVAL, "null mask_of");
    if (n_masks < 0 || (n_masks > 0 && !masks)) return set_err(RQ_EINVAL, "n_masks %d negative, or masks without an array", n_masks);
    return RQ_OK;
}
// The host form sees mask_of: every entry is -1 (unrestricted) or a mask of the table.
static inline int sparse_check_mask_of(const int32_t* mask_of, int B, int n_masks) {
    for (int q = 0; q < B; ++q)
        if (mask_of[q] < -1 || mask_of[q] >= n_masks) return set_err(RQ_EINVAL, "mask_of[%d] is %d, outside -1..%d", q, mask_of[q], n_masks - 1);
    return RQ_OK;
}

// Grouped calls (rq_sparse_set_groups, rq_sparse_topk_grouped*).  The table: one int32 per document, -1 = a group of
// its own, any other value >= 0 (ids need not be dense or small).
#define RQ_SPARSE_GROUP_NONE (-1)
#define RQ_SPARSE_GROUPED_TILE_MAX 4096           // accumulators (32 KiB) + the collapse table (64 KiB) = 96 KiB of the CU's 160 KiB
#define RQ_SPARSE_GROUPED_CHUNK RQ_SPARSE_MAX_K   // candidates the grouped final kernel ranks and walks at a time
#define RQ_SPARSE_GROUPED_SET (4 * RQ_SPARSE_MAX_K)   // slots of its group set: at most k winners + one chunk of groups, load <= 1/2
static inline int sparse_check_groups(const void* h, const int32_t* groups, int64_t n_docs, int64_t handle_docs) {
    if (!h) return set_err(RQ_EINVAL, "null handle");
    if (n_docs != handle_docs) return set_err(RQ_EINVAL, "n_docs %lld, the index holds %lld documents", (long long)n_docs, (long long)handle_docs);
    if (n_docs > 0 && !groups) return set_err(RQ_EINVAL, "null groups");
    for (int64_t i = 0; i < n_docs; ++i)
        if (groups[i] < RQ_SPARSE_GROUP_NONE) return set_err(RQ_EINVAL, "groups[%lld] is %d: a group id is -1 or not negative", (long long)i, groups[i]);
    return RQ_OK;
}
// Both grouped entry points: the masked call's checks with mask_of == NULL legal (every query unrestricted), and the count array.
static inline int sparse_check_grouped(bool has_table, const void* masks, int n_masks, const void* mask_of, const void* out_count) {
    if (!has_table) return set_err(RQ_EINVAL, "no group table: call rq_sparse_set_groups first");
    if (!out_count) return set_err(RQ_EINVAL, "null out_count");
    if (n_masks < 0 || (n_masks > 0 && !masks)) return set_err(RQ_EINVAL, "n_masks %d negative, or masks without an array", n_masks);
    if (!mask_of && n_masks > 0) return set_err(RQ_EINVAL, "masks without mask_of");
    return RQ_OK;
}
// A grouped call runs in tiles of min(tile_docs, 4096) documents: the tile kernel keeps, beside the accumulators, an open-addressing
// table of 2 x tile slots (a uint32 group id and the int32 local index of the group's best document: 8 B per slot) in dynamic LDS.
static inline int sparse_grouped_tile(int tile_docs) { return std::min(tile_docs, RQ_SPARSE_GROUPED_TILE_MAX); }
static inline int sparse_grouped_slots(int tile) { return 2 * tile; }
static inline size_t sparse_grouped_tile_lds(int tile) { return (size_t)tile * sizeof(double) + (size_t)sparse_grouped_slots(tile) * 8; }
// static LDS of the grouped final kernel: one chunk (score bits, rows, groups) and the group set (id + order index), beside the
// selection body's histogram
static inline size_t sparse_grouped_final_lds() { return (size_t)RQ_SPARSE_GROUPED_CHUNK * (8 + 4 + 4) + (size_t)RQ_SPARSE_GROUPED_SET * 8; }
// slot of a group id in a table of `slots` (a power of two): the top bits of a multiplicative hash, so ids that share their low
// bits (multiples of 8 192) or their high bits (values near 2^31) spread; collisions probe linearly
static inline __host__ __device__ unsigned sparse_group_hash(uint32_t g, unsigned log2_slots) { return (g * 2654435761u) >> (32 - log2_slots); }

static inline bool sparse_tile_ok(double v) {
    if (!(v >= RQ_SPARSE_TILE_MIN && v <= RQ_SPARSE_TILE_MAX)) return false;   // (NaN and values no int holds included)
    const int t = (int)v;
    return (double)t == v && (t & (t - 1)) == 0;
}

// A call: `tiles` tiles of tile_docs consecutive documents (the last one may be short; an empty corpus has none), every tile keeps
// its best `slot` = min(k, tile_docs) candidates per query in a slot of its own, the queries go in `rounds` rounds of at most
// `per_round`: round r = queries [r * per_round, min(B, (r + 1) * per_round)).  A query whose candidates alone exceed the cap gets a
// round of its own.
struct SparsePlan {
    int64_t tiles = 0;
    int slot = 0;
    int64_t query_bytes = 0;       // candidate bytes of one query: tiles x slot x 12
    int per_round = 0, rounds = 0;
    size_t cand_elems = 0;         // per_round x tiles x slot
    size_t count_elems = 0;        // per_round x tiles
    // workspace: uint64 score bits [cand_elems], then int32 rows [cand_elems], then int32 counts [count_elems]
    size_t rows_offset() const { return cand_elems * 8; }
    size_t counts_offset() const { return cand_elems * 12; }
    size_t bytes() const { return cand_elems * 12 + count_elems * 4; }
    int round_first(int r) const { return r * per_round; }
    int round_count(int r, int B) const { return std::min(per_round, B - r * per_round); }
};
static inline int64_t sparse_tiles(int64_t n_docs, int tile_docs) { return (n_docs + tile_docs - 1) / tile_docs; }
// cand_cap <= 0: RQ_SPARSE_CAND_CAP
static inline SparsePlan sparse_plan(int64_t n_docs, int tile_docs, int B, int k, int64_t cand_cap) {
    SparsePlan p;
    p.tiles = sparse_tiles(n_docs, tile_docs);
    p.slot = std::min(k, tile_docs);
    p.query_bytes = p.tiles * (int64_t)p.slot * RQ_SPARSE_CAND_BYTES;
    const int64_t cap = cand_cap > 0 ? cand_cap : RQ_SPARSE_CAND_CAP;
    const int64_t fit = p.query_bytes > 0 ? cap / p.query_bytes : (int64_t)B;
    p.per_round = (int)std::max<int64_t>(1, std::min<int64_t>(B, fit));
    p.rounds = (B + p.per_round - 1) / p.per_round;
    p.cand_elems = (size_t)p.per_round * (size_t)p.tiles * (size_t)p.slot;
    p.count_elems = (size_t)p.per_round * (size_t)p.tiles;
    return p;
}

// Launch grids: the tile kernel (tiles, queries of the round), the final kernel (queries of the round); 256 threads each.  The tile
// kernel's dynamic LDS is its accumulator, tile_docs x 8 bytes.
struct SparseGrid { unsigned tile_x = 0, tile_y = 0, final_x = 0, block = RQ_SPARSE_THREADS; size_t tile_lds = 0; };
static inline SparseGrid sparse_grid(const SparsePlan& p, int tile_docs, int queries) {
    SparseGrid g;
    g.tile_x = (unsigned)p.tiles;
    g.tile_y = (unsigned)queries;
    g.final_x = (unsigned)queries;
    g.tile_lds = (size_t)tile_docs * sizeof(double);
    return g;
}
// A grouped call: the plan is sparse_plan over sparse_grouped_tile(tile_docs), the grids are the same, the tile kernel's dynamic LDS
// adds the collapse table, and the final kernel is the grouped one (static LDS: sparse_grouped_final_lds()).
static inline SparseGrid sparse_grouped_grid(const SparsePlan& p, int tile, int queries) {
    SparseGrid g = sparse_grid(p, tile, queries);
    g.tile_lds = sparse_grouped_tile_lds(tile);
    return g;
}
