// rq_sparse.hip -- sparse search on the device (include/rq.h rq_sparse_*): exact BM25 top-k over a device-resident posting index,
// the definition of rq_bm25_topk (include/rq_bm25.h) with the same rows and the same score bits.
//
// rq_sparse_tile_kernel, grid (tiles, queries): a workgroup owns tile_docs consecutive documents and one float64 accumulator per
// document in LDS.  For the query's tokens IN QUERY ORDER it finds the token's postings inside the tile (two binary searches over the
// token's ascending rows, a chunk of 256 tokens at a time, one thread each) and adds their contributions.
//   Bit exactness: a token names a row at most once, so within one token every accumulator is touched by at most one thread, once --
//   no race, no atomic; the barrier after every token keeps the additions to one accumulator in query order.  Every score is thus
//   0.0 + c_1 + c_2 + ... in float64 (no contraction: -ffp-contract=off, and there is nothing to contract), the very additions of the
//   host library.
// A tile in which no token has a posting leaves before it zeroes anything.  Otherwise the tile's best min(k, positives) are cut out
// exactly (rq_sparse_select.h) and written, in any order, to the tile's slot of the workspace with their count.
// rq_sparse_final_kernel, one workgroup per query: the best k of the tiles' candidates by the same selection body, sorted best first
// with ties by descending row (the keys are unique: the result does not depend on the order of the slots), then the padding.
//
// Masked calls (rq_sparse_topk_masked*) run rq_sparse_tile_kernel<true>: query q of the CALL answers under mask
// mask_of[q] ([W] uint32 words, bit r % 32 of word r / 32 = row r is allowed; -1: unrestricted, anything else outside
// [0, n_masks): nothing is allowed).  The mask enters in two places and nowhere else:
//   (a) before any posting is looked up, the workgroup ORs the mask words of its tile (tile_docs is a power of two >= 64: a tile starts
//       on a word boundary and has at most 256 words, one load per thread; the last word of the ragged last tile is cut at n_docs).  A
//       tile in which no document is allowed leaves with count 0 and is counted in `masked`, not in `skipped`.
//   (b) after the accumulation and before anything is counted or selected, the accumulators of the disallowed documents are set to 0.0
//       in one pass.  The positives count, the threshold and the candidate write below it then all see the same masked set -- a count
//       taken before the mask and a selection after it would write fewer candidates than `want` and leave garbage in the slot.
//   Bit exactness: the accumulation is untouched -- the same additions in the same order on every touched document, allowed or not --
//   so an allowed document's score has the bits of the unmasked call, and a disallowed one is exactly the 0.0 that
//   np.where(keep, scores, 0.0) writes before the score > 0 selection of the host definition.
// The unmasked instantiation holds none of this (if constexpr): its code, counters and launches are those of the call before masks.
//
// Grouped calls (rq_sparse_set_groups, rq_sparse_topk_grouped*) run rq_sparse_tile_kernel<*, true> over tiles of
// min(tile_docs, 4096) documents and rq_sparse_final_grouped_kernel: one document per group of the table (-1: a group of its own), the
// definition of BM25Index._search_distinct.
//   (c) after the accumulation and the mask pass (b) and before anything is counted, every document that is not the best of its group
//       INSIDE THE TILE -- the larger (score bits, row) -- is set to 0.0.  Exact: a query's winner is the best document of its group
//       everywhere, so it survives its own tile's collapse; and if k other group-bests of its tile ranked above it, k distinct groups
//       would beat it globally.  So the tile's min(k, tile_docs) best group-bests hold every winner of the tile.
//   The final kernel walks the tiles' candidates (a group at most once per tile) in ranked chunks and emits the first of every group.
// Neither mechanism depends on the order in which threads arrive: the table slot ends at a maximum, the set entry at a minimum.
// The ungrouped instantiations and rq_sparse_final_kernel hold none of this: same instructions as before the grouped calls.
#include "rq_sparse_plan.h"
#include "rq_sparse_select.h"
#include "rq_sparse_handle.h"
#include "rq_stage.h"

struct SparseArgs {
    const int64_t* indptr;      // [n_tokens + 1]
    const int32_t* rows;        // [nnz]
    const double* contrib;      // [nnz]
    int64_t n_tokens, n_docs, tiles;
    const int64_t* q_indptr;    // [B + 1] of the whole call
    const int32_t* q_tokens;    // [n_q_tokens]
    int64_t n_q_tokens;
    int q0;                     // first query of the round
    int k, slot, tile_docs;
    uint64_t* cand_bits;        // [queries of the round][tiles][slot]
    int32_t* cand_rows;
    int32_t* counts;            // [queries of the round][tiles]
    unsigned long long* skipped;
    // masked calls only (rq_sparse_tile_kernel<true>)
    const uint32_t* masks;      // [n_masks][mask_words]
    const int32_t* mask_of;     // [B] of the whole call
    int n_masks;
    int64_t mask_words;         // ceil(n_docs / 32)
    unsigned long long* masked; // tiles that left because their mask allows no document
    int32_t* out_rows;          // [B][k] of the whole call
    double* out_scores;
    // grouped calls only (rq_sparse_tile_kernel<*, true>, rq_sparse_final_grouped_kernel)
    const int32_t* groups;      // [n_docs], -1 = a group of its own
    int group_log2;             // log2 of the collapse table's 2 x tile_docs slots
    int32_t* out_count;         // [B] of the whole call
    unsigned long long* final_chunks;   // the largest number of chunks one query's final walk took
};

// first position in [b, e) whose row is >= v (rows ascending)
__device__ __forceinline__ int64_t sparse_lower_bound(const int32_t* rows, int64_t b, int64_t e, int64_t v) {
    while (b < e) {
        const int64_t m = b + ((e - b) >> 1);
        if ((int64_t)rows[m] < v) b = m + 1;
        else e = m;
    }
    return b;
}

// the accumulator of a tile as candidates: position i = document tile_lo + i, a candidate when its score is positive
struct SparseTileSrc {
    const double* acc;
    int n;
    uint32_t row0;
    __device__ __forceinline__ int64_t size() const { return n; }
    __device__ __forceinline__ bool get(int64_t i, uint64_t& hi, uint32_t& lo) const {
        const double v = acc[i];
        hi = (uint64_t)__double_as_longlong(v);
        lo = row0 + (uint32_t)i;
        return v > 0.0;   // false for NaN, a negative total, an exact cancellation
    }
};

template <bool MASKED, bool GROUPED>
__global__ __launch_bounds__(RQ_SPARSE_THREADS) void rq_sparse_tile_kernel(SparseArgs a) {
    extern __shared__ double s_acc[];   // [tile_docs]; grouped: then the collapse table, uint32 ids and int32 best indices [2 x tile_docs] each
    __shared__ int64_t s_lo[RQ_SPARSE_CHUNK], s_hi[RQ_SPARSE_CHUNK];
    __shared__ SparseSelShared s_sel;
    __shared__ unsigned s_n;
    const int tid = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int ql = (int)blockIdx.y;
    const int64_t tile_lo = tile * (int64_t)a.tile_docs;
    const int64_t tile_hi = tile_lo + a.tile_docs < a.n_docs ? tile_lo + a.tile_docs : a.n_docs;
    const int nloc = (int)(tile_hi - tile_lo);
    const uint32_t* mask = nullptr;   // the mask words of this tile; null: the query is unrestricted
    uint32_t mask_w = 0;              // word tid of them, cut at n_docs (threads beyond the tile's words: 0)
    if constexpr (MASKED) {
        // mask_of is indexed by the query's position in the CALL.  The array may be the caller's device memory: a value outside
        // [-1, n_masks) allows nothing and reads no mask (the manner of the token clamping below).
        const int m = a.mask_of[a.q0 + ql];
        if (m != -1) {
            const int nw = (nloc + 31) >> 5;   // <= tile_docs / 32 <= 256; tile_lo / 32 + nw <= mask_words as tile_hi <= n_docs
            if (m >= 0 && m < a.n_masks) {
                mask = a.masks + (size_t)m * (size_t)a.mask_words + (size_t)(tile_lo >> 5);
                if (tid < nw) {
                    mask_w = mask[tid];
                    if (tid == nw - 1 && (nloc & 31)) mask_w &= (1u << (nloc & 31)) - 1u;   // bits at or beyond n_docs are ignored
                }
            }
            if (!__syncthreads_or(mask_w != 0)) {   // no document of the tile is allowed
                if (tid == 0) {
                    a.counts[(size_t)ql * (size_t)a.tiles + (size_t)tile] = 0;
                    atomicAdd(a.masked, 1ull);
                }
                return;
            }
        }
    }
    // the query's tokens; the arrays may be the caller's device memory, which no host check has seen: stay inside [0, n_q_tokens)
    int64_t t0 = a.q_indptr[a.q0 + ql], t1 = a.q_indptr[a.q0 + ql + 1];
    t0 = t0 < 0 ? 0 : (t0 > a.n_q_tokens ? a.n_q_tokens : t0);
    t1 = t1 < t0 ? t0 : (t1 > a.n_q_tokens ? a.n_q_tokens : t1);
    bool zeroed = false;
    for (int64_t c = t0; c < t1; c += RQ_SPARSE_CHUNK) {
        const int nch = (int)(t1 - c < RQ_SPARSE_CHUNK ? t1 - c : RQ_SPARSE_CHUNK);
        int64_t lo = 0, hi = 0;
        if (tid < nch) {
            const int64_t tok = a.q_tokens[c + tid];
            if (tok >= 0 && tok < a.n_tokens) {   // an id outside the index is an empty posting list
                const int64_t b = a.indptr[tok], e = a.indptr[tok + 1];
                lo = sparse_lower_bound(a.rows, b, e, tile_lo);
                // rows ascend strictly: rows[lo + j] >= tile_lo + j, so the tile's postings end within nloc positions of lo
                hi = sparse_lower_bound(a.rows, lo, e - lo > nloc ? lo + nloc : e, tile_hi);
            }
        }
        s_lo[tid] = lo;
        s_hi[tid] = hi;
        if (!__syncthreads_or(hi > lo)) continue;   // (nobody reads s_lo / s_hi of this chunk)
        if (!zeroed) {
            for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS) s_acc[i] = 0.0;
            zeroed = true;
            __syncthreads();
        }
        for (int j = 0; j < nch; ++j) {
            const int64_t pl = s_lo[j], ph = s_hi[j];
            if (ph <= pl) continue;
            for (int64_t p = pl + tid; p < ph; p += RQ_SPARSE_THREADS) s_acc[(int64_t)a.rows[p] - tile_lo] += a.contrib[p];
            __syncthreads();   // the next token's additions come after this token's: query order
        }
        __syncthreads();       // s_lo / s_hi are free for the next chunk
    }
    int32_t* count = a.counts + (size_t)ql * (size_t)a.tiles + (size_t)tile;
    if (!zeroed) {             // no token of the query has a posting in this tile
        if (tid == 0) {
            *count = 0;
            atomicAdd(a.skipped, 1ull);
        }
        return;
    }
    if constexpr (MASKED) {
        // (b): a disallowed document scores 0.0 from here on (the barrier below orders this pass before every reader).  The words come
        // from the registers of (a) through s_lo, which is free since the loop's last barrier: no second trip to global memory.
        if (mask) {
            uint32_t* s_words = reinterpret_cast<uint32_t*>(s_lo);   // RQ_SPARSE_THREADS words of the 2 x RQ_SPARSE_CHUNK it holds
            s_words[tid] = mask_w;
            __syncthreads();
            for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS)
                if (!((s_words[i >> 5] >> (i & 31)) & 1u)) s_acc[i] = 0.0;
        }
    }
    if constexpr (GROUPED) {
        // (c): of every group, only the tile's best document -- the larger (score bits, row) -- keeps its score; the others score 0.0
        // from here on, like the disallowed ones.  A slot of the table is claimed for a group id by atomicCAS (linear probing: at
        // most nloc <= tile_docs groups in 2 x tile_docs slots), its value is raised to the local index of the best document by a CAS
        // loop over keys read from s_acc, which nobody writes meanwhile: whatever the order of arrival, the slot ends at the maximum.
        uint32_t* s_gid = reinterpret_cast<uint32_t*>(s_acc + a.tile_docs);
        int* s_best = reinterpret_cast<int*>(s_gid + 2 * a.tile_docs);
        const unsigned slots = 2u * (unsigned)a.tile_docs;
        for (unsigned i = tid; i < slots; i += RQ_SPARSE_THREADS) { s_gid[i] = 0xFFFFFFFFu; s_best[i] = -1; }
        __syncthreads();   // (and the mask pass above is complete)
        for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS) {
            const double v = s_acc[i];
            if (!(v > 0.0)) continue;
            const int32_t g = a.groups[tile_lo + i];
            if (g < 0) continue;   // a group of its own
            unsigned s = sparse_group_hash((uint32_t)g, (unsigned)a.group_log2);
            for (;;) {
                const uint32_t prev = atomicCAS(&s_gid[s], 0xFFFFFFFFu, (uint32_t)g);
                if (prev == 0xFFFFFFFFu || prev == (uint32_t)g) break;
                s = (s + 1) & (slots - 1);
            }
            const uint64_t mine = (uint64_t)__double_as_longlong(v);
            int cur = s_best[s];
            for (;;) {
                if (cur >= 0) {
                    const uint64_t other = (uint64_t)__double_as_longlong(s_acc[cur]);
                    if (other > mine || (other == mine && cur > i)) break;   // (cur == i cannot be: i is offered once)
                }
                const int prev = atomicCAS(&s_best[s], cur, i);
                if (prev == cur) break;
                cur = prev;
            }
        }
        __syncthreads();
        for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS) {   // (a thread writes its own documents only and reads no other's score)
            if (!(s_acc[i] > 0.0)) continue;
            const int32_t g = a.groups[tile_lo + i];
            if (g < 0) continue;
            unsigned s = sparse_group_hash((uint32_t)g, (unsigned)a.group_log2);
            while (s_gid[s] != (uint32_t)g) s = (s + 1) & (slots - 1);
            if (s_best[s] != i) s_acc[i] = 0.0;
        }
    }
    const SparseTileSrc src{s_acc, nloc, (uint32_t)tile_lo};
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS) mine += s_acc[i] > 0.0 ? 1u : 0u;
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const unsigned positives = s_n;
    const unsigned want = positives < (unsigned)a.k ? positives : (unsigned)a.k;   // <= slot = min(k, tile_docs)
    __syncthreads();
    if (tid == 0) { *count = (int32_t)want; s_n = 0; }
    uint64_t thr_hi = 0;
    uint32_t thr_lo = 0;
    if (positives > want) sparse_select_threshold(src, want, s_sel, thr_hi, thr_lo);
    __syncthreads();
    const size_t base = ((size_t)ql * (size_t)a.tiles + (size_t)tile) * (size_t)a.slot;
    for (int i = tid; i < nloc; i += RQ_SPARSE_THREADS) {
        uint64_t hi;
        uint32_t lo;
        if (!src.get(i, hi, lo) || !sparse_key_ge(hi, lo, thr_hi, thr_lo)) continue;
        const unsigned j = atomicAdd(&s_n, 1u);
        if (j < (unsigned)a.slot) {
            a.cand_bits[base + j] = hi;
            a.cand_rows[base + j] = (int32_t)lo;
        }
    }
}

// the candidates of one query in the workspace: position i = entry i % slot of tile i / slot, a candidate below the tile's count
struct SparseFinalSrc {
    const uint64_t* bits;
    const int32_t* rows;
    const int32_t* counts;
    int64_t n;
    int slot;
    __device__ __forceinline__ int64_t size() const { return n; }
    __device__ __forceinline__ bool get(int64_t i, uint64_t& hi, uint32_t& lo) const {
        const int64_t t = i / slot;
        if ((int)(i - t * slot) >= counts[t]) return false;
        hi = bits[i];
        lo = (uint32_t)rows[i];
        return true;
    }
};

__global__ __launch_bounds__(RQ_SPARSE_THREADS) void rq_sparse_final_kernel(SparseArgs a) {
    __shared__ uint64_t s_bits[RQ_SPARSE_MAX_K];
    __shared__ int32_t s_rows[RQ_SPARSE_MAX_K];
    __shared__ SparseSelShared s_sel;
    __shared__ unsigned s_n;
    const int tid = (int)threadIdx.x;
    const int ql = (int)blockIdx.x;
    const size_t qt = (size_t)ql * (size_t)a.tiles;
    const int32_t* counts = a.counts + qt;
    const SparseFinalSrc src{a.cand_bits + qt * (size_t)a.slot, a.cand_rows + qt * (size_t)a.slot, counts, a.tiles * (int64_t)a.slot, a.slot};
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int64_t t = tid; t < a.tiles; t += RQ_SPARSE_THREADS) mine += (unsigned)counts[t];
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const unsigned total = s_n;   // <= the query's positive documents < 2^31
    const unsigned want = total < (unsigned)a.k ? total : (unsigned)a.k;
    __syncthreads();
    if (tid == 0) s_n = 0;
    uint64_t thr_hi = 0;
    uint32_t thr_lo = 0;
    if (total > want) sparse_select_threshold(src, want, s_sel, thr_hi, thr_lo);
    __syncthreads();
    if (want > 0)
        for (int64_t i = tid; i < src.n; i += RQ_SPARSE_THREADS) {
            uint64_t hi;
            uint32_t lo;
            if (!src.get(i, hi, lo) || !sparse_key_ge(hi, lo, thr_hi, thr_lo)) continue;
            const unsigned j = atomicAdd(&s_n, 1u);
            if (j < RQ_SPARSE_MAX_K) { s_bits[j] = hi; s_rows[j] = (int32_t)lo; }
        }
    unsigned P = 1;
    while (P < want) P <<= 1;
    __syncthreads();
    for (unsigned i = want + tid; i < P; i += RQ_SPARSE_THREADS) { s_bits[i] = 0; s_rows[i] = -1; }   // below every candidate
    __syncthreads();
    // bitonic sort of P (a power of two) keys, best first: larger score bits, then larger row
    for (unsigned size = 2; size <= P; size <<= 1)
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned t = tid; t < P / 2; t += RQ_SPARSE_THREADS) {
                const unsigned i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t bi = s_bits[i], bj = s_bits[j];
                const int32_t ri = s_rows[i], rj = s_rows[j];
                const bool j_first = bj > bi || (bj == bi && rj > ri);
                if (((i & size) == 0) == j_first) { s_bits[i] = bj; s_bits[j] = bi; s_rows[i] = rj; s_rows[j] = ri; }
            }
            __syncthreads();
        }
    int32_t* orow = a.out_rows + (size_t)(a.q0 + ql) * (size_t)a.k;
    double* osc = a.out_scores + (size_t)(a.q0 + ql) * (size_t)a.k;
    for (unsigned i = tid; i < (unsigned)a.k; i += RQ_SPARSE_THREADS) {
        orow[i] = i < want ? s_rows[i] : -1;
        osc[i] = i < want ? __longlong_as_double((long long)s_bits[i]) : 0.0;
    }
}

// the candidates of one query whose key lies strictly below a bound (the previous chunk's threshold); unbounded: all of them
struct SparseBelowSrc {
    SparseFinalSrc s;
    bool bounded;
    uint64_t b_hi;
    uint32_t b_lo;
    __device__ __forceinline__ int64_t size() const { return s.n; }
    __device__ __forceinline__ bool get(int64_t i, uint64_t& hi, uint32_t& lo) const {
        if (!s.get(i, hi, lo)) return false;
        return !bounded || !sparse_key_ge(hi, lo, b_hi, b_lo);
    }
};

// The final kernel of a grouped call, one workgroup per query.  The tiles' candidates hold a group at most once per tile; they are
// walked in ranked chunks of at most RQ_SPARSE_GROUPED_CHUNK: the next-best chunk is cut out by the selection body (keys strictly
// below the previous chunk's threshold), sorted by the bitonic body of rq_sparse_final_kernel, and walked in order -- a candidate is
// emitted when its group is -1 or has not been walked before.  "Walked before" is an LDS set keyed by group id whose value is the
// ORDER INDEX (chunk x chunk size + rank) of the group's first candidate, lowered by atomicMin: a minimum does not depend on the
// order in which threads arrive.  A candidate is its group's first exactly when the set holds its own order index; the emitted ones
// get their output position from a prefix sum over the chunk.  Every walked group either wins or has won, and the walk stops at k
// winners: the set never holds more than k - 1 + one chunk of groups, half of its RQ_SPARSE_GROUPED_SET slots at the most.
__global__ __launch_bounds__(RQ_SPARSE_THREADS) void rq_sparse_final_grouped_kernel(SparseArgs a) {
    constexpr unsigned CH = RQ_SPARSE_GROUPED_CHUNK, SET = RQ_SPARSE_GROUPED_SET, PER = CH / RQ_SPARSE_THREADS;
    static_assert(SET == 1u << 12 && CH % RQ_SPARSE_THREADS == 0 && 2 * (RQ_SPARSE_MAX_K + CH) <= SET, "the group set: 4 096 slots, at most half full");
    __shared__ uint64_t s_bits[CH];
    __shared__ int32_t s_rows[CH];
    __shared__ int32_t s_grp[CH];
    __shared__ uint32_t s_set_id[SET], s_set_ord[SET];
    __shared__ SparseSelShared s_sel;
    __shared__ unsigned s_n, s_wave[RQ_SPARSE_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int ql = (int)blockIdx.x;
    const size_t qt = (size_t)ql * (size_t)a.tiles;
    const int32_t* counts = a.counts + qt;
    const SparseFinalSrc all{a.cand_bits + qt * (size_t)a.slot, a.cand_rows + qt * (size_t)a.slot, counts, a.tiles * (int64_t)a.slot, a.slot};
    for (unsigned i = tid; i < SET; i += RQ_SPARSE_THREADS) { s_set_id[i] = 0xFFFFFFFFu; s_set_ord[i] = 0xFFFFFFFFu; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int64_t t = tid; t < a.tiles; t += RQ_SPARSE_THREADS) mine += (unsigned)counts[t];
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    unsigned below = s_n;        // candidates not yet walked: < 2^31
    unsigned emitted = 0, chunks = 0;
    SparseBelowSrc src{all, false, 0, 0};
    int32_t* orow = a.out_rows + (size_t)(a.q0 + ql) * (size_t)a.k;
    double* osc = a.out_scores + (size_t)(a.q0 + ql) * (size_t)a.k;
    while (below > 0 && emitted < (unsigned)a.k) {   // (uniform: every thread holds the same counts)
        const unsigned want = below < CH ? below : CH;
        __syncthreads();
        if (tid == 0) s_n = 0;
        uint64_t thr_hi = 0;
        uint32_t thr_lo = 0;
        if (below > want) sparse_select_threshold(src, want, s_sel, thr_hi, thr_lo);
        __syncthreads();
        for (int64_t i = tid; i < src.s.n; i += RQ_SPARSE_THREADS) {
            uint64_t hi;
            uint32_t lo;
            if (!src.get(i, hi, lo) || !sparse_key_ge(hi, lo, thr_hi, thr_lo)) continue;
            const unsigned j = atomicAdd(&s_n, 1u);
            if (j < CH) { s_bits[j] = hi; s_rows[j] = (int32_t)lo; }
        }
        unsigned P = 1;
        while (P < want) P <<= 1;
        __syncthreads();
        for (unsigned i = want + tid; i < P; i += RQ_SPARSE_THREADS) { s_bits[i] = 0; s_rows[i] = -1; }   // below every candidate
        __syncthreads();
        for (unsigned size = 2; size <= P; size <<= 1)
            for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
                for (unsigned t = tid; t < P / 2; t += RQ_SPARSE_THREADS) {
                    const unsigned i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const uint64_t bi = s_bits[i], bj = s_bits[j];
                    const int32_t ri = s_rows[i], rj = s_rows[j];
                    const bool j_first = bj > bi || (bj == bi && rj > ri);
                    if (((i & size) == 0) == j_first) { s_bits[i] = bj; s_bits[j] = bi; s_rows[i] = rj; s_rows[j] = ri; }
                }
                __syncthreads();
            }
        // the groups of the chunk (a candidate's row lies in [0, n_docs): the tile kernel wrote it), and their first order index
        const unsigned base = chunks * CH;
        for (unsigned i = tid; i < want; i += RQ_SPARSE_THREADS) {
            const int32_t g = a.groups[s_rows[i]];
            s_grp[i] = g;
            if (g < 0) continue;
            unsigned s = sparse_group_hash((uint32_t)g, 12);
            for (;;) {
                const uint32_t prev = atomicCAS(&s_set_id[s], 0xFFFFFFFFu, (uint32_t)g);
                if (prev == 0xFFFFFFFFu || prev == (uint32_t)g) break;
                s = (s + 1) & (SET - 1);
            }
            atomicMin(&s_set_ord[s], base + i);
        }
        __syncthreads();
        // thread t owns ranks PER x t .. PER x t + PER - 1: keep flags, then their exclusive prefix sum over the workgroup
        unsigned keep = 0, cnt = 0;
        for (unsigned j = 0; j < PER; ++j) {
            const unsigned i = PER * tid + j;
            if (i >= want) break;
            const int32_t g = s_grp[i];
            bool first = g < 0;
            if (!first) {
                unsigned s = sparse_group_hash((uint32_t)g, 12);
                while (s_set_id[s] != (uint32_t)g) s = (s + 1) & (SET - 1);
                first = s_set_ord[s] == base + i;
            }
            if (first) { keep |= 1u << j; ++cnt; }
        }
        unsigned inc = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, o, 64);
            if ((tid & 63) >= o) inc += v;
        }
        if ((tid & 63) == 63) s_wave[tid >> 6] = inc;
        __syncthreads();
        unsigned before = emitted + inc - cnt, kept = 0;
        for (int w = 0; w < RQ_SPARSE_THREADS / 64; ++w) {
            if (w < (tid >> 6)) before += s_wave[w];
            kept += s_wave[w];
        }
        for (unsigned j = 0; j < PER; ++j) {
            if (!((keep >> j) & 1u)) continue;
            if (before < (unsigned)a.k) {
                orow[before] = s_rows[PER * tid + j];
                osc[before] = __longlong_as_double((long long)s_bits[PER * tid + j]);
            }
            ++before;
        }
        emitted = emitted + kept < (unsigned)a.k ? emitted + kept : (unsigned)a.k;
        src.bounded = true;
        src.b_hi = thr_hi;
        src.b_lo = thr_lo;
        below -= want;
        ++chunks;
    }
    for (unsigned i = emitted + tid; i < (unsigned)a.k; i += RQ_SPARSE_THREADS) { orow[i] = -1; osc[i] = 0.0; }
    if (tid == 0) {
        a.out_count[a.q0 + ql] = (int32_t)emitted;
        atomicMax(a.final_chunks, (unsigned long long)chunks);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static void sparse_free(rq_sparse* h) {
    if (h->own) (void)hipStreamDestroy(h->own);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    free_dev(h->d_indptr, h->d_rows, h->d_contrib, h->ws, h->d_skipped, h->d_groups);   // (d_skipped holds all three counters)
    delete h;
}

extern "C" rq_sparse* rq_sparse_create(int device_id, const int64_t* indptr, const int32_t* rows, const double* contrib, int64_t n_tokens, int64_t n_docs) {
    if (sparse_check_csr(indptr, rows, contrib, n_tokens, n_docs) != RQ_OK) return nullptr;
    const int ndev = rq_device_count();
    if (ndev <= 0) { err_no_device(); return nullptr; }
    if (device_id < 0 || device_id >= ndev) { set_err(RQ_EINVAL, "device %d outside 0..%d", device_id, ndev - 1); return nullptr; }
    DeviceGuard dg_(device_id);
    hipDeviceProp_t prop;
    if (!dg_.ok || hipGetDeviceProperties(&prop, device_id) != hipSuccess) { set_err(RQ_EHIP, "cannot open device %d", device_id); return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(RQ_ENODEVICE, "device %d is %s; this library holds gfx950 code only", device_id, prop.gcnArchName);
        return nullptr;
    }
    rq_sparse* h = new rq_sparse();
    h->device = device_id;
    h->n_tokens = n_tokens;
    h->n_docs = n_docs;
    h->nnz = indptr[n_tokens];
    const size_t nnz = (size_t)h->nnz, pad = nnz ? nnz : 1;   // (empty lists: the kernels still get valid pointers)
    if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess || hipMalloc((void**)&h->d_skipped, 3 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&h->d_indptr, (size_t)(n_tokens + 1) * 8) != hipSuccess || hipMalloc((void**)&h->d_rows, pad * 4) != hipSuccess ||
        hipMalloc((void**)&h->d_contrib, pad * 8) != hipSuccess) {
        (void)hipGetLastError();
        set_err(RQ_ENOMEM, "no room for %zu postings and %lld tokens on device %d", nnz, (long long)n_tokens, device_id);
        sparse_free(h);
        return nullptr;
    }
    if (hipMemcpy(h->d_indptr, indptr, (size_t)(n_tokens + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (nnz && (hipMemcpy(h->d_rows, rows, nnz * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_contrib, contrib, nnz * 8, hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemset(h->d_skipped, 0, 3 * sizeof(unsigned long long)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rq_sparse_tile_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, RQ_SPARSE_TILE_MAX * (int)sizeof(double)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rq_sparse_tile_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, RQ_SPARSE_TILE_MAX * (int)sizeof(double)) != hipSuccess) {
        set_err(RQ_EHIP, "upload of the posting index to device %d failed", device_id);
        sparse_free(h);
        return nullptr;
    }
    return h;
}

extern "C" void rq_sparse_destroy(rq_sparse* h) {
    if (!h) return;
    DeviceGuard dg_(h->device);
    (void)hipDeviceSynchronize();
    sparse_free(h);
}

extern "C" int64_t rq_sparse_postings(const rq_sparse* h) { return h ? h->nnz : 0; }

// Every device form: d_mask_of == nullptr is the unmasked call, d_count != nullptr the grouped one (its tiles are
// sparse_grouped_tile(tile_docs) wide, its tile kernel carries the collapse table, its final kernel is the grouped one).
static int sparse_topk_launch(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                              const uint32_t* d_masks, int n_masks, const int32_t* d_mask_of, int32_t* d_rows, double* d_scores, void* stream,
                              int32_t* d_count = nullptr) {
    if (n_q_tokens < 0 || (n_q_tokens > 0 && !d_q_tokens)) return set_err(RQ_EINVAL, "n_q_tokens %lld negative, or tokens without an array", (long long)n_q_tokens);
    RQ_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const bool grouped = d_count != nullptr;
    const int tile = grouped ? sparse_grouped_tile(h->tile_docs) : h->tile_docs;
    const SparsePlan p = sparse_plan(h->n_docs, tile, B, k, h->cand_cap);
    if (p.bytes() > h->ws_bytes) {   // growing waits for the device once: an earlier call may still read the old block
        HIPCHK(hipDeviceSynchronize());
        free_dev(h->ws);
        h->ws_bytes = 0;
        if (hipMalloc((void**)&h->ws, p.bytes()) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(RQ_ENOMEM, "sparse workspace of %zu bytes (%d queries x %lld tiles x %d candidates)", p.bytes(), p.per_round, (long long)p.tiles, p.slot);
        }
        h->ws_bytes = p.bytes();
    }
    HIPCHK(hipMemsetAsync(h->d_skipped, 0, 3 * sizeof(unsigned long long), s));   // both tile counters and the chunk count
    SparseArgs a;
    a.indptr = h->d_indptr; a.rows = h->d_rows; a.contrib = h->d_contrib;
    a.n_tokens = h->n_tokens; a.n_docs = h->n_docs; a.tiles = p.tiles;
    a.q_indptr = d_q_indptr; a.q_tokens = d_q_tokens; a.n_q_tokens = n_q_tokens;
    a.k = k; a.slot = p.slot; a.tile_docs = tile;
    a.cand_bits = (uint64_t*)h->ws;
    a.cand_rows = (int32_t*)(h->ws + p.rows_offset());
    a.counts = (int32_t*)(h->ws + p.counts_offset());
    a.skipped = h->d_skipped;
    a.masks = d_masks; a.mask_of = d_mask_of; a.n_masks = n_masks;
    a.mask_words = sparse_mask_words(h->n_docs);
    a.masked = h->d_skipped + 1;
    a.out_rows = d_rows; a.out_scores = d_scores;
    a.groups = h->d_groups; a.out_count = d_count; a.final_chunks = h->d_skipped + 2;
    a.group_log2 = 0;
    while ((1 << a.group_log2) < sparse_grouped_slots(tile)) ++a.group_log2;
    h->ev_used = 0;
    const size_t n_ev = h->profile ? 1 + 2 * (size_t)p.rounds : 0;
    while (h->ev.size() < n_ev) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    if (n_ev) HIPCHK(hipEventRecord(h->ev[0], s));
    for (int r = 0; r < p.rounds; ++r) {   // the rounds share the workspace: stream order keeps them apart
        a.q0 = p.round_first(r);
        const SparseGrid g = grouped ? sparse_grouped_grid(p, tile, p.round_count(r, B)) : sparse_grid(p, tile, p.round_count(r, B));
        if (p.tiles > 0) {
            if (grouped && d_mask_of) hipLaunchKernelGGL((rq_sparse_tile_kernel<true, true>), dim3(g.tile_x, g.tile_y), dim3(g.block), g.tile_lds, s, a);
            else if (grouped) hipLaunchKernelGGL((rq_sparse_tile_kernel<false, true>), dim3(g.tile_x, g.tile_y), dim3(g.block), g.tile_lds, s, a);
            else if (d_mask_of) hipLaunchKernelGGL((rq_sparse_tile_kernel<true, false>), dim3(g.tile_x, g.tile_y), dim3(g.block), g.tile_lds, s, a);
            else hipLaunchKernelGGL((rq_sparse_tile_kernel<false, false>), dim3(g.tile_x, g.tile_y), dim3(g.block), g.tile_lds, s, a);
        }
        if (n_ev) HIPCHK(hipEventRecord(h->ev[1 + 2 * (size_t)r], s));
        if (grouped) hipLaunchKernelGGL(rq_sparse_final_grouped_kernel, dim3(g.final_x), dim3(g.block), 0, s, a);
        else hipLaunchKernelGGL(rq_sparse_final_kernel, dim3(g.final_x), dim3(g.block), 0, s, a);
        if (n_ev) HIPCHK(hipEventRecord(h->ev[2 + 2 * (size_t)r], s));
    }
    h->ev_used = n_ev;
    HIPCHK(hipGetLastError());
    h->calls++;
    if (d_mask_of) h->masked_calls++;
    if (grouped) h->grouped_calls++;
    h->rounds_last = p.rounds;
    h->tiles_last = p.tiles * (int64_t)B;
    return RQ_OK;
}

extern "C" int rq_sparse_topk_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                                     int32_t* d_rows, double* d_scores, void* stream) {
    if (int rc = sparse_check_call(h, d_q_indptr, B, k, d_rows, d_scores)) return rc;
    return sparse_topk_launch(h, d_q_indptr, d_q_tokens, B, n_q_tokens, k, nullptr, 0, nullptr, d_rows, d_scores, stream);
}

extern "C" int rq_sparse_topk_masked_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                                            const uint32_t* d_masks, int n_masks, const int32_t* d_mask_of, int32_t* d_rows, double* d_scores,
                                            void* stream) {
    if (int rc = sparse_check_call(h, d_q_indptr, B, k, d_rows, d_scores)) return rc;
    if (int rc = sparse_check_masks(d_masks, n_masks, d_mask_of)) return rc;
    return sparse_topk_launch(h, d_q_indptr, d_q_tokens, B, n_q_tokens, k, d_masks, n_masks, d_mask_of, d_rows, d_scores, stream);
}

extern "C" int rq_sparse_set_groups(rq_sparse* h, const int32_t* groups, int64_t n_docs) {
    if (int rc = sparse_check_groups(h, groups, n_docs, h ? h->n_docs : 0)) return rc;
    RQ_ON_DEVICE(h);
    if (!h->grouped_lds_set) {   // the grouped tile kernels: accumulators + collapse table, 96 KiB at the most
        const int lds = (int)sparse_grouped_tile_lds(RQ_SPARSE_GROUPED_TILE_MAX);
        HIPCHK(hipFuncSetAttribute((const void*)rq_sparse_tile_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)rq_sparse_tile_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        h->grouped_lds_set = true;
    }
    int32_t* fresh = nullptr;
    if (hipMalloc((void**)&fresh, (size_t)(n_docs ? n_docs : 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(RQ_ENOMEM, "no room for a group table of %lld documents on device %d", (long long)n_docs, h->device);
    }
    if (n_docs && hipMemcpy(fresh, groups, (size_t)n_docs * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(fresh);
        return set_err(RQ_EHIP, "upload of the group table to device %d failed", h->device);
    }
    if (h->d_groups) {           // an earlier call may still read the table it replaces
        HIPCHK(hipDeviceSynchronize());
        free_dev(h->d_groups);
    }
    h->d_groups = fresh;
    return RQ_OK;
}

extern "C" int rq_sparse_topk_grouped_device(rq_sparse* h, const int64_t* d_q_indptr, const int32_t* d_q_tokens, int B, int64_t n_q_tokens, int k,
                                             const uint32_t* d_masks, int n_masks, const int32_t* d_mask_of, int32_t* d_rows, double* d_scores,
                                             int32_t* d_count, void* stream) {
    if (int rc = sparse_check_call(h, d_q_indptr, B, k, d_rows, d_scores)) return rc;
    if (int rc = sparse_check_grouped(h->d_groups != nullptr, d_masks, n_masks, d_mask_of, d_count)) return rc;
    return sparse_topk_launch(h, d_q_indptr, d_q_tokens, B, n_q_tokens, k, d_masks, n_masks, d_mask_of, d_rows, d_scores, stream, d_count);
}

extern "C" int rq_sparse_topk(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, int32_t* out_rows, double* out_scores) {
    if (int rc = sparse_check_call(h, q_indptr, B, k, out_rows, out_scores)) return rc;
    if (int rc = sparse_check_queries(q_indptr, q_tokens, B, h->n_tokens)) return rc;
    RQ_ON_DEVICE(h);
    // the tokens of the call alone: positions [q_indptr[0], q_indptr[B]) (the kernel clamps to [0, n_q_tokens), so the array is staged whole)
    const int64_t nq = q_indptr[B];
    const size_t bytes[4] = {(size_t)(B + 1) * 8, (size_t)(nq ? nq : 1) * 4, (size_t)B * (size_t)k * 4, (size_t)B * (size_t)k * 8};
    Stage st(h->own);
    if (st.alloc(bytes, 4, "rq_sparse_topk") != RQ_OK) return st.code();
    st.up(st.at<void>(0), q_indptr, bytes[0]);
    if (nq) st.up(st.at<void>(1), q_tokens, (size_t)nq * 4);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_sparse_topk_device(h, st.at<int64_t>(0), st.at<int32_t>(1), B, nq, k, st.at<int32_t>(2), st.at<double>(3), (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_rows, st.at<void>(2), bytes[2]);
    st.down(out_scores, st.at<void>(3), bytes[3]);
    return st.finish();
}

extern "C" int rq_sparse_topk_masked(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, const uint32_t* masks, int n_masks,
                                     const int32_t* mask_of, int32_t* out_rows, double* out_scores) {
    if (int rc = sparse_check_call(h, q_indptr, B, k, out_rows, out_scores)) return rc;
    if (int rc = sparse_check_queries(q_indptr, q_tokens, B, h->n_tokens)) return rc;
    if (int rc = sparse_check_masks(masks, n_masks, mask_of)) return rc;
    if (int rc = sparse_check_mask_of(mask_of, B, n_masks)) return rc;
    RQ_ON_DEVICE(h);
    const int64_t nq = q_indptr[B];
    const size_t mask_bytes = (size_t)n_masks * (size_t)sparse_mask_words(h->n_docs) * 4;
    const size_t bytes[6] = {(size_t)(B + 1) * 8, (size_t)(nq ? nq : 1) * 4, (size_t)B * (size_t)k * 4, (size_t)B * (size_t)k * 8,
                             mask_bytes ? mask_bytes : 4, (size_t)B * 4};
    Stage st(h->own);
    if (st.alloc(bytes, 6, "rq_sparse_topk_masked") != RQ_OK) return st.code();
    st.up(st.at<void>(0), q_indptr, bytes[0]);
    if (nq) st.up(st.at<void>(1), q_tokens, (size_t)nq * 4);
    if (mask_bytes) st.up(st.at<void>(4), masks, mask_bytes);
    st.up(st.at<void>(5), mask_of, bytes[5]);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_sparse_topk_masked_device(h, st.at<int64_t>(0), st.at<int32_t>(1), B, nq, k, st.at<uint32_t>(4), n_masks, st.at<int32_t>(5),
                                                st.at<int32_t>(2), st.at<double>(3), (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_rows, st.at<void>(2), bytes[2]);
    st.down(out_scores, st.at<void>(3), bytes[3]);
    return st.finish();
}

extern "C" int rq_sparse_topk_grouped(rq_sparse* h, const int64_t* q_indptr, const int32_t* q_tokens, int B, int k, const uint32_t* masks, int n_masks,
                                      const int32_t* mask_of, int32_t* out_rows, double* out_scores, int32_t* out_count) {
    if (int rc = sparse_check_call(h, q_indptr, B, k, out_rows, out_scores)) return rc;
    if (int rc = sparse_check_grouped(h->d_groups != nullptr, masks, n_masks, mask_of, out_count)) return rc;
    if (int rc = sparse_check_queries(q_indptr, q_tokens, B, h->n_tokens)) return rc;
    if (mask_of)
        if (int rc = sparse_check_mask_of(mask_of, B, n_masks)) return rc;
    RQ_ON_DEVICE(h);
    const int64_t nq = q_indptr[B];
    const size_t mask_bytes = mask_of ? (size_t)n_masks * (size_t)sparse_mask_words(h->n_docs) * 4 : 0;
    const size_t bytes[7] = {(size_t)(B + 1) * 8, (size_t)(nq ? nq : 1) * 4, (size_t)B * (size_t)k * 4, (size_t)B * (size_t)k * 8,
                             mask_bytes ? mask_bytes : 4, (size_t)B * 4, (size_t)B * 4};
    Stage st(h->own);
    if (st.alloc(bytes, 7, "rq_sparse_topk_grouped") != RQ_OK) return st.code();
    st.up(st.at<void>(0), q_indptr, bytes[0]);
    if (nq) st.up(st.at<void>(1), q_tokens, (size_t)nq * 4);
    if (mask_bytes) st.up(st.at<void>(4), masks, mask_bytes);
    if (mask_of) st.up(st.at<void>(5), mask_of, bytes[5]);
    if (st.code() != RQ_OK) return st.code();
    const int rc = rq_sparse_topk_grouped_device(h, st.at<int64_t>(0), st.at<int32_t>(1), B, nq, k, mask_bytes ? st.at<uint32_t>(4) : nullptr, mask_of ? n_masks : 0,
                                                 mask_of ? st.at<int32_t>(5) : nullptr, st.at<int32_t>(2), st.at<double>(3), st.at<int32_t>(6), (void*)h->own);
    st.launched();
    if (rc != RQ_OK) return rc;
    st.down(out_rows, st.at<void>(2), bytes[2]);
    st.down(out_scores, st.at<void>(3), bytes[3]);
    st.down(out_count, st.at<void>(6), bytes[6]);
    return st.finish();
}

extern "C" int rq_sparse_set_option(rq_sparse* h, const char* name, double value) {
    if (!h || !name) return set_err(RQ_EINVAL, "null argument");
    if (!strcmp(name, "tile_docs")) {
        if (!sparse_tile_ok(value)) return set_err(RQ_EINVAL, "tile_docs %g is not a power of two in %d..%d", value, RQ_SPARSE_TILE_MIN, RQ_SPARSE_TILE_MAX);
        h->tile_docs = (int)value;
        return RQ_OK;
    }
    if (!strcmp(name, "cand_cap")) {
        if (!(value >= 0) || value > 9e18) return set_err(RQ_EINVAL, "cand_cap %g", value);
        h->cand_cap = (int64_t)value;
        return RQ_OK;
    }
    if (!strcmp(name, "profile")) {
        h->profile = value != 0;
        return RQ_OK;
    }
    return set_err(RQ_EINVAL, "unknown or read-only sparse option '%s'", name);
}

extern "C" double rq_sparse_get_option(const rq_sparse* h, const char* name) {
    if (!h || !name) { set_err(RQ_EINVAL, "null argument"); return -1.0; }
    if (!strcmp(name, "tile_docs")) return (double)h->tile_docs;
    if (!strcmp(name, "cand_cap")) return (double)h->cand_cap;
    if (!strcmp(name, "calls")) return (double)h->calls;
    if (!strcmp(name, "masked_calls")) return (double)h->masked_calls;
    if (!strcmp(name, "grouped_calls")) return (double)h->grouped_calls;
    if (!strcmp(name, "grouped")) return h->d_groups ? 1.0 : 0.0;
    if (!strcmp(name, "score_calls")) return (double)h->score_calls;
    if (!strcmp(name, "rounds_last")) return (double)h->rounds_last;
    if (!strcmp(name, "tiles_last")) return (double)h->tiles_last;
    const bool masked_tiles = !strcmp(name, "masked_tiles_last"), final_chunks = !strcmp(name, "final_chunks_last");
    if (masked_tiles || final_chunks || !strcmp(name, "skipped_tiles_last")) {   // waits for the device
        DeviceGuard dg_(h->device);
        unsigned long long v = 0;
        if (!dg_.ok || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, h->d_skipped + (final_chunks ? 2 : masked_tiles ? 1 : 0), sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) {
            set_err(RQ_EHIP, "cannot read the %s counter", final_chunks ? "final-chunk" : masked_tiles ? "masked-tile" : "skipped-tile");
            return -1.0;
        }
        return (double)v;
    }
    if (!strcmp(name, "profile")) return (double)h->profile;
    const bool tile_ms = !strcmp(name, "tile_ms_last");
    if (tile_ms || !strcmp(name, "final_ms_last")) {   // waits for the device; -1: the last call was not profiled
        DeviceGuard dg_(h->device);
        if (h->ev_used < 3 || !dg_.ok || hipDeviceSynchronize() != hipSuccess) { set_err(RQ_EINVAL, "the last call recorded no events (option \"profile\")"); return -1.0; }
        double ms = 0.0;
        for (size_t i = tile_ms ? 1 : 2; i < h->ev_used; i += 2) {
            float one = 0.f;
            if (hipEventElapsedTime(&one, h->ev[i - 1], h->ev[i]) != hipSuccess) { set_err(RQ_EHIP, "hipEventElapsedTime failed"); return -1.0; }
            ms += one;
        }
        return ms;
    }
    set_err(RQ_EINVAL, "unknown sparse option '%s'", name);
    return -1.0;
}
