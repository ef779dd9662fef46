// rq_hybrid_plan.h -- the host side of hybrid fusion (include/rq.h rq_hybrid_*, rq_sparse_score_rows*) that needs no device: the
// validation of the key space at create time and the inverse map it yields, the checks of a call's arguments, the instantiation of
// the fuse kernel chosen by the candidate count, its threads and its LDS bytes, and the grid of the row-scoring kernel.  Plain
// arithmetic in the manner of rq_sparse_plan.h: no HIP runtime call, nothing is written outside what the caller hands in
// (tests/native/hybrid_plan_check.cpp runs it on the host).
#pragma once
#include "rq_index.h"

#define RQ_HYBRID_MIN_PAD 64                      // the smallest instantiation: one wave
#define RQ_HYBRID_MAX_THREADS 256
#define RQ_HYBRID_SCORE_THREADS 256               // rq_sparse_score_rows_device: one thread per (query, row) pair

// What rq_hybrid_create refuses: sizes that do not nest (0 <= nb <= n_keys < 2^31, n_dense >= 0), a key outside [0, n_keys), and a
// dense_key that is not injective (two dense rows with one key: the duplicate detection of the fusion relies on at most one dense
// position per key).  On success dense_row [n_keys] holds the inverse map, -1 where no dense row has the key.
static inline int hybrid_check_create(int64_t nb, int64_t n_dense, const int64_t* dense_key, const uint8_t* known, int64_t n_keys, std::vector<int32_t>& dense_row) {
    if (nb < 0 || n_dense < 0 || n_keys < 0) return set_err(RQ_EINVAL, "negative nb, n_dense or n_keys");
    if (n_keys >= ((int64_t)1 << 31)) return set_err(RQ_EINVAL, "n_keys %lld is 2^31 or more", (long long)n_keys);
    if (nb > n_keys) return set_err(RQ_EINVAL, "nb %lld exceeds n_keys %lld", (long long)nb, (long long)n_keys);
    if (n_dense >= ((int64_t)1 << 31)) return set_err(RQ_EINVAL, "n_dense %lld is 2^31 or more", (long long)n_dense);
    if (n_dense > 0 && !dense_key) return set_err(RQ_EINVAL, "null dense_key with %lld dense rows", (long long)n_dense);
    if (n_keys > 0 && !known) return set_err(RQ_EINVAL, "null known with %lld keys", (long long)n_keys);
    dense_row.assign((size_t)n_keys, -1);
    for (int64_t j = 0; j < n_dense; ++j) {
        const int64_t key = dense_key[j];
        if (key < 0 || key >= n_keys) return set_err(RQ_EINVAL, "dense_key[%lld] = %lld outside 0..%lld", (long long)j, (long long)key, (long long)n_keys - 1);
        if (dense_row[(size_t)key] >= 0)
            return set_err(RQ_EINVAL, "dense_key is not injective: rows %d and %lld share key %lld", dense_row[(size_t)key], (long long)j, (long long)key);
        dense_row[(size_t)key] = (int32_t)j;
    }
    return RQ_OK;
}

// Both pool-taking calls (pointers are only tested for null; a pool of width 0 needs no arrays).
static inline int hybrid_check_pools(const void* h, const void* sp_rows, const void* de_rows, int B, int K1, int K2) {
    if (!h) return set_err(RQ_EINVAL, "null handle");
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (K1 < 0 || K1 > RQ_SPARSE_MAX_K) return set_err(RQ_EINVAL, "K1 %d outside 0..%d", K1, RQ_SPARSE_MAX_K);
    if (K2 < 0 || K2 > RQ_MAX_K) return set_err(RQ_EINVAL, "K2 %d outside 0..%d", K2, RQ_MAX_K);
    if (K1 + K2 < 1) return set_err(RQ_EINVAL, "K1 + K2 is 0: no candidates");
    if ((K1 > 0 && !sp_rows) || (K2 > 0 && !de_rows)) return set_err(RQ_EINVAL, "null pool rows");
    return RQ_OK;
}
static inline int hybrid_check_missing(const void* h, const void* sp_rows, const void* de_rows, int B, int K1, int K2, const void* miss_dense, const void* miss_sparse) {
    if (int rc = hybrid_check_pools(h, sp_rows, de_rows, B, K1, K2)) return rc;
    if ((K1 > 0 && !miss_dense) || (K2 > 0 && !miss_sparse)) return set_err(RQ_EINVAL, "null miss array");
    return RQ_OK;
}
static inline int hybrid_check_fuse(const void* h, const void* sp_rows, const void* sp_scores, const void* de_rows, const void* de_scores, int B, int K1, int K2,
                                    const void* miss_dense, const void* extra_dense, const void* miss_sparse, const void* extra_sparse, int top_k,
                                    const void* keys, const void* b, const void* d, const void* hy, const void* count) {
    if (int rc = hybrid_check_pools(h, sp_rows, de_rows, B, K1, K2)) return rc;
    if ((K1 > 0 && !sp_scores) || (K2 > 0 && !de_scores)) return set_err(RQ_EINVAL, "null pool scores");
    if (top_k < 1 || top_k > RQ_MAX_K) return set_err(RQ_EINVAL, "top_k %d outside 1..%d", top_k, RQ_MAX_K);
    if ((extra_dense && !miss_dense) || (extra_sparse && !miss_sparse)) return set_err(RQ_EINVAL, "an extra array without its miss array");
    if (!keys || !b || !d || !hy || !count) return set_err(RQ_EINVAL, "null output");
    return RQ_OK;
}

// rq_hybrid_set_groups: one int32 per key, -1 = a group of its own, any other value >= 0 (the conventions of rq_sparse_set_groups).
static inline int hybrid_check_groups(const void* h, const int32_t* key_group, int64_t n_keys, int64_t handle_keys) {
    if (!h) return set_err(RQ_EINVAL, "null handle");
    if (n_keys != handle_keys) return set_err(RQ_EINVAL, "n_keys %lld, the key space holds %lld keys", (long long)n_keys, (long long)handle_keys);
    if (n_keys > 0 && !key_group) return set_err(RQ_EINVAL, "null key_group");
    for (int64_t i = 0; i < n_keys; ++i)
        if (key_group[i] < -1) return set_err(RQ_EINVAL, "key_group[%lld] is %d: a group id is -1 or not negative", (long long)i, key_group[i]);
    return RQ_OK;
}

// The fuse kernel is instantiated for `pad` candidates, the count K1 + K2 rounded up to a power of two in 64 .. 2 048: the smallest
// pools run a one-wave workgroup over 64 slots and do not pay for the sorts and the LDS of 2 048.
static inline int hybrid_pad(int n_cand) {
    int p = RQ_HYBRID_MIN_PAD;
    while (p < n_cand) p <<= 1;
    return p;   // n_cand <= RQ_HYBRID_MAX_CAND by hybrid_check_pools
}
static inline int hybrid_threads(int pad) { return std::max(64, std::min(RQ_HYBRID_MAX_THREADS, pad / 2)); }
// LDS of one workgroup.  Both kernels: the sort array (8 B per slot) and one flag byte per slot.  The fuse kernel also: b and d
// (8 B each), the position that travels with the second sort (4 B), and 4 values per wave for the reduction.
static inline size_t hybrid_lds_bytes(int pad, bool fuse) {
    const size_t waves = (size_t)hybrid_threads(pad) / 64;
    return (size_t)pad * (fuse ? 8 + 1 + 16 + 4 : 8 + 1) + (fuse ? waves * 32 : 0);
}

// The grouped fuse kernel adds nothing: its third sort runs in the sort array, its keep flags in the flag bytes, both spent by then.
static inline size_t hybrid_grouped_lds_bytes(int pad) { return hybrid_lds_bytes(pad, true); }

// rq_sparse_score_rows*: 1 <= B <= 65535, 1 <= m <= RQ_MAX_SCORE_ROWS, non-null pointers; one thread per pair.
static inline int hybrid_check_score_rows(const void* h, const void* q_indptr, int B, const void* rows, int m, const void* scores) {
    if (!h || !q_indptr || !rows || !scores) return set_err(RQ_EINVAL, "null argument");
    if (B < 1 || B > 65535) return set_err(RQ_EINVAL, "B %d outside 1..65535", B);
    if (m < 1 || m > RQ_MAX_SCORE_ROWS) return set_err(RQ_EINVAL, "m %d outside 1..%d", m, RQ_MAX_SCORE_ROWS);
    return RQ_OK;
}
static inline unsigned hybrid_score_blocks(int B, int m) {   // <= 65535 x 65536 / 256 < 2^24
    return (unsigned)(((int64_t)B * m + RQ_HYBRID_SCORE_THREADS - 1) / RQ_HYBRID_SCORE_THREADS);
}
