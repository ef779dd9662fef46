"""The yardstick of hybrid fusion on the device (include/rq.h rq_hybrid_*, rq_sparse_score_rows*), in pure numpy, with no import of
the code under test: the definition of include/rq.h "hybrid fusion" -- the arithmetic of HybridRetriever._fuse_batch_rows made
explicit -- and the key spaces and pools that the CPU tier (tests/test_hybrid.py: this oracle against _fuse_batch_rows itself, value
for value) and the GPU tier (tests/test_gpu_hybrid.py: the device route against this oracle, bit for bit) share.

    key space   keys 0 .. nb-1 are the sparse rows, dense row j has key dense_key[j] (injective), known[key] per key,
                dense_row[key] the inverse map (-1: none)
    candidates  positions 0 .. K1+K2-1, sparse pool first; b, d float64, the missing side 0.0; a row outside its index is absent
    valid       present and known[key]; a key in both pools: the sparse position takes the dense position's d, the dense one goes
    missing     valid sparse position without a dense score -> dense_row[key]; valid dense-only position with key < nb -> key; else -1
    extras      where a miss entry is >= 0 (and the position is a valid candidate that lacks that score) the extra replaces the 0.0
    maxima      numpy's max over the valid candidates (a NaN makes it NaN); 0, NaN and infinite become 1.0
    h           (b / max_b + d / max_d) / 2 in float64
    order       h descending, -0.0 as +0.0, a NaN h as -inf; equal h by ascending position; the first top_k of the valid candidates
    output      key, b, d, h (as computed: a NaN stays a NaN), position; count = min(valid, top_k); padding (-1, 0.0, 0.0, 0.0, -1)
The host path differs in one place only: np.argsort puts a NaN sort key behind the dropped entries.
"""
import numpy as np

MAX_CAND = 2048


def key_space(nb, dense_key, known):
    dense_key = np.asarray(dense_key, np.int64).reshape(-1)
    known = np.asarray(known).astype(bool).reshape(-1)
    assert nb <= len(known) and len(np.unique(dense_key)) == len(dense_key) and (len(dense_key) == 0 or (dense_key.min() >= 0 and dense_key.max() < len(known)))
    dense_row = np.full(len(known), -1, np.int64)
    dense_row[dense_key] = np.arange(len(dense_key), dtype=np.int64)
    return {"nb": int(nb), "n_dense": len(dense_key), "n_keys": len(known), "dense_key": dense_key, "known": known, "dense_row": dense_row}


def _candidates(ks, sp_rows, de_rows):
    """keys [B][K1 + K2] (-1: absent), valid, and per row the (first, second) positions of the documents in both pools"""
    sp_rows, de_rows = np.asarray(sp_rows, np.int64), np.asarray(de_rows, np.int64)
    B, K1, K2 = sp_rows.shape[0], sp_rows.shape[1], de_rows.shape[1]
    sp_in = (sp_rows >= 0) & (sp_rows < ks["nb"])
    de_in = (de_rows >= 0) & (de_rows < ks["n_dense"])
    sp_keys = np.where(sp_in, sp_rows, -1)
    de_keys = np.where(de_in, ks["dense_key"][np.where(de_in, de_rows, 0)], -1) if ks["n_dense"] else np.full((B, K2), -1, np.int64)
    keys = np.concatenate([sp_keys, de_keys], axis=1)
    valid = keys >= 0
    valid &= ks["known"][np.where(valid, keys, 0)] if ks["n_keys"] else False
    order = np.argsort(keys, axis=1, kind="stable")
    sk = np.take_along_axis(keys, order, 1)
    r, j = np.nonzero((sk[:, 1:] == sk[:, :-1]) & (sk[:, 1:] >= 0))
    first, second = order[r, j], order[r, j + 1]
    valid[r, second] = False
    have_dense = np.zeros(keys.shape, bool)
    have_dense[:, K1:] = True
    have_dense[r, first] = True
    return keys, valid, have_dense, (r, first, second)


def missing(ks, sp_rows, de_rows):
    """(miss_dense int64 [B][K1], miss_sparse int32 [B][K2])"""
    keys, valid, have_dense, _ = _candidates(ks, sp_rows, de_rows)
    K1 = np.asarray(sp_rows).shape[1]
    need = valid[:, :K1] & ~have_dense[:, :K1]
    miss_dense = np.where(need, ks["dense_row"][np.where(need, keys[:, :K1], 0)], -1).astype(np.int64) if ks["n_keys"] else np.full(need.shape, -1, np.int64)
    miss_sparse = np.where(valid[:, K1:] & (keys[:, K1:] < ks["nb"]), keys[:, K1:], -1).astype(np.int32)
    return miss_dense, miss_sparse


def fuse(ks, sp_rows, sp_scores, de_rows, de_scores, top_k, miss_dense=None, extra_dense=None, miss_sparse=None, extra_sparse=None):
    """(keys int32, b, d, h float64, positions int32 -- all [B][top_k] -- and count int32 [B])"""
    assert (extra_dense is None or miss_dense is not None) and (extra_sparse is None or miss_sparse is not None)
    keys, valid, have_dense, (r, first, second) = _candidates(ks, sp_rows, de_rows)
    B, K1, K2 = keys.shape[0], np.asarray(sp_rows).shape[1], np.asarray(de_rows).shape[1]
    N = K1 + K2
    assert 1 <= N <= MAX_CAND and top_k >= 1
    bsc = np.concatenate([np.asarray(sp_scores, np.float64).reshape(B, K1), np.zeros((B, K2))], axis=1)
    dsc = np.concatenate([np.zeros((B, K1)), np.asarray(de_scores, np.float32).reshape(B, K2).astype(np.float64)], axis=1)
    bsc[keys < 0] = 0.0
    dsc[keys < 0] = 0.0
    dsc[r, first] = dsc[r, second]
    if extra_dense is not None and K1:
        take = (np.asarray(miss_dense) >= 0) & valid[:, :K1] & ~have_dense[:, :K1]
        dsc[:, :K1] = np.where(take, np.asarray(extra_dense, np.float32).astype(np.float64), dsc[:, :K1])
    if extra_sparse is not None and K2:
        take = (np.asarray(miss_sparse) >= 0) & valid[:, K1:]
        bsc[:, K1:] = np.where(take, np.asarray(extra_sparse, np.float64), bsc[:, K1:])
    out_keys, out_pos = np.full((B, top_k), -1, np.int32), np.full((B, top_k), -1, np.int32)
    out_b, out_d, out_h = np.zeros((B, top_k)), np.zeros((B, top_k)), np.zeros((B, top_k))
    count = np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        neg_inf = -np.inf
        max_b = np.where(valid, bsc, neg_inf).max(axis=1, initial=neg_inf)
        max_d = np.where(valid, dsc, neg_inf).max(axis=1, initial=neg_inf)
        max_b = np.where((max_b == 0) | ~np.isfinite(max_b), 1.0, max_b)
        max_d = np.where((max_d == 0) | ~np.isfinite(max_d), 1.0, max_d)
        h = (bsc / max_b[:, None] + dsc / max_d[:, None]) / 2
        rank = np.where(np.isnan(h), neg_inf, np.where(h == 0, 0.0, h))
        for q in range(B):
            pos = np.flatnonzero(valid[q])
            sel = pos[np.lexsort((pos, -rank[q, pos]))][:top_k]
            n = len(sel)
            count[q] = n
            out_keys[q, :n], out_pos[q, :n] = keys[q, sel], sel
            out_b[q, :n], out_d[q, :n], out_h[q, :n] = bsc[q, sel], dsc[q, sel], h[q, sel]
    return out_keys, out_b, out_d, out_h, out_pos, count


def same(got, want):
    """Every array identical; the float64 ones identical in their bits."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype != w.dtype or g.shape != w.shape:
            return False
        if not (np.array_equal(g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else np.array_equal(g, w)):
            return False
    return True


def sparse_score_rows(ix, q_indptr, q_tokens, rows):
    """rows int [B][m] -> float64 [B][m]: the entries of the full score vector of tests/sparse_oracle.py's definition (contributions added
    in query order from 0.0, with repetition; a token id outside the index is an empty list); a row outside [0, n_docs) scores 0.0."""
    rows = np.asarray(rows, np.int64)
    B, n_docs = rows.shape[0], ix["n_docs"]
    out = np.zeros(rows.shape, np.float64)
    inside = (rows >= 0) & (rows < n_docs)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            if n_docs == 0 or not inside[b].any():
                continue
            scores = np.zeros(n_docs, np.float64)
            for j in q_tokens[q_indptr[b]: q_indptr[b + 1]]:
                if 0 <= j < ix["n_tokens"]:
                    lo, hi = ix["indptr"][j], ix["indptr"][j + 1]
                    scores[ix["rows"][lo:hi]] += ix["contrib"][lo:hi]
            out[b] = np.where(inside[b], scores[np.clip(rows[b], 0, n_docs - 1)], 0.0)
    return out


# ---- key spaces and pools ------------------------------------------------------------------------------------------------------------
def random_space(rng, nb, n_dense, shared, unknown=0.15):
    """`shared` dense rows hold a document BM25 holds too (a random sparse row each); the others get nb + j.  About `unknown` of the keys
    are not known to the document store."""
    dense_key = nb + np.arange(n_dense, dtype=np.int64)
    shared = min(shared, nb, n_dense)
    if shared:
        dense_key[rng.choice(n_dense, shared, replace=False)] = rng.choice(nb, shared, replace=False)
    return key_space(nb, dense_key, rng.random(nb + n_dense) >= unknown)


def random_pools(rng, ks, B, K1, K2, fill=0.9, overlap=0.3, stray=0.05, negative=False):
    """Pools in the layout of rq_sparse_topk_device and rq_search_device: distinct rows, scores best first, -1 / 0.0 padded.  About
    `overlap` of a dense pool are the dense rows of documents of the sparse pool (where they exist); about `stray` of the dense rows lie
    outside [0, n_dense) and of the sparse rows outside [0, nb)."""
    sp_rows, sp_scores = np.full((B, K1), -1, np.int32), np.zeros((B, K1), np.float64)
    de_rows, de_scores = np.full((B, K2), -1, np.int64), np.zeros((B, K2), np.float32)
    nb, nd = ks["nb"], ks["n_dense"]
    for q in range(B):
        c1 = min(nb, K1 if rng.random() < 0.5 else int(rng.integers(0, K1 + 1) * fill)) if K1 else 0
        rows = rng.choice(nb, c1, replace=False) if c1 else np.zeros(0, np.int64)
        sp_rows[q, :c1] = rows
        sp_scores[q, :c1] = np.sort(rng.uniform(0.05, 30.0, c1))[::-1]
        if c1 and stray:
            hit = rng.random(c1) < stray
            sp_rows[q, :c1][hit] = nb + rng.integers(0, 5, int(hit.sum()))
        c2 = min(nd, K2 if rng.random() < 0.5 else int(rng.integers(0, K2 + 1) * fill)) if K2 else 0
        if c2:
            twins = ks["dense_row"][rows] if c1 else np.zeros(0, np.int64)
            twins = twins[twins >= 0]
            twins = twins[rng.random(len(twins)) < overlap][:c2]
            rest = np.setdiff1d(rng.choice(nd, min(nd, c2 + len(twins)), replace=False), twins)[: c2 - len(twins)]
            drows = rng.permutation(np.concatenate([twins, rest]))
            c2 = len(drows)
            de_rows[q, :c2] = drows
            sc = np.sort(rng.uniform(-1.0, 1.0, c2).astype(np.float32))[::-1]
            de_scores[q, :c2] = -np.abs(sc) - np.float32(0.01) if negative else sc
            if stray:
                hit = rng.random(c2) < stray
                de_rows[q, :c2][hit] = np.where(rng.random(int(hit.sum())) < 0.5, nd + rng.integers(0, 5, int(hit.sum())), -7)
    return sp_rows, sp_scores, de_rows, de_scores


def case(name, ks, pools, top_ks, native_only=False):
    return {"name": name, "ks": ks, "pools": pools, "top_ks": tuple(top_ks), "native_only": native_only}


def extras_for(c):
    """The miss lists of a case and extra scores for EVERY position (where a miss entry is -1 the extra must be ignored)."""
    rng = np.random.default_rng(len(c["name"]) + 1000)
    sp_rows, _, de_rows, _ = c["pools"]
    miss_dense, miss_sparse = missing(c["ks"], sp_rows, de_rows)
    extra_dense = rng.uniform(-1.0, 1.0, miss_dense.shape).astype(np.float32)
    extra_sparse = rng.uniform(0.0, 25.0, miss_sparse.shape)
    if c["name"].startswith("negative"):
        extra_dense = -np.abs(extra_dense) - np.float32(0.01)
    return {"miss_dense": miss_dense, "extra_dense": extra_dense, "miss_sparse": miss_sparse, "extra_sparse": extra_sparse}


def cases():
    rng = np.random.default_rng(17)
    out = []
    ks = random_space(rng, 3000, 2500, 1500)
    # ---- candidate counts around the instantiations (64, 128, 256, 512, 1 024, 2 048) and the batch sizes ----
    for K1, K2, B in ((1, 0, 3), (0, 1, 3), (1, 1, 3), (31, 32, 3), (32, 32, 1), (33, 32, 3), (128, 127, 3), (128, 128, 3), (129, 128, 3), (500, 500, 3),
                      (1024, 1024, 3), (100, 100, 70), (40, 0, 3), (0, 40, 3)):
        out.append(case(f"n{K1 + K2}_{K1}x{K2}_b{B}", ks, random_pools(rng, ks, B, K1, K2), (1, 10, 1024)))
    full = (np.stack([rng.permutation(3000)[:20] for _ in range(3)]).astype(np.int32), np.sort(rng.uniform(0.05, 30.0, (3, 20)))[:, ::-1].copy(),
            np.stack([rng.permutation(2500)[:20] for _ in range(3)]).astype(np.int64), np.sort(rng.uniform(-1, 1, (3, 20)).astype(np.float32))[:, ::-1].copy())
    # ---- top_k at the valid count and one above it: three queries with the same 12 valid candidates (4 of 8 + 8 are in both pools) ----
    kn = key_space(10, np.array([0, 1, 2, 3, 10, 11, 12, 13], np.int64), np.ones(14, bool))
    sp = np.tile(np.arange(8, dtype=np.int32), (3, 1))
    de = np.tile(np.arange(8, dtype=np.int64), (3, 1))
    out.append(case("count12_topk_at_and_above", kn, (sp, np.sort(rng.uniform(1, 9, (3, 8)))[:, ::-1].copy(), de, np.sort(rng.uniform(0, 1, (3, 8)).astype(np.float32))[:, ::-1].copy()),
                    (1, 11, 12, 13, 1024)))
    # ---- all padding ----
    pad = random_pools(rng, ks, 3, 16, 16)
    out.append(case("sparse_pool_all_padding", ks, (np.full_like(pad[0], -1), np.zeros_like(pad[1]), pad[2], pad[3]), (1, 10)))
    out.append(case("dense_pool_all_padding", ks, (pad[0], pad[1], np.full_like(pad[2], -1), np.zeros_like(pad[3])), (1, 10)))
    out.append(case("both_pools_all_padding", ks, (np.full_like(pad[0], -1), np.zeros_like(pad[1]), np.full_like(pad[2], -1), np.zeros_like(pad[3])), (1, 10)))
    # ---- a document in both pools at the first and at the last position of each ----
    kb = key_space(50, np.concatenate([np.arange(40, dtype=np.int64), 50 + np.arange(10, dtype=np.int64)]), np.ones(100, bool))
    sp = np.array([np.arange(10), np.arange(10)], np.int32)
    sps = np.array([np.linspace(9, 1, 10), np.linspace(9, 1, 10)])
    de = np.array([[0, 41, 42, 43, 44, 45, 46, 47, 48, 9], [9, 41, 42, 43, 44, 45, 46, 47, 48, 0]], np.int64)
    des = np.array([np.linspace(0.9, 0.1, 10), np.linspace(0.9, 0.1, 10)], np.float32)
    out.append(case("both_pools_first_and_last", kb, (sp, sps, de, des), (1, 5, 18, 19, 20)))
    # ---- a run of exactly tied h across the sparse / dense boundary, cut by top_k: b = max_b alone and d = max_d alone are both 0.5 ----
    sp = np.array([[0, 1, 2, 3, 4, 5]], np.int32)
    sps = np.array([[4.0, 4.0, 4.0, 4.0, 2.0, 1.0]])
    de = np.array([[40, 41, 42, 43, 44, 45]], np.int64)
    des = np.array([[0.5, 0.5, 0.5, 0.5, 0.25, 0.125]], np.float32)
    out.append(case("tie_run_over_the_boundary", kb, (sp, sps, de, des), (1, 3, 4, 5, 6, 7, 8, 9, 12)))
    # ---- signs, zeros and non-finite values ----
    out.append(case("negative_dense_scores", ks, random_pools(rng, ks, 3, 40, 40, negative=True), (1, 10, 80)))
    z = random_pools(rng, ks, 3, 30, 30)
    out.append(case("zero_dense_scores", ks, (z[0], z[1], z[2], np.zeros_like(z[3])), (1, 10, 60)))
    out.append(case("zero_and_negative_zero", ks, (z[0], np.zeros_like(z[1]), z[2], np.where(np.arange(30)[None, :] % 2 == 0, np.float32(-0.0), np.float32(0.0)) * np.ones_like(z[3])), (10, 60)))
    i = random_pools(rng, ks, 3, 30, 30, stray=0.0, overlap=0.0)
    sps = i[1].copy()
    sps[:, 0] = np.inf
    out.append(case("inf_sparse_score", ks, (i[0], sps, i[2], i[3]), (1, 10, 60)))
    des = i[3].copy()
    des[:, -5:] = -np.inf
    out.append(case("minus_inf_dense_scores", ks, (i[0], i[1], i[2], des), (1, 10, 60)))
    out.append(case("all_dense_minus_inf", ks, (i[0], i[1], i[2], np.full_like(i[3], -np.inf)), (1, 10, 60)))
    # a NaN h: +inf from the sparse pool and -inf from the dense pool on the same document (max_b becomes 1.0, max_d is 0.5: inf - inf)
    sp = np.array([[0, 1, 2, 3]], np.int32)
    sps = np.array([[np.inf, 3.0, 2.0, 1.0]])
    de = np.array([[41, 42, 0, 43]], np.int64)
    des = np.array([[0.5, 0.25, -np.inf, -np.inf]], np.float32)
    out.append(case("nan_hybrid_score", kb, (sp, sps, de, des), (1, 3, 6, 7, 8), native_only=True))
    # ---- the key space: nothing known, no dense index, every dense row beyond the sparse index ----
    ku = key_space(3000, ks["dense_key"], np.zeros(ks["n_keys"], bool))
    out.append(case("no_key_known", ku, random_pools(rng, ku, 3, 20, 20), (1, 10)))
    k0 = key_space(3000, np.zeros(0, np.int64), rng.random(3000) >= 0.15)
    p0 = random_pools(rng, k0, 3, 20, 20)
    out.append(case("n_dense_0", k0, (p0[0], p0[1], np.tile(np.arange(20, dtype=np.int64), (3, 1)), np.ones((3, 20), np.float32)), (1, 10, 40)))
    kd = random_space(rng, 100, 2000, 0, unknown=0.3)
    out.append(case("dense_only_keys", kd, random_pools(rng, kd, 3, 50, 200), (1, 10, 250)))
    out.append(case("full_pools_no_padding", ks, full, (1, 40, 41)))
    return out
