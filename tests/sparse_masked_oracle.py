"""The yardstick of the MASKED sparse top-k routes (include/rq_bm25.h rq_bm25_topk_masked, include/rq.h rq_sparse_topk_masked), in pure
numpy on top of tests/sparse_oracle.py, with no import of the code under test.  It is that file's `topk` with

    scores = np.where(keep, scores, 0.0)

before the selection -- the line of BM25Index.search(..., allowed_ids=) -- and it also gives the two tile counters a masked device call
reports and the mask cases both tiers share (tests/test_sparse_masked.py on the CPU, tests/test_gpu_sparse_masked.py on the GPU).

    masks    [n_masks][W] uint32, W = ceil(n_docs / 32): bit r % 32 of word r / 32 set = document row r is allowed; bits at or beyond
             n_docs are ignored
    mask_of  [B] int32: the mask of query q, -1 = unrestricted; any other value outside [0, n_masks) allows nothing (the device form's
             rule; the blocking forms refuse it)
"""
import numpy as np

import sparse_oracle as so


def words(n_docs):
    return (int(n_docs) + 31) // 32


def pack(keep, dirty=False):
    """A boolean array [n_docs] as mask words.  dirty: the bits of the last word at or beyond n_docs are all set -- they must be ignored."""
    keep = np.asarray(keep, bool)
    n = len(keep)
    bits = np.zeros(words(n) * 32, bool)
    bits[:n] = keep
    if dirty:
        bits[n:] = True
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def table(keeps, dirty=False):
    """[n_masks][W] from a list of boolean arrays (an empty list: a table of no masks)."""
    keeps = list(keeps)
    n = len(keeps[0]) if keeps else 0
    return np.stack([pack(k, dirty) for k in keeps]) if keeps else np.zeros((0, words(n)), np.uint32)


def unpack(mask_words, n_docs):
    return np.unpackbits(np.ascontiguousarray(mask_words, "<u4").view(np.uint8), bitorder="little")[:n_docs].astype(bool)


def keep_of(masks, mask_of, q, n_docs):
    """The allowed documents of query q: None = unrestricted."""
    m = int(mask_of[q])
    if m == -1:
        return None
    if m < 0 or masks is None or m >= len(masks):
        return np.zeros(n_docs, bool)
    return unpack(masks[m], n_docs)


def topk(ix, q_indptr, q_tokens, k, masks, mask_of):
    """sparse_oracle.topk with every document outside the query's allowed set at 0.0 before the score > 0 selection."""
    indptr, rows, contrib, n_docs = ix["indptr"], ix["rows"], ix["contrib"], ix["n_docs"]
    B = len(q_indptr) - 1
    out_rows, out_scores = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            scores = np.zeros(n_docs, np.float64)
            for j in q_tokens[q_indptr[b]: q_indptr[b + 1]]:
                if 0 <= j < ix["n_tokens"]:
                    lo, hi = indptr[j], indptr[j + 1]
                    scores[rows[lo:hi]] += contrib[lo:hi]
            keep = keep_of(masks, mask_of, b, n_docs)
            if keep is not None:
                scores = np.where(keep, scores, 0.0)
            pos = np.flatnonzero(scores > 0)
            sel = pos[np.lexsort((-pos, -scores[pos]))[:k]]
            out_rows[b, :len(sel)] = sel
            out_scores[b, :len(sel)] = scores[sel]
    return out_rows, out_scores


def tile_counters(ix, q_indptr, q_tokens, tile, masks, mask_of):
    """(masked_tiles_last, skipped_tiles_last) of one masked device call, exact: a (query, tile) pair whose mask allows no document of
    the tile is MASKED and is looked at no further; of the others, a pair in which no token of the query has a posting is SKIPPED."""
    indptr, rows, n_docs = ix["indptr"], ix["rows"], ix["n_docs"]
    tiles = -(-n_docs // tile)
    masked = skipped = 0
    for b in range(len(q_indptr) - 1):
        touched = np.zeros(tiles, bool)
        for j in q_tokens[q_indptr[b]: q_indptr[b + 1]]:
            if 0 <= j < ix["n_tokens"]:
                touched[rows[indptr[j]: indptr[j + 1]] // tile] = True
        keep = keep_of(masks, mask_of, b, n_docs)
        allowed = np.ones(tiles, bool) if keep is None else np.array([keep[t * tile: (t + 1) * tile].any() for t in range(tiles)], bool)
        masked += int((~allowed).sum())
        skipped += int((allowed & ~touched).sum())
    return masked, skipped


def mask_cases(n_docs, seed=0):
    """The four masks every index of sparse_oracle.cases() is crossed with: name -> boolean array [n_docs]."""
    rng = np.random.default_rng(1000 + seed)
    one = np.zeros(n_docs, bool)
    one[int(rng.integers(0, n_docs))] = True
    return {"all_ones": np.ones(n_docs, bool), "empty": np.zeros(n_docs, bool), "random_half": rng.random(n_docs) < 0.5, "one_row": one}


same = so.same
