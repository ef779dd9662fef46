"""The yardstick of the sparse (BM25) top-k routes, in pure numpy, with no import of the code under test: the definition of
include/rq_bm25.h rq_bm25_topk and include/rq.h rq_sparse_topk, and the posting indexes and query batches that the CPU tier
(tests/test_sparse.py: this oracle against librq_bm25.so, bit for bit) and the GPU tier (tests/test_gpu_sparse.py: the device route
against this oracle, bit for bit) share.

    score(q, d) = the float64 sum of contrib[p] over the query's tokens, with repetition, added in query order from 0.0
                  (the accumulation loop of BM25Index.search_batch_rows's numpy branch: scores[rows[lo:hi]] += contrib[lo:hi])
    selection   = score > 0 only, a stable sort by (-score, -row), the first k; rows padded with -1, scores with 0.0
"""
import numpy as np

DEFAULT_TILE = 4096      # include/rq.h "tile_docs"
MAX_TILE = 8192


def topk(ix, q_indptr, q_tokens, k):
    """ix: dict(indptr, rows, contrib, n_tokens, n_docs).  A token id outside [0, n_tokens) is an empty posting list (the device form's
    rule; the host forms refuse such a query before they score anything)."""
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
            pos = np.flatnonzero(scores > 0)
            sel = pos[np.lexsort((-pos, -scores[pos]))[:k]]
            out_rows[b, :len(sel)] = sel
            out_scores[b, :len(sel)] = scores[sel]
    return out_rows, out_scores


def same(got, want):
    """Rows identical and every score identical in its bits."""
    return (got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
            and np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)))


# ---- posting indexes -----------------------------------------------------------------------------------------------------------------
def csr(lists, n_docs):
    """lists[t] = (rows ascending, contributions) of token t."""
    indptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(r) for r, _ in lists], out=indptr[1:])
    rows = np.concatenate([np.asarray(r, np.int32) for r, _ in lists] + [np.zeros(0, np.int32)]).astype(np.int32)
    contrib = np.concatenate([np.asarray(c, np.float64) for _, c in lists] + [np.zeros(0)]).astype(np.float64)
    return {"indptr": indptr, "rows": rows, "contrib": contrib, "n_tokens": len(lists), "n_docs": int(n_docs)}


def random_lists(rng, n_docs, n_tokens):
    """Skewed document frequencies, as a vocabulary has them: token t is in about n_docs / (t + 1) documents; contributions of BM25's size."""
    out = []
    for t in range(n_tokens):
        df = max(1, min(n_docs, int(n_docs / (t + 1) * rng.uniform(0.5, 1.0))))
        r = np.sort(rng.choice(n_docs, df, replace=False))
        out.append((r, rng.uniform(0.05, 4.0, df)))
    return out


def queries(rng, n_tokens, B, lo=1, hi=8):
    lens = rng.integers(lo, hi + 1, B)
    q_indptr = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=q_indptr[1:])
    return q_indptr, rng.integers(0, n_tokens, int(q_indptr[-1])).astype(np.int32)


def ragged(lists_of_tokens):
    q_indptr = np.zeros(len(lists_of_tokens) + 1, np.int64)
    np.cumsum([len(q) for q in lists_of_tokens], out=q_indptr[1:])
    flat = [t for q in lists_of_tokens for t in q]
    return q_indptr, np.asarray(flat, np.int32).reshape(-1)


def case(name, ix, q, k, **opts):
    """opts: tile_docs (None = the default), cand_cap, and what the GPU tier also asserts: min_skipped, rounds."""
    return {"name": name, "ix": ix, "q_indptr": q[0], "q_tokens": q[1], "k": k, "tile_docs": opts.pop("tile_docs", None), **opts}


def edge_lists(rng, n_docs, tile):
    """A random index plus: a token in every document; a token in one document of the last tile (the last row); a token with postings
    exactly on a tile's first and last row; a token with no posting; a token that only touches one tile in the middle."""
    lists = random_lists(rng, n_docs, 8)
    lists.append((np.arange(n_docs), rng.uniform(0.1, 1.0, n_docs)))                       # 8: every document
    lists.append((np.array([n_docs - 1]), np.array([2.0])))                                # 9: the last row
    edge = sorted({r for r in (0, tile - 1, tile, 2 * tile - 1, 2 * tile, n_docs - 1) if 0 <= r < n_docs})
    lists.append((np.array(edge), rng.uniform(1.0, 2.0, len(edge))))                       # 10: tile_lo and tile_hi - 1
    lists.append((np.zeros(0, np.int32), np.zeros(0)))                                     # 11: empty list
    mid = np.arange(min(tile, n_docs - 1), min(tile + 7, n_docs))
    lists.append((mid, rng.uniform(1.0, 2.0, len(mid))))                                   # 12: one tile only
    return lists


def edge_queries(rng):
    q = [[8], [9], [10], [12], [9, 10], [8, 10, 9, 8], [11], [], [11, 11]] + [list(rng.integers(0, 13, n)) for n in (2, 5, 9)]
    return ragged(q)


def batch_index():
    rng = np.random.default_rng(11)
    return csr(random_lists(rng, 2000, 40), 2000)


def cases():
    rng = np.random.default_rng(5)
    out = []
    # ---- tiling ----
    for n_docs in (1, 63, 64, 65, 200):
        out.append(case(f"tile64_n{n_docs}", csr(edge_lists(rng, n_docs, 64), n_docs), edge_queries(rng), 10, tile_docs=64, min_skipped=1 if n_docs > 128 else 0))
    for n_docs in (8193, 20000):
        out.append(case(f"tile_default_n{n_docs}", csr(edge_lists(rng, n_docs, DEFAULT_TILE), n_docs), edge_queries(rng), 100, min_skipped=1))
        out.append(case(f"tile_max_n{n_docs}", csr(edge_lists(rng, n_docs, MAX_TILE), n_docs), edge_queries(rng), 100, tile_docs=MAX_TILE, min_skipped=1))
    # ---- order of additions ----
    d = 70
    order = csr([([d], [1e16]), ([d], [1.0]), ([d], [-1e16]), ([d], [3.0]), ([3, d], [0.7, 0.1])], 100)
    out.append(case("order_of_additions", order, ragged([[0, 1, 2, 3], [0, 2, 1, 3], [1, 3, 0, 2], [3, 1, 0, 2], [1, 0, 2, 3], [4, 4, 4], [4] * 6, [4] * 10]), 5, tile_docs=64))
    long_ix = csr(random_lists(rng, 300, 20), 300)
    out.append(case("query_of_300_tokens", long_ix, ragged([list(rng.integers(0, 20, 300)), list(rng.integers(0, 20, 257)), list(rng.integers(0, 20, 256)), [3]]), 50, tile_docs=64))
    # ---- selection ----
    inf, nan = np.inf, np.nan
    sel = csr([([0, 1, 2, 3, 4, 9], [2.5, 1.0, nan, inf, inf, 1.5]), ([0, 1, 2, 4, 8], [-2.5, -3.0, 1.0, -inf, 0.5]), ([5, 130], [0.25, 0.25])], 140)
    out.append(case("cancel_negative_nan_inf", sel, ragged([[0, 1], [1, 0], [0], [1], [0, 1, 2], [2, 2]]), 10, tile_docs=64))
    tied_rows = np.sort(rng.choice(700, 500, replace=False))
    better = np.sort(rng.choice(700, 30, replace=False))
    ties = csr([(tied_rows, np.full(500, 1.25)), (better, rng.uniform(0.5, 1.0, 30))], 700)
    for k in (100, 37, 499, 500):
        out.append(case(f"tie_run_k{k}", ties, ragged([[0], [0, 1], [1, 0]]), k, tile_docs=64))
    full = csr([(np.arange(64), rng.uniform(0.1, 1.0, 64)), (np.arange(64), np.full(64, 0.5))], 64)
    out.append(case("one_full_tile_k10", full, ragged([[0], [1], [0, 1]]), 10, tile_docs=64))
    many = csr(edge_lists(rng, 3000, 64), 3000)
    for k in (1, 100, 1024):
        out.append(case(f"k{k}_tile64", many, edge_queries(rng), k, tile_docs=64))
    out.append(case("k1024_default_tile", csr(edge_lists(rng, 20000, DEFAULT_TILE), 20000), ragged([[8], [9], [0, 1, 8], [11], []]), 1024))
    out.append(case("k1024_max_tile", csr(edge_lists(rng, 20000, MAX_TILE), 20000), ragged([[8], [9], [0, 1, 8], [11], []]), 1024, tile_docs=MAX_TILE))
    # ---- batches and rounds ----
    bix = batch_index()
    for B in (1, 3, 70, 500):
        out.append(case(f"batch{B}", bix, queries(np.random.default_rng(B), 40, B), 20, tile_docs=256))
    # 8 tiles x min(20, 256) x 12 bytes = 1 920 bytes per query: a cap of 30 queries cuts 70 into 30 + 30 + 10
    out.append(case("batch70_three_rounds", bix, queries(np.random.default_rng(70), 40, 70), 20, tile_docs=256, cand_cap=30 * 1920, rounds=3))
    return out
