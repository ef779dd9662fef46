"""Sparse search on the device (include/rq.h rq_sparse_*, csrc/rq_sparse.hip) against tests/sparse_oracle.py: rows identical and every
score identical in its bits, no tolerance, no case left out.  tests/test_sparse.py shows that the oracle and librq_bm25.so agree bit
for bit on the same cases, so the device route and the host library share one definition."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = so.cases()
_WANT = {}


def _want(case):
    """The oracle's answer, computed once per case."""
    if case["name"] not in _WANT:
        _WANT[case["name"]] = so.topk(case["ix"], case["q_indptr"], case["q_tokens"], case["k"])
    return _WANT[case["name"]]


def _index(ix, **options):
    sp = _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    for name, value in options.items():
        if value is not None:
            sp.set_option(name, value)
    return sp


def _by(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_route_equals_the_oracle_bit_for_bit(case):
    """Tiling (n_docs around the tile, ragged last tile, postings on tile_lo and tile_hi - 1, a token in every document, untouched
    tiles), the order of additions (1e16 / 1 / -1e16 / 3 in several orders, repeated tokens, 300 tokens = two chunks), the selection
    (cancellation, negative, NaN, +inf, a tie run cut by k over several tiles, a full tile, k = 1 / 100 / 1024, k beyond the positives,
    empty queries, empty lists), batches of 1 / 3 / 70 / 500 and a call in three rounds."""
    sp = _index(case["ix"], tile_docs=case["tile_docs"], cand_cap=case.get("cand_cap"))
    try:
        B = len(case["q_indptr"]) - 1
        got = sp.topk(case["q_indptr"], case["q_tokens"], B, case["k"])
        want = _want(case)
        assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))[:5]
        assert so.same(got, want)
        tile = case["tile_docs"] or so.DEFAULT_TILE
        tiles = -(-case["ix"]["n_docs"] // tile)
        assert sp.get_option("tiles_last") == tiles * B and sp.get_option("calls") == 1 and sp.postings == int(case["ix"]["indptr"][-1])
        assert sp.get_option("rounds_last") == case.get("rounds", 1)
        skipped = sp.get_option("skipped_tiles_last")
        assert case.get("min_skipped", 0) <= skipped <= tiles * B
        # results never depend on the tile: the same call with another tile size
        sp.set_option("tile_docs", 128 if tile != 128 else 64)
        assert so.same(sp.topk(case["q_indptr"], case["q_tokens"], B, case["k"]), want)
    finally:
        sp.close()


def test_untouched_tiles_leave_early_and_are_counted():
    case = _by("tile64_n200")                                   # 4 tiles; token 12 has postings in tile 1 only, token 11 nowhere
    sp = _index(case["ix"], tile_docs=64)
    try:
        q = so.ragged([[12], [11], [], [12, 11]])
        assert so.same(sp.topk(*q, 4, 10), so.topk(case["ix"], *q, 10))
        assert sp.get_option("skipped_tiles_last") == 3 + 4 + 4 + 3 and sp.get_option("tiles_last") == 16
        q = so.ragged([[8]])                                    # a token in every document: no tile is skipped
        assert so.same(sp.topk(*q, 1, 10), so.topk(case["ix"], *q, 10)) and sp.get_option("skipped_tiles_last") == 0
    finally:
        sp.close()


def test_two_calls_in_a_row_with_a_growing_batch_and_another_k():
    """One handle, one workspace: a small call, a larger one that grows the workspace, a smaller k again, then rounds -- every answer
    right, whatever the workspace held before."""
    ix = so.batch_index()
    sp = _index(ix, tile_docs=256)
    try:
        for B, k in ((3, 5), (70, 50), (70, 7), (3, 1024), (1, 1)):
            q = so.queries(np.random.default_rng(100 + B + k), 40, B)
            assert so.same(sp.topk(*q, B, k), so.topk(ix, *q, k)), (B, k)
        sp.set_option("cand_cap", 30 * 8 * 20 * 12)
        q = so.queries(np.random.default_rng(70), 40, 70)
        assert so.same(sp.topk(*q, 70, 20), so.topk(ix, *q, 20)) and sp.get_option("rounds_last") == 3
        sp.set_option("cand_cap", 1)                            # one query per round
        assert so.same(sp.topk(*q, 70, 20), so.topk(ix, *q, 20)) and sp.get_option("rounds_last") == 70
        sp.set_option("cand_cap", 0)
        assert so.same(sp.topk(*q, 70, 20), so.topk(ix, *q, 20)) and sp.get_option("rounds_last") == 1
        assert sp.get_option("calls") == 8
    finally:
        sp.close()


def test_device_form_on_a_side_stream_and_an_unknown_token_is_an_empty_list():
    import torch
    case = _by("tile64_n200")
    ix = case["ix"]
    sp = _index(ix, tile_docs=64)
    try:
        n_tok = ix["n_tokens"]
        q_indptr, q_tokens = so.ragged([[8, n_tok, 10], [n_tok], [9, -1, 9], [n_tok + 5, 12], [], [0, 1, 2]])
        B, k = 6, 10
        want = so.topk(ix, q_indptr, q_tokens, k)               # the oracle takes an id outside the index as an empty list
        known = so.ragged([[8, 10], [], [9, 9], [12], [], [0, 1, 2]])
        assert so.same(want, so.topk(ix, *known, k))
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_ptr = torch.from_numpy(q_indptr).cuda()
            d_tok = torch.from_numpy(q_tokens).cuda()
            d_rows = torch.full((B, k), 77, dtype=torch.int32, device="cuda")
            d_scores = torch.full((B, k), 7.0, dtype=torch.float64, device="cuda")
            sp.topk_device(d_ptr, d_tok, B, len(q_tokens), k, d_rows, d_scores, stream=stream.cuda_stream)
            got = (d_rows.cpu().numpy(), d_scores.cpu().numpy())
        stream.synchronize()
        assert so.same(got, want)
        assert so.same(got, sp.topk(*known, B, k))              # the host form's answer for the same queries without the unknown ids
        with pytest.raises(_native.RqError, match="token id"):  # which the host form refuses
            sp.topk(q_indptr, q_tokens, B, k)
    finally:
        sp.close()


def test_refusals():
    ix = _by("tile64_n65")["ix"]
    sp = _index(ix)
    try:
        q = so.ragged([[0, 1]])
        for B, k in ((1, 0), (1, 1025), (1, -1)):
            with pytest.raises(_native.RqError, match="k "):
                sp.topk(*q, B, k)
        with pytest.raises(_native.RqError, match="B "):
            sp.topk(np.zeros(1, np.int64), np.zeros(0, np.int32), 0, 5)
        with pytest.raises(_native.RqError, match="token id"):
            sp.topk(*so.ragged([[0, ix["n_tokens"]]]), 1, 5)
        with pytest.raises(_native.RqError, match="decreases"):
            sp.topk(np.array([0, 2, 1], np.int64), np.array([0, 1], np.int32), 2, 5)
        for bad in (63, 100, 16384, 0):
            with pytest.raises(_native.RqError, match="tile_docs"):
                sp.set_option("tile_docs", bad)
        with pytest.raises(_native.RqError):
            sp.set_option("calls", 1)
        assert sp.get_option("no_such_option") == -1 and "unknown" in _native.last_error()
        assert sp.get_option("tile_docs") == so.DEFAULT_TILE and sp.get_option("calls") == 0
        assert so.same(sp.topk(*q, 1, 5), so.topk(ix, *q, 5))   # and the handle still answers
    finally:
        sp.close()
    with pytest.raises(_native.RqError, match="ascending"):
        _native.SparseIndex(np.array([0, 3], np.int64), np.array([0, 2, 1], np.int32), np.ones(3), 1, 3)
    with pytest.raises(_native.RqError, match="ascending"):
        _native.SparseIndex(np.array([0, 2], np.int64), np.array([1, 1], np.int32), np.ones(2), 1, 3)
    with pytest.raises(_native.RqError, match="outside"):
        _native.SparseIndex(np.array([0, 1], np.int64), np.array([3], np.int32), np.ones(1), 1, 3)


# ---- through the seam ----------------------------------------------------------------------------------------------------------------
def _passages(rng, n, first=0):
    """Passages of 12 to 30 words from a skewed vocabulary of 300 (the generator of tools/bm25_scale.py at a test's size)."""
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    return [si.Document(id=f"p{first + i}", text=" ".join(f"w{w}" for w in rng.choice(300, rng.integers(12, 31), p=p))) for i in range(n)]


def _questions(rng, n):
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    return [" ".join(f"w{w}" for w in rng.choice(300, rng.integers(1, 10), p=p)) for _ in range(n - 2)] + ["", "zzz unknown words"]


def test_bm25_index_gpu_backend_equals_the_host_backend_and_follows_adds():
    rng = np.random.default_rng(3)
    bm = si.BM25Index()
    bm.add_documents(_passages(rng, 3000))
    qs = _questions(rng, 40)
    host = bm.search_batch_rows(qs, 50, backend="host")
    assert (host[0] >= 0).sum() > 1000
    assert so.same(bm.search_batch_rows(qs, 50, backend="gpu"), host)
    assert so.same(bm.search_batch_rows(qs, 50, backend="auto"), host)
    first = bm._csr()["sparse"]
    assert first.n_docs == 3000 and bm.search_batch(qs, 50, backend="gpu") == bm.search_batch(qs, 50) and bm._csr()["sparse"] is first
    bm.add_documents(_passages(rng, 200, first=3000))           # idf and avgdl change: new arrays, a new device index
    host = bm.search_batch_rows(qs, 50, backend="host")
    assert so.same(bm.search_batch_rows(qs, 50, backend="gpu"), host)
    assert bm._csr()["sparse"] is not first and bm._csr()["sparse"].n_docs == 3200 and first._h is None
    assert bm.search_batch(qs, 7, backend="gpu") == [bm.search(q, 7) for q in qs]


def test_hybrid_retriever_sparse_backend_gpu_equals_host(tmp_path):
    rng = np.random.default_rng(4)
    docs = _passages(rng, 600)
    qs = _questions(rng, 12)
    outs = {}
    for backend in ("host", "gpu"):
        r = _retriever(tmp_path / backend, backend)
        r.add_documents(docs)
        outs[backend] = ([[(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score) for x in res] for res in r.hybrid_search_batch(qs, top_k=10, retrieval_pool_size=40)],
                         r.get_scores_for_router_batch(qs, num_passages=10))
        if backend == "gpu":
            assert r.bm25_index._csr().get("sparse") is not None and r.bm25_index._csr()["sparse"].get_option("calls") >= 2
        else:
            assert r.bm25_index._csr().get("sparse") is None
        r.close()
    assert outs["gpu"][0] == outs["host"][0] and any(outs["host"][0])
    assert outs["gpu"][1] == outs["host"][1]


def _retriever(path, backend):
    from rag_uq_amd.embedders import HashEmbedder
    os.makedirs(path, exist_ok=True)
    return si.HybridRetriever(bm25_persist_path=str(path / "bm25.pkl"), chroma_persist_path=str(path / "dense"), embedder=HashEmbedder(), sparse_backend=backend)
