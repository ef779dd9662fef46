"""Hybrid fusion on the device (include/rq.h rq_hybrid_*, rq_sparse_score_rows*, csrc/rq_hybrid.hip) against tests/hybrid_oracle.py:
every key, position, count and score identical in its bits, no tolerance, no case left out.  tests/test_hybrid.py shows that the oracle
and HybridRetriever._fuse_batch_rows agree value for value, so the device route and the host path share one definition."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hybrid_oracle as ho  # noqa: E402
import sparse_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ho.cases()
SPARSE_CASES = so.cases()


def _map(ks):
    return _native.HybridMap(ks["nb"], ks["dense_key"], ks["known"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fuse_and_missing_equal_the_oracle_bit_for_bit(case):
    """Candidate counts around every instantiation (1, 2, 63, 64, 65, 255, 256, 257, 1 000, 2 048), a pool of width 0, pools that are all
    padding, top_k of 1 / at the valid count / one above / 1 024, batches of 1 / 3 / 70, a document in both pools at the first and last
    position of each, a tie run over the pool boundary cut by top_k, negative / zero / infinite scores, a NaN hybrid score, unknown keys,
    dense-only keys, rows outside the indexes, no dense index -- each with and without the four extra arrays."""
    ks, pools = case["ks"], case["pools"]
    hm = _map(ks)
    try:
        miss = hm.missing(pools[0], pools[2])
        want_miss = ho.missing(ks, pools[0], pools[2])
        assert ho.same(miss, want_miss), [np.argwhere(g != w)[:5] for g, w in zip(miss, want_miss)]
        extras = ho.extras_for(case)
        calls = 1
        for kw in ({}, extras):
            for top_k in case["top_ks"]:
                got = hm.fuse(*pools, top_k, **kw)
                want = ho.fuse(ks, *pools, top_k, **kw)
                calls += 1
                for name, g, w in zip(("keys", "b", "d", "h", "pos", "count"), got, want):
                    assert ho.same((g,), (w,)), (name, top_k, bool(kw), np.argwhere(g != w)[:5])
        assert hm.get_option("calls") == calls and hm.get_option("missing_calls") == 1 and hm.get_option("fuse_calls") == calls - 1
        assert hm.get_option("n_keys") == ks["n_keys"] and hm.get_option("nb") == ks["nb"] and hm.get_option("n_dense") == ks["n_dense"]
    finally:
        hm.close()


def test_only_one_side_completed_and_the_device_form_on_a_side_stream():
    import torch
    case = next(c for c in CASES if c["name"] == "n200_100x100_b70")
    ks, (sp_rows, sp_scores, de_rows, de_scores) = case["ks"], case["pools"]
    e = ho.extras_for(case)
    hm = _map(ks)
    try:
        for kw in ({"miss_dense": e["miss_dense"], "extra_dense": e["extra_dense"]}, {"miss_sparse": e["miss_sparse"], "extra_sparse": e["extra_sparse"]},
                   {"miss_dense": e["miss_dense"], "miss_sparse": e["miss_sparse"]}):
            assert ho.same(hm.fuse(sp_rows, sp_scores, de_rows, de_scores, 50, **kw), ho.fuse(ks, sp_rows, sp_scores, de_rows, de_scores, 50, **kw)), list(kw)
        B, K1, K2, k = 70, 100, 100, 30
        want = ho.fuse(ks, sp_rows, sp_scores, de_rows, de_scores, k, **e)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d = {n: torch.from_numpy(np.ascontiguousarray(a)).cuda() for n, a in (("sr", sp_rows), ("ss", sp_scores), ("dr", de_rows), ("ds", de_scores),
                                                                                  ("ed", e["extra_dense"]), ("es", e["extra_sparse"]))}
            d_md = torch.full((B, K1), 77, dtype=torch.int64, device="cuda")
            d_ms = torch.full((B, K2), 77, dtype=torch.int32, device="cuda")
            hm.missing_device(d["sr"], d["dr"], B, K1, K2, d_md, d_ms, stream=stream.cuda_stream)
            keys, pos = torch.full((B, k), 77, dtype=torch.int32, device="cuda"), torch.full((B, k), 77, dtype=torch.int32, device="cuda")
            b, dd, h = (torch.full((B, k), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
            count = torch.full((B,), 77, dtype=torch.int32, device="cuda")
            hm.fuse_device(d["sr"], d["ss"], d["dr"], d["ds"], B, K1, K2, k, keys, b, dd, h, pos, count, stream.cuda_stream,
                           d_miss_dense=d_md, d_extra_dense=d["ed"], d_miss_sparse=d_ms, d_extra_sparse=d["es"])
            got = tuple(t.cpu().numpy() for t in (keys, b, dd, h, pos, count))
            got_miss = (d_md.cpu().numpy(), d_ms.cpu().numpy())
        stream.synchronize()
        assert ho.same(got_miss, (e["miss_dense"], e["miss_sparse"])) and ho.same(got, want)
    finally:
        hm.close()


def test_refusals():
    case = CASES[3]
    ks, pools = case["ks"], case["pools"]
    hm = _map(ks)
    try:
        e = ho.extras_for(case)
        for top_k in (0, -1, 1025):
            with pytest.raises(_native.RqError, match="top_k"):
                hm.fuse(*pools, top_k)
        with pytest.raises(_native.RqError, match="without its miss"):
            hm.fuse(*pools, 5, extra_dense=e["extra_dense"])
        with pytest.raises(_native.RqError, match="without its miss"):
            hm.fuse(*pools, 5, extra_sparse=e["extra_sparse"], miss_dense=e["miss_dense"])
        with pytest.raises(_native.RqError, match="no candidates"):
            hm.fuse(np.zeros((2, 0), np.int32), np.zeros((2, 0)), np.zeros((2, 0), np.int64), np.zeros((2, 0), np.float32), 5)
        with pytest.raises(_native.RqError, match="K1 "):
            hm.missing(np.zeros((1, 1025), np.int32), np.zeros((1, 1), np.int64))
        with pytest.raises(_native.RqError, match="B "):
            hm.missing(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int64))
        assert hm.get_option("no_such_option") == -1 and "unknown" in _native.last_error() and hm.get_option("calls") == 0
        assert ho.same(hm.fuse(*pools, 5), ho.fuse(ks, *pools, 5))          # and the handle still answers
    finally:
        hm.close()
    with pytest.raises(_native.RqError, match="injective"):
        _native.HybridMap(4, np.array([1, 5, 1], np.int64), np.ones(7, bool))
    with pytest.raises(_native.RqError, match="outside"):
        _native.HybridMap(4, np.array([1, 7], np.int64), np.ones(7, bool))


# ---- rq_sparse_score_rows* ---------------------------------------------------------------------------------------------------------------
def _rows_for(case, m, rng):
    """[B][m] rows: random rows of the corpus with -1, rows >= n_docs and repeats among them (m = 1: one row each)."""
    n, B = case["ix"]["n_docs"], len(case["q_indptr"]) - 1
    rows = rng.integers(-1, n + 2, size=(B, m)).astype(np.int32)
    if m >= 8:
        rows[:, 1] = rows[:, 0]
        rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = -1, n, n - 1, 0
    return rows


@pytest.mark.parametrize("case", SPARSE_CASES, ids=[c["name"] for c in SPARSE_CASES])
def test_sparse_score_rows_equals_the_oracle_bit_for_bit(case):
    """The cases of tests/sparse_oracle.py (tiling, the order of additions 1e16 / 1 / -1e16 / 3, repeated tokens, a query of 300 tokens,
    cancellation, NaN and infinite contributions, empty queries and lists, batches of 1 .. 500) with m of 1, 64, 257 and 4 096: rows
    -1 and >= n_docs, repeated rows; and the rows the top-k returns score what it returned."""
    ix = case["ix"]
    sp = _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    try:
        B = len(case["q_indptr"]) - 1
        rng = np.random.default_rng(B + ix["n_docs"])
        for i, m in enumerate((1, 64, 257, 4096)):
            rows = _rows_for(case, m, rng)
            got = sp.score_rows(case["q_indptr"], case["q_tokens"], B, rows)
            want = ho.sparse_score_rows(ix, case["q_indptr"], case["q_tokens"], rows)
            assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (m, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
            assert sp.get_option("score_calls") == i + 1
        top_rows, top_scores = sp.topk(case["q_indptr"], case["q_tokens"], B, case["k"])
        again = sp.score_rows(case["q_indptr"], case["q_tokens"], B, top_rows)
        assert np.array_equal(again.view(np.uint64), top_scores.view(np.uint64))
    finally:
        sp.close()


def test_sparse_score_rows_device_form_on_a_side_stream_and_an_unknown_token():
    import torch
    case = next(c for c in SPARSE_CASES if c["name"] == "tile64_n200")
    ix = case["ix"]
    sp = _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    try:
        n_tok = ix["n_tokens"]
        q_indptr, q_tokens = so.ragged([[8, n_tok, 10], [n_tok], [9, -1, 9], [n_tok + 5, 12], [], [0, 1, 2]])
        B, m = 6, 257
        rows = np.random.default_rng(2).integers(-1, 202, size=(B, m)).astype(np.int32)
        want = ho.sparse_score_rows(ix, q_indptr, q_tokens, rows)
        assert np.array_equal(want, ho.sparse_score_rows(ix, *so.ragged([[8, 10], [], [9, 9], [12], [], [0, 1, 2]]), rows)) and want.any()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_ptr, d_tok, d_rows = torch.from_numpy(q_indptr).cuda(), torch.from_numpy(q_tokens).cuda(), torch.from_numpy(rows).cuda()
            d_scores = torch.full((B, m), 7.0, dtype=torch.float64, device="cuda")
            sp.score_rows_device(d_ptr, d_tok, B, len(q_tokens), d_rows, m, d_scores, stream=stream.cuda_stream)
            got = d_scores.cpu().numpy()
        stream.synchronize()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        with pytest.raises(_native.RqError, match="token id"):              # which the host form refuses
            sp.score_rows(q_indptr, q_tokens, B, rows)
        for bad_m in (0, _native.MAX_SCORE_ROWS + 1):
            with pytest.raises(_native.RqError, match="m "):
                sp.score_rows(*so.ragged([[0]]), 1, np.zeros((1, bad_m), np.int32))
    finally:
        sp.close()


# ---- through the seam --------------------------------------------------------------------------------------------------------------------
def _passages(rng, n, first=0):
    """Passages of 12 to 30 words from a skewed vocabulary of 300 (the generator of tests/test_gpu_sparse.py)."""
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    return [si.Document(id=f"p{first + i}", text=" ".join(f"w{w}" for w in rng.choice(300, rng.integers(12, 31), p=p))) for i in range(n)]


def _questions(rng, n):
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    return [" ".join(f"w{w}" for w in rng.choice(300, rng.integers(1, 10), p=p)) for _ in range(n - 2)] + ["", "zzz unknown words"]


def _retriever(path, fusion):
    from rag_uq_amd.embedders import HashEmbedder
    os.makedirs(path, exist_ok=True)
    return si.HybridRetriever(bm25_persist_path=str(path / "bm25.pkl"), chroma_persist_path=str(path / "dense"), embedder=HashEmbedder(), sparse_backend="gpu",
                              fusion_backend=fusion)


def _answers(r, qs, top_k, pool, complete):
    return ([[(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score) for x in res] for res in r.hybrid_search_batch(qs, top_k=top_k, retrieval_pool_size=pool, complete_scores=complete)],
            [tuple(t) for t in r.get_scores_for_router_batch(qs, num_passages=top_k, retrieval_pool_size=pool, complete_scores=complete)])


def test_hybrid_retriever_fusion_backend_gpu_equals_host(tmp_path):
    """Two retrievers over the same 600 passages, fused on the host and on the device: hybrid_search_batch and
    get_scores_for_router_batch equal value for value, complete_scores off and on, pools smaller and larger than top_k; the map follows
    an add; the option counters show that the device branch ran."""
    rng = np.random.default_rng(4)
    docs, more = _passages(rng, 600), _passages(rng, 50, first=600)
    qs = _questions(rng, 12)
    host, gpu = _retriever(tmp_path / "host", "host"), _retriever(tmp_path / "gpu", "gpu")
    try:
        for r in (host, gpu):
            r.add_documents(docs)
            r.bm25_index.add_documents(more[:20])                            # BM25 only: dense rows and sparse rows no longer line up
            r.dense_index.add_documents(more[30:])                           # dense only, known to the store or not
            for d in more[:40]:
                r.documents[d.id] = d
        calls = 0
        for top_k, pool in ((10, 40), (20, 7), (5, 1)):
            for complete in (False, True):
                want = _answers(host, qs, top_k, pool, complete)
                got = _answers(gpu, qs, top_k, pool, complete)
                calls += 2
                assert got[0] == want[0] and any(want[0]), (top_k, pool, complete)
                assert got[1] == want[1], (top_k, pool, complete)
        first = gpu._key_space()["map"]
        assert first is not None and first.get_option("fuse_calls") == calls and first.get_option("missing_calls") == calls // 2
        assert host._key_space()["map"] is None and gpu.bm25_index._csr()["sparse"].get_option("score_calls") == calls // 2
        later = _passages(rng, 30, first=700)
        for r in (host, gpu):
            r.add_documents(later)
        assert _answers(gpu, qs, 10, 40, True) == _answers(host, qs, 10, 40, True)
        assert gpu._key_space()["map"] is not first and first._h is None and gpu._key_space()["map"].n_keys == first.n_keys + 60
        auto = _retriever(tmp_path / "auto", "auto")
        auto.add_documents(docs[:100])
        assert _answers(auto, qs, 10, 40, True) == _answers(auto, qs, 10, 40, True) and auto.fusion_backend == "auto"
        no_sparse = si.HybridRetriever(bm25_persist_path=str(tmp_path / "n.pkl"), dense_index=gpu.dense_index, fusion_backend="gpu")
        no_sparse.bm25_index.add_documents(docs[:10])
        with pytest.raises(_native.RqError, match="sparse_backend"):
            no_sparse.hybrid_search_batch(qs, top_k=5)
    finally:
        host.close()
        gpu.close()


def test_bm25_index_score_rows_batch_gpu_backend_equals_the_host_backend():
    rng = np.random.default_rng(3)
    bm = si.BM25Index()
    bm.add_documents(_passages(rng, 3000))
    qs = _questions(rng, 40)
    rows = rng.integers(-1, 3003, size=(40, 100))
    host = bm.score_rows_batch(qs, rows)
    assert (host != 0).sum() > 500
    for backend in ("gpu", "auto"):
        got = bm.score_rows_batch(qs, rows, backend=backend)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), host.view(np.uint64)), backend
