"""Grouped hybrid fusion on the device (include/rq.h rq_hybrid_set_groups, rq_hybrid_fuse_grouped*, csrc/rq_hybrid.hip)
against tests/hybrid_grouped_oracle.py, bit for bit, and the batch calls of HybridRetriever with `distinct_by=` on the device route
(grouped BM25 pool, grouped dense pool, grouped fusion, the unchanged rerank) against the per-query host calls they are defined by."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hybrid_grouped_oracle as hgo  # noqa: E402
import hybrid_oracle as ho  # noqa: E402
import router_scenario as rs  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ho.cases()


def _map(ks, key_group=None):
    hm = _native.HybridMap(ks["nb"], ks["dense_key"], ks["known"])
    if key_group is not None:
        hm.set_groups(key_group)
    return hm


def _check(hm, ks, key_group, pools, top_k, what=None):
    got = hm.fuse_grouped(*pools, top_k)
    want = hgo.fuse(ks, key_group, *pools, top_k)
    assert np.array_equal(got[5], want[5]) and np.array_equal(got[0], want[0]), (what, got[5], want[5], np.argwhere(got[0] != want[0])[:5])
    assert hgo.same(got, want), what
    return want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_fusion_case_under_group_tables(case):
    """Every key space and pool of tests/hybrid_oracle.py -- candidate counts around every instantiation up to the full 2 048, pools of
    width 0, all padding, keys in both pools, tie runs, a NaN h, unknown keys, no dense index -- under three tables: a few large groups
    with -1 keys between them, 50 groups, and every key a group of its own (the ungrouped fusion)."""
    ks, pools = case["ks"], case["pools"]
    rng = np.random.default_rng(len(case["name"]))
    hm = _map(ks)
    try:
        with pytest.raises(_native.RqError, match="no group table"):
            hm.fuse_grouped(*pools, 1)
        for n_groups in (4, 50):
            key_group = rng.integers(-1, n_groups, ks["n_keys"]).astype(np.int32)
            hm.set_groups(key_group)
            for top_k in case["top_ks"]:
                _check(hm, ks, key_group, pools, top_k, (n_groups, top_k))
        own = np.full(ks["n_keys"], -1, np.int32)
        hm.set_groups(own)
        for top_k in case["top_ks"]:
            want = _check(hm, ks, own, pools, top_k, ("own", top_k))
            plain = hm.fuse(*pools, top_k)
            assert ho.same(plain, ho.fuse(ks, *pools, top_k)) and (case["name"] == "nan_hybrid_score" or ho.same(plain, want))
        assert hm.get_option("grouped") == 1 and hm.get_option("grouped_calls") == 3 * len(case["top_ks"])
    finally:
        hm.close()


def test_the_full_2048_candidates_with_50_groups_and_fewer_groups_than_top_k():
    case = next(c for c in CASES if c["name"].startswith("n2048_"))
    ks, pools = case["ks"], case["pools"]
    key_group = (np.arange(ks["n_keys"]) % 50).astype(np.int32)
    hm = _map(ks, key_group)
    try:
        for top_k in (1, 49, 50, 51, 1024):
            want = _check(hm, ks, key_group, pools, top_k, top_k)
        assert want[5].max() == 50 and (want[0][:, 50:] == -1).all() and (want[3][:, 50:] == 0.0).all()
    finally:
        hm.close()


def test_groups_across_both_pools_merged_keys_ties_and_group_none():
    """40 shared documents (sparse row r = dense row r) and 10 dense-only ones.  Query 0: the same group under different keys in the two
    pools (sparse key 1, dense-only key 52).  Query 1: key 0 is in both pools, its merged candidate wins over its group-mate key 2.
    Query 2: the merged key 0 loses to its group-mate key 2.  Query 3: h ties across groups and inside one, resolved by position.
    Query 4: group -1 keys between grouped ones, none collapsed."""
    ks = ho.key_space(50, np.concatenate([np.arange(40, dtype=np.int64), 50 + np.arange(10, dtype=np.int64)]), np.ones(60, bool))
    key_group = np.full(60, -1, np.int32)
    key_group[[0, 2, 4]] = 7
    key_group[[1, 52]] = 8
    key_group[[10, 11, 12, 13]] = [20, 21, 20, 21]
    key_group[[53, 54]] = 9
    sp_rows = np.array([[1, 3, 5, -1], [0, 2, 6, -1], [2, 0, 6, -1], [10, 11, 12, 13], [0, 30, 2, 31]], np.int32)
    sp_scores = np.array([[4.0, 3.0, 2.0, 0.0], [4.0, 3.0, 2.0, 0.0], [4.0, 1.0, 0.5, 0.0], [2.0, 2.0, 2.0, 2.0], [4.0, 3.0, 2.0, 1.0]])
    de_rows = np.array([[42, 43, 44, -1], [0, 45, 46, -1], [0, 45, 46, -1], [47, 48, -1, -1], [32, 43, 44, 33]], np.int64)
    de_scores = np.array([[0.9, 0.5, 0.4, 0.0], [0.9, 0.5, 0.4, 0.0], [0.2, 0.9, 0.4, 0.0], [0.5, 0.5, 0.0, 0.0], [0.9, 0.8, 0.7, 0.6]], np.float32)
    pools = (sp_rows, sp_scores, de_rows, de_scores)
    hm = _map(ks, key_group)
    try:
        for top_k in (1, 2, 3, 8):
            want = _check(hm, ks, key_group, pools, top_k, top_k)
        keys, count = want[0], want[5]
        assert keys[0].tolist()[:4] == [1, 3, 53, 5] and count[0] == 4                    # key 52 (dense row 42) falls to its group-mate key 1, 54 to 53
        assert keys[1][0] == 0 and 2 not in keys[1] and want[2][1][0] == np.float32(0.9)  # the merged candidate carries both scores and wins
        assert keys[2][0] == 2 and 0 not in keys[2]                                       # ... and loses: max_d is still taken over all candidates
        assert keys[3].tolist()[:4] == [10, 11, 57, 58] and count[3] == 4                 # ties: positions 0 and 1 stand for groups 20 and 21
        assert count[4] == 6 and set(keys[4][:6]) == {0, 30, 31, 32, 33, 53}              # group 7 once, group 9 once, every -1 key kept
        ungrouped = ho.fuse(ks, *pools, 8)
        assert ungrouped[5].tolist() == [6, 5, 5, 6, 8]
    finally:
        hm.close()


def test_device_form_feeds_the_rerank_layout_and_the_refusals():
    import torch
    case = next(c for c in CASES if c["name"] == "n200_100x100_b70")
    ks, (sp_rows, sp_scores, de_rows, de_scores) = case["ks"], case["pools"]
    key_group = (np.arange(ks["n_keys"]) % 37).astype(np.int32)
    B, K1, K2, k = 70, 100, 100, 20
    hm = _map(ks, key_group)
    try:
        want = hgo.fuse(ks, key_group, sp_rows, sp_scores, de_rows, de_scores, k)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sp_rows, sp_scores, de_rows, de_scores)]
            keys = torch.full((B, k), 77, dtype=torch.int32, device="cuda")
            b, dd, h = (torch.full((B, k), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
            count = torch.full((B,), 55, dtype=torch.int32, device="cuda")
            hm.fuse_grouped_device(*d, B, K1, K2, k, keys, b, dd, h, None, count, stream=stream.cuda_stream)
            got = (keys.cpu().numpy(), b.cpu().numpy(), dd.cpu().numpy(), h.cpu().numpy(), count.cpu().numpy())
        stream.synchronize()
        assert hgo.same(got, want[:4] + (want[5],))
        for bad in (np.full(ks["n_keys"], -2, np.int32), np.zeros(ks["n_keys"] + 1, np.int32)):
            with pytest.raises(_native.RqError):
                hm.set_groups(bad)
        with pytest.raises(_native.RqError, match="top_k"):
            hm.fuse_grouped(sp_rows, sp_scores, de_rows, de_scores, 0)
        assert hm.get_option("grouped_calls") == 1 == hm.get_option("fuse_calls")
    finally:
        hm.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _rows(out):
    return [[(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score) for x in res] for res in out]


def test_batch_calls_with_distinct_by_on_the_device_route_equal_the_per_query_host_calls(tmp_path):
    """2 000 chunks of 40 titles, 24 questions, every backend "gpu": hybrid_search_batch and get_scores_for_router_batch equal the loop of
    the per-query calls value for value (ids, bm25, dense and hybrid scores, counts), without and with `allowed_ids`; route_batch equals
    the host route over the same columns: ids, b, d and the order identical, the gate weights within 2e-6 (the bound of
    tests/test_router.py), and h = w*d + (1 - w)*b within what that bound can move it, 2e-6 * (|b| + |d|) plus four roundings."""
    docs, questions, _ = rs.corpus()
    docs, questions = docs[:2000], questions[:22] + questions[-2:]
    allowed = {f"p{i}" for i in range(0, 2000, 3)} | {"nobody"}
    r = rs.retriever(tmp_path, sparse_backend="gpu", fusion_backend="gpu", router_backend="gpu")
    gate = rs.gate()
    try:
        r.add_documents(docs)
        for kw in ({}, {"allowed_ids": allowed}):
            for top_k, pool in ((10, 50), (30, 20)):
                want = [r.hybrid_search(q, top_k, pool, distinct_by="title", **kw) for q in questions]
                assert sum(len(x) for x in want) > 150 and all(len({x.title for x in res}) == len(res) for res in want)
                assert _rows(want) != _rows([r.hybrid_search(q, top_k, pool, **kw) for q in questions])
                assert _rows(r.hybrid_search_batch(questions, top_k, pool, distinct_by="title", **kw)) == _rows(want), (list(kw), top_k, pool)
                cols = r.get_scores_for_router_batch(questions, top_k, retrieval_pool_size=pool, distinct_by="title", **kw)
                assert [tuple(c) for c in cols] == [tuple(r.get_scores_for_router(q, top_k, retrieval_pool_size=pool, distinct_by="title", **kw)) for q in questions]
            hm, sp = r._key_space()["map"], r.bm25_index._csr()["sparse"]
            before = (hm.get_option("grouped_calls"), sp.get_option("grouped_calls"), gate.native(0).get_option("rerank_calls"))
            got, got_w = r.route_batch(questions, gate, 10, num_passages=20, retrieval_pool_size=50, distinct_by="title", return_weights=True, **kw)
            assert (hm.get_option("grouped_calls"), sp.get_option("grouped_calls"), gate.native(0).get_option("rerank_calls")) == tuple(x + 1 for x in before)
            r.sparse_backend = r.fusion_backend = r.router_backend = "host"
            want, want_w = r.route_batch(questions, gate, 10, num_passages=20, retrieval_pool_size=50, distinct_by="title", return_weights=True, **kw)
            r.sparse_backend = r.fusion_backend = r.router_backend = "gpu"
            assert rs.separated(want) and sum(len(x) for x in want) > 150
            a, e = _rows(got), _rows(want)
            assert [[x[:3] for x in res] for res in a] == [[x[:3] for x in res] for res in e], list(kw)
            np.testing.assert_allclose(got_w, want_w, rtol=0, atol=2e-6)
            for ra, re_ in zip(a, e):
                for x, y in zip(ra, re_):
                    mag = abs(x[1]) + abs(x[2])
                    assert abs(x[3] - y[3]) <= 2e-6 * mag + 4 * 2.0 ** -53 * mag, (x, y)
        with pytest.raises(ValueError, match="complete_scores"):
            r.hybrid_search_batch(questions, 10, distinct_by="title", complete_scores=True)
        with pytest.raises(ValueError, match="allowed_ids_each"):
            r.route_batch(questions, gate, 10, distinct_by="title", allowed_ids_each=[None] * len(questions))
    finally:
        gate.close()
        r.close()
