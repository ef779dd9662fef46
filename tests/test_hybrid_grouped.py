"""Grouped hybrid batches (`distinct_by=` on HybridRetriever.hybrid_search_batch / get_scores_for_router_batch / route_batch /
dense_search_batch), the parts that need no GPU: over a host stand-in for NativeIndex the host batch route equals the per-query calls it
is defined by, value for value; tests/hybrid_grouped_oracle.py equals HybridRetriever._fuse(..., distinct_by=); and the refusals.  The
GPU side is tests/test_gpu_hybrid_grouped.py."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_oracle as gro  # noqa: E402
import hybrid_grouped_oracle as hgo  # noqa: E402
import hybrid_oracle as ho  # noqa: E402
import router_scenario as rs  # noqa: E402


class _StubFilter(_native.RowFilter):
    def __init__(self, index, keep):
        self._index, self._h, self.keep, self.count, self.closed = index, None, keep, int(keep.sum()), False

    def close(self):
        self.closed = True


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the dense oracles over the fp16 rows,
    with groups and one filter (the manner of tests/test_grouped.py's stand-in)."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), True)
        self.dim = self.x16.shape[1]
        self.groups = np.full(len(self), -1, np.int64)
        self.grouped_calls = 0

    def __len__(self):
        return self.x16.shape[0]

    def add_f32(self, x, normalize=True):
        self.x16 = np.concatenate([self.x16, orc.prepare_rows_f32(np.asarray(x, np.float32), True)])
        self.groups = np.concatenate([self.groups, np.full(len(x), -1, np.int64)])

    def make_filter(self, rows):
        keep = np.zeros(len(self), bool)
        keep[np.asarray(rows, np.int64)] = True
        return _StubFilter(self, keep)

    def set_groups(self, groups, row_begin=0):
        self.groups[row_begin:row_begin + len(groups)] = groups

    def search(self, q, k, metric=0, *, row_filter=None):
        if row_filter is None:
            return orc.dense_topk(q, self.x16, k, metric)
        allowed = np.flatnonzero(row_filter.keep)
        s, r = orc.dense_topk(q, self.x16[allowed], min(k, len(allowed)), metric)
        pad = k - s.shape[1]
        return (np.concatenate([s, np.zeros((len(s), pad), np.float32)], axis=1),
                np.concatenate([np.where(r >= 0, allowed[np.where(r >= 0, r, 0)], -1), np.full((len(s), pad), -1, np.int64)], axis=1))

    def search_grouped(self, q, k, metric=0, *, row_filter=None):
        self.grouped_calls += 1
        return gro.grouped_topk(q, self.x16, self.groups, k, metric, None if row_filter is None else row_filter.keep)


def _retriever(tmp_path):
    """600 chunks of 40 titles (every 17th without a title), in both indexes; 20 more that only BM25 holds and 20 that only the dense
    index holds; 16 questions."""
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    docs, questions, _ = rs.corpus()
    docs = [si.Document(id=d.id, text=d.text, title="" if i % 17 == 0 else d.title, metadata={"section": i % 3}) for i, d in enumerate(docs[:640])]
    dense = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32)), [], [], embedder=RandomProjectionEmbedder(16))
    os.makedirs(tmp_path, exist_ok=True)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    r.add_documents(docs[:600])
    r.bm25_index.add_documents(docs[600:620])
    r.dense_index.add_documents(docs[620:640])
    for d in docs[600:630]:
        r.documents[d.id] = d
    return r, questions[:14] + questions[-2:]


def _rows(out):
    return [[(x.doc_id, x.text, x.bm25_score, x.dense_score, x.hybrid_score, x.title) for x in res] for res in out]


def test_host_batch_route_equals_the_per_query_calls_value_for_value(tmp_path):
    r, qs = _retriever(tmp_path)
    allowed = {f"p{i}" for i in range(0, 640, 3)} | {"nobody"}
    try:
        for key in ("title", "section"):
            for kw in ({}, {"allowed_ids": allowed}):
                for top_k, pool in ((10, 40), (30, 8)):
                    want = [r.hybrid_search(q, top_k, pool, distinct_by=key, **kw) for q in qs]
                    assert any(want) and _rows(want) != _rows([r.hybrid_search(q, top_k, pool, **kw) for q in qs])
                    if key == "title":
                        assert all(len({x.title for x in res if x.title}) == sum(1 for x in res if x.title) for res in want)
                    assert _rows(r.hybrid_search_batch(qs, top_k, pool, distinct_by=key, **kw)) == _rows(want), (key, list(kw), top_k, pool)
                    cols = r.get_scores_for_router_batch(qs, top_k, retrieval_pool_size=pool, distinct_by=key, **kw)
                    loop = [r.get_scores_for_router(q, top_k, retrieval_pool_size=pool, distinct_by=key, **kw) for q in qs]
                    assert [tuple(c) for c in cols] == [tuple(c) for c in loop], (key, list(kw), top_k, pool)
                    assert all(len(c[0]) == top_k for c in cols)
                    dense = r.dense_search_batch(qs, pool, distinct_by=key, **kw)
                    assert dense == [r.dense_search(q, pool, distinct_by=key, **kw) for q in qs] and any(dense)
        flt = r.make_filter(allowed)                                            # a reusable filter serves the grouped calls too
        assert _rows(r.hybrid_search_batch(qs, 10, 40, distinct_by="title", allowed_ids=flt)) == _rows(r.hybrid_search_batch(qs, 10, 40, distinct_by="title", allowed_ids=allowed))
        flt.close()
        assert r.hybrid_search_batch([], 10, distinct_by="title") == [] and r.hybrid_search_batch(qs, 0, 40, distinct_by="title") == [[] for _ in qs]
    finally:
        r.close()


def test_route_batch_with_distinct_by_is_the_host_gate_over_the_grouped_columns(tmp_path):
    r, qs = _retriever(tmp_path)
    gate = rs.gate()
    try:
        out, w = r.route_batch(qs, gate, 5, num_passages=12, retrieval_pool_size=40, distinct_by="title", return_weights=True)
        cols = r.get_scores_for_router_batch(qs, 12, retrieval_pool_size=40, distinct_by="title")
        for q, (b, d, ids, _) in enumerate(cols):
            keys = np.where(np.array(ids, dtype=object) != "", np.arange(12, dtype=np.int32), -1)[None, :]
            _, wb, wd, ww, wh, pos, count = gate.rerank(keys, np.array([b]), np.array([d]), np.array([12]), 5)
            assert [x.doc_id for x in out[q]] == [ids[p] for p in pos[0][:count[0]]]
            assert [(x.bm25_score, x.dense_score, x.hybrid_score) for x in out[q]] == list(zip(wb[0][:count[0]], wd[0][:count[0]], wh[0][:count[0]]))
            assert np.array_equal(w[q], ww[0])
        assert r.route(qs[0], gate, 5, num_passages=12, retrieval_pool_size=40, distinct_by="title") == out[0] or _rows([r.route(qs[0], gate, 5, num_passages=12, retrieval_pool_size=40, distinct_by="title")]) == _rows(out[:1])
    finally:
        r.close()


def test_oracle_equals_fuse_with_distinct_by(tmp_path):
    """tests/hybrid_grouped_oracle.py over the retriever's own key space, pools and key groups against `_fuse(..., distinct_by=)`."""
    r, qs = _retriever(tmp_path)
    try:
        bm, dn = r.bm25_index, r.dense_index
        c = r._key_space()
        ks = ho.key_space(c["nb"], c["dense_key"], c["known"])
        key_group = r._key_groups(c, "title")
        assert key_group.dtype == np.int32 and len(key_group) == len(c["ids"]) and (key_group == -1).sum() > 30 and key_group.max() == 39
        sp_rows, sp_scores = bm.search_batch_rows(qs, 40, distinct_by="title")
        de_scores, de_rows = dn.search_rows_batch(qs, 40, distinct_by="title")
        for top_k in (1, 10, 80):
            keys, b, d, h, _, count = hgo.fuse(ks, key_group, sp_rows, sp_scores, de_rows, de_scores, top_k)
            for q in range(len(qs)):
                sparse = [(bm.doc_ids[i], s) for i, s in zip(sp_rows[q], sp_scores[q]) if i >= 0]
                dense = [(dn._ids[i], float(s)) for i, s in zip(de_rows[q], de_scores[q]) if i >= 0]
                want = r._fuse(sparse, dense, top_k, None, "title")
                n = int(count[q])
                assert [(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score) for x in want] == list(zip(c["ids"][keys[q, :n]], b[q, :n], d[q, :n], h[q, :n])), (top_k, q)
    finally:
        r.close()


def test_refusals(tmp_path):
    r, qs = _retriever(tmp_path)
    gate = rs.gate()
    each = [None] * len(qs)
    try:
        for call in (lambda **kw: r.hybrid_search_batch(qs, 10, **kw), lambda **kw: r.get_scores_for_router_batch(qs, 10, **kw),
                     lambda **kw: r.route_batch(qs, gate, 10, **kw)):
            with pytest.raises(ValueError, match="distinct_by does not combine with complete_scores"):
                call(distinct_by="title", complete_scores=True)
            with pytest.raises(ValueError, match="distinct_by does not combine with allowed_ids_each"):
                call(distinct_by="title", allowed_ids_each=each)
            with pytest.raises(ValueError, match="per_group"):
                call(distinct_by="title", per_group=2)
            assert len(call(distinct_by="title", per_group=1)) == len(qs)
        with pytest.raises(ValueError, match="distinct_by does not combine with complete_scores"):          # the per-query call's own words
            r.hybrid_search(qs[0], distinct_by="title", complete_scores=True)
        with pytest.raises(ValueError, match="distinct_by does not combine with complete_scores"):
            r.get_scores_for_router(qs[0], distinct_by="title", complete_scores=True)
        with pytest.raises(ValueError, match="allowed_ids_each"):
            r.dense_search_batch(qs, 10, distinct_by="title", allowed_ids_each=each)
        with pytest.raises(ValueError, match="per_group"):
            r.dense_search_batch(qs, 10, distinct_by="title", per_group=2)
        r.fusion_backend = "gpu"                                                # the device route's refusals apply unchanged
        with pytest.raises(_native.RqError, match="fusion_backend='gpu'"):
            r.hybrid_search_batch(qs, 10, distinct_by="title")
    finally:
        r.close()
