"""Filtered hybrid batches (HybridRetriever.hybrid_search_batch / get_scores_for_router_batch / dense_search_batch with `allowed_ids=` and
`allowed_ids_each=`), the parts that need no GPU: over a host stand-in for NativeIndex, query q of the batch call equals the per-query
call with that query's entry, value for value -- both metrics, complete_scores off and on, pools smaller and larger than top_k --
and the reusable filter, its staleness and the refusals.  The GPU side is tests/test_gpu_hybrid_filtered.py."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle  # noqa: E402


class _StubFilter(_native.RowFilter):
    """Stand-in for an rq_filter of _StubNative: the allowed rows as a boolean array, and the number of rows it was made over."""

    def __init__(self, index, keep):
        self._index, self._h, self.keep, self.count, self.rows, self.closed = index, None, keep, int(keep.sum()), len(index), False

    def close(self):
        self.closed = True


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the dense oracles over the fp16 rows,
    in the manner of tests/test_hybrid.py's, extended by make_filter, the filtered search and search_filtered_each -- query q over the
    rows of filters[q], k_eff = min(k, allowed rows), (0.0, -1) padded (include/rq.h "per-query filters")."""
    device, devices = 0, [0]

    def __init__(self, x, normalize):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), normalize)
        self.dim = self.x16.shape[1]
        self.each_calls = 0

    def __len__(self):
        return self.x16.shape[0]

    def make_filter(self, mask_or_rows):
        keep = np.zeros(len(self), bool)
        keep[np.asarray(mask_or_rows, np.int64)] = True
        return _StubFilter(self, keep)

    def _one(self, q, k, metric, flt):
        out_s, out_r = np.zeros(k, np.float32), np.full(k, -1, np.int64)
        if flt is not None and (flt.closed or flt.rows != len(self) or flt._index is not self):
            raise _native.RqError("rq_search_filtered: the filter is stale, closed or of another index")
        allowed = np.arange(len(self)) if flt is None else np.flatnonzero(flt.keep)
        if len(allowed):
            s, r = orc.topk_from_scores(orc.exact_scores(q[None, :], self.x16[allowed], metric), k)
            n = int((r[0] >= 0).sum())
            out_s[:n], out_r[:n] = s[0][:n], allowed[r[0][:n]]
        return out_s, out_r

    def search(self, q, k, metric=0, *, row_filter=None):
        return self.search_filtered_each(q, k, [row_filter] * np.atleast_2d(q).shape[0], metric, _count=False)

    def search_filtered_each(self, q, k, filters, metric=0, _count=True):
        q = np.atleast_2d(np.asarray(q, np.float32))
        assert len(filters) == q.shape[0]
        self.each_calls += int(_count)
        out = [self._one(q[b], k, metric, filters[b]) for b in range(q.shape[0])]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def score_rows(self, q, rows, metric=0):
        return score_oracle.pairs(q, self.x16, rows, metric)


def _scenario(tmp_path, metric, **keywords):
    """The scenario of tests/test_hybrid.py::_scenario -- documents in both pools, only in the dense index, dense ids the store does not
    know, questions without a BM25 hit, duplicates with tied scores, all-negative dense scores under the inner product -- plus five
    documents that only BM25 holds."""
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    os.makedirs(tmp_path, exist_ok=True)
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(120)]
    texts[30:34] = [texts[5]] * 4
    docs = [si.Document(id=f"p{i}", text=t, title=f"T{i}") for i, t in enumerate(texts)]
    queries = [" ".join(rng.choice(vocab, size=4)) for _ in range(30)] + [texts[5], "nothing known here", texts[110], ""]
    emb = RandomProjectionEmbedder(16)

    class NegEmb:
        dim = 16

        def embed(self, ts):
            return -np.abs(emb.embed(ts))
    vec = emb.embed(texts)
    extra_ids = [f"ghost{i}" for i in range(5)] + [f"donly{i}" for i in range(6)]
    extra_vec = emb.embed([texts[i] + " w1" for i in range(11)])
    if metric == "ip":
        vec, extra_vec = np.abs(vec), np.abs(extra_vec)
    stub = _StubNative(np.concatenate([vec, extra_vec]), normalize=metric == "cosine")
    dense = si.DenseIndex.from_native(stub, [d.id for d in docs] + extra_ids, embedder=NegEmb() if metric == "ip" else emb, metric=metric)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense, **keywords)
    bonly = [si.Document(id=f"bonly{i}", text=" ".join(rng.choice(vocab, size=6))) for i in range(5)]
    r.bm25_index.add_documents(docs[:100] + bonly)
    for d in docs + bonly:
        r.documents[d.id] = d
    for i in range(6):
        r.documents[f"donly{i}"] = si.Document(id=f"donly{i}", text=f"dense only {i}")
    return r, queries


def _entries(n):
    """One entry per query: None, an empty set, a set only BM25 knows, a set only the dense index knows, ids unknown to both, two tenants
    (one of them with unknown ids and ids of every kind), entries shared by object, in a scrambled arrangement."""
    tenant_a = {f"p{i}" for i in range(0, 120, 2)} | {"donly0", "donly1", "bonly0", "ghost1"}
    tenant_b = [f"p{i}" for i in range(20, 60)] + ["nobody1", "donly2", "bonly3", "bonly4"]
    pool = [None, set(), {f"bonly{i}" for i in range(5)}, {f"donly{i}" for i in range(6)} | {f"p{i}" for i in range(100, 120)}, ["nobody1", "nobody2"],
            tenant_a, tenant_b, tenant_a, {"p5", "p30", "p31", "p32", "p33"}]
    order = np.random.default_rng(17).permutation(n * len(pool))[:n] % len(pool)
    each = [pool[int(i)] for i in order]
    assert all(any(e is p for e in each) for p in pool)
    return each


def _values(results):
    return [[(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score, x.text) for x in res] for res in results]


@pytest.mark.parametrize("complete", [False, True], ids=["plain", "complete_scores"])
@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_filtered_batch_calls_equal_the_per_query_calls_value_for_value(tmp_path, metric, complete):
    r, queries = _scenario(tmp_path, metric)
    each = _entries(len(queries))
    restricted = 0
    for top_k, pool in ((10, 50), (20, 7), (100, 100), (3, 1)):
        calls = r.dense_index._index.each_calls
        got = r.hybrid_search_batch(queries, top_k, pool, complete_scores=complete, allowed_ids_each=each)
        assert r.dense_index._index.each_calls == calls + 1                    # one per-query-filtered dense call for the whole batch
        want = [r.hybrid_search(q, top_k, pool, complete_scores=complete, **si._given(allowed_ids=e)) for q, e in zip(queries, each)]
        assert _values(got) == _values(want), (metric, complete, top_k, pool)
        free = r.hybrid_search_batch(queries, top_k, pool, complete_scores=complete)
        restricted += sum(a != b for a, b in zip(_values(got), _values(free)))
        assert all(_values([g]) == _values([f]) for g, f, e in zip(got, free, each) if e is None)
        assert all(g == [] for g, e in zip(got, each) if e is not None and not set(e) & (set(r.bm25_index.doc_ids) | set(r.dense_index._ids)))
        router = r.get_scores_for_router_batch(queries, top_k, retrieval_pool_size=pool, complete_scores=complete, allowed_ids_each=each)
        assert router == [r.get_scores_for_router(q, top_k, retrieval_pool_size=pool, complete_scores=complete, **si._given(allowed_ids=e)) for q, e in zip(queries, each)]
        assert [row[2][:len(g)] for row, g in zip(router, got)] == [[x.doc_id for x in g] for g in got]
    assert restricted > 40
    # one set for the whole batch
    one = each[[i for i, e in enumerate(each) if e is not None and len(e) > 30][0]]
    assert _values(r.hybrid_search_batch(queries, 10, 50, complete_scores=complete, allowed_ids=one)) \
        == _values(r.hybrid_search_batch(queries, 10, 50, complete_scores=complete, allowed_ids_each=[one] * len(queries))) \
        == _values([r.hybrid_search(q, 10, 50, complete_scores=complete, allowed_ids=one) for q in queries])
    assert r.get_scores_for_router_batch(queries, 10, complete_scores=complete, allowed_ids=one) \
        == [r.get_scores_for_router(q, 10, complete_scores=complete, allowed_ids=one) for q in queries]
    # every entry None: the unfiltered call
    assert _values(r.hybrid_search_batch(queries, 10, 50, complete_scores=complete, allowed_ids_each=[None] * len(queries))) \
        == _values(r.hybrid_search_batch(queries, 10, 50, complete_scores=complete))


def test_dense_search_batch_takes_the_keywords(tmp_path):
    r, queries = _scenario(tmp_path, "cosine")
    each = _entries(len(queries))
    want = [r.dense_search(q, 15, **si._given(allowed_ids=e)) for q, e in zip(queries, each)]
    assert r.dense_search_batch(queries, 15, allowed_ids_each=each) == want and want != r.dense_search_batch(queries, 15)
    flt = r.make_filter(each[0] or {"p1", "p2"})
    assert r.dense_search_batch(queries, 15, allowed_ids=flt) == [r.dense_search(q, 15, allowed_ids=flt.ids) for q in queries]
    flt.close()


def test_make_filter_is_reusable_and_goes_stale_after_an_add(tmp_path):
    r, queries = _scenario(tmp_path, "cosine")
    ids = [f"p{i}" for i in range(0, 120, 3)] + ["bonly1", "donly3", "nobody"]
    flt = r.make_filter(ids)
    assert isinstance(flt, si.HybridFilter) and flt.ids == frozenset(ids) and len(flt) == len(ids)
    assert flt.sparse.count == len([d for d in ids if d in set(r.bm25_index.doc_ids)]) and flt.sparse.words.dtype == np.uint32
    assert isinstance(flt.dense, _native.RowFilter) and len(flt.dense) == len([d for d in ids if d in set(r.dense_index._ids)])
    want = _values([r.hybrid_search(q, 10, 50, allowed_ids=ids) for q in queries])
    for _ in range(2):
        assert _values(r.hybrid_search_batch(queries, 10, 50, allowed_ids=flt)) == want
        assert not flt.dense.closed                                            # a caller's own filter is not closed by the call
    other = {"p1", "p2", "p3", "bonly0"}
    mixed = [flt if i % 3 == 0 else (other if i % 3 == 1 else None) for i in range(len(queries))]
    assert _values(r.hybrid_search_batch(queries, 10, 50, complete_scores=True, allowed_ids_each=mixed)) \
        == _values([r.hybrid_search(q, 10, 50, complete_scores=True, **si._given(allowed_ids=None if e is None else (ids if e is flt else other)))
                    for q, e in zip(queries, mixed)])
    assert r.get_scores_for_router_batch(queries, 10, allowed_ids=flt) == [r.get_scores_for_router(q, 10, allowed_ids=ids) for q in queries]
    r.bm25_index.add_documents([si.Document(id="late", text="w1 w2 w3")])
    for call in (lambda: r.hybrid_search_batch(queries, 10, 50, allowed_ids=flt), lambda: r.get_scores_for_router_batch(queries, 10, allowed_ids_each=[flt] + [None] * (len(queries) - 1)),
                 lambda: r.dense_search_batch(queries, 10, allowed_ids=flt)):
        with pytest.raises(_native.RqError, match="stale"):
            call()
    flt.close()
    fresh = r.make_filter(ids)                                                 # made over the grown index: it answers again
    assert _values(r.hybrid_search_batch(queries, 10, 50, allowed_ids=fresh)) == _values([r.hybrid_search(q, 10, 50, allowed_ids=ids) for q in queries])
    fresh.close()


def test_refusals(tmp_path):
    r, queries = _scenario(tmp_path, "cosine")
    B = len(queries)
    bare = r.dense_index.make_filter(["p1", "p2"])
    for call in (r.hybrid_search_batch, r.get_scores_for_router_batch, r.dense_search_batch):
        if call != r.dense_search_batch:                                       # a bare dense filter says nothing about BM25 rows
            with pytest.raises(ValueError, match="RowFilter"):
                call(queries, 5, allowed_ids=bare)
            with pytest.raises(ValueError, match="RowFilter"):
                call(queries, 5, allowed_ids_each=[None] * (B - 1) + [bare])
        with pytest.raises(ValueError, match="allowed_ids_each does not combine with allowed_ids"):
            call(queries, 5, allowed_ids={"p1"}, allowed_ids_each=[None] * B)
        with pytest.raises(ValueError, match="one entry per query"):
            call(queries, 5, allowed_ids_each=[None] * (B + 1))
    assert r.dense_search_batch(queries, 5, allowed_ids=bare) == [r.dense_search(q, 5, allowed_ids=bare) for q in queries]   # the dense call alone takes one
    with pytest.raises(ValueError, match="sparse mask"):
        r.hybrid_search_batch(queries, 5, allowed_ids=r.bm25_index.make_mask(["p1"]))
    # ids made into filters for one call are closed when it returns, and when it raises
    made = []
    make = r.dense_index._index.make_filter
    r.dense_index._index.make_filter = lambda rows: made.append(make(rows)) or made[-1]
    r.hybrid_search_batch(queries, 5, 20, allowed_ids_each=[{"p1", "p2"}] * B)
    assert len(made) == 1 and made[0].closed                                   # one filter for one object
    r.dense_index._index.search_filtered_each = None
    with pytest.raises(TypeError):
        r.hybrid_search_batch(queries, 5, 20, allowed_ids={"p3"})
    assert len(made) == 2 and made[1].closed
