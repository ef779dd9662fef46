"""Which device-form native calls the batch calls of HybridRetriever make on the device route (sparse_backend, fusion_backend and
router_backend "gpu"), in which order and with which arguments, for every combination of the restricting keywords: recording wrappers
over _native.NativeIndex, SparseIndex, HybridMap and RouterGate call through to the real methods.  The expected sequences are written
out; a fixup depends on the data, so sequences are compared without them, and every fixup that did occur must follow its own search
directly (only search_flush_device may sit between a plain search and its fixup) with the same B, k, filter and stream.  Every case also
equals the host route value for value (the comparisons of tests/test_gpu_hybrid_grouped.py).  tests/test_hybrid_dispatch.py pins the
host side over stand-ins."""
import inspect
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import router_scenario as rs  # noqa: E402

pytestmark = pytest.mark.gpu

N, B, POOL, TOP = 48, 3, 8, 5
WRAPPED = {
    "NativeIndex": ("search_device", "search_fixup_device", "search_flush_device", "search_filtered_each_device", "search_filtered_each_fixup_device",
                    "search_grouped_device", "search_grouped_fixup_device", "score_rows_device"),
    "SparseIndex": ("topk_device", "topk_grouped_device", "score_rows_device"),
    "HybridMap": ("missing_device", "fuse_device", "fuse_grouped_device"),
    "RouterGate": ("rerank_device",),
}
SIZES = ("B", "k", "K1", "K2", "top_k", "P", "top_r", "m")
EXTRA = ("d_miss_dense", "d_extra_dense", "d_miss_sparse", "d_extra_sparse")
FIXUP_OF = {"NativeIndex.search_fixup_device": "NativeIndex.search_device", "NativeIndex.search_filtered_each_fixup_device": "NativeIndex.search_filtered_each_device",
            "NativeIndex.search_grouped_fixup_device": "NativeIndex.search_grouped_device"}


def _recorder(log, cls, name):
    real = getattr(cls, name)
    signature = inspect.signature(real)

    def call(self, *args, **keywords):
        given = signature.bind(self, *args, **keywords)
        given.apply_defaults()
        p = given.arguments
        rec = {"fn": f"{cls.__name__}.{name}", "stream": p["stream"], **{s: int(p[s]) for s in SIZES if s in p}}
        if "d_mask_of" in p:
            rec["masks"] = (p["d_masks"] is not None, p["d_mask_of"] is not None)
        if "row_filter" in p:
            rec["row_filter"] = p["row_filter"]
        if "filters" in p:
            rec["filters"] = list(p["filters"])
        if name == "fuse_device":
            rec["extra"] = [e for e in EXTRA if p[e] is not None]
        log.append(rec)
        return real(self, *args, **keywords)
    return call


@pytest.fixture
def scene(tmp_path, monkeypatch):
    """One retriever with every backend "gpu" over 48 passages of four titles, its gate, the log of the wrapped calls and the filters
    `make_filter` made."""
    rng = np.random.default_rng(9)
    docs = [si.Document(id=f"p{i}", text=rs._words(rng, 12, 31), title=f"T{i % 4}") for i in range(N)]
    questions = [rs._words(rng, 2, 8) for _ in range(B)]
    log, made = [], []
    for cls, names in WRAPPED.items():
        for name in names:
            monkeypatch.setattr(getattr(_native, cls), name, _recorder(log, getattr(_native, cls), name))
    r = rs.retriever(tmp_path, sparse_backend="gpu", fusion_backend="gpu", router_backend="gpu")
    gate = rs.gate()
    make = r.make_filter
    monkeypatch.setattr(r, "make_filter", lambda ids: made.append(make(ids)) or made[-1])
    yield r, gate, docs, questions, log, made
    gate.close()
    r.close()


def _rows(out):
    return [[(x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score) for x in res] for res in out]


def _strip(log):
    """The log without the fixups, and without stream and filter objects: what the literals below spell out."""
    return [{k: v for k, v in rec.items() if k not in ("stream", "row_filter", "filters")} for rec in log if rec["fn"] not in FIXUP_OF]


def _check_log(log):
    """One stream -- torch's current one -- for every call, and every fixup right behind its own search with that search's arguments."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    assert log and all(rec["stream"] == stream for rec in log), [rec["stream"] for rec in log]
    for i, rec in enumerate(log):
        if rec["fn"] in FIXUP_OF:
            j = i - 1
            if rec["fn"] == "NativeIndex.search_fixup_device" and log[j]["fn"] == "NativeIndex.search_flush_device":
                j -= 1
            search = log[j]
            assert j >= 0 and search["fn"] == FIXUP_OF[rec["fn"]], (i, [x["fn"] for x in log])
            assert {k: v for k, v in search.items() if k != "fn"} == {k: v for k, v in rec.items() if k != "fn"}, (search, rec)


def _on_host(r, run):
    r.sparse_backend = r.fusion_backend = r.router_backend = "host"
    try:
        return run()
    finally:
        r.sparse_backend = r.fusion_backend = r.router_backend = "gpu"


def _sparse(grouped=False, masks=(False, False), k=POOL):
    return dict(fn="SparseIndex.topk_grouped_device" if grouped else "SparseIndex.topk_device", B=B, k=k, masks=masks)


def _fuse(grouped=False, extra=(), K1=POOL, K2=POOL):
    if grouped:
        return dict(fn="HybridMap.fuse_grouped_device", B=B, K1=K1, K2=K2, top_k=TOP)
    return dict(fn="HybridMap.fuse_device", B=B, K1=K1, K2=K2, top_k=TOP, extra=list(extra))


PLAIN_DENSE = [dict(fn="NativeIndex.search_device", B=B, k=POOL), dict(fn="NativeIndex.search_flush_device")]
COMPLETIONS = [dict(fn="HybridMap.missing_device", B=B, K1=POOL, K2=POOL), dict(fn="NativeIndex.score_rows_device", B=B, m=POOL),
               dict(fn="SparseIndex.score_rows_device", B=B, m=POOL)]
RERANK = dict(fn="RouterGate.rerank_device", B=B, P=TOP, top_r=3)
EVEN = [f"p{i}" for i in range(0, N, 2)]
SEQUENCES = {   # case -> (keywords, the calls of ONE batch call without fixups)
    "plain": ({}, [_sparse()] + PLAIN_DENSE + [_fuse()]),
    "complete_scores": (dict(complete_scores=True), [_sparse()] + PLAIN_DENSE + COMPLETIONS + [_fuse(extra=EXTRA)]),
    "allowed_ids_each": (dict(allowed_ids_each=[None, EVEN, EVEN]), [_sparse(masks=(True, True)), dict(fn="NativeIndex.search_filtered_each_device", B=B, k=POOL), _fuse()]),
    "distinct_by": (dict(distinct_by="title"), [_sparse(True), dict(fn="NativeIndex.search_grouped_device", B=B, k=POOL), _fuse(True)]),
    "distinct_by+allowed_ids": (dict(distinct_by="title", allowed_ids=EVEN),
                                [_sparse(True, (True, True)), dict(fn="NativeIndex.search_grouped_device", B=B, k=POOL), _fuse(True)]),
}


def _check_filters(case, log, made):
    """The filters the dense search was handed are the ones made for this call, one per distinct object of ids, closed by now."""
    if case == "allowed_ids_each":
        (flt,) = made
        (rec,) = [x for x in log if x["fn"] == "NativeIndex.search_filtered_each_device"]
        assert rec["filters"][0] is None and isinstance(rec["filters"][1], _native.RowFilter) and rec["filters"][1] is rec["filters"][2]
        assert flt.dense is None and flt.sparse is not None           # (closed: HybridFilter.close drops the dense half it closed)
    elif case == "distinct_by+allowed_ids":
        (flt,) = made
        (rec,) = [x for x in log if x["fn"] == "NativeIndex.search_grouped_device"]
        assert isinstance(rec["row_filter"], _native.RowFilter) and flt.dense is None
    else:
        assert not made and all(x.get("row_filter") is None and "filters" not in x for x in log)


@pytest.mark.parametrize("case", list(SEQUENCES))
def test_hybrid_batch_calls_on_the_device_route(scene, case):
    r, gate, docs, questions, log, made = scene
    r.add_documents(docs)
    keywords, want = SEQUENCES[case]
    got = r.hybrid_search_batch(questions, TOP, POOL, **keywords)
    _check_log(log)
    assert _strip(log) == want, [x["fn"] for x in log]
    _check_filters(case, log, made)
    del log[:], made[:]
    cols = r.get_scores_for_router_batch(questions, TOP, retrieval_pool_size=POOL, **keywords)
    _check_log(log)
    assert _strip(log) == want, [x["fn"] for x in log]                  # the fused rows are asked for once per call
    _check_filters(case, log, made)
    del log[:], made[:]
    host, host_cols = _on_host(r, lambda: (r.hybrid_search_batch(questions, TOP, POOL, **keywords), r.get_scores_for_router_batch(questions, TOP, retrieval_pool_size=POOL, **keywords)))
    assert not log
    assert _rows(got) == _rows(host) and sum(len(x) for x in host) > B and [tuple(c) for c in cols] == [tuple(c) for c in host_cols]


@pytest.mark.parametrize("case", ["plain", "allowed_ids_each"])
def test_route_batch_on_the_device_route(scene, case):
    r, gate, docs, questions, log, made = scene
    r.add_documents(docs)
    keywords, want = SEQUENCES[case]
    run = lambda: r.route_batch(questions, gate, 3, num_passages=TOP, retrieval_pool_size=POOL, return_weights=True, **keywords)
    got, got_w = run()
    _check_log(log)
    assert _strip(log) == want + [RERANK], [x["fn"] for x in log]
    _check_filters(case, log, made)
    del log[:], made[:]
    host, host_w = _on_host(r, run)
    assert not log and rs.separated(host) and sum(len(x) for x in host) > B
    a, e = _rows(got), _rows(host)
    assert [[x[:3] for x in res] for res in a] == [[x[:3] for x in res] for res in e]          # ids, b, d and the order
    np.testing.assert_allclose(got_w, host_w, rtol=0, atol=2e-6)                                 # (the bound of tests/test_router.py)
    for ra, re_ in zip(a, e):
        for x, y in zip(ra, re_):
            mag = abs(x[1]) + abs(x[2])
            assert abs(x[3] - y[3]) <= 2e-6 * mag + 4 * 2.0 ** -53 * mag, (x, y)


def test_a_dense_index_without_rows_and_a_pool_above_the_row_count(scene):
    r, gate, docs, questions, log, made = scene
    r.bm25_index.add_documents(docs)                                     # the dense index holds nothing: no dense call at all, K2 = 0
    for d in docs:
        r.documents[d.id] = d
    for keywords, want in (({}, [_sparse(), _fuse(K2=0)]),
                           (dict(complete_scores=True), [_sparse(), dict(fn="HybridMap.missing_device", B=B, K1=POOL, K2=0), _fuse(K2=0)])):
        del log[:]
        got = r.hybrid_search_batch(questions, TOP, POOL, **keywords)
        _check_log(log)
        assert _strip(log) == want and len(log) == len(want), [x["fn"] for x in log]
        del log[:]
        host = _on_host(r, lambda: r.hybrid_search_batch(questions, TOP, POOL, **keywords))
        assert _rows(got) == _rows(host) and sum(len(x) for x in host) > B and all(x.dense_score == 0.0 for res in host for x in res)
    r.dense_index.add_documents(docs)                                    # 48 rows, a pool of 100: the sparse pool is padded, the dense k is the row count
    del log[:]
    got = r.hybrid_search_batch(questions, TOP, 100)
    _check_log(log)
    assert _strip(log) == [_sparse(k=100), dict(fn="NativeIndex.search_device", B=B, k=N), dict(fn="NativeIndex.search_flush_device"), _fuse(K1=100, K2=N)]
    del log[:]
    assert _rows(got) == _rows(_on_host(r, lambda: r.hybrid_search_batch(questions, TOP, 100))) and not made
