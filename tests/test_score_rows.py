"""Scoring given rows (rq_score_rows) and completed hybrid pools, the parts that need no GPU: the header's documentation, the loud
failure without a device, the binding's argument checks, the host plan (csrc/rq_score_plan.h) under the sanitizers,
BM25Index.score_rows against get_scores bit for bit, and `complete_scores` on the Python seam over a stub dense backend whose
score_rows is the oracle (tests/score_oracle.py).  The GPU side is tests/test_gpu_score_rows.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_score_rows_device", "rq_score_rows"]


def test_header_documents_both_calls_and_both_options():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
    assert re.search(r"#define RQ_MAX_SCORE_ROWS 65536\b", code) and _native.MAX_SCORE_ROWS == 65536
    assert re.search(r"rq_score_rows_device\(rq_index\* idx, const float\* d_queries, int B, const int64_t\* d_rows, int m, int metric,\s*float\* d_scores, void\* stream\)", code)
    assert re.search(r"rq_score_rows\(rq_index\* idx, const float\* queries, int B, const int64_t\* rows, int m, int metric, float\* out_scores\)", code)
    doc = h[h.index("scoring given rows"):h.index("int rq_score_rows_device(")]
    for word in ('"score_calls"', '"score_pairs"', "absent entry", "-1 included", "0.0", "Duplicates are allowed", "need not be sorted", "GLOBAL rows", "row_offset",
                 "empty index", "STORED fp16 row", "-inf", "zero-norm query", "same bits", "gather route", "rq_search", '"pipeline" = 0', "stream order",
                 "defers nothing", "no bin records", "index's own stream", "B x dim x 4 + B x m x 12", "RQ_ENOMEM", "RQ_EINVAL", "1 <= B <= 65535",
                 "1 <= m <= RQ_MAX_SCORE_ROWS", "RQ_EUNSUPPORTED", "multi-device", "RQ_ENODEVICE", "rq_search_train_device", "hints", '"pipeline" 1 and 2',
                 "rq_timing is untouched", "B x m per call"):
        assert word in doc, word


def test_calls_fail_loudly_without_a_device_or_with_null_arguments():
    lib = _native.load_library()
    want = -2 if _native.device_count() == 0 else -1                  # RQ_ENODEVICE / RQ_EINVAL
    buf = np.zeros(8, np.float32)
    rows = np.zeros(8, np.int64)
    for call in (lambda: lib.rq_score_rows_device(None, _native._ptr(buf), 1, _native._ptr(rows), 4, 0, _native._ptr(buf), None),
                 lambda: lib.rq_score_rows(None, _native._ptr(buf), 1, _native._ptr(rows), 4, 0, _native._ptr(buf))):
        assert call() == want
        if want == -2:
            assert "RQ_ENODEVICE" in _native.last_error() and "no CPU fallback" in _native.last_error()
        else:
            assert "null argument" in _native.last_error()
    if _native.device_count() == 0:
        with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
            _native.NativeIndex(768, 0)


class _NoLibrary(_native.NativeIndex):
    """A NativeIndex whose library must not be reached: argument errors are raised before it is called."""

    def __init__(self, dim):
        self.dim = dim
        self._h = None

        class _Boom:
            def __getattr__(self, name):
                raise AssertionError(f"the library was called ({name})")
        self._lib = _Boom()

    def close(self):
        pass


def test_python_refuses_bad_shapes_and_sizes_before_the_library_is_called():
    idx = _NoLibrary(8)
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="queries"):
        idx.score_rows(np.zeros((2, 9), np.float32), np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match="queries"):
        idx.score_rows(np.zeros((2, 2, 8), np.float32), np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match="one list per query"):
        idx.score_rows(q, np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError, match="one list per query"):
        idx.score_rows(q, np.zeros((2, 3, 1), np.int64))
    with pytest.raises(ValueError, match="integers"):
        idx.score_rows(q, np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="m 0"):
        idx.score_rows(q, np.zeros((2, 0), np.int64))
    with pytest.raises(ValueError, match="m 65537"):
        idx.score_rows(q, np.zeros((2, _native.MAX_SCORE_ROWS + 1), np.int64))
    with pytest.raises(ValueError, match="metric"):
        idx.score_rows(q, np.zeros((2, 3), np.int64), metric=2)
    with pytest.raises(ValueError, match="B 0"):
        idx.score_rows(np.zeros((0, 8), np.float32), np.zeros((0, 3), np.int64))
    for B, m, metric in ((0, 4, 0), (65536, 4, 0), (1, 0, 0), (1, _native.MAX_SCORE_ROWS + 1, 0), (1, 4, -1), (1, 4, 2)):
        with pytest.raises(ValueError):
            idx.score_rows_device(1, B, 2, m, metric, 3)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_takes_exact_scores_along_the_lists():
    x16 = orc.synthetic_corpus(200, 48, seed=5)
    x16[7] = 0
    x16[9, 3] = np.float16(np.inf)
    q = orc.synthetic_queries(3, 48, seed=6)
    q[2] = 0
    rows = np.array([[0, 7, 9, 199, 200, -1, 7, 5], [5, 5, 5, 150, 9, 1000, -7, 0], [9, 7, 0, 1, 2, 3, 4, 5]], np.int64)
    for metric in (orc.METRIC_COSINE, orc.METRIC_IP):
        with np.errstate(invalid="ignore", over="ignore"):
            full = orc.exact_scores(q, x16, metric)
        got = so.pairs(q, x16, rows, metric)
        for b in range(3):
            for j, r in enumerate(rows[b]):
                want = 0.0 if not 0 <= r < 200 else (-np.inf if np.isnan(full[b, r]) else full[b, r])
                assert got[b, j] == np.float32(want) or abs(float(got[b, j]) - float(want)) <= 1e-7, (metric, b, j)
        assert got[0, 1] == 0.0 and got[0, 4] == 0.0 and got[0, 5] == 0.0
        shifted = so.pairs(q, x16, rows + 1000, metric, row_offset=1000)
        assert np.array_equal(shifted.view(np.uint32), got.view(np.uint32))
        assert not so.pairs(q, x16, rows, metric, row_offset=1000)[:2, :5].any()          # everything below the offset is absent
    assert so.pairs(q, x16, rows)[0, 2] == -np.inf                                        # cosine against a row that holds an inf: NaN -> -inf
    assert not so.pairs(q, x16[:0], rows).any()


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------
def test_plan_and_argument_checks_on_the_host(tmp_path):
    """tests/native/score_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "score_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "score_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- BM25Index.score_rows ------------------------------------------------------------------------------------------------------
def _fusion_corpus():
    """The corpus and questions of test_host_logic.test_batched_fusion_in_row_space_equals_the_per_query_path."""
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(120)]
    texts[30:34] = [texts[5]] * 4
    docs = [si.Document(id=f"p{i}", text=t, title=f"T{i}") for i, t in enumerate(texts)]
    queries = [" ".join(rng.choice(vocab, size=4)) for _ in range(30)] + [texts[5], "nothing known here", texts[110], ""]
    return vocab, texts, docs, queries


def test_bm25_score_rows_equals_get_scores_bit_for_bit():
    vocab, texts, docs, queries = _fusion_corpus()
    b = si.BM25Index()
    assert b.score_rows("w1 w2", [0, -1, 5]).tolist() == [0.0, 0.0, 0.0]                  # an empty index
    b.add_documents(docs[:100])
    rng = np.random.default_rng(11)
    queries = queries + ["w1 w1 w1 w2", "w3 unknowntoken w3 w4 anotherunknown", "w5 " * 9, "unknown only"]     # repeated and unknown tokens
    for round_ in range(2):
        n = len(b)
        lists = [np.arange(n), np.arange(n)[::-1], rng.integers(-1, n, size=57), np.array([-1, 5, 5, 30, 31, -1, 5, n - 1, 0, -5, n, n + 7]),
                 np.zeros(0, np.int64), np.full(4, -1)]
        for q in queries:
            full = b.get_scores(b._tokenize(q))
            for rows in lists:
                rows = np.asarray(rows, np.int64)
                want = np.where((rows >= 0) & (rows < n), full[np.clip(rows, 0, n - 1)], 0.0)
                got = b.score_rows(q, rows)
                assert got.dtype == np.float64 and got.shape == rows.shape
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (round_, q)
        rows = rng.integers(-1, n, size=(len(queries), 23))
        got = b.score_rows_batch(queries, rows)
        want = np.stack([np.where(rows[i] >= 0, b.get_scores(b._tokenize(q))[np.maximum(rows[i], 0)], 0.0) for i, q in enumerate(queries)])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert any((got[i] != 0).any() for i in range(len(queries)))
        b.add_documents(docs[100:])                                                        # again after an add: idf and avgdl changed
    with pytest.raises(ValueError):
        b.score_rows_batch(queries, np.zeros((2, 3), np.int64))


# ---- complete_scores on the Python seam ------------------------------------------------------------------------------------------
class _StubFilter:
    def __init__(self, rows):
        self.rows = np.unique(np.asarray(rows, np.int64))
        self.count = int(self.rows.size)

    def close(self):
        pass


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the oracles over the fp16 rows."""
    device, devices = 0, [0]

    def __init__(self, x, normalize):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), normalize)
        self.dim = self.x16.shape[1]
        self.score_calls = []

    def __len__(self):
        return self.x16.shape[0]

    def make_filter(self, rows):
        return _StubFilter(rows)

    def search(self, q, k, metric=0, *, row_filter=None):
        q = np.atleast_2d(np.asarray(q, np.float32))                    # one query at a time, as the oracle scores: the same bits in a batch
        out_s, out_r = np.zeros((q.shape[0], k), np.float32), np.full((q.shape[0], k), -1, np.int64)
        keep = np.arange(len(self)) if row_filter is None else row_filter.rows
        for b in range(q.shape[0]):
            s, r = orc.topk_from_scores(orc.exact_scores(q[b:b + 1], self.x16, metric)[:, keep], k)
            out_s[b], out_r[b] = s[0], np.where(r[0] >= 0, keep[np.maximum(r[0], 0)], -1)
        return out_s, out_r

    def score_rows(self, q, rows, metric=0):
        self.score_calls.append(np.asarray(rows).shape)
        return so.pairs(q, self.x16, rows, metric)


def _retriever(tmp_path, metric):
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    vocab, texts, docs, queries = _fusion_corpus()
    emb = RandomProjectionEmbedder(16)

    class NegEmb:
        dim = 16
        def embed(self, ts): return -np.abs(emb.embed(ts))
    vec = emb.embed(texts)
    extra_ids = [f"ghost{i}" for i in range(5)] + [f"donly{i}" for i in range(6)]
    extra_vec = emb.embed([texts[i] + " w1" for i in range(11)])
    if metric == "ip":
        vec, extra_vec = np.abs(vec), np.abs(extra_vec)
    stub = _StubNative(np.concatenate([vec, extra_vec]), normalize=metric == "cosine")
    q_emb = NegEmb() if metric == "ip" else emb
    dense = si.DenseIndex.from_native(stub, [d.id for d in docs] + extra_ids, embedder=q_emb, metric=metric)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    r.bm25_index.add_documents(docs[:100])
    for d in docs:
        r.documents[d.id] = d
    for i in range(6):
        r.documents[f"donly{i}"] = si.Document(id=f"donly{i}", text=f"dense only {i}")
    return r, stub, q_emb, queries


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_complete_scores_fills_in_the_full_corpus_scores(tmp_path, monkeypatch, metric):
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    r, stub, q_emb, queries = _retriever(tmp_path, metric)
    dense, bm = r.dense_index, r.bm25_index
    m = _native.METRIC_IP if metric == "ip" else _native.METRIC_COSINE
    filled_d = filled_b = 0
    for num, pool in ((10, 50), (20, 7), (100, 100), (3, 1)):
        plain = [r.hybrid_search(q, top_k=num, retrieval_pool_size=pool) for q in queries]
        assert [r.hybrid_search(q, top_k=num, retrieval_pool_size=pool, complete_scores=False) for q in queries] == plain
        assert r.hybrid_search_batch(queries, top_k=num, retrieval_pool_size=pool, complete_scores=False) == r.hybrid_search_batch(queries, top_k=num, retrieval_pool_size=pool)
        assert r.get_scores_for_router_batch(queries, num, retrieval_pool_size=pool, complete_scores=False) == r.get_scores_for_router_batch(queries, num, retrieval_pool_size=pool)
        assert [r.get_scores_for_router(q, num, retrieval_pool_size=pool, complete_scores=False) for q in queries] == \
               [r.get_scores_for_router(q, num, retrieval_pool_size=pool) for q in queries]
        stub.score_calls.clear()
        got_batch = r.hybrid_search_batch(queries, top_k=num, retrieval_pool_size=pool, complete_scores=True)
        assert len(stub.score_calls) <= 1 and all(s[0] == len(queries) for s in stub.score_calls)             # ONE scoring call for the batch
        got = [r.hybrid_search(q, top_k=num, retrieval_pool_size=pool, complete_scores=True) for q in queries]
        assert got_batch == got, (num, pool)                                                                   # batch = per query, value for value
        want_router = [r.get_scores_for_router(q, num, retrieval_pool_size=pool, complete_scores=True) for q in queries]
        got_router = r.get_scores_for_router_batch(queries, num, retrieval_pool_size=pool, complete_scores=True)
        assert [tuple(g) for g in got_router] == [tuple(w) for w in want_router], (num, pool)
        for q, res, (rb, rd, rid, _) in zip(queries, got, want_router):
            assert rid[:len(res)] == [x.doc_id for x in res] and rb[:len(res)] == [x.bm25_score for x in res] and rd[:len(res)] == [x.dense_score for x in res]
            full_d = so.pairs(q_emb.embed([q]), stub.x16, np.arange(len(stub))[None, :], m)[0].astype(np.float64)
            full_b = bm.get_scores(bm._tokenize(q))
            plain_ids = {x.doc_id: x for x in r.hybrid_search(q, top_k=10 ** 6, retrieval_pool_size=pool)}
            for x in res:
                assert x.dense_score == full_d[dense._row_of[x.doc_id]], (q, x.doc_id)                       # every passage here is in the dense index
                row = bm._row_of_id().get(x.doc_id)
                assert x.bm25_score == (full_b[row] if row is not None else 0.0), (q, x.doc_id)              # not held by BM25: stays 0.0
                filled_d += plain_ids[x.doc_id].dense_score == 0.0 and x.dense_score != 0.0
                filled_b += plain_ids[x.doc_id].bm25_score == 0.0 and x.bm25_score != 0.0
            assert set(x.doc_id for x in res) <= set(plain_ids)                                              # the same candidates: nothing is added to the union
    assert filled_d > 50 and filled_b > 50                                                                     # (the case list really had scores to fill in)
    # allowed_ids: both pools hold allowed ids only, so do the completed results
    allowed = [f"p{i}" for i in range(0, 120, 3)] + ["donly1", "ghost2", "nobody"]
    res = r.hybrid_search(queries[0], top_k=50, retrieval_pool_size=20, allowed_ids=allowed, complete_scores=True)
    assert res and {x.doc_id for x in res} <= set(allowed)
    assert {x.doc_id for x in res} == {x.doc_id for x in r.hybrid_search(queries[0], top_k=50, retrieval_pool_size=20, allowed_ids=allowed)}
    full_d = so.pairs(q_emb.embed([queries[0]]), stub.x16, np.arange(len(stub))[None, :], m)[0].astype(np.float64)
    assert all(x.dense_score == full_d[dense._row_of[x.doc_id]] for x in res)


def test_dense_index_scores_vectors_rows_and_ids(tmp_path):
    r, stub, q_emb, queries = _retriever(tmp_path, "cosine")
    dense = r.dense_index
    qv = q_emb.embed(queries[:3])
    rows = np.array([[0, 5, -1, 130, 131, 5], [1, 2, 3, 4, 5, 6], [-1, -1, -1, -1, -1, -1]], np.int64)
    want = so.pairs(qv, stub.x16, rows)
    assert np.array_equal(dense.score_vectors(qv, rows).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dense.score_rows_batch(queries[:3], rows).view(np.uint32), want.view(np.uint32))
    ids = ["p5", "nobody", "donly0", "p0", "p5"]
    got = dense.score_ids(queries[0], ids)
    assert isinstance(got, list) and got[1] == 0.0 and got[0] == got[4] == float(want[0, 1]) and got[3] == float(want[0, 0])
    assert got[2] == float(so.pairs(qv[:1], stub.x16, [[125]])[0, 0])
    found = {d: s for d, s, _ in dense.search(queries[0], 131)}
    assert all(got[i] == found[d] for i, d in enumerate(ids) if d in found)                # what a search reports for that passage
    assert dense.score_ids(queries[0], []) == []
    with pytest.raises(ValueError):
        dense.score_vectors(qv, rows[:2])
    with pytest.raises(ValueError):
        dense.score_vectors(np.zeros((3, 15), np.float32), rows)
    empty = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32), True), [], embedder=q_emb)
    assert empty.score_ids("anything", ["a", "b"]) == [0.0, 0.0] and not empty.score_vectors(qv, rows).any() and not empty.score_rows_batch(queries[:3], rows).any()

    class _Multi(_StubNative):
        devices = [0, 0]
    multi = si.DenseIndex.from_native(_Multi(stub.x16.astype(np.float32), True), dense._ids, embedder=q_emb)
    for call in (lambda: multi.score_vectors(qv, rows), lambda: multi.score_rows_batch(queries[:3], rows), lambda: multi.score_ids("w1", ["p1"])):
        with pytest.raises(_native.RqError, match="need a single-device index"):
            call()
