"""Hybrid fusion on the device (include/rq.h rq_hybrid_*, rq_sparse_score_rows*), the parts that need no GPU: the header and the
binding, the host plan (csrc/rq_hybrid_plan.h) under the sanitizers, the yardstick (tests/hybrid_oracle.py) against
HybridRetriever._fuse_batch_rows itself and against BM25Index.score_rows_batch, value for value, and the keyword checks with the loud
failure without a device.  The GPU side is tests/test_gpu_hybrid.py."""
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
import hybrid_oracle as ho  # noqa: E402
import score_oracle  # noqa: E402
import sparse_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_hybrid_create", "rq_hybrid_destroy", "rq_hybrid_get_option", "rq_hybrid_missing_device", "rq_hybrid_missing", "rq_hybrid_fuse_device",
             "rq_hybrid_fuse", "rq_sparse_score_rows_device", "rq_sparse_score_rows"]


def test_header_declares_and_documents_the_hybrid_calls():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES and hasattr(_native.load_library(), name)
    assert re.search(r"#define\s+RQ_HYBRID_MAX_CAND\s+2048", code) and _native.HYBRID_MAX_CAND == 2048 == ho.MAX_CAND
    doc = h[h.index("hybrid fusion: both pools"):h.index("typedef struct rq_hybrid rq_hybrid;")]
    for word in ("KEY SPACE", "INJECTIVE", "known[key]", "dense_row[key]", "COPIED", "sparse pool first", "valid = present and known[key]", "miss_dense", "miss_sparse",
                 "the extra replaces the 0.0", "NaN among them", "0, NaN or infinite", "(b / max_b + d / max_d) / 2", "no fused", "-0.0 as +0.0", "ascending candidate position",
                 "ranks as -inf", "min(valid candidates, top_k)", "(-1, 0.0, 0.0, 0.0)", "no read or write outside", "RQ_SPARSE_MAX_K", "K1 + K2 >= 1", "row offset 0",
                 "One workgroup per query", "64 KiB", "no workspace", "stream order", "without its miss array", "RQ_EINVAL", "RQ_ENODEVICE", "no HIP device",
                 '"fuse_calls"', '"missing_calls"', '"calls"', "Not extended", "MMR"):
        assert word in doc, word
    sparse_doc = h[h.index("sparse search: exact BM25"):h.index("typedef struct rq_sparse rq_sparse;")]
    for word in ("rq_sparse_score_rows_device", "IN QUERY ORDER", "scores 0.0 and reads nothing", "binary search", "no atomics", "RQ_MAX_SCORE_ROWS", "rq_sparse_score_rows:"):
        assert word in sparse_doc, word
    assert "a device form of BM25Index.score_rows" not in h and "fusion of the sparse" not in h           # no longer "Not extended"


def test_plan_and_validation_on_the_host(tmp_path):
    """tests/native/hybrid_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "hybrid_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "hybrid_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- the oracle against _fuse_batch_rows itself ------------------------------------------------------------------------------------------
class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the dense oracles over the fp16 rows."""
    device, devices = 0, [0]

    def __init__(self, x, normalize):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), normalize)
        self.dim = self.x16.shape[1]

    def __len__(self):
        return self.x16.shape[0]

    def search(self, q, k, metric=0, *, row_filter=None):
        q = np.atleast_2d(np.asarray(q, np.float32))
        out_s, out_r = np.zeros((q.shape[0], k), np.float32), np.full((q.shape[0], k), -1, np.int64)
        for b in range(q.shape[0]):
            s, r = orc.topk_from_scores(orc.exact_scores(q[b:b + 1], self.x16, metric), k)
            out_s[b], out_r[b] = s[0], r[0]
        return out_s, out_r

    def score_rows(self, q, rows, metric=0):
        return score_oracle.pairs(q, self.x16, rows, metric)


def _scenario(tmp_path, metric, **keywords):
    """The corpus, stores and questions of test_host_logic.test_batched_fusion_in_row_space_equals_the_per_query_path, rebuilt: documents
    in both pools, only in BM25, only in the dense index, dense ids the store does not know, questions without a BM25 hit, duplicates
    with tied scores, and -- inner product with a negated query -- all-negative dense scores."""
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    os.makedirs(tmp_path, exist_ok=True)
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(120)]
    texts[30:34] = [texts[5]] * 4
    docs = [si.Document(id=f"p{i}", text=t, title=f"T{i}") for i, t in enumerate(texts)]
    queries =[" ".join(rng.choice(vocab, size=4)) for _ in range(30)] + [texts[5], "nothing known here", texts[110], ""]
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
    dense = si.DenseIndex.from_native(stub, [d.id for d in docs] + extra_ids, embedder=NegEmb() if metric == "ip" else emb, metric=metric)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense, **keywords)
    r.bm25_index.add_documents(docs[:100])
    for d in docs:
        r.documents[d.id] = d
    for i in range(6):
        r.documents[f"donly{i}"] = si.Document(id=f"donly{i}", text=f"dense only {i}")
    return r, queries


@pytest.mark.parametrize("complete", [False, True], ids=["plain", "complete_scores"])
@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_oracle_equals_the_host_fusion_value_for_value(tmp_path, metric, complete):
    """hybrid_oracle.fuse over the pools that _fuse_batch_rows draws returns exactly its ids, scores, hybrid scores and counts: both
    metrics, the four (top_k, pool) pairs, complete_scores off and on -- with the miss lists of hybrid_oracle.missing scored by the two
    indexes' own row-scoring calls.  The scenario has no NaN hybrid score (the one place where the two definitions part)."""
    r, queries = _scenario(tmp_path, metric)
    bm, dn = r.bm25_index, r.dense_index
    filled = 0
    for top_k, pool in ((10, 50), (20, 7), (100, 100), (3, 1)):
        ids, b, d, hy, count = r._fuse_batch_rows(queries, top_k, pool, complete)
        assert not np.isnan(hy).any()
        c = r._key_space()
        ks = ho.key_space(c["nb"], c["dense_key"], c["known"])
        assert np.array_equal(ks["dense_row"], c["dense_row"]) and c["injective"]
        sp_rows, sp_scores = bm.search_batch_rows(queries, pool)
        de_scores, de_rows = dn.search_rows_batch(queries, pool)
        extras = {}
        if complete:
            miss_dense, miss_sparse = ho.missing(ks, sp_rows, de_rows)
            extras = {"miss_dense": miss_dense, "extra_dense": dn.score_rows_batch(queries, miss_dense), "miss_sparse": miss_sparse,
                      "extra_sparse": bm.score_rows_batch(queries, miss_sparse)}
            filled += int((miss_dense >= 0).sum()) + int((miss_sparse >= 0).sum())
        keys, ob, od, oh, pos, ocount = ho.fuse(ks, sp_rows, sp_scores, de_rows, de_scores, top_k, **extras)
        assert np.array_equal(ocount, count) and (count > 0).any() and (pool >= top_k or (count < top_k).any())
        live = np.arange(top_k)[None, :] < count[:, None]
        assert np.array_equal(c["ids"][np.where(live, keys, 0)][live], ids[live]) and (keys[~live] == -1).all() and (pos[~live] == -1).all()
        for got, want in ((ob, b), (od, d), (oh, hy)):
            assert got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (metric, complete, top_k, pool)
    assert (filled > 100) == complete


@pytest.mark.parametrize("case", so.cases(), ids=[c["name"] for c in so.cases()])
def test_oracle_scores_rows_as_bm25index_does(case):
    """hybrid_oracle.sparse_score_rows against the full score vector of tests/sparse_oracle.py's definition, bit for bit, on its cases:
    every row of the corpus (in pieces of at most 4 096), rows outside it and repeated rows."""
    ix, q_indptr, q_tokens = case["ix"], case["q_indptr"], case["q_tokens"]
    B, n = len(q_indptr) - 1, ix["n_docs"]
    m = min(n, 4096)
    rows = np.tile(np.concatenate([np.arange(m), [-1, n, n + 7, 0, 0, m - 1]]), (B, 1))
    got = ho.sparse_score_rows(ix, q_indptr, q_tokens, rows)
    assert got.dtype == np.float64 and not got[:, m: m + 3].any() and np.array_equal(got[:, m + 3].view(np.uint64), got[:, 0].view(np.uint64))
    top_rows, top_scores = so.topk(ix, q_indptr, q_tokens, case["k"])
    for b in range(B):                                                      # what the top-k returned is what the row scores
        hit = (top_rows[b] >= 0) & (top_rows[b] < m)
        assert np.array_equal(got[b, top_rows[b][hit]].view(np.uint64), top_scores[b][hit].view(np.uint64))


def test_oracle_row_scores_equal_bm25index_score_rows_batch():
    """... and against BM25Index.score_rows_batch itself over the CSR arrays of a real index, bit for bit: repeated and unknown tokens,
    rows -1, >= n_docs and repeated, before and after an add."""
    rng = np.random.default_rng(11)
    vocab = [f"w{i}" for i in range(40)]
    bm = si.BM25Index()
    bm.add_documents([si.Document(id=f"p{i}", text=" ".join(rng.choice(vocab, size=6))) for i in range(100)])
    queries = [" ".join(rng.choice(vocab, size=4)) for _ in range(12)] + ["w1 w1 w1 w2", "w3 unknowntoken w3 w4 anotherunknown", "w5 " * 9, "unknown only", ""]
    for round_ in range(2):
        n = len(bm)
        rows = rng.integers(-1, n + 3, size=(len(queries), 23))
        rows[:, :3] = rows[:, 3:4]
        c = bm._csr()
        ix = {"indptr": c["indptr"], "rows": c["rows"], "contrib": c["contrib"], "n_tokens": len(c["tid"]), "n_docs": c["n_docs"]}
        q_indptr, q_tokens = so.ragged([[c["tid"][t] for t in bm._tokenize(q) if t in c["tid"]] for q in queries])
        want = bm.score_rows_batch(queries, rows)
        got = ho.sparse_score_rows(ix, q_indptr, q_tokens, rows)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and (want != 0).any() and np.array_equal(bm.score_rows_batch(queries, rows, backend="host"), want)
        bm.add_documents([si.Document(id=f"n{i}", text=" ".join(rng.choice(vocab, size=5))) for i in range(20)])


def test_the_cases_hold_what_they_are_meant_to_hold():
    by = {c["name"]: c for c in ho.cases()}
    assert {sum(np.asarray(c["pools"][i]).shape[1] for i in (0, 2)) for c in by.values()} >= {1, 2, 63, 64, 65, 255, 256, 257, 2048}
    assert {c["pools"][0].shape[0] for c in by.values()} >= {1, 3, 70}
    assert [n for n, c in by.items() if c["native_only"]] == ["nan_hybrid_score"]
    for c in by.values():                                                   # rows within one pool are distinct
        for rows, n in ((c["pools"][0], c["ks"]["nb"]), (c["pools"][2], c["ks"]["n_dense"])):
            for row in np.asarray(rows):
                live = row[(row >= 0) & (row < n)]
                assert len(np.unique(live)) == len(live), c["name"]
    c = by["nan_hybrid_score"]
    keys, b, d, h, pos, count = ho.fuse(c["ks"], *c["pools"], 8)
    assert count[0] == 7 and np.isnan(h[0, 5]) and keys[0, 5] == 0 and h[0, 6] == -np.inf and keys[0, 0] == 1      # the NaN ranks as -inf: before the -inf at a later position
    c = by["tie_run_over_the_boundary"]
    keys, b, d, h, pos, count = ho.fuse(c["ks"], *c["pools"], 7)
    assert (h[0, :7] == 0.5).all() and pos[0, :7].tolist() == [0, 1, 2, 3, 6, 7, 8]                                   # equal h: ascending position, cut inside the run
    c = by["both_pools_first_and_last"]
    keys, b, d, h, pos, count = ho.fuse(c["ks"], *c["pools"], 20)
    assert count.tolist() == [18, 18] and (pos[:, :18] != 10).all() and (pos[:, :18] != 19).all() and d[0][pos[0] == 0][0] == np.float32(0.9) and d[1][pos[1] == 9][0] == np.float32(0.9)
    c = by["count12_topk_at_and_above"]
    assert [ho.fuse(c["ks"], *c["pools"], k)[5].tolist() for k in (11, 12, 13)] == [[11] * 3, [12] * 3, [12] * 3]
    c = by["negative_dense_scores"]
    assert (c["pools"][3][c["pools"][2] >= 0] < 0).all()
    c = by["inf_sparse_score"]
    assert np.isinf(ho.fuse(c["ks"], *c["pools"], 1)[3]).any()
    md, ms = ho.missing(by["n200_100x100_b70"]["ks"], by["n200_100x100_b70"]["pools"][0], by["n200_100x100_b70"]["pools"][2])
    assert (md >= 0).sum() > 100 and (ms >= 0).sum() > 100 and ((md == -1) & (by["n200_100x100_b70"]["pools"][0] >= 0)).any()
    e = ho.extras_for(by["n200_100x100_b70"])
    assert not ho.same(ho.fuse(by["n200_100x100_b70"]["ks"], *by["n200_100x100_b70"]["pools"], 10, **e), ho.fuse(by["n200_100x100_b70"]["ks"], *by["n200_100x100_b70"]["pools"], 10))


# ---- keywords ------------------------------------------------------------------------------------------------------------------------------
def test_fusion_backend_keyword_is_checked_and_host_is_the_default(tmp_path):
    with pytest.raises(ValueError, match="fusion_backend"):
        si.HybridRetriever(bm25_persist_path=None, dense_index=object(), fusion_backend="cuda")
    r, queries = _scenario(tmp_path, "cosine")
    assert r.fusion_backend == "host" and r.sparse_backend == "host"
    bm = r.bm25_index
    with pytest.raises(ValueError, match="backend"):
        bm.score_rows_batch(queries[:2], np.zeros((2, 3), np.int64), backend="cuda")
    assert si.BM25Index().score_rows_batch(["w1"], [[0, 1]], backend="gpu").tolist() == [[0.0, 0.0]]              # the empty-index return stays
    assert r._key_space()["injective"]                                                                            # an id held twice is seen once per rebuild
    r.dense_index._ids.append(r.dense_index._ids[4])                                                              # (the stamp changes: a rebuild)
    assert not r._key_space()["injective"]


def test_no_device_means_loud_failure_not_fallback(tmp_path):
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    r, queries = _scenario(tmp_path, "cosine", fusion_backend="gpu", sparse_backend="gpu")
    with pytest.raises(_native.RqError, match="fusion_backend='gpu'.*no HIP device"):
        r.hybrid_search_batch(queries, top_k=5, retrieval_pool_size=10)
    with pytest.raises(_native.RqError, match="fusion_backend='gpu'"):
        r.get_scores_for_router_batch(queries, num_passages=5, complete_scores=True)
    host, _ = _scenario(tmp_path / "h", "cosine")
    auto, _ = _scenario(tmp_path / "a", "cosine", fusion_backend="auto", sparse_backend="auto")
    assert auto.hybrid_search_batch(queries, top_k=5, retrieval_pool_size=10) == host.hybrid_search_batch(queries, top_k=5, retrieval_pool_size=10)
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        r.bm25_index.score_rows_batch(queries[:2], np.zeros((2, 3), np.int64), backend="gpu")
    want = host.bm25_index.score_rows_batch(queries[:2], np.array([[0, 5, -1], [7, 7, 200]]))
    assert np.array_equal(host.bm25_index.score_rows_batch(queries[:2], np.array([[0, 5, -1], [7, 7, 200]]), backend="auto"), want)
    ks = ho.cases()[0]["ks"]
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        _native.HybridMap(ks["nb"], ks["dense_key"], ks["known"])
    with pytest.raises(_native.RqError, match="injective"):                                                       # refused before the device is looked for
        _native.HybridMap(4, np.array([1, 1], np.int64), np.ones(6, bool))
    with pytest.raises(_native.RqError, match="outside"):
        _native.HybridMap(4, np.array([1, 6], np.int64), np.ones(6, bool))
    lib = _native.load_library()
    assert lib.rq_hybrid_fuse(None, None, None, None, None, 1, 1, 1, None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert lib.rq_hybrid_missing(None, None, None, 1, 1, 1, None, None) == -1 and lib.rq_sparse_score_rows(None, None, None, 1, None, 1, None) == -1
    assert lib.rq_hybrid_get_option(None, b"calls") == -1.0
    lib.rq_hybrid_destroy(None)
