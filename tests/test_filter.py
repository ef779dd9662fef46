"""Filtered searches, the parts that need no GPU: the route rule (csrc/rq_filter_plan.h, on the host), the bitmap the binding
packs, the header's documentation, the loud failure without a device, and the Python seam -- `allowed_ids` to rows on the dense
side, masked BM25 scores on the sparse side -- over a stub dense backend.  The GPU side is tests/test_gpu_filter.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import bm25_oracle
from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_filter_create", "rq_filter_create_device", "rq_filter_count", "rq_filter_destroy", "rq_search_filtered",
             "rq_search_filtered_device", "rq_search_fixup_filtered_device"]


def test_route_rule_on_the_host(tmp_path):
    """tests/native/filter_plan_check.cpp: the four routes, the boundaries of each rule, never the scan route with fewer than k
    occupied partitions, nothing written to the index -- as a stand-alone host program under the address and UB sanitizers (host code only: the flags are
    given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "filter_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "filter_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 70, 4101])
def test_bitmap_packing_matches_the_c_bit_order(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.4
    words = _native.pack_row_mask(mask, n)
    assert words.dtype == np.uint32 and words.flags.c_contiguous and words.size == (n + 31) // 32
    assert np.array_equal(words, fo.pack_bits_reference(mask))
    rows = np.flatnonzero(mask)
    assert np.array_equal(_native.pack_row_mask(rows[::-1], n), words)                       # row numbers, any order
    assert np.array_equal(_native.pack_row_mask(np.concatenate([rows, rows]), n), words)    # duplicates are harmless
    if n:
        with pytest.raises(ValueError):
            _native.pack_row_mask([n], n)
        with pytest.raises(ValueError):
            _native.pack_row_mask([-1], n)
    with pytest.raises(ValueError):
        _native.pack_row_mask(np.ones(n + 1, dtype=bool), n)


def test_header_documents_every_new_call_and_option():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
    assert "typedef struct rq_filter rq_filter;" in code
    doc = h[h.index("filtered searches"):h.index("typedef struct rq_filter rq_filter;")] + h[h.index("rq_filter_destroy(rq_filter* f);"):h.index("int rq_search_filtered(")]
    for word in ('"filter_route"', '"filter_route_last"', '"filter_repaired"', "stale filter", "RQ_EUNSUPPORTED", "RQ_EINVAL", "n_rows / 8", "4 n_rows",
                 "row_offset", "zero-norm", "min(k, allowed rows)", '"epi" = 0', '"wide_batch" = 2', "int8 image", "rq_search_train_device", "rq_index_destroy"):
        assert word in doc, word


def test_filter_creation_fails_loudly():
    lib = _native.load_library()
    bits = _native.pack_row_mask(np.ones(64, dtype=bool), 64)
    assert not lib.rq_filter_create(None, _native._ptr(bits), 64)
    if _native.device_count() == 0:
        assert "RQ_ENODEVICE" in _native.last_error() and "no HIP device" in _native.last_error()
    else:
        assert "null argument" in _native.last_error()
    assert not lib.rq_filter_create_device(None, None, 64, None)
    assert lib.rq_filter_count(None) == -1          # RQ_EINVAL
    lib.rq_filter_destroy(None)                      # harmless
    q = np.zeros((1, 8), np.float32)
    out_s, out_r = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64)
    assert lib.rq_search_filtered(None, None, _native._ptr(q), 1, 1, 0, _native._ptr(out_s), _native._ptr(out_r)) == -1


class _StubFilter:
    def __init__(self, rows):
        self.rows = np.unique(np.asarray(rows, np.int64))
        self.count = int(self.rows.size)
        self.closed = 0

    def close(self):
        self.closed += 1


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): brute force in float64 with the
    canonical order, and the filtered form of it -- the top-k over the filter's rows only, k entries, (0.0, -1) padded."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x = np.asarray(x, np.float64)
        self.dim = self.x.shape[1]
        self.made = []

    def __len__(self):
        return self.x.shape[0]

    def make_filter(self, rows):
        self.made.append(_StubFilter(rows))
        return self.made[-1]

    def search(self, q, k, metric=0, *, row_filter=None):
        q = np.atleast_2d(np.asarray(q, np.float64))
        sc = q @ self.x.T
        if metric == 0:
            sc = sc / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(self.x, axis=1)[None, :] + 1e-30)
        sc = sc.astype(np.float32)
        allowed = np.arange(len(self)) if row_filter is None else row_filter.rows
        rows = np.full((q.shape[0], k), -1, np.int64); out = np.zeros((q.shape[0], k), np.float32)
        for b in range(q.shape[0]):
            o = allowed[np.lexsort((allowed, -sc[b, allowed].astype(np.float64)))[:k]]
            rows[b, :len(o)] = o; out[b, :len(o)] = sc[b, o]
        return out, rows


def test_allowed_ids_on_the_python_seam(tmp_path, monkeypatch):
    """DenseIndex maps ids to rows (unknown ids ignored, its own filter closed, a caller's filter left open); BM25 scores are masked
    before the selection (scores of oracle/bm25_oracle.py); HybridRetriever fuses the two masked pools; without the keyword every
    result is what it was."""
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(120)]
    texts[30:34] = [texts[5]] * 4                                          # exact ties on both sides
    docs = [si.Document(id=f"p{i}", text=t, title=f"T{i}") for i, t in enumerate(texts)]
    emb = RandomProjectionEmbedder(16)
    vec = emb.embed(texts)
    stub = _StubNative(vec)
    dense = si.DenseIndex.from_native(stub, [d.id for d in docs], embedder=emb)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    r.bm25_index.add_documents(docs)
    for d in docs:
        r.documents[d.id] = d
    allowed_rows = [5, 30, 31, 33, 2, 77, 78, 100, 119]
    allowed = [f"p{i}" for i in allowed_rows] + ["ghost"]
    mask = np.zeros(120, dtype=bool)
    mask[allowed_rows] = True
    queries = [" ".join(rng.choice(vocab, size=4)) for _ in range(10)] + [texts[5], "nothing known here", ""]
    for qtext in queries:
        before = len(stub.made)
        # dense side
        got = dense.search(qtext, 5, allowed_ids=allowed)
        assert len(stub.made) == before + 1 and stub.made[-1].rows.tolist() == sorted(allowed_rows) and stub.made[-1].closed == 1
        s_all, r_all = stub.search(emb.embed([qtext]), 120)
        want = [(f"p{i}", float(s)) for s, i in zip(s_all[0], r_all[0]) if mask[i]][:5]
        assert [(d, s) for d, s, _ in got] == want
        assert dense.search_batch([qtext], 5, allowed_ids=allowed)[0] == got == dense.search_vectors(emb.embed([qtext]), 5, allowed_ids=allowed)[0]
        rows = dense.search_rows_batch([qtext], 5, allowed_ids=allowed)[1][0]
        assert [f"p{i}" for i in rows if i >= 0] == [d for d, _ in want]
        assert r.dense_search(qtext, 5, allowed_ids=allowed) == want
        # sparse side: the oracle's scores, masked, then the reference's selection (ties by descending row)
        sc = bm25_oracle.bm25_scores([bm25_oracle.tokenize(t) for t in texts], bm25_oracle.tokenize(qtext))
        sc = np.where(mask, sc, 0.0)
        top = [i for i in np.argsort(sc, kind="stable")[::-1][:7] if sc[i] > 0]
        sparse = r.bm25_search(qtext, 7, allowed_ids=allowed)
        assert [d for d, _ in sparse] == [f"p{i}" for i in top]
        np.testing.assert_allclose([s for _, s in sparse], sc[top], rtol=1e-12)
        # fusion of the two masked pools
        res = r.hybrid_search(qtext, top_k=6, retrieval_pool_size=7, allowed_ids=allowed)
        assert res == r._fuse(sparse, r.dense_search(qtext, 7, allowed_ids=allowed), 6)
        assert {x.doc_id for x in res} <= set(allowed)
        assert r.get_scores_for_router(qtext, 6, retrieval_pool_size=7, allowed_ids=allowed) == r._router_arrays(res, 6)
    # a reusable filter is used as it is and stays open
    mine = dense.make_filter(allowed)
    n_made = len(stub.made)
    assert dense.search(texts[5], 3, allowed_ids=mine) == dense.search(texts[5], 3, allowed_ids=allowed)
    assert len(stub.made) == n_made + 1 and mine.closed == 0                  # (the second call made its own)
    # unknown ids only: nothing is allowed
    assert dense.search(texts[5], 3, allowed_ids=["ghost"]) == [] and r.bm25_search(texts[5], 3, allowed_ids=["ghost"]) == []
    assert r.hybrid_search(texts[5], top_k=3, allowed_ids=["ghost"]) == []
    # without the keyword nothing changes
    assert dense.search(texts[5], 5) == [(f"p{i}", float(s), "") for s, i in zip(*[a[0] for a in stub.search(emb.embed([texts[5]]), 5)])]
    assert [d for d, _ in r.bm25_search(texts[5], 5)] == [d for d, _ in bm25_oracle.bm25_search([d.id for d in docs], texts, texts[5], 5)]
