"""Diversified search (MMR), the parts that need no GPU: the header's documentation, the loud failure without a device, the
binding's argument checks, the oracle against a naive Gram-matrix form, the host plan (csrc/rq_mmr_plan.h) under the sanitizers,
and the Python seam of DenseIndex / HybridRetriever over a stub dense backend.  The GPU side is tests/test_gpu_mmr.py."""
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
import mmr_oracle as mo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_mmr_select_device", "rq_search_mmr"]


def test_header_documents_both_calls_and_the_option():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
    assert re.search(r"rq_mmr_select_device\([^)]*double lambda[^)]*float\* d_mmr, void\* stream\)", code)
    assert re.search(r"rq_search_mmr\([^)]*const rq_filter\* f[^)]*int fetch_k, double lambda[^)]*float\* out_mmr\)", code)
    doc = h[h.index("diversified search"):h.index("int rq_mmr_select_device(")]
    for word in ('"mmr_calls"', "absent candidate", "NaN rel_i", "row_offset", "lowest position", "k_eff = min(k, present candidates)", "1e-30", "no fused multiply-add",
                 "(0.0, -1, 0.0)", "lambda = 1", "lambda = 0", "RQ_EINVAL", "RQ_EUNSUPPORTED", "RQ_ENODEVICE", "stale filter", "one thread at a time",
                 "rq_search_train_device", "hints", '"pipeline" 1 and 2', "multi-device", "must be distinct", "passed through", '"pipeline" = 0'):
        assert word in doc, word


def test_calls_fail_loudly_without_a_device_or_with_null_arguments():
    lib = _native.load_library()
    want = -2 if _native.device_count() == 0 else -1                  # RQ_ENODEVICE / RQ_EINVAL
    buf = np.zeros(8, np.float32)
    rows = np.zeros(8, np.int64)
    assert lib.rq_mmr_select_device(None, _native._ptr(rows), _native._ptr(buf), 1, 4, 2, 0.5, 0, _native._ptr(buf), _native._ptr(rows), None, None) == want
    if want == -2:
        assert "RQ_ENODEVICE" in _native.last_error() and "no CPU fallback" in _native.last_error()
    else:
        assert "null argument" in _native.last_error()
    assert lib.rq_search_mmr(None, None, _native._ptr(buf), 1, 2, 4, 0.5, 0, _native._ptr(buf), _native._ptr(rows), None) == want
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


@pytest.mark.parametrize("lam", [-0.1, 1.0001, float("nan"), float("inf"), "0.5", None])
def test_python_refuses_a_lambda_outside_the_unit_interval(lam):
    idx = _NoLibrary(8)
    with pytest.raises(ValueError, match="lambda_mult"):
        idx.search_mmr(np.zeros((1, 8), np.float32), 2, 4, lam)
    with pytest.raises(ValueError, match="lambda_mult"):
        idx.mmr_select_device(1, 2, 1, 4, 2, lam, 0, 3, 4)


def test_python_refuses_bad_sizes_before_the_library_is_called():
    idx = _NoLibrary(8)
    q = np.zeros((1, 8), np.float32)
    for k, fetch in ((5, 4), (0, 4), (1, 0), (1, _native.MAX_K + 1), (_native.MAX_K + 1, _native.MAX_K + 1)):
        with pytest.raises(ValueError):
            idx.search_mmr(q, k, fetch, 0.5)
        with pytest.raises(ValueError):
            idx.mmr_select_device(1, 2, 1, fetch, k, 0.5, 0, 3, 4)
    with pytest.raises(ValueError):
        idx.mmr_select_device(1, 2, 0, 4, 2, 0.5, 0, 3, 4)                       # B = 0
    with pytest.raises(ValueError, match="queries"):
        idx.search_mmr(np.zeros((1, 9), np.float32), 2, 4, 0.5)
    with pytest.raises(ValueError, match="RowFilter"):
        idx.search_mmr(q, 2, 4, 0.5, row_filter=object())


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [orc.METRIC_COSINE, orc.METRIC_IP])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_oracle_equals_the_naive_gram_matrix_form(lam, metric):
    x16 = orc.synthetic_corpus(300, 48, seed=5, clustered=True)
    rng = np.random.default_rng(int(lam * 10) + metric)
    for trial in range(4):
        rows = rng.choice(300, size=24, replace=False).astype(np.int64)
        rel = rng.standard_normal(24).astype(np.float32)
        s, r, v = mo.mmr_select(rel, rows, x16, 9, lam, metric)
        chosen, vals = mo.naive_gram_mmr(rel, x16[rows], 9, lam, metric)
        assert r.tolist() == rows[chosen].tolist(), (trial, lam)
        assert np.array_equal(s, rel[chosen]) and np.allclose(v, vals, rtol=0, atol=1e-6)


def test_oracle_lambda_one_is_the_relevance_order_and_lambda_zero_shows_the_penalties():
    x16 = orc.synthetic_corpus(500, 64, seed=8)
    q = orc.synthetic_queries(6, 64, seed=9)
    gs, gr = orc.dense_topk(q, x16, 12)
    s, r, v = mo.mmr_topk(q, x16, 12, 40, 1.0)
    assert np.array_equal(r, gr) and np.array_equal(s.view(np.uint32), gs.view(np.uint32)) and np.array_equal(v, s)
    cs, cr = orc.dense_topk(q, x16, 40)
    s0, r0, v0 = mo.mmr_select_batch(cs, cr, x16, 5, 0.0)
    assert np.array_equal(r0[:, 0], cr[:, 0]) and not v0[:, 0].any()            # all v are 0: position 0
    for b in range(6):
        picked = r0[b]
        for t in range(1, 5):
            sims = orc.exact_scores(x16[picked[:t]].astype(np.float32), x16[picked[t:t + 1]])[:, 0]
            assert v0[b, t] == -sims.max()


def test_oracle_ties_absent_candidates_and_padding():
    x16 = orc.synthetic_corpus(100, 256, seed=2)
    x16[10] = x16[11] = x16[3]                                                  # three identical rows
    rows = np.array([50, 11, 3, 10, -1, 100, 99, 7], np.int64)
    rel = np.array([0.1, 0.9, 0.9, 0.9, 5.0, 5.0, np.nan, 0.2], np.float32)
    s, r, v = mo.mmr_select(rel, rows, x16, 8, 1.0)
    assert r.tolist() == [11, 3, 10, 7, 50, -1, -1, -1] and s[5:].tolist() == [0, 0, 0] and v[5:].tolist() == [0, 0, 0]
    s, r, v = mo.mmr_select(rel, rows, x16, 4, 0.5)
    assert r[0] == 11 and set(r[1:3].tolist()) == {7, 50} and r[3] == 3      # the copies are pushed back; the lower position first
    assert mo.mmr_select(rel, np.full(8, -1, np.int64), x16, 3, 0.5)[1].tolist() == [-1, -1, -1]
    s, r, v = mo.mmr_select(rel, rows + 1000, x16, 2, 1.0, row_offset=1000)
    assert r.tolist() == [1011, 1003]                                            # (row 999 = -1 + 1000 lies below the offset)
    # following somebody else's path: the oracle names its own choice at every step
    s, r, v, pos = mo.mmr_select(rel, rows, x16, 3, 1.0, follow=[2, 1, 3])
    assert pos == [1, 1, 3] and r.tolist() == [11, 11, 10]


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------
def test_plan_and_argument_checks_on_the_host(tmp_path):
    """tests/native/mmr_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags are
    given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "mmr_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "mmr_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- the Python seam ---------------------------------------------------------------------------------------------------------
class _StubFilter:
    def __init__(self, rows):
        self.rows = np.unique(np.asarray(rows, np.int64))
        self.count = int(self.rows.size)
        self.closed = 0

    def close(self):
        self.closed += 1


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the oracle over fp16 rows."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), True)
        self.dim = self.x16.shape[1]
        self.made, self.calls = [], []

    def __len__(self):
        return self.x16.shape[0]

    def make_filter(self, rows):
        self.made.append(_StubFilter(rows))
        return self.made[-1]

    def search(self, q, k, metric=0, *, row_filter=None):
        return orc.dense_topk(q, self.x16, k, metric)

    def search_mmr(self, q, k, fetch_k, lambda_mult=0.5, metric=0, *, row_filter=None, return_mmr=False):
        self.calls.append((int(k), int(fetch_k), float(lambda_mult), row_filter))
        mask = None
        if row_filter is not None:
            mask = np.zeros(len(self), dtype=bool)
            mask[row_filter.rows] = True
        s, r, _ = mo.mmr_topk(q, self.x16, k, fetch_k, lambda_mult, metric, mask)
        return s, r


def test_mmr_on_the_python_seam(tmp_path, monkeypatch):
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    rng = np.random.default_rng(4)
    vocab = [f"w{i}" for i in range(30)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(90)]
    texts[40:44] = [texts[5]] * 4                                               # verbatim copies
    ids = [f"p{i}" for i in range(90)]
    emb = RandomProjectionEmbedder(16)
    stub = _StubNative(emb.embed(texts))
    dense = si.DenseIndex.from_native(stub, ids, texts, embedder=emb)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    qv = emb.embed([texts[5]])
    # tuples in selection order, the score is the cosine; clamping of fetch_k to [top_k, min(len, MAX_K)]
    got = dense.search_mmr(texts[5], 6, 20, 0.5)
    assert stub.calls[-1] == (6, 20, 0.5, None)
    s, rr, _ = mo.mmr_topk(qv, stub.x16, 6, 20, 0.5)
    assert got == [(ids[i], float(sc), texts[i]) for sc, i in zip(s[0], rr[0])]
    assert [d for d, _, _ in got] != [d for d, _, _ in dense.search(texts[5], 6)]            # the copies were pushed back
    assert dense.search_mmr_batch([texts[5], texts[7]], 6, 20, 0.5)[0] == got == dense.search_mmr_vectors(qv, 6, 20, 0.5)[0]
    assert r.dense_search_mmr(texts[5], 6, 20, 0.5) == [(d, sc) for d, sc, _ in got]
    dense.search_mmr(texts[5], 6, 3)
    assert stub.calls[-1][:2] == (6, 6)                                                      # fetch_k below top_k
    dense.search_mmr(texts[5], 6, 10 ** 6)
    assert stub.calls[-1][:2] == (6, 90)                                                     # beyond the index
    dense.search_mmr(texts[5], 500, 10)
    assert stub.calls[-1][:2] == (90, 90)                                                    # top_k beyond the index
    assert dense.search_mmr(texts[5], 6, 20, 1.0) == dense.search(texts[5], 6)               # lambda = 1: the plain search
    # allowed_ids: ids make a filter that is closed again; a reusable filter stays open; unknown ids are ignored
    allowed_rows = [5, 40, 41, 2, 77, 78, 80, 89]
    allowed = [f"p{i}" for i in allowed_rows] + ["ghost"]
    n_made = len(stub.made)
    got = dense.search_mmr(texts[5], 4, 20, 0.5, allowed_ids=allowed)
    assert len(stub.made) == n_made + 1 and stub.made[-1].rows.tolist() == sorted(allowed_rows) and stub.made[-1].closed == 1
    assert stub.calls[-1][3] is stub.made[-1] and {d for d, _, _ in got} <= set(allowed) and len(got) == 4
    mine = dense.make_filter(allowed)
    n_made = len(stub.made)
    assert dense.search_mmr(texts[5], 4, 20, 0.5, allowed_ids=mine) == got and len(stub.made) == n_made and mine.closed == 0
    assert r.dense_search_mmr(texts[5], 4, 20, 0.5, allowed_ids=mine) == [(d, sc) for d, sc, _ in got]
    assert len(dense.search_mmr(texts[5], 20, 50, 0.5, allowed_ids=allowed)) == len(allowed_rows)     # fewer allowed than top_k: no padding tuples
    # nothing to search, nothing asked for
    n_calls = len(stub.calls)
    assert dense.search_mmr(texts[5], 0, 20) == [] and dense.search_mmr_batch([], 5) == [] and dense.search_mmr_vectors(np.zeros((2, 16)), -1) == [[], []]
    empty = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32)), [], embedder=emb)
    assert empty.search_mmr("anything", 5) == [] and len(stub.calls) == n_calls
    with pytest.raises(ValueError):
        dense.search_mmr(texts[5], 5, 20, 1.5)
    with pytest.raises(ValueError):
        dense.search_mmr_vectors(np.zeros((1, 15), np.float32), 5)
    none = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b2.pkl"), chroma_persist_path=str(tmp_path / "c2"), dense_index=dense)
    none.dense_index = None
    assert none.dense_search_mmr("x") == []
