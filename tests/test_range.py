"""Range searches (rq_search_range*), the parts that need no GPU: the header's documentation, the loud failure without a device, the
binding's argument checks, the oracle's own edge cases (tests/range_oracle.py), the host plan (csrc/rq_range_plan.h) under the
sanitizers and DenseIndex.search_threshold / count_above on the Python seam over a stub backend whose search_range is the oracle.
The GPU side is tests/test_gpu_range.py."""
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
import nonfinite_oracle as nfo  # noqa: E402
import range_oracle as ro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_search_range_device", "rq_search_range_fixup_device", "rq_search_range"]


def test_header_documents_the_three_calls_and_the_options():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
    dev = (r"\(rq_index\* idx, const rq_filter\* f, const float\* d_queries, int B, const float\* d_thr, int cap, int metric,\s*float\* d_scores, "
           r"int64_t\* d_rows, uint64_t\* d_keys, int64_t\* d_count, int\* d_status, void\* stream\)")
    assert re.search(r"rq_search_range_device" + dev, code) and re.search(r"rq_search_range_fixup_device" + dev, code)
    assert re.search(r"rq_search_range\(rq_index\* idx, const rq_filter\* f, const float\* queries, int B, const float\* thr, int cap, int metric,\s*"
                     r"float\* out_scores, int64_t\* out_rows, int64_t\* out_count\)", code)
    doc = h[h.index("range searches: every row"):h.index("int rq_search_range_device(")]
    for word in ('"range_route"', '"range_route_last"', '"range_calls"', '"range_repaired"', '"range_cand_cap"', '"range_bins_last"', "s >= thr[q]", "fp32 values",
                 "NaN score counts as -inf", "-0.0 is +0.0", "zero-norm query", "count[q] (int64)", "exact, also when it exceeds cap", "canonical order",
                 "row_offset + local row", "(0.0, -1)", "key 0", "must be finite", "count 0 and status 0", "thr <= 0", "thr > 0", "allowed count", "empty index",
                 "1 <= cap <= RQ_MAX_K", "1 <= B <= 65535", "RQ_EINVAL", "RQ_EUNSUPPORTED", "multi-device", "RQ_ENODEVICE", "stale filter", '"pipeline" = 0',
                 "stream order", "no host synchronisation", "int8 image", "NaN row scale", "SCAN (1)", "GATHER (2)", "EXACT (3)", "never depend on the route",
                 "re-scores most of the shard", "rq_search_train_device", "hints", '"pipeline" 1 and 2', "rq_timing counts", "same bits", "nextafter",
                 "SAME arguments", "Returns the number repaired", "index's own stream", "RQ_ENOMEM"):
        assert word in doc, word


def test_calls_fail_loudly_without_a_device_or_with_null_arguments():
    lib = _native.load_library()
    want = -2 if _native.device_count() == 0 else -1                  # RQ_ENODEVICE / RQ_EINVAL
    buf = np.zeros(8, np.float32)
    rows = np.zeros(8, np.int64)
    cnt = np.zeros(1, np.int64)
    st = np.zeros(1, np.int32)
    p = _native._ptr
    for call in (lambda: lib.rq_search_range_device(None, None, p(buf), 1, p(buf), 4, 0, p(buf), p(rows), None, p(cnt), p(st), None),
                 lambda: lib.rq_search_range_fixup_device(None, None, p(buf), 1, p(buf), 4, 0, p(buf), p(rows), None, p(cnt), p(st), None),
                 lambda: lib.rq_search_range(None, None, p(buf), 1, p(buf), 4, 0, p(buf), p(rows), p(cnt))):
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


def test_python_refuses_bad_arguments_before_the_library_is_called():
    idx = _NoLibrary(8)
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="queries"):
        idx.search_range(np.zeros((2, 9), np.float32), 0.5, 10)
    for cap in (0, -1, _native.MAX_K + 1):
        with pytest.raises(ValueError, match=f"cap {cap}"):
            idx.search_range(q, 0.5, cap)
    with pytest.raises(ValueError, match="B 0"):
        idx.search_range(np.zeros((0, 8), np.float32), 0.5, 10)
    with pytest.raises(ValueError, match="metric"):
        idx.search_range(q, 0.5, 10, metric=2)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            idx.search_range(q, bad, 10)
        with pytest.raises(ValueError, match="finite"):
            idx.search_range(q, np.array([0.5, bad], np.float32), 10)
    for shape in ((3,), (1,), (2, 1), (0,)):
        with pytest.raises(ValueError, match="one per query"):
            idx.search_range(q, np.zeros(shape, np.float32), 10)
    with pytest.raises(ValueError, match="row_filter"):
        idx.search_range(q, 0.5, 10, row_filter=object())
    for B, cap, metric in ((0, 4, 0), (65536, 4, 0), (1, 0, 0), (1, _native.MAX_K + 1, 0), (1, 4, -1), (1, 4, 2)):
        with pytest.raises(ValueError):
            idx.search_range_device(1, B, 2, cap, metric, 3, 4, None, 5, 6)
        with pytest.raises(ValueError):
            idx.search_range_fixup_device(1, B, 2, cap, metric, 3, 4, None, 5, 6)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_ties_cap_zero_norm_and_nan_rows():
    x16 = orc.synthetic_corpus(200, 48, seed=5)
    x16[50] = x16[20]
    x16[120] = x16[20]                                   # three identical rows: one score, three rows
    x16[7] = np.nan
    x16[9, 3] = np.float16(np.inf)
    q = orc.synthetic_queries(3, 48, seed=6)
    q[0] = x16[20].astype(np.float32)
    q[0, 3] = 0                                          # (against the inf of row 9: 0 x inf = NaN -> -inf under both metrics)
    q[2] = 0
    for metric in (orc.METRIC_COSINE, orc.METRIC_IP):
        s = nfo.scores(q, x16, metric)
        assert s[0, 20] == s[0, 50] == s[0, 120] == s[0].max()
        t = s[0, 20]
        sc, rows, cnt = ro.search_range(q, x16, [t, 0.0, 0.0], 5, metric)
        assert cnt[0] == 3 and rows[0].tolist() == [20, 50, 120, -1, -1] and (sc[0, :3] == t).all() and not sc[0, 3:].any()       # ties all count
        sc, rows, cnt = ro.search_range(q, x16, [t, 0.0, 0.0], 2, metric)
        assert cnt[0] == 3 and rows[0].tolist() == [20, 50]                                                                      # the cap cuts a tie by row order
        assert ro.search_range(q, x16, [np.nextafter(t, np.float32(np.inf)), 0, 0], 5, metric)[2][0] == 0                        # one ulp above: nothing
        # a zero-norm query: every row at 0.0 when thr <= 0 (NaN and inf rows included), nothing when thr > 0
        assert cnt[2] == 200 and rows[2].tolist() == [0, 1] and not sc[2].any()
        sc, rows, cnt = ro.search_range(q, x16, [0.0, 0.0, np.float32(1e-30)], 4, metric)
        assert cnt[2] == 0 and (rows[2] == -1).all()
        sc, rows, cnt = ro.search_range(q, x16, -1.0, 4, metric, row_offset=1000, mask=np.arange(200) % 3 == 1)
        assert cnt[2] == 67 and rows[2].tolist() == [1001, 1004, 1007, 1010]
        # NaN rows score -inf: never in range, whatever the (finite) threshold
        lo = np.float32(-3.0e38)
        sc, rows, cnt = ro.search_range(q, x16, lo, 200, metric)
        assert 7 not in rows[1] and cnt[1] == 200 - int(np.isneginf(s[1]).sum()) and np.isneginf(s[1, 7])
        assert (np.diff(sc[1, :cnt[1]].astype(np.float64)) <= 0).all()
        # a non-finite threshold (device forms): nothing
        assert ro.search_range(q, x16, [np.nan, np.inf, -np.inf], 4, metric)[2].tolist() == [0, 0, 0]
    assert ro.search_range(q, x16[:0], 0.0, 3)[2].tolist() == [0, 0, 0]
    # threshold_for: the midpoint of a real gap, a quarter of the gap away from both neighbours at least
    srt = np.sort(nfo.scores(q[1:2], x16)[0][np.isfinite(nfo.scores(q[1:2], x16)[0])])[::-1]
    thr, r = ro.threshold_for(srt, 10, 4e-6)
    assert abs(r - 10) <= 8 and srt[r - 1] > thr > srt[r] and (srt >= thr).sum() == r
    assert ro.threshold_for(srt, 0, 4e-6)[1] == 0 and ro.threshold_for(srt, 0, 4e-6)[0] > srt[0]
    assert ro.threshold_for(np.full(40, 0.5), 10, 4e-6) is None


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------
def test_plan_and_argument_checks_on_the_host(tmp_path):
    """tests/native/range_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "range_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "range_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- DenseIndex / HybridRetriever on the Python seam ------------------------------------------------------------------------------
class _StubFilter:
    def __init__(self, rows):
        self.rows = np.unique(np.asarray(rows, np.int64))

    def close(self):
        pass


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the oracle over the fp16 rows."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), True)
        self.dim = self.x16.shape[1]
        self.calls = []

    def __len__(self):
        return self.x16.shape[0]

    def make_filter(self, rows):
        return _StubFilter(rows)

    def search_range(self, q, threshold, cap, metric=0, *, row_filter=None):
        self.calls.append((np.asarray(q).shape, cap))
        mask = None
        if row_filter is not None:
            mask = np.zeros(len(self), bool)
            mask[row_filter.rows] = True
        return ro.search_range(q, self.x16, threshold, cap, metric, mask=mask)


def test_dense_index_threshold_searches_and_counts(tmp_path, monkeypatch):
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    emb = RandomProjectionEmbedder(16)
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(120)]
    texts[30:34] = [texts[5]] * 4
    ids = [f"p{i}" for i in range(120)]
    stub = _StubNative(emb.embed(texts))
    dense = si.DenseIndex.from_native(stub, ids, texts, embedder=emb)
    qv = emb.embed([texts[5], texts[77]])
    s = nfo.scores(qv, stub.x16)
    dup = dense.search_threshold(texts[5], 0.98)
    assert [d for d, _, _ in dup] == ["p5", "p30", "p31", "p32", "p33"] and all(sc >= 0.98 for _, sc, _ in dup) and dup[0][2] == texts[5]     # near-duplicates on ingest
    assert dense.count_above(texts[5], 0.98) == 5 and dense.count_above(texts[5], 1.5) == 0 and dense.search_threshold(texts[5], 1.5) == []   # abstaining
    thr = float(np.sort(s[1])[::-1][20]) + 1e-7
    want = int((s[1] >= np.float32(thr)).sum())
    assert dense.count_above(texts[77], thr) == want and len(dense.search_threshold(texts[77], thr, max_results=7)) == min(7, want)
    assert len(dense.search_threshold(texts[77], thr, max_results=500)) == want
    both = dense.search_threshold_batch([texts[5], texts[77]], [0.98, thr], 3)
    assert [d for d, _, _ in both[0]] == ["p5", "p30", "p31"] and both[1] == dense.search_threshold(texts[77], thr, 3)
    assert dense.search_threshold_vectors(qv, [0.98, thr], 3) == both
    allowed = ["p30", "p32", "p77", "nobody"]
    assert [d for d, _, _ in dense.search_threshold(texts[5], 0.98, allowed_ids=allowed)] == ["p30", "p32"] and dense.count_above(texts[5], 0.98, allowed_ids=allowed) == 2
    flt = dense.make_filter(allowed)
    assert dense.count_above(texts[5], -1.0, allowed_ids=flt) == 3
    assert dense.search_threshold(texts[5], 0.5, max_results=0) == [] and dense.search_threshold_batch([], 0.5) == []
    assert stub.calls and all(c[1] <= _native.MAX_K for c in stub.calls)
    with pytest.raises(ValueError):
        dense.search_threshold_vectors(np.zeros((1, 15), np.float32), 0.5)
    empty = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32)), [], embedder=emb)
    assert empty.search_threshold("anything", 0.1) == [] and empty.count_above("anything", -1.0) == 0

    class _Multi(_StubNative):
        devices = [0, 0]
    multi = si.DenseIndex.from_native(_Multi(stub.x16.astype(np.float32)), ids, embedder=emb)
    for call in (lambda: multi.search_threshold("w1", 0.5), lambda: multi.count_above("w1", 0.5)):
        with pytest.raises(_native.RqError, match="need a single-device index"):
            call()
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    assert r.dense_search_threshold(texts[5], 0.98, 3) == [(d, sc) for d, sc, _ in dup[:3]]
    assert r.dense_search_threshold(texts[5], 0.98, allowed_ids=allowed) == [(d, sc) for d, sc, _ in dense.search_threshold(texts[5], 0.98, allowed_ids=allowed)]
