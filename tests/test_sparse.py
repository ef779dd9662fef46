"""Sparse search on the device (include/rq.h rq_sparse_*), the parts that need no GPU: the yardstick (tests/sparse_oracle.py) against
librq_bm25.so bit for bit on every case the GPU tier uses, the host plan (csrc/rq_sparse_plan.h) under the sanitizers, the header and
the binding, and the loud failure without a device.  The GPU side is tests/test_gpu_sparse.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_sparse_create", "rq_sparse_destroy", "rq_sparse_postings", "rq_sparse_topk", "rq_sparse_topk_device", "rq_sparse_set_option", "rq_sparse_get_option"]
CASES = so.cases()


def test_header_declares_and_documents_the_sparse_calls():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES and hasattr(_native.load_library(), name)
    assert re.search(r"#define\s+RQ_SPARSE_MAX_K\s+1024", code) and _native.SPARSE_MAX_K == 1024
    for word in ("IN QUERY ORDER", "DESCENDING row", "STRICTLY ascending", "COPIED", "12 B per posting", "8 B per", "EMPTY", "tile_docs", "cand_cap",
                 "rounds_last", "tiles_last", "skipped_tiles_last", "Not extended", "allowed_ids", "distinct_by", "multi-device"):
        assert word in h, word


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_agrees_with_the_host_library_bit_for_bit(case):
    """One definition for both tiers: what the GPU tests compare against is what librq_bm25.so returns, rows and score bits."""
    ix = case["ix"]
    h = _native.bm25_create(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    try:
        B = len(case["q_indptr"]) - 1
        want = so.topk(ix, case["q_indptr"], case["q_tokens"], case["k"])
        for n_threads in (1, 3):
            assert so.same(_native.bm25_topk(h, case["q_indptr"], case["q_tokens"], B, case["k"], n_threads), want), n_threads
    finally:
        _native.bm25_destroy(h)


def test_the_cases_hold_what_they_are_meant_to_hold():
    """The order of additions matters in the order case, repeated tokens are not a product, ties are cut inside their run, the specials
    are left out -- so a route that passes them has been asked the question."""
    by = {c["name"]: c for c in CASES}
    c = by["order_of_additions"]
    rows, sc = so.topk(c["ix"], c["q_indptr"], c["q_tokens"], c["k"])
    sums = [float(sc[q][list(rows[q]).index(70)]) if 70 in rows[q] else 0.0 for q in range(5)]
    assert sums[0] == 3.0 and sums[1] == 4.0 and sums[4] == 3.0 and sums[2] == 4.0, sums            # 1e16 + 1 - 1e16 + 3 is 3 or 4 by the order
    # 3 repeats: c + c + c is always the rounding of 3 c (2 c is exact); 6 repeats of 0.1 are 0.6, not 6 * 0.1 = 0.6000000000000001
    assert sc[5][list(rows[5]).index(70)] == 0.1 + 0.1 + 0.1 and sc[6][list(rows[6]).index(70)] == 0.6 != 6 * 0.1
    c = by["cancel_negative_nan_inf"]
    rows, sc = so.topk(c["ix"], c["q_indptr"], c["q_tokens"], c["k"])
    assert rows[0].tolist()[:4] == [3, 9, 8, -1] and sc[0][0] == np.inf and rows[3].tolist()[:3] == [2, 8, -1]
    assert rows[5].tolist()[:3] == [130, 5, -1]                                                     # equal scores: descending row
    c = by["tie_run_k100"]
    rows, sc = so.topk(c["ix"], c["q_indptr"], c["q_tokens"], c["k"])
    assert (sc[0] == 1.25).all() and (np.diff(rows[0]) < 0).all() and len(set(rows[0] // 64)) > 1   # the cut falls inside the run, over several tiles
    c = by["query_of_300_tokens"]
    assert int(np.diff(c["q_indptr"]).max()) == 300
    assert (so.topk(by["k1024_default_tile"]["ix"], *so.ragged([[8]]), 1024)[0] >= 0).all()          # more than k positives at k = 1024
    assert {"tile64_n1", "tile64_n63", "tile64_n64", "tile64_n65", "tile64_n200", "tile_default_n8193", "tile_default_n20000", "batch1", "batch3", "batch70",
            "batch500", "batch70_three_rounds", "k1_tile64", "k100_tile64", "k1024_tile64", "one_full_tile_k10"} <= set(by)


def test_plan_and_validation_on_the_host(tmp_path):
    """tests/native/sparse_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "sparse_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "sparse_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def _small_index():
    bm = si.BM25Index()
    bm.add_documents([si.Document(id=f"d{i}", text=t) for i, t in enumerate(["red green blue", "green green yellow", "blue red red violet", "yellow"])])
    return bm


def test_backend_keyword_is_checked_and_host_is_unchanged():
    bm = _small_index()
    qs = ["green red", "violet", "nothing known", ""]
    want = bm.search_batch_rows(qs, 3)
    assert so.same(bm.search_batch_rows(qs, 3, backend="host"), want)
    assert bm.search_batch(qs, 3, backend="host") == bm.search_batch(qs, 3) == [bm.search(q, 3) for q in qs]
    with pytest.raises(ValueError):
        bm.search_batch_rows(qs, 3, backend="cuda")
    with pytest.raises(ValueError):
        si.HybridRetriever(bm25_persist_path=None, dense_index=object(), sparse_backend="cuda")
    c = bm._csr()
    assert so.same(want, so.topk({"indptr": c["indptr"], "rows": c["rows"], "contrib": c["contrib"], "n_tokens": len(c["tid"]), "n_docs": c["n_docs"]},
                                 *_query_csr(bm, qs), 3))
    empty = si.BM25Index()
    assert empty.search_batch(qs, 3, backend="gpu") == [[] for _ in qs] and empty.search_batch_rows(qs, 3, backend="gpu")[0].shape == (4, 3)   # the empty-index returns stay


def _query_csr(bm, qs):
    tid = bm._csr()["tid"]
    return so.ragged([[tid[t] for t in bm._tokenize(q) if t in tid] for q in qs])


def test_no_device_means_loud_failure_not_fallback():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    ix = CASES[0]["ix"]
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    assert not _native.sparse_available()
    bm = _small_index()
    qs = ["green red", "violet"]
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        bm.search_batch_rows(qs, 3, backend="gpu")
    with pytest.raises(_native.RqError):
        bm.search_batch(qs, 3, backend="gpu")
    assert so.same(bm.search_batch_rows(qs, 3, backend="auto"), bm.search_batch_rows(qs, 3))       # auto: the host when no device is visible
    assert bm.search_batch(qs, 3, backend="host") == [bm.search(q, 3) for q in qs]
    # malformed arrays are refused before the device is looked for
    with pytest.raises(_native.RqError, match="ascending"):
        _native.SparseIndex(np.array([0, 2], np.int64), np.array([1, 0], np.int32), np.array([1.0, 1.0]), 1, 2)
    lib = _native.load_library()
    assert lib.rq_sparse_topk(None, None, None, 1, 1, None, None) == -1 and lib.rq_sparse_postings(None) == 0
    lib.rq_sparse_destroy(None)
