"""Grouped sparse search (`distinct_by=` on BM25Index.search_batch / search_batch_rows; include/rq.h rq_sparse_set_groups,
rq_sparse_topk_grouped*), the parts that need no GPU: the yardstick (tests/sparse_grouped_oracle.py) against BM25Index._search_distinct
over the index's own arrays -- rows, score bits and counts, masks included --, the host batch call against the per-query call it is
defined by, the plan header as a stand-alone program under the host sanitizers, and the header.  The GPU side is
tests/test_gpu_sparse_grouped.py."""
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
import sparse_grouped_oracle as go  # noqa: E402
import sparse_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")


def test_header_declares_and_documents_the_grouped_calls():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in ("rq_sparse_set_groups", "rq_sparse_topk_grouped", "rq_sparse_topk_grouped_device", "rq_hybrid_set_groups", "rq_hybrid_fuse_grouped",
                 "rq_hybrid_fuse_grouped_device"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES and hasattr(_native.load_library(), name)
    doc = h[h.index("sparse search: exact BM25"):h.index("typedef struct rq_sparse rq_sparse;")]
    hybrid_doc = h[h.index("hybrid fusion: both pools"):h.index("typedef struct rq_hybrid rq_hybrid;")]
    for section in (doc, hybrid_doc):                                           # the closing notes no longer list distinct_by
        assert "distinct_by" not in section[section.rindex("Not extended:"):]
    for word in ("rq_hybrid_fuse_grouped_device", "4 B per key", "before the collapse", "first candidate of every group", "count = min(kept, top_k)",
                 "rq_router_rerank_device consumes"):
        assert word in hybrid_doc, word
    for word in ("rq_sparse_topk_grouped_device", "4 B per document", "-1 = a group of its own", "need not be dense", "_search_distinct", "DESCENDING row",
                 "out_count", "in-tile collapse", "atomicCAS", "min(\"tile_docs\", 4096)", "96 KiB", "strictly below the previous chunk's threshold",
                 '"grouped_calls"', '"final_chunks_last"', '"grouped"'):
        assert word in doc, word
    lib = _native.load_library()
    assert lib.rq_sparse_set_groups(None, None, 0) == -1 and lib.rq_hybrid_set_groups(None, None, 0) == -1
    assert lib.rq_sparse_topk_grouped(None, None, None, 1, 1, None, 0, None, None, None, None) == -1
    assert lib.rq_sparse_topk_grouped_device(None, None, None, 1, 0, 1, None, 0, None, None, None, None, None) == -1
    assert lib.rq_hybrid_fuse_grouped(None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, None, None) == -1


def test_plan_and_validation_on_the_host(tmp_path):
    """tests/native/sparse_grouped_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the
    flags are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "sparse_grouped_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "sparse_grouped_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def _corpus():
    """150 chunks of 40 titles; every eleventh chunk has no title (a group of its own), some texts repeat (exact score ties between
    and inside groups)."""
    rng = np.random.default_rng(8)
    p = 1.0 / np.arange(1, 61) ** 0.9
    p /= p.sum()
    texts = [" ".join(f"w{w}" for w in rng.choice(60, rng.integers(4, 12), p=p)) for i in range(150)]
    for i in range(20, 150, 13):
        texts[i] = texts[i - 9]
    docs = [si.Document(id=f"d{i}", text=texts[i], title="" if i % 11 == 0 else f"t{(i * 7) % 40}", metadata={"section": i % 3} if i % 5 else {}) for i in range(150)]
    bm = si.BM25Index()
    bm.add_documents(docs)
    qs = [" ".join(f"w{w}" for w in rng.choice(60, rng.integers(1, 7), p=p)) for _ in range(14)] + ["", "zzz unknown words", texts[11]]
    return bm, qs


def _entries(n):
    tenant_a = {f"d{i}" for i in range(0, 150, 3)}
    tenant_b = [f"d{i}" for i in range(100, 150)] + ["ghost1"]
    pool = [tenant_a, None, tenant_b, set(), ("d7", "d40", "d149"), tenant_a]
    return [pool[i % len(pool)] for i in range(n)]


def _as_arrays(bm, lists, k):
    row_of = bm._row_of_id()
    rows, scores = np.full((len(lists), k), -1, np.int32), np.zeros((len(lists), k))
    for b, res in enumerate(lists):
        rows[b, :len(res)] = [row_of[d] for d, _ in res]
        scores[b, :len(res)] = [s for _, s in res]
    return rows, scores, np.array([len(r) for r in lists], np.int32)


@pytest.mark.parametrize("key", ["title", "section"])
def test_oracle_equals_search_distinct_on_rows_bits_and_counts(key):
    bm, qs = _corpus()
    c = bm._csr()
    ix = {"indptr": c["indptr"], "rows": c["rows"], "contrib": c["contrib"], "n_tokens": len(c["tid"]), "n_docs": c["n_docs"]}
    groups = bm._group_table(c, key)
    assert groups.dtype == np.int32 and (groups == -1).sum() >= 13 and groups.max() < 40
    tid = c["tid"]
    q = so.ragged([[tid[t] for t in bm._tokenize(x) if t in tid] for x in qs])
    each = _entries(len(qs))
    masks, mask_of = bm._mask_table(each)
    for k in (1, 5, 40, 200):
        want = _as_arrays(bm, [bm._search_distinct(x, k, key) for x in qs], k)
        got = go.topk(ix, *q, k, groups)
        assert go.same(got, want), k
        want = _as_arrays(bm, [bm._search_distinct(x, k, key, e) for x, e in zip(qs, each)], k)
        got = go.topk(ix, *q, k, groups, masks, mask_of)
        assert go.same(got, want), k
        assert (got[2] < (so.topk(ix, *q, k)[0] >= 0).sum(axis=1)).any() or k == 1         # the collapse changes answers
        # and the row form of the host batch call is the oracle's answer, row for row
        assert so.same(bm.search_batch_rows(qs, k, distinct_by=key, allowed_ids_each=each), got[:2])


def test_host_batch_search_equals_the_per_query_search_it_is_defined_by():
    bm, qs = _corpus()
    each = _entries(len(qs))
    for k in (1, 5, 200):
        want = [bm.search(q, k, distinct_by="title") for q in qs]
        assert any(want) and want != [bm.search(q, k) for q in qs] or k == 1
        assert bm.search_batch(qs, k, distinct_by="title") == want
        assert bm.search_batch(qs, k, distinct_by="title", use_native=False) == want
        want = [bm.search(q, k, distinct_by="title", **si._given(allowed_ids=e)) for q, e in zip(qs, each)]
        assert bm.search_batch(qs, k, distinct_by="title", allowed_ids_each=each) == want
        one = each[0]
        assert bm.search_batch(qs, k, distinct_by="title", allowed_ids=one) == [bm.search(q, k, distinct_by="title", allowed_ids=one) for q in qs]
        m = bm.make_mask(one)
        assert bm.search_batch(qs, k, distinct_by="title", allowed_ids=m) == bm.search_batch(qs, k, distinct_by="title", allowed_ids=one)
    assert bm.search_batch(qs, 5, distinct_by="nosuchfield") == bm.search_batch(qs, 5)      # every document a group of its own
    assert bm.search_batch(qs, 0, distinct_by="title") == [[] for _ in qs] == si.BM25Index().search_batch(qs, 5, distinct_by="title")
    assert bm.search_batch_rows([], 5, distinct_by="title")[0].shape == (0, 5)


def test_the_group_table_is_cached_per_key_and_dropped_with_the_arrays():
    bm, qs = _corpus()
    c = bm._csr()
    t = bm._group_table(c, "title")
    assert bm._group_table(c, "title") is t and bm._group_table(c, "section") is not t and set(c["groups"]) == {"title", "section"}
    bm.add_documents([si.Document(id="late", text="w1 w2 w3", title="t0")])
    c2 = bm._csr()
    assert c2 is not c and "groups" not in c2 and len(bm._group_table(c2, "title")) == 151
    with pytest.raises(ValueError, match="allowed_ids_each does not combine with allowed_ids"):
        bm.search_batch(qs, 3, distinct_by="title", allowed_ids={"d1"}, allowed_ids_each=[None] * len(qs))
    with pytest.raises(ValueError, match="backend"):
        bm.search_batch(qs, 3, distinct_by="title", backend="tpu")
