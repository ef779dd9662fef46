"""Searches with one filter per query (include/rq.h "per-query filters"), the parts that need no GPU: the plan
(csrc/rq_filter_each_plan.h, on the host), the header's documentation and the binding's signatures, the loud failures without a
device, and the Python seam -- `allowed_ids_each=` on DenseIndex over a stub backend.  The GPU side is tests/test_gpu_filter_each.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_search_filtered_each", "rq_search_filtered_each_device", "rq_search_fixup_filtered_each_device"]
NEW_OPTIONS = ['"filter_each_calls"', '"filter_each_groups_last"', '"filter_each_ragged_last"', '"filter_each_rounds_last"',
               '"filter_each_shared_exact_last"', '"filter_each_routes_last"', '"filter_each_key_cap"']


def test_plan_on_the_host(tmp_path):
    """tests/native/filter_each_plan_check.cpp: grouping by first appearance, NULL, contiguity, every group routed by its own B_g, the
    shared exact rule at 12 and 13 filters per 64 queries, the forced routes, round cutting at the key cap, nothing written -- as a
    stand-alone host program under the address and UB sanitizers (host code only: the flags go to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "filter_each_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC,
                    os.path.join(os.path.dirname(__file__), "native", "filter_each_plan_check.cpp"), "-o", exe], check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def test_header_documents_every_new_call_and_option():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
        assert len(_native._SIGNATURES[name][1]) == (8 if name == "rq_search_filtered_each" else 11)
    # the new section follows the single-filter calls and leaves their text alone
    assert h.index("per-query filters") > h.index("int rq_search_fixup_filtered_device(")
    assert code.index("rq_search_filtered_each_device(") > code.index("rq_search_fixup_filtered_device(")
    doc = h[h.index("per-query filters"):h.index("int rq_search_filtered_each_device(")]
    for word in NEW_OPTIONS + ['"filter_route"', '"filter_route_last"', '"filter_repaired"', "HOST array", "NULL entry", "never kept", "row_offset", "zero-norm",
                               "min(k, allowed rows of THAT query's", "RQ_EUNSUPPORTED", "RQ_EINVAL", "stale filter", "before anything is enqueued", "d_status is required",
                               '"pipeline" = 0', "int8 image", "rq_search_train_device", "returns the number repaired", "ragged", "shared exact", "1 GiB",
                               "one search and B queries"]:
        assert word in doc, word
    plan = open(os.path.join(CSRC, "rq_filter_each_plan.h")).read()
    rule = plan[plan.index("// Rule 4"):plan.index("#define RQ_FILTER_EACH_KEY_CAP")]
    assert re.search(r"#define RQ_FILTER_EACH_EXACT_GROUPS\s+\d+", rule) and "measured" in rule and "3.45 ms" in rule and "285 us" in rule


def test_the_calls_fail_loudly():
    lib = _native.load_library()
    q = np.zeros((2, 8), np.float32)
    s, r = np.full((2, 3), 7.0, np.float32), np.full((2, 3), 7, np.int64)
    arr = (_native.C.c_void_p * 2)(None, None)
    assert lib.rq_search_filtered_each(None, arr, _native._ptr(q), 2, 3, 0, _native._ptr(s), _native._ptr(r)) == -1      # RQ_EINVAL
    assert lib.rq_search_filtered_each_device(None, arr, None, 2, 3, 0, None, None, None, None, None) == -1
    assert lib.rq_search_fixup_filtered_each_device(None, arr, None, 2, 3, 0, None, None, None, None, None) == -1
    assert (s == 7.0).all() and (r == 7).all()


class _StubFilter:
    def __init__(self, rows):
        self.rows = np.unique(np.asarray(rows, np.int64))
        self.count = int(self.rows.size)
        self.closed = 0

    def close(self):
        self.closed += 1


class _StubNative:
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): brute force in float64 with the
    canonical order; the each-form ranks every query over its own filter's rows, k entries, (0.0, -1) padded."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x = np.asarray(x, np.float64)
        self.dim = self.x.shape[1]
        self.made, self.each_calls = [], []

    def __len__(self):
        return self.x.shape[0]

    def make_filter(self, rows):
        self.made.append(_StubFilter(rows))
        return self.made[-1]

    def _rank(self, q, k, metric, allowed):
        sc = q @ self.x.T
        if metric == 0:
            sc = sc / (np.linalg.norm(q) * np.linalg.norm(self.x, axis=1) + 1e-30)
        sc = sc.astype(np.float32)
        o = allowed[np.lexsort((allowed, -sc[allowed].astype(np.float64)))[:k]]
        rows = np.full(k, -1, np.int64); out = np.zeros(k, np.float32)
        rows[:len(o)] = o; out[:len(o)] = sc[o]
        return out, rows

    def search(self, q, k, metric=0, *, row_filter=None):
        q = np.atleast_2d(np.asarray(q, np.float64))
        return self.search_filtered_each(q, k, [row_filter] * q.shape[0], metric, _record=False)

    def search_filtered_each(self, q, k, filters, metric=0, _record=True):
        q = np.atleast_2d(np.asarray(q, np.float64))
        assert len(filters) == q.shape[0]
        if _record:
            self.each_calls.append(list(filters))
        res = [self._rank(q[b], k, metric, np.arange(len(self)) if f is None else f.rows) for b, f in enumerate(filters)]
        return np.stack([s for s, _ in res]), np.stack([r for _, r in res])


def test_allowed_ids_each_on_the_python_seam(monkeypatch):
    """One entry per query; id lists become filters for the call (one per distinct OBJECT) and are closed afterwards, a caller's
    filter stays open, None leaves a query unrestricted; every query equals the single-filter search of its own entry; the length
    must match and the keyword does not combine with allowed_ids, distinct_by or per_group."""
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    rng = np.random.default_rng(5)
    vocab = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(90)]
    emb = RandomProjectionEmbedder(16)
    stub = _StubNative(emb.embed(texts))
    dense = si.DenseIndex.from_native(stub, [f"p{i}" for i in range(90)], embedder=emb)
    tenant_a = [f"p{i}" for i in range(0, 90, 3)] + ["ghost"]
    tenant_b = [f"p{i}" for i in range(1, 90, 3)]
    mine = dense.make_filter([f"p{i}" for i in range(40, 50)])
    n_before = len(stub.made)
    queries = [texts[0], texts[1], texts[2], texts[45], texts[3], "nothing known here"]
    each = [tenant_a, tenant_b, tenant_a, mine, None, ["ghost"]]
    got = dense.search_batch(queries, 5, allowed_ids_each=each)
    assert len(stub.each_calls) == 1 and len(stub.each_calls[0]) == 6                      # ONE native call for the batch
    made = stub.made[n_before:]
    assert len(made) == 3 and [m.closed for m in made] == [1, 1, 1] and mine.closed == 0   # tenant_a once, tenant_b, ["ghost"]
    flt = stub.each_calls[0]
    assert flt[0] is flt[2] and flt[0] is not flt[1] and flt[3] is mine and flt[4] is None and flt[5].count == 0
    assert flt[0].rows.tolist() == list(range(0, 90, 3))
    for qtext, entry, res in zip(queries, each, got):
        want = dense.search(qtext, 5) if entry is None else dense.search(qtext, 5, allowed_ids=entry)
        assert res == want
    assert got[5] == [] and [d for d, _, _ in got[3]][0] == "p45"
    vec = emb.embed(queries)
    assert dense.search_vectors(vec, 5, allowed_ids_each=each) == got
    rows = dense.search_rows_batch(queries, 5, allowed_ids_each=each)[1]
    assert [[f"p{i}" for i in r if i >= 0] for r in rows] == [[d for d, _, _ in res] for res in got]
    # equal lists that are different objects are different filters
    n_before = len(stub.made)
    dense.search_batch(queries[:2], 5, allowed_ids_each=[list(tenant_b), list(tenant_b)])
    assert len(stub.made) == n_before + 2
    # refusals
    for call in (lambda **kw: dense.search_batch(queries, 5, **kw), lambda **kw: dense.search_vectors(vec, 5, **kw),
                 lambda **kw: dense.search_rows_batch(queries, 5, **kw)):
        with pytest.raises(ValueError, match="one entry per query"):
            call(allowed_ids_each=each[:5])
        with pytest.raises(ValueError, match="does not combine"):
            call(allowed_ids_each=each, allowed_ids=tenant_a)
        with pytest.raises(ValueError, match="does not combine"):
            call(allowed_ids_each=each, distinct_by="title")
        with pytest.raises(ValueError):
            call(allowed_ids_each=each, distinct_by="title", per_group=2)
    # without the keyword nothing changes
    assert dense.search_batch(queries[:2], 5) == [dense.search(q, 5) for q in queries[:2]]
    assert len(stub.each_calls) == 4
