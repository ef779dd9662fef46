"""Grouped searches, the parts that need no GPU: the header's documentation, the loud failure without a device, the binding's
argument checks, the oracle (tests/group_oracle.py) against a naive dict-based collapse, the host plan (csrc/rq_group_plan.h) under
the sanitizers, and the Python seam of DenseIndex / BM25Index / HybridRetriever over a stub dense backend.  The GPU side is
tests/test_gpu_grouped.py."""
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
import group_oracle as gro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_index_set_groups", "rq_index_get_groups", "rq_group_collapse_device", "rq_search_grouped_device", "rq_search_grouped_fixup_device",
             "rq_search_grouped"]


def test_header_documents_every_call_option_and_rule():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
    assert re.search(r"#define RQ_GROUP_NONE \(-1\)", code) and _native.GROUP_NONE == -1
    assert re.search(r"rq_index_set_groups\(rq_index\* idx, int64_t row_begin, int64_t n_rows, const int32_t\* groups\)", code)
    assert re.search(r"rq_group_collapse_device\([^)]*const int32_t\* d_cand_groups, int B, int m, int k,[^)]*int32_t\* d_groups, uint64_t\* d_keys, int\* d_status, void\* stream\)", code)
    for name in ("rq_search_grouped_device", "rq_search_grouped_fixup_device"):
        assert re.search(name + r"\(rq_index\* idx, const rq_filter\* f, const float\* d_queries, int B, int k, int metric,[^)]*int32_t\* d_groups, uint64_t\* d_keys, int\* d_status, void\* stream\)", code)
    assert re.search(r"rq_search_grouped\(rq_index\* idx, const rq_filter\* f, const float\* queries, int B, int k, int metric,[^)]*int32_t\* out_groups\)", code)
    doc = h[h.index("grouped searches: the best row"):h.index("#define RQ_GROUP_NONE")]
    for word in ("RQ_GROUP_NONE (-1)", "group of its own", "need not be dense", "score descending, then row ascending", "NaN counts as -inf", "-0.0 is +0.0",
                 "zero-norm query", "rows in play", "winner", "k_eff = min(k, distinct groups among the rows in play)", "(0.0, -1, RQ_GROUP_NONE)", "key 0",
                 "bit for bit", "k_eff = 1", "lowest row of each of the first k_eff groups", "same bits as rq_score_rows",
                 "as an\n *   append does", "4 B per row", "rq_index_reserve", "host copy", "appended later are RQ_GROUP_NONE", "NOT written by\n *   rq_save",
                 "absent candidate", "rq_mmr_select_device", "may be NULL", "looked up by row", "merged from several shards", "DESIGN.md 4.16",
                 "at least k\n *   distinct groups", '"pipeline" = 0', "rq_search_filtered_device", "m1", "proven", "every row in play", "synchronises",
                 "Rung 2", "Rung 3", "exclusion loop", "temporary rq_filter", "at least one group", "rq_search_mmr", "RQ_EINVAL", "stale filter", "RQ_EUNSUPPORTED",
                 "RQ_ENODEVICE", "group_size > 1", "per-group member counts", "rq_search_train_device", "hints", '"pipeline" 1 and 2', '"scan_ahead"',
                 "counts a grouped call as a search", '"group_fetch"', '"group_fetch_cap"', '"range_cand_cap"', '"group_calls"', '"group_repaired"',
                 '"group_rounds_last"'):
        assert word in doc, word


def test_calls_fail_loudly_without_a_device_or_with_null_arguments():
    lib = _native.load_library()
    want = -2 if _native.device_count() == 0 else -1                  # RQ_ENODEVICE / RQ_EINVAL
    P = _native._ptr
    buf, rows, ids, st = np.zeros(8, np.float32), np.zeros(8, np.int64), np.zeros(8, np.int32), np.zeros(2, np.int32)
    calls = [lambda: lib.rq_index_set_groups(None, 0, 4, P(ids)), lambda: lib.rq_index_get_groups(None, 0, 4, P(ids)),
             lambda: lib.rq_group_collapse_device(None, P(rows), P(buf), None, 1, 4, 2, P(buf), P(rows), P(ids), None, P(st), None),
             lambda: lib.rq_search_grouped_device(None, None, P(buf), 1, 2, 0, P(buf), P(rows), P(ids), None, P(st), None),
             lambda: lib.rq_search_grouped_fixup_device(None, None, P(buf), 1, 2, 0, P(buf), P(rows), P(ids), None, P(st), None),
             lambda: lib.rq_search_grouped(None, None, P(buf), 1, 2, 0, P(buf), P(rows), P(ids))]
    for call in calls:
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
    q = np.zeros((1, 8), np.float32)
    for k in (0, -1, _native.MAX_K + 1):
        with pytest.raises(ValueError):
            idx.search_grouped(q, k)
        with pytest.raises(ValueError):
            idx.search_grouped_device(1, 1, k, 0, 2, 3, 4, None, 5)
        with pytest.raises(ValueError):
            idx.search_grouped_fixup_device(1, 1, k, 0, 2, 3, 4, None, 5)
    for B, m, k in ((0, 4, 2), (65536, 4, 2), (1, 0, 1), (1, _native.MAX_K + 1, 2), (1, 4, 5), (1, 4, 0)):
        with pytest.raises(ValueError):
            idx.group_collapse_device(1, 2, None, B, m, k, 3, 4, 5, None, 6)
    with pytest.raises(ValueError):
        idx.search_grouped_device(1, 0, 2, 0, 2, 3, 4, None, 5)                  # B = 0
    with pytest.raises(ValueError, match="metric"):
        idx.search_grouped(q, 2, 2)
    with pytest.raises(ValueError, match="queries"):
        idx.search_grouped(np.zeros((1, 9), np.float32), 2)
    with pytest.raises(ValueError, match="RowFilter"):
        idx.search_grouped(q, 2, row_filter=object())
    for bad in (np.array([0, -2]), np.array([0.5, 1.0]), np.array([[1, 2]]), np.array([2 ** 31]), "ab"):
        with pytest.raises(ValueError):
            idx.set_groups(bad)
    with pytest.raises(ValueError):
        idx.set_groups(np.array([1, 2]), -1)
    with pytest.raises(ValueError):
        idx.get_groups(-1, 2)
    with pytest.raises(ValueError):
        idx.get_groups(0, -2)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_equals_a_naive_dict_collapse_on_random_lists_with_ties():
    rng = np.random.default_rng(7)
    for trial in range(200):
        m = int(rng.integers(1, 60))
        k = int(rng.integers(1, m + 1))
        rows = rng.choice(500, size=m, replace=False).astype(np.int64)
        scores = rng.integers(-3, 4, size=m).astype(np.float32) / 2            # few distinct values: ties everywhere, -0.0 among them
        scores[scores == 0] = rng.choice(np.float32([0.0, -0.0]), size=int((scores == 0).sum()))
        if trial % 5 == 0:
            scores[rng.integers(0, m)] = -np.inf
        groups = rng.integers(-1, max(m // 3, 1), size=m).astype(np.int64)
        if trial % 7 == 0:
            groups[rng.integers(0, m)] = 2 ** 31 - 1
        s, r, g, status = gro.collapse(scores, rows, groups, k, 500)
        naive = gro.naive_dict_collapse(scores, rows, groups, k)
        k_eff = len(naive)
        assert r[:k_eff].tolist() == [n[0] for n in naive] and g[:k_eff].tolist() == [n[2] for n in naive], trial
        assert s[:k_eff].tolist() == [n[1] for n in naive] and not (np.signbit(s) & (s == 0)).any(), trial      # (-0.0 leaves as +0.0)
        assert (r[k_eff:] == -1).all() and not s[k_eff:].any() and (g[k_eff:] == -1).all()
        distinct = len({("g", int(x)) if x >= 0 else ("r", int(y)) for x, y in zip(groups, rows)})
        assert status == (0 if distinct >= k else 1) and k_eff == min(k, distinct)


def test_oracle_absent_candidates_row_offset_and_the_full_ranking():
    rows = np.array([50, 11, 3, 10, -1, 100, 99, 7, 1011], np.int64)
    scores = np.array([0.1, 0.9, 0.9, 0.9, 5.0, 5.0, np.nan, 0.2, 0.3], np.float32)
    groups = np.array([4, 4, -1, 9, 9, 9, 9, 9, 9], np.int64)
    s, r, g, status = gro.collapse(scores, rows, groups, 5, 100)
    assert r.tolist() == [3, 10, 11, -1, -1] and g.tolist() == [-1, 9, 4, -1, -1] and s.tolist() == [np.float32(0.9)] * 3 + [0, 0] and status == 1
    s, r, g, status = gro.collapse(scores, rows + 1000, groups, 2, 100, row_offset=1000)
    assert r.tolist() == [1003, 1010] and status == 0                            # (row 999 = -1 + 1000 lies below the offset, 2011 beyond the shard)
    assert gro.lookup_groups(np.array([[1005, 999, -1, 1100]]), np.arange(100), 1000).tolist() == [[5, -1, -1, -1]]
    # from a full ranking: equal to collapsing dense_topk(k = N); with a mask only allowed rows take part; no group set = the plain search
    x16 = orc.synthetic_corpus(300, 48, seed=5, clustered=True)
    q = orc.synthetic_queries(5, 48, seed=6)
    grp = np.arange(300) // 7
    fs, fr = orc.dense_topk(q, x16, 300)
    ws, wr, wg = gro.grouped_topk(q, x16, grp, 12)
    cs, cr, cg, _ = gro.collapse_batch(fs, fr, gro.lookup_groups(fr, grp), 12, 300)
    assert np.array_equal(wr, cr) and np.array_equal(wg, cg) and np.array_equal(ws.view(np.uint32), cs.view(np.uint32))
    assert all(len(set(row.tolist())) == 12 for row in wg)
    mask = np.arange(300) % 3 == 0
    ms, mr, mg = gro.grouped_topk(q, x16, grp, 12, mask=mask)
    assert (mr % 3 == 0).all() and all(len(set(row.tolist())) == 12 for row in mg)
    ps, pr = orc.dense_topk(q, x16, 12)
    ns, nr, ng = gro.grouped_topk(q, x16, np.full(300, -1), 12)
    assert np.array_equal(nr, pr) and np.array_equal(ns.view(np.uint32), ps.view(np.uint32)) and (ng == -1).all()
    os_, or_, og = gro.grouped_topk(q, x16, np.zeros(300, np.int64), 12)
    assert np.array_equal(or_[:, 0], pr[:, 0]) and (or_[:, 1:] == -1).all()    # one group for all rows: k_eff = 1
    zs, zr, zg = gro.grouped_topk(np.zeros((1, 48), np.float32), x16, grp, 5)
    assert zr[0].tolist() == [0, 7, 14, 21, 28] and not zs.any()               # a zero-norm query: the lowest row of each of the first groups


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------
def test_plan_and_argument_checks_on_the_host(tmp_path):
    """tests/native/group_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "group_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "group_plan_check.cpp"), "-o", exe],
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
        self.groups = np.full(len(self), -1, np.int64)
        self.made, self.pushes, self.calls = [], [], []

    def __len__(self):
        return self.x16.shape[0]

    def grow(self, x):
        self.x16 = np.concatenate([self.x16, orc.prepare_rows_f32(np.asarray(x, np.float32), True)])
        self.groups = np.concatenate([self.groups, np.full(len(x), -1, np.int64)])

    def add_f32(self, x, normalize=True):
        self.grow(x)

    def make_filter(self, rows):
        self.made.append(_StubFilter(rows))
        return self.made[-1]

    def set_groups(self, groups, row_begin=0):
        groups = np.asarray(groups)
        assert groups.dtype == np.int32 and row_begin + len(groups) <= len(self)
        self.pushes.append((int(row_begin), groups.tolist()))
        self.groups[row_begin:row_begin + len(groups)] = groups

    def search(self, q, k, metric=0, *, row_filter=None):
        return orc.dense_topk(q, self.x16, k, metric)

    def search_grouped(self, q, k, metric=0, *, row_filter=None):
        self.calls.append((int(k), row_filter))
        mask = None
        if row_filter is not None:
            mask = np.zeros(len(self), dtype=bool)
            mask[row_filter.rows] = True
        return gro.grouped_topk(q, self.x16, self.groups, k, metric, mask)


def test_distinct_by_on_the_python_seam(tmp_path, monkeypatch):
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    rng = np.random.default_rng(4)
    vocab = [f"w{i}" for i in range(30)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(90)]
    titles = [f"article {i // 6}" for i in range(90)]                        # 15 articles of six passages
    titles[3] = ""                                                            # an empty title
    sections = [None if i % 9 == 0 else f"s{i % 4}" for i in range(90)]      # a second key; missing for every ninth passage
    docs = [si.Document(id=f"p{i}", text=texts[i], title=titles[i], metadata={} if sections[i] is None else {"section": sections[i]}) for i in range(90)]
    emb = RandomProjectionEmbedder(16)
    stub = _StubNative(np.zeros((0, 16), np.float32))
    dense = si.DenseIndex.from_native(stub, [], [], embedder=emb)
    dense.add_documents(docs[:60])
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    r.bm25_index.add_documents(docs[:60])
    r.documents.update({d.id: d for d in docs})
    query = texts[7]
    qv = emb.embed([query])

    def title_ids(n):
        table, out = {}, []
        for t in titles[:n]:
            out.append(-1 if not t else table.setdefault(t, len(table)))
        return out
    # the lazy id mapping: nothing is pushed before the first grouped call; then every row, ids in first-seen order, "" = its own group
    assert stub.pushes == []
    plain = dense.search(query, 8)
    assert stub.pushes == [] and len({titles[int(d[1:])] for d, _, _ in plain}) < 8       # the plain search repeats an article
    got = dense.search(query, 8, distinct_by="title")
    assert stub.pushes == [(0, title_ids(60))] and stub.pushes[0][1][3] == -1
    ws, wr, _ = gro.grouped_topk(qv, stub.x16, np.array(title_ids(60)), 8)
    assert got == [(f"p{i}", float(s), texts[i]) for s, i in zip(ws[0], wr[0])]
    assert len({titles[int(d[1:])] for d, _, _ in got}) == 8
    assert dense.search_batch([query, texts[9]], 8, distinct_by="title")[0] == got == dense.search_vectors(qv, 8, distinct_by="title")[0]
    assert dense.search_rows_batch([query], 8, distinct_by="title")[1].tolist() == wr.tolist()
    assert len(stub.pushes) == 1                                                          # nothing new: nothing pushed
    # rows added later: only they are pushed, and the mapping goes on
    dense.add_documents(docs[60:])
    r.bm25_index.add_documents(docs[60:])
    dense.search(query, 8, distinct_by="title")
    assert len(stub.pushes) == 2 and stub.pushes[1] == (60, title_ids(90)[60:])
    # switching keys re-pushes everything; a missing key means its own group
    got = dense.search(query, 30, distinct_by="section")
    table = {}
    want_ids = [-1 if s is None else table.setdefault(s, len(table)) for s in sections]
    assert len(stub.pushes) == 3 and stub.pushes[2] == (0, want_ids)
    secs = [sections[int(d[1:])] for d, _, _ in got]
    assert len(got) == 4 + 10 and sorted(s for s in secs if s is not None) == ["s0", "s1", "s2", "s3"] and secs.count(None) == 10
    dense.search(query, 8, distinct_by="title")
    assert len(stub.pushes) == 4 and stub.pushes[3] == (0, title_ids(90))
    # k beyond the groups: no padding tuples; allowed_ids combine (ids make a filter that is closed again, a reusable one stays open)
    assert len(dense.search(query, 50, distinct_by="title")) == 15 + 1
    allowed = [f"p{i}" for i in range(0, 90, 2)] + ["ghost"]
    got = dense.search(query, 8, allowed_ids=allowed, distinct_by="title")
    assert stub.calls[-1][1] is stub.made[-1] and stub.made[-1].closed == 1 and {d for d, _, _ in got} <= set(allowed)
    assert len({titles[int(d[1:])] for d, _, _ in got}) == 8
    mine = dense.make_filter(allowed)
    assert dense.search(query, 8, allowed_ids=mine, distinct_by="title") == got and mine.closed == 0
    assert r.dense_search(query, 8, distinct_by="title") == [(d, s) for d, s, _ in dense.search(query, 8, distinct_by="title")]
    assert r.dense_search(query, 8) == [(d, s) for d, s, _ in dense.search(query, 8)]     # without the keyword: the plain search
    # BM25: collapsed on the host with its own tie rule (score descending, ties by DESCENDING row)
    bm = r.bm25_index
    scores = bm.get_scores(bm._tokenize(query))
    order = sorted((i for i in range(90) if scores[i] > 0), key=lambda i: (-scores[i], -i))
    want, seen = [], set()
    for i in order:
        if titles[i] and titles[i] in seen:
            continue
        seen.add(titles[i])
        want.append((f"p{i}", float(scores[i])))
    assert bm.search(query, 6, distinct_by="title") == want[:6] == r.bm25_search(query, 6, distinct_by="title")
    assert len(bm.search(query, 90, distinct_by="title")) == len(want)
    assert bm.search(query, 6) == [(f"p{i}", float(scores[i])) for i in order[:6]]        # without the keyword: as before
    sub = bm.search(query, 6, allowed_ids=allowed, distinct_by="title")
    assert {d for d, _ in sub} <= set(allowed) and len({titles[int(d[1:])] for d, _ in sub}) == len(sub)
    # the fused list holds one passage per title, in hybrid order, and is collapsed by the best hybrid score
    fused = r.hybrid_search(query, 6, 20, distinct_by="title")
    ft = [x.title for x in fused]
    assert len(fused) == 6 and len(set(ft)) == 6
    assert [x.hybrid_score for x in fused] == sorted((x.hybrid_score for x in fused), reverse=True)
    every = r._fuse(r.bm25_search(query, 20, distinct_by="title"), r.dense_search(query, 20, distinct_by="title"), 10 ** 6)
    best = {}
    for x in every:
        best.setdefault(x.title or x.doc_id, x)
    assert [x.doc_id for x in fused] == [x.doc_id for x in list(best.values())[:6]]
    assert [x.doc_id for x in r.hybrid_search(query, 6, 20)] == [x.doc_id for x in r._fuse(r.bm25_search(query, 20), r.dense_search(query, 20), 6)]
    with pytest.raises(ValueError):
        r.hybrid_search(query, 6, 20, distinct_by="title", complete_scores=True)
    # nothing to search, nothing asked for
    n_calls = len(stub.calls)
    assert dense.search(query, 0, distinct_by="title") == [] and dense.search_batch([], 5, distinct_by="title") == []
    empty = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32)), [], embedder=emb)
    assert empty.search("anything", 5, distinct_by="title") == [] and len(stub.calls) == n_calls
    none = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b2.pkl"), chroma_persist_path=str(tmp_path / "c2"), dense_index=dense)
    none.dense_index = None
    assert none.dense_search("x", distinct_by="title") == []
