"""Group members (the best s rows of each of the top k groups), the parts that need no GPU: the header's documentation, the loud
failure without a device, the binding's argument checks, the oracle (tests/group_members_oracle.py) against a naive dict-of-lists
form and against the grouped oracle at s = 1, the host plan and the member-table builder (csrc/rq_group_members_plan.h) under the
sanitizers, and `per_group=` on the Python seam over a stub dense backend.  The GPU side is tests/test_gpu_group_members.py."""
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
import group_members_oracle as gmo  # noqa: E402
import group_oracle as gro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_group_fill_device", "rq_search_group_members_device", "rq_search_group_members_fixup_device", "rq_search_group_members"]


def test_header_documents_every_call_option_and_rule():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES
        assert code.index(name + "(") > code.index("#define RQ_GROUP_NONE"), f"{name} is declared after RQ_GROUP_NONE"
    assert re.search(r"#define RQ_GROUP_FILL_MAX 4096", code)
    assert re.search(r"rq_group_fill_device\(rq_index\* idx, const rq_filter\* f, const float\* d_queries, int B, int k, int s, int metric, const int64_t\* d_win_rows,\s*"
                     r"const int32_t\* d_win_groups, float\* d_scores, int64_t\* d_rows, int32_t\* d_count, int\* d_status, void\* stream\)", code)
    for name in ("rq_search_group_members_device", "rq_search_group_members_fixup_device"):
        assert re.search(name + r"\(rq_index\* idx, const rq_filter\* f, const float\* d_queries, int B, int k, int s, int metric, float\* d_scores,\s*"
                         r"int64_t\* d_rows, int32_t\* d_groups, int32_t\* d_count, int\* d_status, void\* stream\)", code)
    assert re.search(r"rq_search_group_members\(rq_index\* idx, const rq_filter\* f, const float\* queries, int B, int k, int s, int metric, float\* out_scores, int64_t\* out_rows,\s*"
                     r"int32_t\* out_groups, int32_t\* out_count\)", code)
    doc = h[h.index("group members: the best s rows"):h.index("#define RQ_GROUP_FILL_MAX")]
    for word in ("k x s <= RQ_MAX_K", "exactly as rq_search_grouped defines them", "k_eff = min(k, distinct groups among the rows in play)", "rows in play",
                 "score descending, then row ascending", "NaN counts as -inf", "-0.0 is\n *     +0.0", "zero-norm query scores every row 0.0", "-inf row is still a row",
                 "group of one", "min(s, rows in play of that group)", "(0.0, -1)", "(0.0, -1, RQ_GROUP_NONE, count 0)", "s = 1 is rq_search_grouped's answer bit for bit",
                 "member 0 of every slot is that slot's winner", "bits rq_score_rows returns", "csrc/rq_rowdot.h", "rq_score_rows_device", "count 1 and the result is rq_search's",
                 "lowest s rows in play of each of the first k_eff groups", "through the group, not through the ranking", "sorted by (id, row)", "need not be dense",
                 "binary search", "FIRST call", "dropped by rq_index_set_groups", "append does not invalidate", "rq_index_destroy", "rq_save stays as it is",
                 "4 B per grouped row + 8 B per distinct group", "one workgroup per (query, group slot)", "RQ_GROUP_FILL_MAX = 4096", "32 KiB", "count = -1",
                 "status\n *   becomes 1", "pure fill", "absent slot", "count 0", "same group may stand in two slots", "defers nothing", "no bin records",
                 "iff the grouped stage proved the query and every\n *   slot was filled", "SAME arguments", "synchronises", "Rung 2 and Rung 3", "exact route",
                 "temporary rq_filter", "usual ladder", "rq_search_grouped", "RQ_EINVAL", "1 <= B <= 65535", "stale filter", "RQ_EUNSUPPORTED", "RQ_ENODEVICE",
                 "keys (d_keys)", "merging members across shards", "DESIGN.md 4.16", "rq_search_train_device", "hints", '"pipeline" 1 and 2',
                 "counts the call as a search", '"group_fill_cap"', "can only lower", '"group_table_builds"', '"group_fill_calls"', '"group_fill_repaired"',
                 '"group_fill_rows_last"', "waits for the device"):
        assert word in doc, word
    grouped = h[h.index("grouped searches: the best row"):h.index("#define RQ_GROUP_NONE")]
    assert "rq_search_group_members*" in grouped and "group_size > 1" in grouped and "per-group member counts" in grouped


def test_calls_fail_loudly_without_a_device_or_with_null_arguments():
    lib = _native.load_library()
    want = -2 if _native.device_count() == 0 else -1                  # RQ_ENODEVICE / RQ_EINVAL
    P = _native._ptr
    buf, rows, ids, st = np.zeros(8, np.float32), np.zeros(8, np.int64), np.zeros(8, np.int32), np.zeros(2, np.int32)
    calls = [lambda: lib.rq_group_fill_device(None, None, P(buf), 1, 2, 2, 0, P(rows), P(ids), P(buf), P(rows), P(ids), P(st), None),
             lambda: lib.rq_search_group_members_device(None, None, P(buf), 1, 2, 2, 0, P(buf), P(rows), P(ids), P(ids), P(st), None),
             lambda: lib.rq_search_group_members_fixup_device(None, None, P(buf), 1, 2, 2, 0, P(buf), P(rows), P(ids), P(ids), P(st), None),
             lambda: lib.rq_search_group_members(None, None, P(buf), 1, 2, 2, 0, P(buf), P(rows), P(ids), P(ids))]
    for call in calls:
        assert call() == want
        if want == -2:
            assert "RQ_ENODEVICE" in _native.last_error() and "no CPU fallback" in _native.last_error()
        else:
            assert "null argument" in _native.last_error()


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
    for k, s in ((0, 1), (1, 0), (-1, 2), (2, -1), (_native.MAX_K + 1, 1), (1, _native.MAX_K + 1), (205, 5), (129, 8), (2 ** 16, 2 ** 16)):
        with pytest.raises(ValueError):
            idx.search_group_members(q, k, s)
        with pytest.raises(ValueError):
            idx.search_group_members_device(1, 1, k, s, 0, 2, 3, 4, 5, 6)
        with pytest.raises(ValueError):
            idx.search_group_members_fixup_device(1, 1, k, s, 0, 2, 3, 4, 5, 6)
        with pytest.raises(ValueError):
            idx.group_fill_device(1, 1, k, s, 0, 2, 3, 4, 5, 6, 7)
    for B in (0, 65536):
        with pytest.raises(ValueError):
            idx.search_group_members_device(1, B, 2, 2, 0, 2, 3, 4, 5, 6)
        with pytest.raises(ValueError):
            idx.group_fill_device(1, B, 2, 2, 0, 2, 3, 4, 5, 6, 7)
    with pytest.raises(ValueError, match="metric"):
        idx.search_group_members(q, 2, 2, 2)
    with pytest.raises(ValueError, match="queries"):
        idx.search_group_members(np.zeros((1, 9), np.float32), 2, 2)
    with pytest.raises(ValueError, match="RowFilter"):
        idx.search_group_members(q, 2, 2, row_filter=object())


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_equals_a_naive_dict_of_lists_on_random_lists_with_ties():
    rng = np.random.default_rng(17)
    sizes_seen = set()
    for trial in range(300):
        m = int(rng.integers(1, 80))
        k = int(rng.integers(1, 12))
        s = int(rng.integers(1, 6))
        offset = int(rng.choice([0, 1000]))
        rows = rng.choice(500, size=m, replace=False).astype(np.int64)
        scores = rng.integers(-3, 4, size=m).astype(np.float32) / 2            # few distinct values: ties everywhere, -0.0 among them
        scores[scores == 0] = rng.choice(np.float32([0.0, -0.0]), size=int((scores == 0).sum()))
        if trial % 5 == 0:
            scores[rng.integers(0, m)] = -np.inf
        if trial % 6 == 0:
            scores[rng.integers(0, m)] = np.nan                               # counts as -inf, still a member
        groups = rng.integers(-1, max(m // 4, 1), size=m).astype(np.int64)    # groups smaller than, equal to and larger than s
        if trial % 7 == 0:
            groups[rng.integers(0, m)] = 2 ** 31 - 1
        mask = rng.random(m) < 0.8 if trial % 3 == 0 else np.ones(m, bool)
        play = np.flatnonzero(mask)
        gs, gr, gg, gc = gmo.members(scores[play], rows[play] + offset, groups[play], k, s)
        naive = gmo.naive_dict_of_lists(scores[play], rows[play] + offset, groups[play], k, s)
        k_eff = len(naive)
        distinct = len({("g", int(x)) if x >= 0 else ("r", int(y)) for x, y in zip(groups[play], rows[play])})
        assert k_eff == min(k, distinct), trial
        for j, (g, mem) in enumerate(naive):
            assert gg[j] == g and gc[j] == len(mem), trial
            assert gr[j, :len(mem)].tolist() == [r for r, _ in mem] and gs[j, :len(mem)].tolist() == [v for _, v in mem], trial
            assert (gr[j, len(mem):] == -1).all() and not gs[j, len(mem):].any(), trial
            in_play = int((groups[play] == g).sum()) if g >= 0 else 1
            assert gc[j] == min(s, in_play), trial
            sizes_seen.add(int(np.sign(in_play - s)))
        assert (gr[k_eff:] == -1).all() and not gs[k_eff:].any() and (gg[k_eff:] == -1).all() and not gc[k_eff:].any(), trial
        assert not (np.signbit(gs) & (gs == 0)).any() and not np.isnan(gs).any(), trial      # -0.0 leaves as +0.0, NaN as -inf
    assert sizes_seen == {-1, 0, 1}                                              # groups smaller than, equal to and larger than s


def test_oracle_from_the_full_ranking_and_its_identities():
    x16 = orc.synthetic_corpus(300, 48, seed=5, clustered=True)
    q = orc.synthetic_queries(5, 48, seed=6)
    scores = orc.exact_scores(q, x16, orc.METRIC_COSINE)
    grp = np.arange(300) // 7
    grp[::11] = -1
    mask = np.arange(300) % 3 != 0
    for m, off in ((None, 0), (mask, 0), (None, 5000)):
        # s = 1 is the grouped answer
        ws, wr, wg = gro.grouped_from_scores(scores, grp, 12, m, off)
        ms, mr, mg, mc = gmo.members_from_scores(scores, grp, 12, 1, m, off)
        assert np.array_equal(mr[:, :, 0], wr) and np.array_equal(mg, wg) and np.array_equal(ms[:, :, 0].view(np.uint32), ws.view(np.uint32))
        assert np.array_equal(mc, (wr >= 0).astype(np.int32))
        # member 0 is the winner, whatever s; a larger s only extends every slot
        for s in (2, 3, 8):
            bs, br, bg, bc = gmo.members_from_scores(scores, grp, 12, s, m, off)
            assert np.array_equal(br[:, :, 0], wr) and np.array_equal(bg, wg) and np.array_equal(bs[:, :, 0].view(np.uint32), ws.view(np.uint32))
            in_play = np.ones(300, bool) if m is None else m
            for b in range(5):
                for j in range(12):
                    rows_j = br[b, j, :bc[b, j]] - off
                    want_n = 1 if bg[b, j] < 0 else int(((grp == bg[b, j]) & in_play).sum())
                    assert bc[b, j] == min(s, want_n) and in_play[rows_j].all()
                    assert (grp[rows_j] == bg[b, j]).all() if bg[b, j] >= 0 else rows_j.tolist() == [wr[b, j] - off]
                    sc = scores[b, rows_j]
                    assert np.array_equal(bs[b, j, :bc[b, j]], sc) and (np.diff(sc) <= 0).all()
    # no group set: every slot has count 1 and the result is the plain search's
    ps, pr = orc.dense_topk(q, x16, 12)
    ns, nr, ng, nc = gmo.members_topk(q, x16, np.full(300, -1), 12, 3)
    assert np.array_equal(nr[:, :, 0], pr) and np.array_equal(ns[:, :, 0].view(np.uint32), ps.view(np.uint32)) and (nc == 1).all() and (ng == -1).all() and (nr[:, :, 1:] == -1).all()
    # a zero-norm query: the lowest s rows in play of each of the first k_eff groups
    zs, zr, zg, zc = gmo.members_topk(np.zeros((1, 48), np.float32), x16, np.arange(300) // 7, 3, 4)
    assert zr[0].tolist() == [[0, 1, 2, 3], [7, 8, 9, 10], [14, 15, 16, 17]] and not zs.any() and (zc == 4).all()
    # every row in one group: k_eff = 1
    os_, or_, og, oc = gmo.members_topk(q, x16, np.zeros(300, np.int64), 4, 5)
    assert np.array_equal(or_[:, 0, :], pr[:, :5]) and (oc[:, 0] == 5).all() and (oc[:, 1:] == 0).all() and (or_[:, 1:] == -1).all()
    assert gmo.table_sizes([3, -1, 3, 9, 3]) == {3: 3, 9: 1}
    assert gmo.oversized_queries(np.array([[3, 9], [9, -1]]), [3, -1, 3, 9, 3], 2).tolist() == [True, False]


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------
def test_plan_table_builder_and_argument_checks_on_the_host(tmp_path):
    """tests/native/group_members_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the
    flags are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "group_members_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "group_members_plan_check.cpp"), "-o", exe],
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
    """Host stand-in for _native.NativeIndex (test scaffolding, the product has no CPU backend): the oracles over fp16 rows."""
    device, devices = 0, [0]

    def __init__(self, x):
        self.x16 = orc.prepare_rows_f32(np.asarray(x, np.float32), True)
        self.dim = self.x16.shape[1]
        self.groups = np.full(len(self), -1, np.int64)
        self.made, self.calls = [], []

    def __len__(self):
        return self.x16.shape[0]

    def add_f32(self, x, normalize=True):
        self.x16 = np.concatenate([self.x16, orc.prepare_rows_f32(np.asarray(x, np.float32), True)])
        self.groups = np.concatenate([self.groups, np.full(len(x), -1, np.int64)])

    def make_filter(self, rows):
        self.made.append(_StubFilter(rows))
        return self.made[-1]

    def set_groups(self, groups, row_begin=0):
        self.groups[row_begin:row_begin + len(groups)] = np.asarray(groups)

    def _mask(self, row_filter):
        if row_filter is None:
            return None
        mask = np.zeros(len(self), dtype=bool)
        mask[row_filter.rows] = True
        return mask

    def search(self, q, k, metric=0, *, row_filter=None):
        return orc.dense_topk(q, self.x16, k, metric)

    def search_grouped(self, q, k, metric=0, *, row_filter=None):
        self.calls.append(("grouped", int(k), 1, row_filter))
        return gro.grouped_topk(q, self.x16, self.groups, k, metric, self._mask(row_filter))

    def search_group_members(self, q, k, group_size, metric=0, *, row_filter=None):
        assert int(k) * int(group_size) <= _native.MAX_K
        self.calls.append(("members", int(k), int(group_size), row_filter))
        return gmo.members_topk(q, self.x16, self.groups, k, group_size, metric, self._mask(row_filter))


def test_per_group_on_the_python_seam(tmp_path, monkeypatch):
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    monkeypatch.setattr(_native, "RowFilter", _StubFilter)
    rng = np.random.default_rng(4)
    vocab = [f"w{i}" for i in range(30)]
    texts = [" ".join(rng.choice(vocab, size=6)) for _ in range(90)]
    sizes = [1, 2, 3, 4] * 9                                                     # 36 articles of one to four passages
    titles = [f"article {a}" for a, n in enumerate(sizes) for _ in range(n)]
    titles[5] = ""                                                            # an empty title: a group of its own
    docs = [si.Document(id=f"p{i}", text=texts[i], title=titles[i], metadata={}) for i in range(90)]
    emb = RandomProjectionEmbedder(16)
    stub = _StubNative(np.zeros((0, 16), np.float32))
    dense = si.DenseIndex.from_native(stub, [], [], embedder=emb)
    dense.add_documents(docs)
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=dense)
    r.bm25_index.add_documents(docs)
    r.documents.update({d.id: d for d in docs})
    query = texts[7]
    qv = emb.embed([query])
    table, ids = {}, []
    for t in titles:
        ids.append(-1 if not t else table.setdefault(t, len(table)))
    ids = np.array(ids)

    got = dense.search(query, 8, distinct_by="title", per_group=3)
    assert stub.calls[-1][:3] == ("members", 8, 3) and np.array_equal(stub.groups, ids)
    ws, wr, wg, wc = gmo.members_topk(qv, stub.x16, ids, 8, 3)
    want = [(f"p{i}", float(s), texts[i]) for j in range(8) for s, i in zip(ws[0, j, :wc[0, j]], wr[0, j, :wc[0, j]])]
    assert got == want and len(got) == int(wc.sum()) and 8 < len(got) < 24      # group by group, members best first, no padding entries
    by_title = [titles[int(d[1:])] or d for d, _, _ in got]
    assert len(set(by_title)) == 8 and all(by_title.count(t) <= 3 for t in set(by_title))
    assert [t for i, t in enumerate(by_title) if i == 0 or by_title[i - 1] != t] == list(dict.fromkeys(by_title))      # a group's members are adjacent
    one = dense.search(query, 8, distinct_by="title")
    assert [g for i, g in enumerate(got) if i == 0 or by_title[i - 1] != by_title[i]] == one                        # member 0 of every group is today's answer
    assert dense.search_batch([query, texts[9]], 8, distinct_by="title", per_group=3)[0] == got == dense.search_vectors(qv, 8, distinct_by="title", per_group=3)[0]
    assert r.dense_search(query, 8, distinct_by="title", per_group=3) == [(d, s) for d, s, _ in got]
    # per_group = 1 or absent: the grouped call, today's result
    n_calls = len(stub.calls)
    assert dense.search(query, 8, distinct_by="title", per_group=1) == one == dense.search(query, 8, distinct_by="title", per_group=None)
    assert all(c[0] == "grouped" for c in stub.calls[n_calls:])
    assert r.dense_search(query, 8, distinct_by="title", per_group=1) == [(d, s) for d, s, _ in one]
    # combines with allowed_ids (ids make a filter that is closed again, a reusable one stays open)
    allowed = [f"p{i}" for i in range(0, 90, 2)] + ["ghost"]
    sub = dense.search(query, 8, allowed_ids=allowed, distinct_by="title", per_group=2)
    assert stub.calls[-1][3] is stub.made[-1] and stub.made[-1].closed == 1 and {d for d, _, _ in sub} <= set(allowed)
    mask = np.zeros(90, bool)
    mask[::2] = True
    fs, fr, fg, fc = gmo.members_topk(qv, stub.x16, ids, 8, 2, mask=mask)
    assert [d for d, _, _ in sub] == [f"p{i}" for j in range(8) for i in fr[0, j, :fc[0, j]]]
    mine = dense.make_filter(allowed)
    assert dense.search(query, 8, allowed_ids=mine, distinct_by="title", per_group=2) == sub and mine.closed == 0
    # top_k is clamped so that k x per_group stays within MAX_K; k beyond the groups: no padding tuples
    everything = dense.search(query, 2000, distinct_by="title", per_group=4)
    assert stub.calls[-1][:3] == ("members", 90, 4) and len(everything) == 90 and {d for d, _, _ in everything} == {f"p{i}" for i in range(90)}
    dense.search(query, 2000, distinct_by="title", per_group=100)
    assert stub.calls[-1][:3] == ("members", _native.MAX_K // 100, 100)
    # refusals
    for bad in (0, -1, 2.5, "2", True):
        with pytest.raises(ValueError):
            dense.search(query, 8, distinct_by="title", per_group=bad)
    with pytest.raises(ValueError):
        dense.search(query, 8, distinct_by="title", per_group=_native.MAX_K + 1)
    for call in (dense.search, dense.search_batch, dense.search_vectors, r.dense_search):
        with pytest.raises(ValueError, match="distinct_by"):
            call(query if call in (dense.search, r.dense_search) else ([query] if call is dense.search_batch else qv), 8, per_group=2)
    for call in (r.bm25_index.search, r.bm25_search, r.hybrid_search):
        with pytest.raises(ValueError, match="per_group"):
            call(query, 6, distinct_by="title", per_group=2)
        assert call(query, 6, distinct_by="title", per_group=1) == call(query, 6, distinct_by="title")
    with pytest.raises(ValueError, match="per_group"):
        dense.search_rows_batch([query], 8, distinct_by="title", per_group=2)
    # nothing to search, nothing asked for
    n_calls = len(stub.calls)
    assert dense.search(query, 0, distinct_by="title", per_group=2) == [] and dense.search_batch([], 5, distinct_by="title", per_group=2) == []
    empty = si.DenseIndex.from_native(_StubNative(np.zeros((0, 16), np.float32)), [], embedder=emb)
    assert empty.search("anything", 5, distinct_by="title", per_group=2) == [] and len(stub.calls) == n_calls
