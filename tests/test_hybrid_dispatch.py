"""Which native call the batch calls of HybridRetriever reach -- hybrid_search_batch, get_scores_for_router_batch, route_batch under a host
gate and dense_search_batch -- for every combination of the restricting keywords (`allowed_ids`, `allowed_ids_each`, `complete_scores`,
`distinct_by`), over a real BM25Index on the host backend and a DenseIndex over the recording stand-ins of tests/test_dense_dispatch.py,
so no library and no device is needed.  Pinned here: the dense native method, how often, k / metric / filters / row_filter, one made
filter per distinct object of ids and its closing (also when the native call raises), a caller's own HybridFilter left open, which
embedder path ran, what an index of someone else's is handed, the order and the texts of the refusals, and the early returns.  What the
calls COMPUTE is the business of the feature tests (test_hybrid, test_hybrid_filtered, test_hybrid_grouped, test_router)."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import router_scenario as rs  # noqa: E402
from test_dense_dispatch import D, EVEN, EVEN_ROWS, GROUPS, N, SEARCHES, _answer, _DevEmb, _Emb, _Filter, _Native, _stub_filter_class  # noqa: E402,F401

Q = ["w1 x2", "w3", "x4 w0 w2", "nothing known"]
B, TOP, POOL = len(Q), 5, 8
DOCS = [si.Document(id=f"p{i}", text=f"w{i % 5} x{i % 7} w{(i * 3) % 5}", title=f"t{i % 6}") for i in range(N)]
GATE = rs.gate()


def _retriever(native=None, emb=None, dense="own", docs=DOCS):
    """(retriever, native stand-in, embedder): BM25 over `docs`, and a DenseIndex over the stand-in (`dense` = "own"), no dense index
    (None), or whatever object is given."""
    native = _Native() if native is None else native
    emb = _Emb() if emb is None else emb
    if isinstance(dense, str):
        dense = si.DenseIndex.from_native(native, [f"p{i}" for i in range(len(native))], embedder=emb, metric="cosine")
        dense._metas = [{"title": f"t{i % 6}"} for i in range(len(native))]
    r = si.HybridRetriever(bm25_persist_path=None, dense_index=dense)
    if dense is None:
        r.dense_index = None
    if docs:
        r.bm25_index.add_documents(docs)
    for d in DOCS:
        r.documents[d.id] = d
    return r, native, emb


ENTRIES = {   # name -> call(retriever, queries, n, keywords)
    "hybrid_search_batch": lambda r, q, n, kw: r.hybrid_search_batch(q, n, POOL, **kw),
    "get_scores_for_router_batch": lambda r, q, n, kw: r.get_scores_for_router_batch(q, n, retrieval_pool_size=POOL, **kw),
    "route_batch": lambda r, q, n, kw: r.route_batch(q, GATE, n, num_passages=n, retrieval_pool_size=POOL, **kw),
    "dense_search_batch": lambda r, q, n, kw: r.dense_search_batch(q, POOL, **kw),
}
HYBRID = [e for e in ENTRIES if e != "dense_search_batch"]
SHARED = list(EVEN)
CASES = ["none", "ids", "each", "complete", "distinct", "distinct+ids"]


def _keywords(case, mine):
    return {"none": {}, "ids": dict(allowed_ids=EVEN), "each": dict(allowed_ids_each=[None, SHARED, SHARED, mine]), "complete": dict(complete_scores=True),
            "distinct": dict(distinct_by="title"), "distinct+ids": dict(distinct_by="title", allowed_ids=EVEN)}[case]


def _searches(native):
    return [c for c in native.calls if c["fn"] in SEARCHES]


def _ids_of(entry, got):
    """the ids an answer names, question by question, padding dropped"""
    if entry == "get_scores_for_router_batch":
        return [[d for d in c[2] if d] for c in got]
    if entry == "dense_search_batch":
        return [[d for d, _ in res] for res in got]
    return [[x.doc_id for x in res] for res in got]


@pytest.fixture
def device_rows(monkeypatch):
    """The two steps of DenseIndex that need torch, replaced by recorders: (queries, top_k) of a search, (queries, rows) of a scoring."""
    seen = []
    monkeypatch.setattr(si.DenseIndex, "_search_device_rows", lambda self, t, top_k: seen.append(("search", t, top_k)) or _answer(t.shape[0], min(top_k, len(self))))
    monkeypatch.setattr(si.DenseIndex, "_score_device_rows", lambda self, t, rows: seen.append(("score", t, rows.shape)) or np.full(rows.shape, 0.5, np.float32))
    return seen


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("entry,case", [(e, c) for e in ENTRIES for c in CASES if (e, c) != ("dense_search_batch", "complete")])      # (it has no complete_scores)
def test_batch_routes_over_this_modules_indexes(entry, case, on_device, device_rows):
    r, native, emb = _retriever(emb=_DevEmb() if on_device else _Emb())
    mine = r.make_filter(EVEN[:3])
    own = native.made[0]
    assert mine.dense is own and own.rows == EVEN_ROWS[:3] and mine.sparse is not None and len(native.made) == 1
    got = ENTRIES[entry](r, Q, TOP, _keywords(case, mine))
    made = native.made[1:]
    calls = _searches(native)
    if case in ("none", "complete") and on_device:       # the unrestricted routes take the queries where the embedder left them, embedded once
        assert (emb.dev, emb.host) == (1, 0) and [(s[0], s[1].shape, s[2]) for s in device_rows if s[0] == "search"] == [("search", (B, D), POOL)]
        assert not calls and not made
        assert [s[0] for s in device_rows] == (["search", "score"] if case == "complete" else ["search"])
        assert case != "complete" or device_rows[1][1] is device_rows[0][1]          # the vectors that searched are the vectors that score
    else:
        assert not device_rows and emb.host == 1 and getattr(emb, "dev", 0) == 0
        first = calls[0]
        assert first["B"] == B and first["k"] == POOL and first["metric"] == _native.METRIC_COSINE
        if case == "none":
            assert calls == [dict(fn="search", B=B, k=POOL, metric=0)] and not made      # (a plain backend's search takes no row_filter keyword)
        elif case == "complete":
            assert [c["fn"] for c in calls] == ["search", "score_rows"] and "row_filter" not in first and not made
            assert np.shape(calls[1]["rows"]) == (B, POOL) and calls[1]["B"] == B
        elif case == "ids":
            (flt,) = made                                                                 # one object of ids for the batch: one filter
            assert calls == [dict(fn="search_filtered_each", B=B, k=POOL, metric=0, filters=[flt] * B)] and flt.rows == EVEN_ROWS
        elif case == "each":
            (flt,) = made                                                                 # one list object given twice: one filter
            assert calls == [dict(fn="search_filtered_each", B=B, k=POOL, metric=0, filters=[None, flt, flt, own])] and flt.rows == EVEN_ROWS
        elif case == "distinct":
            assert calls == [dict(fn="search_grouped", B=B, k=POOL, metric=0, row_filter=None)] and not made
        else:
            (flt,) = made
            assert calls == [dict(fn="search_grouped", B=B, k=POOL, metric=0, row_filter=flt)] and flt.rows == EVEN_ROWS
    assert all(m.closed == 1 for m in made) and own.closed == 0 and mine.dense is own
    assert native.pushed == ([(0, GROUPS)] if case.startswith("distinct") else [])
    assert len(got) == B
    if entry == "get_scores_for_router_batch":
        assert all(isinstance(c, tuple) and [type(x) for x in c] == [list] * 4 and [len(x) for x in c] == [TOP] * 4 for c in got)
        assert all(isinstance(c[0][0], float) and isinstance(c[2][0], str) and c[3] == [r.documents[d].text if d else "" for d in c[2]] for c in got)
    if entry in HYBRID and entry != "route_batch":
        # the list view and the results name the same passages: one column producer
        other = "hybrid_search_batch" if entry == "get_scores_for_router_batch" else "get_scores_for_router_batch"
        assert _ids_of(entry, got) == _ids_of(other, ENTRIES[other](r, Q, TOP, _keywords(case, mine)))
    if entry == "route_batch":
        res, w = ENTRIES[entry](r, Q, TOP, dict(return_weights=True, **_keywords(case, mine)))
        assert _ids_of(entry, res) == _ids_of(entry, got) and w.shape == (B, TOP) and w.dtype == np.float64
        cols = ENTRIES["get_scores_for_router_batch"](r, Q, TOP, _keywords(case, mine))
        assert [sorted(x) for x in _ids_of(entry, got)] == [sorted(x) for x in _ids_of("get_scores_for_router_batch", cols)]      # num_passages = top_k: a reorder
    assert all(m.closed == 1 for m in native.made[1:]) and own.closed == 0


def test_dense_search_batch_takes_a_bare_row_filter_and_equal_lists_are_two_filters():
    r, native, emb = _retriever()
    bare = r.dense_index.make_filter(EVEN[:3])
    r.dense_search_batch(Q, POOL, allowed_ids=bare)
    assert _searches(native) == [dict(fn="search_filtered_each", B=B, k=POOL, metric=0, filters=[bare] * B)] and bare.closed == 0
    native.calls.clear()
    r.dense_search_batch(Q, POOL, allowed_ids=bare, distinct_by="title")
    assert _searches(native) == [dict(fn="search_grouped", B=B, k=POOL, metric=0, row_filter=bare)] and bare.closed == 0 and len(native.made) == 1
    for entry in ENTRIES:
        native.calls.clear()
        del native.made[1:]
        ENTRIES[entry](r, Q, TOP, dict(allowed_ids_each=[EVEN, list(EVEN), None, EVEN]))
        (call,) = _searches(native)
        one, two = native.made[1:]
        assert call["filters"] == [one, two, None, one] and one.closed == two.closed == 1, entry


@pytest.mark.parametrize("case", ["ids", "each", "distinct+ids"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_made_filters_are_closed_when_the_native_call_raises(entry, case):
    fn = "search_grouped" if case == "distinct+ids" else "search_filtered_each"
    r, native, emb = _retriever(_Native(fail=fn))
    mine = r.make_filter(EVEN[:3])
    with pytest.raises(RuntimeError, match=fn + " failed"):
        ENTRIES[entry](r, Q, TOP, _keywords(case, mine))
    assert len(native.made) == 2 and native.made[1].closed == 1 and native.made[0].closed == 0 and len(_searches(native)) == 1


class _Foreign:
    """A dense index of someone else's: `search(query, top_k)` and only the keywords its caller was given."""

    def __init__(self):
        self.seen = []

    def search(self, query, top_k, **kw):
        self.seen.append(("search", query, top_k, kw))
        return [("p1", 0.5, "text"), ("p4", 0.25, "text")]


class _ForeignBatch(_Foreign):
    def search_batch(self, queries, top_k, **kw):
        self.seen.append(("search_batch", queries, top_k, kw))
        return [[("p1", 0.5, "text"), ("p4", 0.25, "text")] for _ in queries]


@pytest.mark.parametrize("batched", [False, True], ids=["search", "search_batch"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_index_of_someone_elses_receives_only_the_keywords_that_were_given(entry, batched):
    foreign = _ForeignBatch() if batched else _Foreign()
    r, _, _ = _retriever(dense=foreign)
    mine = r.make_filter(EVEN[:3])
    assert mine.dense is None and mine.sparse is not None
    hybrid = entry != "dense_search_batch"
    even, three = sorted(EVEN), sorted(EVEN[:3])
    want = {   # case -> what the dense side sees: ("search_batch", keywords) once, or ("search", keywords of query q) for every query
        "none": ("search_batch", {}) if batched else ("search", [{}] * B),
        "ids": ("search", [dict(allowed_ids=even)] * B) if hybrid else
               ("search_batch", dict(allowed_ids_each=[even] * B)) if batched else ("search", [dict(allowed_ids=even)] * B),
        "each": ("search", [{}, dict(allowed_ids=even), dict(allowed_ids=even), dict(allowed_ids=three)]) if hybrid else
                ("search_batch", dict(allowed_ids_each=[None, even, even, three])) if batched else
                ("search", [{}, dict(allowed_ids=even), dict(allowed_ids=even), dict(allowed_ids=three)]),
        "distinct": ("search", [dict(distinct_by="title")] * B) if hybrid or not batched else ("search_batch", dict(distinct_by="title")),
        "distinct+ids": ("search", [dict(distinct_by="title", allowed_ids=even)] * B) if hybrid else
                        ("search_batch", dict(distinct_by="title", allowed_ids=even)) if batched else ("search", [dict(distinct_by="title", allowed_ids=even)] * B),
    }
    norm = lambda kw: {k: sorted(v) if k == "allowed_ids" else [e if e is None else sorted(e) for e in v] if k == "allowed_ids_each" else v for k, v in kw.items()}
    for case in CASES:
        foreign.seen.clear()
        if case == "complete":
            if hybrid:
                with pytest.raises(_native.RqError, match="^complete_scores needs this module's DenseIndex on the dense side$"):
                    ENTRIES[entry](r, Q, TOP, _keywords(case, mine))
            continue
        got = ENTRIES[entry](r, Q, TOP, _keywords(case, mine))
        assert len(got) == B
        how, kws = want[case]
        if how == "search_batch":
            ((fn, queries, top_k, kw),) = foreign.seen
            assert (fn, queries, top_k) == ("search_batch", Q, POOL) and isinstance(queries, list) and norm(kw) == kws, (case, foreign.seen)
        else:
            assert [(s[0], s[1], s[2]) for s in foreign.seen] == [("search", q, POOL) for q in Q], (case, foreign.seen)
            assert [norm(s[3]) for s in foreign.seen] == kws, (case, foreign.seen)
            if hybrid:
                assert all(isinstance(s[3].get("allowed_ids", []), list) for s in foreign.seen)
    if hybrid and entry != "route_batch":                # the columns are the results' columns
        a, b = (ENTRIES[e](r, Q, TOP, {}) for e in ("hybrid_search_batch", "get_scores_for_router_batch"))
        assert [([x.bm25_score for x in res], [x.dense_score for x in res], [x.doc_id for x in res], [x.text for x in res]) for res in a] == \
            [tuple(col[:len(res)] for col in c) for c, res in zip(b, a)]
        assert all(len(col) == TOP and col[len(res):] == [pad] * (TOP - len(res)) for c, res in zip(b, a) for col, pad in zip(c, (0.0, 0.0, "", "")))


def test_refusals_their_order_and_their_texts():
    r, native, emb = _retriever()
    mine = r.make_filter(EVEN[:3])
    bare = r.dense_index.make_filter(EVEN[:3])
    mask = r.bm25_index.make_mask(EVEN[:3])
    each = [None] * B
    one_side = "^the hybrid batch calls take ids or a HybridRetriever.make_filter result: a dense RowFilter or a sparse mask covers one side only$"
    for entry in ENTRIES:
        what = entry
        run = lambda **kw: ENTRIES[entry](r, Q, TOP, kw)
        hybrid = entry != "dense_search_batch"
        complete = dict(complete_scores=True) if hybrid else {}
        # per_group first, whatever else is wrong
        with pytest.raises(ValueError, match=rf"^{what} returns one passage per group: per_group=2 is not supported \(use DenseIndex.search\)$"):
            run(distinct_by="title", per_group=2, allowed_ids_each=[None], **complete)
        with pytest.raises(ValueError, match=rf"^{what} returns one passage per group: per_group=2 is not supported"):
            run(per_group=2)
        if hybrid:                                         # then distinct_by with complete_scores, before allowed_ids_each is looked at
            with pytest.raises(ValueError, match="^distinct_by does not combine with complete_scores$"):
                run(distinct_by="title", complete_scores=True, allowed_ids_each=[None])
        with pytest.raises(ValueError, match=rf"^{what}: distinct_by does not combine with allowed_ids_each \(the grouped dense search takes one filter for the batch: allowed_ids\)$"):
            run(distinct_by="title", allowed_ids_each=[None])                             # (before the entries are counted)
        with pytest.raises(ValueError, match="^allowed_ids_each does not combine with allowed_ids, distinct_by or per_group$"):
            run(allowed_ids_each=each, allowed_ids=EVEN)
        with pytest.raises(ValueError, match=f"^allowed_ids_each needs one entry per query: {B} queries, 1 entries$"):
            run(allowed_ids_each=[bare])                                                  # (counted before the entries are looked at)
        for bad in ((bare, mask) if hybrid else (mask,)):
            with pytest.raises(ValueError, match=one_side):
                run(allowed_ids=bad)
            with pytest.raises(ValueError, match=one_side):
                run(allowed_ids_each=[None, EVEN, bad, mine])
    for kw, text in ((dict(num_passages=0), "^num_passages 0 and top_k 5 must be at least 1$"), (dict(num_passages=5, top_k=0), "^num_passages 5 and top_k 0 must be at least 1$")):
        kw = dict(dict(top_k=5), **kw)
        with pytest.raises(ValueError, match=text):                                       # after the distinct_by checks, before the filters and the empty batch
            r.route_batch(Q, GATE, allowed_ids_each=[None], **kw)
        with pytest.raises(ValueError, match=text):
            r.route_batch([], GATE, **kw)
        with pytest.raises(ValueError, match="^route_batch returns one passage per group"):
            r.route_batch(Q, GATE, per_group=3, distinct_by="title", **kw)
        with pytest.raises(ValueError, match="^distinct_by does not combine with complete_scores$"):
            r.route_batch(Q, GATE, complete_scores=True, distinct_by="title", **kw)
    assert not _searches(native) and len(native.made) == 2 and emb.host == 0
    assert all(len(ENTRIES[entry](r, Q, TOP, dict(distinct_by="title", per_group=1))) == B for entry in ENTRIES)      # (1 is what they return)
    native.calls.clear()
    # a stale filter: refused when the filters are made, after every check of the keywords; what was made before it is closed
    r.bm25_index.add_documents([si.Document(id="late", text="w1 late")])
    stale = rf"^the hybrid filter is stale: made over \({N}, {N}\) \(BM25, dense\) passages, the indexes hold \({N + 1}, {N}\)$"
    for entry in ENTRIES:
        for kw in (dict(allowed_ids=mine), dict(allowed_ids_each=[None, EVEN, mine, EVEN]), dict(allowed_ids=mine, distinct_by="title")):
            del native.made[2:]
            with pytest.raises(_native.RqError, match=stale):
                ENTRIES[entry](r, Q, TOP, kw)
            assert all(m.closed == 1 for m in native.made[2:]) and len(native.made[2:]) == (1 if "allowed_ids_each" in kw and entry != "dense_search_batch" else 0), (entry, list(kw))
    assert not _searches(native) and native.made[0].closed == 0 and emb.host == len(ENTRIES)


def test_early_returns_in_their_order():
    r, native, emb = _retriever()
    empty_cols = ([], [], [], [])
    # an empty batch: nothing is embedded or searched -- but the entries are still counted, except by route_batch, which answers first
    for kw in ({}, dict(complete_scores=True), dict(distinct_by="title"), dict(allowed_ids=EVEN), dict(allowed_ids_each=[])):
        assert r.hybrid_search_batch([], TOP, POOL, **kw) == [] and r.get_scores_for_router_batch([], TOP, retrieval_pool_size=POOL, **kw) == []
        assert r.route_batch([], GATE, TOP, **kw) == []
        res, w = r.route_batch([], GATE, 7, num_passages=3, return_weights=True, **kw)
        assert res == [] and w.shape == (0, 3)
        if not kw or "distinct_by" in kw:
            assert r.dense_search_batch([], POOL, **kw) == []
    assert r.route_batch([], GATE, TOP, allowed_ids_each=[None]) == []
    for entry in ENTRIES:
        if entry != "route_batch":
            with pytest.raises(ValueError, match="one entry per query: 0 queries, 1 entries"):
                ENTRIES[entry](r, [], TOP, dict(allowed_ids_each=[None]))
    assert not native.calls and not native.made and emb.host == 0
    # top_k <= 0 comes second: the fused rows are not asked for, the pools are still drawn (one plain batch search) and cut to nothing
    for top_k in (0, -1):
        native.calls.clear()
        got = r.hybrid_search_batch(Q, top_k, POOL)
        assert _searches(native) == [dict(fn="search", B=B, k=POOL, metric=0)]
        if top_k == 0:                                                                 # (a negative top_k is the reference's slice: not pinned)
            assert got == [[]] * B and r.get_scores_for_router_batch(Q, 0, retrieval_pool_size=POOL) == [empty_cols] * B
            assert _searches(native) == [dict(fn="search", B=B, k=POOL, metric=0)] * 2
    assert not native.made and emb.host == 3
    # no dense index: the sparse pools alone, whatever the keywords; nothing dense is made, embedded or searched
    nd, native, emb = _retriever(dense=None)
    for kw in ({}, dict(allowed_ids=EVEN), dict(allowed_ids_each=[None, EVEN, EVEN, None]), dict(distinct_by="title")):
        got = nd.hybrid_search_batch(Q, TOP, POOL, **kw)
        assert sum(len(x) for x in got) > B and all(x.dense_score == 0.0 for res in got for x in res)
        assert [[x.doc_id for x in res] for res in got] == [[d for d in c[2] if d] for c in nd.get_scores_for_router_batch(Q, TOP, retrieval_pool_size=POOL, **kw)]
        assert [len(x) for x in nd.route_batch(Q, GATE, TOP, num_passages=TOP, retrieval_pool_size=POOL, **kw)] == [len(x) for x in got]
        assert nd.dense_search_batch(Q, POOL, **kw) == [[]] * B
    assert nd.make_filter(EVEN).dense is None and not native.calls and not native.made and emb.host == 0
    # an empty BM25 index: the dense pools alone, from the same single native call
    nb, native, emb = _retriever(docs=None)
    for kw, fn in (({}, "search"), (dict(allowed_ids=EVEN), "search_filtered_each"), (dict(distinct_by="title"), "search_grouped")):
        native.calls.clear()
        got = nb.hybrid_search_batch(Q, TOP, POOL, **kw)
        assert [c["fn"] for c in _searches(native)] == [fn] and [len(x) for x in got] == [TOP] * B and all(x.bm25_score == 0.0 for res in got for x in res)
    assert len(native.made) == 1 and native.made[0].closed == 1 and emb.host == 3
    assert nb.make_filter(EVEN).sparse is None
    # an empty dense index: nothing is searched, nothing is embedded for the plain route
    ne, native, emb = _retriever(_Native(0))
    assert sum(len(x) for x in ne.hybrid_search_batch(Q, TOP, POOL)) > B and not native.calls and emb.host == 0
