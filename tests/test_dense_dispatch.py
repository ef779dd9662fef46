"""Which native call every public entry point of DenseIndex / HybridRetriever reaches, with which arguments, for every combination of
the restricting keywords (`allowed_ids`, `distinct_by`, `per_group`, `allowed_ids_each`) -- over a recording stand-in for
_native.NativeIndex and one for _native.RowFilter, so no library and no device is needed.  Pinned here: the native method, how often,
k / group_size / cap / fetch_k / metric, the identity and the closing of filters, which embedder path ran, the order of the early outs
and the texts of the refusals.  What the calls COMPUTE is the business of the feature tests (test_filter, test_grouped, ...)."""
import logging

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

N, D = 24, 8
EVEN = [f"p{i}" for i in range(0, N, 2)]
EVEN_ROWS = list(range(0, N, 2))
GROUPS = [i % 6 for i in range(N)]
SEARCHES = ("search", "search_filtered_each", "search_grouped", "search_group_members", "search_mmr", "search_range", "score_rows")


class _Filter:
    """Stand-in for _native.RowFilter: remembers its rows and how often it was closed."""

    def __init__(self, rows):
        self.rows = [int(r) for r in rows]
        self.count = len(self.rows)
        self.closed = 0

    def close(self):
        self.closed += 1


def _answer(*shape):
    """(scores, rows) of the given shape: descending scores, rows that every index of at least N rows holds"""
    n = int(np.prod(shape))
    return np.linspace(1.0, 0.0, n, dtype=np.float32).reshape(shape), (np.arange(n, dtype=np.int64) % N).reshape(shape)


class _Native:
    """Recording stand-in for _native.NativeIndex: every call appends what it was given to `calls`; `fail` names a method that raises."""
    device = 0

    def __init__(self, n=N, devices=(0,), fail=None):
        self.n, self.dim, self.devices, self.fail = n, D, list(devices), fail
        self.calls, self.made, self.pushed = [], [], []

    def __len__(self):
        return self.n

    def _call(self, fn, q, **kw):
        self.calls.append(dict(fn=fn, B=int(np.shape(q)[0]), **kw))
        if self.fail == fn:
            raise RuntimeError(f"{fn} failed")
        return self.calls[-1]["B"]

    def make_filter(self, rows):
        self.made.append(_Filter(rows))
        return self.made[-1]

    def set_groups(self, groups, row_begin=0):
        self.pushed.append((int(row_begin), np.asarray(groups).tolist()))

    def search(self, q, k, metric=0, **kw):          # (`row_filter` is recorded only when it was handed over)
        return _answer(self._call("search", q, k=k, metric=metric, **kw), k)

    def search_device(self, *a, **kw):
        raise AssertionError("no test here goes as far as the device call")

    def search_filtered_each(self, q, k, filters, metric=0):
        return _answer(self._call("search_filtered_each", q, k=k, metric=metric, filters=list(filters)), k)

    def search_grouped(self, q, k, metric=0, *, row_filter=None):
        B = self._call("search_grouped", q, k=k, metric=metric, row_filter=row_filter)
        return _answer(B, k) + (np.zeros((B, k), np.int32),)

    def search_group_members(self, q, k, group_size, metric=0, *, row_filter=None):
        B = self._call("search_group_members", q, k=k, group_size=group_size, metric=metric, row_filter=row_filter)
        return _answer(B, k, group_size) + (np.zeros((B, k), np.int32), np.full((B, k), group_size, np.int32))

    def search_mmr(self, q, k, fetch_k, lambda_mult=0.5, metric=0, *, row_filter=None):
        return _answer(self._call("search_mmr", q, k=k, fetch_k=fetch_k, lambda_mult=lambda_mult, metric=metric, row_filter=row_filter), k)

    def search_range(self, q, threshold, cap, metric=0, *, row_filter=None):
        B = self._call("search_range", q, threshold=threshold, cap=cap, metric=metric, row_filter=row_filter)
        return _answer(B, cap) + (np.full(B, 99, np.int64),)

    def score_rows(self, q, rows, metric=0):
        self._call("score_rows", q, rows=np.asarray(rows).tolist(), metric=metric)
        return np.full(np.shape(rows), 0.5, np.float32)


class _Emb:
    dim = D

    def __init__(self, dim=D):
        self.dim, self.host = dim, 0

    def embed(self, texts):
        self.host += 1
        return np.ones((len(texts), self.dim), np.float32)


class _Tensor:
    """What `embed_device` leaves in HBM, as far as the routes that stop before torch look at it."""

    def __init__(self, B):
        self.shape, self.device = (B, D), "hbm"


class _DevEmb(_Emb):
    def __init__(self, fail=False):
        super().__init__()
        self.dev, self.fail = 0, fail

    def embed_device(self, texts):
        self.dev += 1
        if self.fail:
            raise RuntimeError("no device")
        return _Tensor(len(texts))


@pytest.fixture(autouse=True)
def _stub_filter_class(monkeypatch):
    monkeypatch.setattr(_native, "RowFilter", _Filter)


@pytest.fixture
def device_rows(monkeypatch):
    """`_search_device_rows` (the first step that needs torch) replaced by a recorder of (queries, top_k)."""
    seen = []
    monkeypatch.setattr(si.DenseIndex, "_search_device_rows", lambda self, t, top_k: seen.append((t, top_k)) or _answer(t.shape[0], min(top_k, len(self))))
    return seen


def _dense(native=None, emb=None, metric="cosine"):
    native = _Native() if native is None else native
    di = si.DenseIndex.from_native(native, [f"p{i}" for i in range(len(native))], embedder=_Emb() if emb is None else emb, metric=metric)
    di._metas = [{"title": f"t{i % 6}"} for i in range(len(native))]
    return di, native


def _hybrid(di):
    return si.HybridRetriever(bm25_persist_path=None, dense_index=di)


def _searches(native):
    return [c for c in native.calls if c["fn"] in SEARCHES]


ENTRIES = {   # name -> call(dense, B, top_k, keywords)
    "search": lambda di, B, k, kw: di.search("q", k, **kw),
    "dense_search": lambda di, B, k, kw: _hybrid(di).dense_search("q", k, **kw),
    "search_batch": lambda di, B, k, kw: di.search_batch(["q"] * B, k, **kw),
    "search_vectors": lambda di, B, k, kw: di.search_vectors(np.ones((B, D), np.float32), k, **kw),
    "search_rows_batch": lambda di, B, k, kw: di.search_rows_batch(["q"] * B, k, **kw),
}
ENTRY_BATCHES = [(e, B) for e in ENTRIES for B in ((1,) if e in ("search", "dense_search") else (1, 3))]
CASES = {     # name -> (keywords, native method, group_size, filter: None / "made" from ids / "mine", the caller's own)
    "none": ({}, "search", None, None),
    "ids": (dict(allowed_ids=EVEN), "search", None, "made"),
    "filter": (dict(allowed_ids="mine"), "search", None, "mine"),
    "distinct": (dict(distinct_by="title"), "search_grouped", None, None),
    "distinct+ids": (dict(distinct_by="title", allowed_ids=EVEN), "search_grouped", None, "made"),
    "distinct+filter": (dict(distinct_by="title", allowed_ids="mine"), "search_grouped", None, "mine"),
    "per_group=1": (dict(distinct_by="title", per_group=1), "search_grouped", None, None),
    "per_group=1+ids": (dict(distinct_by="title", per_group=1, allowed_ids=EVEN), "search_grouped", None, "made"),
    "per_group=3": (dict(distinct_by="title", per_group=3), "search_group_members", 3, None),
    "per_group=3+ids": (dict(distinct_by="title", per_group=3, allowed_ids=EVEN), "search_group_members", 3, "made"),
    "per_group=3+filter": (dict(distinct_by="title", per_group=3, allowed_ids="mine"), "search_group_members", 3, "mine"),
}


def _keywords(kw, mine):
    return {k: (mine if isinstance(v, str) and v == "mine" else v) for k, v in kw.items()}


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry,B", ENTRY_BATCHES)
def test_search_routes(entry, B, case, on_device, device_rows):
    kw, fn, group_size, which = CASES[case]
    emb = _DevEmb() if on_device else _Emb()
    di, native = _dense(emb=emb)
    mine = di.make_filter(EVEN[:3])
    kw = _keywords(kw, mine)
    if entry == "search_rows_batch" and group_size:
        with pytest.raises(ValueError, match="search_rows_batch returns one passage per group: per_group=3 is not supported"):
            ENTRIES[entry](di, B, 5, kw)
        assert not _searches(native) and len(native.made) == 1 and emb.host == 0
        return
    got = ENTRIES[entry](di, B, 5, kw)
    embeds = entry != "search_vectors"
    if case == "none" and on_device and embeds:      # the unrestricted route alone takes the queries where the embedder left them
        assert not _searches(native) and (emb.dev, emb.host) == (1, 0)
        assert len(device_rows) == 1 and device_rows[0][0].shape == (B, D) and device_rows[0][1] == 5
    else:
        assert not device_rows and emb.host == (1 if embeds else 0) and getattr(emb, "dev", 0) == 0
        (call,) = _searches(native)
        assert call["fn"] == fn and call["B"] == B and call["k"] == 5 and call["metric"] == _native.METRIC_COSINE
        assert call.get("group_size") == group_size
        if fn == "search" and which is None:
            assert "row_filter" not in call          # (a plain backend's search takes no such keyword)
        elif which is None:
            assert call["row_filter"] is None and len(native.made) == 1
        elif which == "made":
            assert call["row_filter"] is native.made[-1] and len(native.made) == 2
            assert native.made[-1].rows == EVEN_ROWS and native.made[-1].closed == 1
        else:
            assert call["row_filter"] is mine and len(native.made) == 1
        assert native.pushed == ([(0, GROUPS)] if "distinct_by" in kw else [])
    assert mine.closed == 0
    width = 5 * (group_size or 1)
    if entry == "search_rows_batch":
        assert got[0].shape == got[1].shape == (B, 5) and got[0].dtype == np.float32 and got[1].dtype == np.int64
    elif entry in ("search", "dense_search"):
        assert len(got) == width and len(got[0]) == (3 if entry == "search" else 2) and got[0][0] == "p0"
    else:
        assert [len(g) for g in got] == [width] * B and got[0][0][0] == "p0" and isinstance(got[0][0][1], float)
    if "distinct_by" in kw:                          # the groups are pushed once per key, not once per call
        ENTRIES[entry](di, B, 5, kw)
        assert native.pushed == [(0, GROUPS)]


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("entry", ["search_batch", "search_vectors", "search_rows_batch"])
def test_allowed_ids_each_routes(entry, on_device, device_rows):
    emb = _DevEmb() if on_device else _Emb()
    di, native = _dense(emb=emb)
    mine = di.make_filter(EVEN[:3])
    other = list(EVEN)
    for each, made, same in (([EVEN, mine, EVEN], 1, (0, 2)), ([None, EVEN, other], 2, None), ([None, None, None], 0, None), ([EVEN], 1, None), ([mine], 0, None), ([None], 0, None)):
        native.calls.clear()
        del native.made[1:]
        ENTRIES[entry](di, len(each), 5, dict(allowed_ids_each=each))
        (call,) = _searches(native)
        assert call["fn"] == "search_filtered_each" and call["B"] == len(each) and call["k"] == 5 and call["metric"] == 0
        flt = call["filters"]
        assert len(native.made) == 1 + made and all(m.closed == 1 and m.rows == EVEN_ROWS for m in native.made[1:]) and mine.closed == 0
        assert [f is None for f in flt] == [e is None for e in each] and [f is mine for f in flt] == [e is mine for e in each]
        assert all(f in native.made[1:] for f, e in zip(flt, each) if e is not None and e is not mine)
        if same:
            assert flt[same[0]] is flt[same[1]]      # one list object given twice: one filter
        elif made == 2:
            assert flt[1] is not flt[2]              # equal lists that are two objects: two filters
    assert not device_rows and getattr(emb, "dev", 0) == 0
    # validated before anything else is looked at: before the empty answers, before the dimension
    wrong = np.ones((2, D + 1), np.float32)
    for d2, _ in (_dense(emb=emb), _dense(_Native(0), emb=emb)):
        for top_k in (5, 0):
            for bad_kw, text in ((dict(allowed_ids_each=[None]), "allowed_ids_each needs one entry per query: 2 queries, 1 entries"),
                                 (dict(allowed_ids_each=[None, None], allowed_ids=EVEN), "allowed_ids_each does not combine with allowed_ids, distinct_by or per_group"),
                                 (dict(allowed_ids_each=[None, None], distinct_by="title"), "does not combine"),
                                 (dict(allowed_ids_each=[None, None], distinct_by="title", per_group=1), "does not combine")):
                with pytest.raises(ValueError, match=text):
                    d2.search_vectors(wrong, top_k, **bad_kw) if entry == "search_vectors" else ENTRIES[entry](d2, 2, top_k, bad_kw)
    with pytest.raises(ValueError, match="one entry per query: 0 queries, 1 entries"):
        ENTRIES[entry](di, 0, 5, dict(allowed_ids_each=[None]))


@pytest.mark.parametrize("case", [c for c, v in CASES.items() if v[3]] + ["each", "mmr", "range"])
def test_filters_are_closed_when_the_native_call_raises(case):
    if case in CASES:
        kw, fn = CASES[case][:2]
    else:
        kw, fn = {"each": (None, "search_filtered_each"), "mmr": (dict(allowed_ids=EVEN), "search_mmr"), "range": (dict(allowed_ids=EVEN), "search_range")}[case]
    di, native = _dense(_Native(fail=fn))
    mine = di.make_filter(EVEN[:3])
    with pytest.raises(RuntimeError, match=fn + " failed"):
        if case == "each":
            di.search_batch(["q"] * 3, 5, allowed_ids_each=[EVEN, mine, list(EVEN)])
        elif case == "mmr":
            di.search_mmr("q", 5, **kw)
        elif case == "range":
            di.search_threshold("q", 0.3, **kw)
        else:
            di.search_batch(["q"], 5, **_keywords(kw, mine))
    made = native.made[1:]
    want = 2 if case == "each" else 0 if case.endswith("filter") else 1
    assert len(made) == want and all(m.closed == 1 for m in made) and mine.closed == 0 and len(_searches(native)) == 1


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("which", [None, "made", "mine"])
def test_mmr_range_and_scoring_routes(which, on_device, device_rows):
    emb = _DevEmb() if on_device else _Emb()
    di, native = _dense(emb=emb, metric="ip")
    r = _hybrid(di)
    mine = di.make_filter(EVEN[:3])
    kw = {} if which is None else dict(allowed_ids=EVEN if which == "made" else mine)
    vec = np.ones((3, D), np.float32)

    def one_call(fn, B):
        (call,) = _searches(native)
        assert call["fn"] == fn and call["B"] == B and call["metric"] == _native.METRIC_IP
        assert call["row_filter"] is {None: None, "mine": mine, "made": native.made[-1]}[which]
        assert len(native.made) == (2 if which == "made" else 1) and all(m.closed == 1 for m in native.made[1:]) and mine.closed == 0
        native.calls.clear()
        del native.made[1:]
        return call

    for B, run in ((1, lambda: di.search_mmr("q", 5, 50, 0.25, **kw)), (3, lambda: di.search_mmr_batch(["q"] * 3, 5, 50, 0.25, **kw)),
                   (3, lambda: di.search_mmr_vectors(vec, 5, 50, 0.25, **kw)), (1, lambda: r.dense_search_mmr("q", 5, 50, 0.25, **kw))):
        got = run()
        call = one_call("search_mmr", B)
        assert (call["k"], call["fetch_k"], call["lambda_mult"]) == (5, N, 0.25) and isinstance(call["lambda_mult"], float)
        assert len(got) == (5 if B == 1 else 3)
    di.search_mmr("q", 5, 2, **kw)                      # fetch_k is clamped to [top_k, min(len, MAX_K)]
    call = one_call("search_mmr", 1)
    assert (call["k"], call["fetch_k"], call["lambda_mult"]) == (5, 5, 0.5)
    di.search_mmr("q", 100, 7, **kw)
    call = one_call("search_mmr", 1)
    assert (call["k"], call["fetch_k"]) == (N, N)

    for B, cap, run in ((1, 7, lambda: di.search_threshold("q", 0.3, 7, **kw)), (3, 7, lambda: di.search_threshold_batch(["q"] * 3, 0.3, 7, **kw)),
                        (3, 7, lambda: di.search_threshold_vectors(vec, 0.3, 7, **kw)), (1, 7, lambda: r.dense_search_threshold("q", 0.3, 7, **kw)),
                        (1, 100, lambda: di.search_threshold("q", 0.3, **kw)), (1, _native.MAX_K, lambda: di.search_threshold("q", 0.3, 5000, **kw)),
                        (1, 1, lambda: di.count_above("q", 0.3, **kw))):
        got = run()
        call = one_call("search_range", B)
        assert call["cap"] == cap and call["threshold"] == 0.3
        assert got == 99 if cap == 1 else len(got) == (cap if B == 1 else 3)
    assert not device_rows and getattr(emb, "dev", 0) == 0      # (these queries take the host path)

    if which is None:
        rows = np.array([[3, -1, 5, 3]] * 3)
        assert di.score_vectors(vec, rows).shape == (3, 4)
        (call,) = _searches(native)
        assert call == dict(fn="score_rows", B=3, rows=rows.tolist(), metric=_native.METRIC_IP)
        native.calls.clear()
        if not on_device:
            assert di.score_rows_batch(["q"] * 3, rows).dtype == np.float32 and di.score_ids("q", ["p3", "ghost", "p5"]) == [0.5, 0.5, 0.5]
            assert [(c["fn"], c["B"], c["rows"]) for c in _searches(native)] == [("score_rows", 3, rows.tolist()), ("score_rows", 1, [[3, -1, 5]])]
        native.calls.clear()
        assert di.score_rows_batch(["q"], [[-1, -1]]).tolist() == [[0.0, 0.0]] and di.score_ids("q", []) == [] and not _searches(native)


def test_the_clamp_of_k():
    di, native = _dense()
    vec = np.ones((1, D), np.float32)
    for kw, top_k, k in (({}, 100, N), (dict(allowed_ids=EVEN), 100, N), (dict(distinct_by="title"), 100, N), (dict(allowed_ids_each=[EVEN]), 100, N),
                         (dict(distinct_by="title", per_group=3), 100, N), (dict(distinct_by="title", per_group=100), 100, _native.MAX_K // 100),
                         (dict(distinct_by="title", per_group=_native.MAX_K), 7, 1), ({}, 7.9, 7)):
        di.search_vectors(vec, top_k, **kw)
        assert _searches(native)[-1]["k"] == k and isinstance(_searches(native)[-1]["k"], int)
    assert di.search_rows_batch(["q"], 100)[1].shape == (1, N)
    big, native = _dense(_Native(_native.MAX_K + 76))
    for kw in ({}, dict(allowed_ids=EVEN), dict(distinct_by="title"), dict(allowed_ids_each=[None])):
        big.search_vectors(vec, 5000, **kw)
        assert _searches(native)[-1]["k"] == _native.MAX_K
    big.search_vectors(vec, 5000, distinct_by="title", per_group=3)
    assert (_searches(native)[-1]["k"], _searches(native)[-1]["group_size"]) == (_native.MAX_K // 3, 3)
    big.search_mmr_vectors(vec, 10, 5000)
    assert (_searches(native)[-1]["k"], _searches(native)[-1]["fetch_k"]) == (10, _native.MAX_K)
    big.search_mmr_vectors(vec, 5000, 5)
    assert (_searches(native)[-1]["k"], _searches(native)[-1]["fetch_k"]) == (_native.MAX_K, _native.MAX_K)
    with pytest.raises(ValueError, match=f"per_group {_native.MAX_K + 1} beyond {_native.MAX_K}"):
        big.search_vectors(vec, 5, distinct_by="title", per_group=_native.MAX_K + 1)


def test_embed_queries_and_the_embedded_forms(device_rows, caplog):
    host, dev = _Emb(), _DevEmb()
    di, native = _dense(emb=host)
    kind, m = di._embed_queries(["a", "b"])
    assert kind == "host" and m.shape == (2, D) and m.dtype == np.float32
    di, native = _dense(emb=dev)
    kind, t = di._embed_queries(["a", "b"])
    assert kind == "device" and isinstance(t, _Tensor) and (dev.dev, dev.host) == (1, 0)
    assert di._embed_queries(["a"], host_only=True)[0] == "host" and dev.dev == 1
    assert _dense(_Native(devices=(0, 1)), emb=dev)[0]._embed_queries(["a"])[0] == "host" and dev.dev == 1      # several devices: host buffers only
    assert _dense(_Native(0), emb=dev)[0]._embed_queries(["a"])[0] == "host" and dev.dev == 1                   # nothing to search yet
    broken = _DevEmb(fail=True)
    for run in (lambda d: d._embed_queries(["a"])[0] == "host", lambda d: d.search_batch(["a"], 5) and True, lambda d: d.search_rows_batch(["a"], 5) and True):
        caplog.clear()
        d2, n2 = _dense(emb=broken)
        with caplog.at_level(logging.ERROR, logger=si.logger.name):
            assert run(d2)
        assert "Device embedding failed (no device); falling back to the host path" in caplog.text
    assert (broken.dev, broken.host) == (3, 3) and [c["fn"] for c in n2.calls] == ["search"] and not device_rows
    # `_search_embedded`: the rows form over vectors that are already embedded
    s, rws = di._search_embedded(("host", np.ones((3, D), np.float32)), 5)
    assert rws.shape == (3, 5) and native.calls[-1] == dict(fn="search", B=3, k=5, metric=0)
    di._search_embedded(("host", np.ones((3, D), np.float32)), 100, EVEN)
    assert native.calls[-1]["k"] == N and native.calls[-1]["row_filter"] is native.made[-1] and native.made[-1].closed == 1
    n_calls = len(native.calls)
    di._search_embedded(("device", t), 5)
    assert device_rows == [(t, 5)] and len(native.calls) == n_calls
    for qv, top_k, d2 in ((("host", np.ones((3, D + 1), np.float32)), 0, di), (("device", _Tensor(3)), 5, _dense(_Native(0), emb=dev)[0])):
        s, rws = d2._search_embedded(qv, top_k)
        assert s.shape == rws.shape == (3, 0) and s.dtype == np.float32 and rws.dtype == np.int64
    assert di._score_embedded(("host", np.ones((1, D), np.float32)), np.array([[2, -1]])).tolist() == [[0.5, 0.5]] and native.calls[-1]["fn"] == "score_rows"
    # the completed fusion embeds once and searches through `_search_embedded` with the pool size as k
    di, native = _dense(emb=host)
    _hybrid(di).hybrid_search("q", 5, 10, complete_scores=True)
    assert [(c["fn"], c["k"]) for c in native.calls] == [("search", 10)]
    _hybrid(di).hybrid_search("q", 5, 10, complete_scores=True, allowed_ids=iter(EVEN))
    assert native.calls[-1]["k"] == 10 and native.calls[-1]["row_filter"].rows == EVEN_ROWS and native.made[-1].closed == 1


def test_early_outs_come_before_the_dimension_check():
    wrong = np.ones((2, D + 1), np.float32)
    nothing, native0 = _dense(_Native(0))
    di, native = _dense()
    for d2 in (nothing, di):
        for top_k in ((5, 0, -1) if d2 is nothing else (0, -1)):
            for kw in ({}, dict(allowed_ids=EVEN), dict(distinct_by="title"), dict(distinct_by="title", per_group=3), dict(allowed_ids_each=[None, EVEN])):
                assert d2.search_vectors(wrong, top_k, **kw) == [[], []] and d2.search_batch(["a", "b"], top_k, **kw) == [[], []]
                assert d2.search("a", top_k, **{k: v for k, v in kw.items() if k != "allowed_ids_each"}) == []
                if "per_group" not in kw:
                    s, rws = d2.search_rows_batch(["a", "b"], top_k, **kw)
                    assert s.shape == rws.shape == (2, 0) and s.dtype == np.float32 and rws.dtype == np.int64
            assert d2.search_mmr_vectors(wrong, top_k) == [[], []] and d2.search_mmr("a", top_k) == []
        assert d2.search_threshold_vectors(wrong, 0.3, 0) == [[], []] and d2.search_threshold("a", 0.3, -1) == []
        assert d2.search_batch([], 5) == [] and nothing.search_batch([], 5, allowed_ids_each=[]) == [] and d2.search_mmr_batch([], 5) == [] and d2.search_threshold_batch([], 0.3) == []
        s, rws = d2.search_rows_batch([], 5)
        assert s.shape == rws.shape == (0, 0)
    assert nothing.search_threshold_vectors(wrong, 0.3) == [[], []] and nothing.count_above("a", 0.3) == 0
    assert nothing.score_vectors(wrong, [[1, 2], [3, 4]]).tolist() == [[0.0, 0.0], [0.0, 0.0]] and nothing.score_ids("a", ["p1"]) == [0.0]
    assert di.score_vectors(wrong, np.zeros((2, 0), np.int64)).shape == (2, 0)
    assert not native0.calls and not native.calls and not native0.made and not native.made and not native.pushed
    # ... and what is checked before them
    for d2 in (nothing, di):
        with pytest.raises(ValueError, match="per_group needs distinct_by"):
            d2.search_vectors(wrong, 0, per_group=2)
        with pytest.raises(ValueError, match="per_group must be an integer >= 1, got 0"):
            d2.search_batch([], 5, distinct_by="title", per_group=0)
        with pytest.raises(ValueError, match=r"lambda_mult must lie within \[0, 1\], got 1.5"):
            d2.search_mmr_vectors(wrong, 0, lambda_mult=1.5)
        with pytest.raises(ValueError, match=r"expected \[2\]\[m\] rows, one list per query, got \(1, 2\)"):
            d2.score_vectors(wrong, [[1, 2]])
        with pytest.raises(ValueError, match=r"expected \[2\]\[m\] rows, one list per query, got \(1, 2\)"):
            d2.score_rows_batch(["a", "b"], [[1, 2]])
    # with something to search, the dimension is checked before any native call
    for run in (lambda: di.search_vectors(wrong, 5), lambda: di.search_vectors(wrong, 5, allowed_ids=EVEN), lambda: di.search_vectors(wrong, 5, distinct_by="title", per_group=3),
                lambda: di.search_vectors(wrong, 5, allowed_ids_each=[None, EVEN]), lambda: di.search_mmr_vectors(wrong, 5), lambda: di.search_threshold_vectors(wrong, 0.3),
                lambda: di.score_vectors(wrong, [[1], [2]])):
        with pytest.raises(ValueError, match=rf"query dimension {D + 1} does not match the index \({D}\)"):
            run()
    assert not native.calls and not native.made and not native.pushed


class _Plain:
    """A backend that holds rows and searches them, nothing else."""
    device, devices, dim = 0, [0], D

    def __len__(self):
        return N

    def search(self, q, k, metric=0):
        return _answer(int(np.shape(q)[0]), k)


class _Groups(_Plain):
    def make_filter(self, rows):
        return _Filter(rows)

    def set_groups(self, groups, row_begin=0):
        pass


def test_refusals_say_what_the_index_lacks():
    vec = np.ones((1, D), np.float32)
    di = _dense(_Plain())[0]
    assert len(di.search("q", 5)) == 5 and di.search_rows_batch(["q"], 5)[1].shape == (1, 5)
    for text, runs in (("filtered searches need a single-device index that holds rows",
                        (lambda d: d.make_filter(EVEN), lambda d: d.search("q", 5, allowed_ids=EVEN), lambda d: d.search_rows_batch(["q"], 5, allowed_ids_each=[EVEN]))),
                       ("grouped searches need a single-device index",
                        (lambda d: d.search("q", 5, distinct_by="title"), lambda d: d.search_vectors(vec, 5, distinct_by="title", per_group=3),
                         lambda d: _dense(_Groups())[0].search("q", 5, distinct_by="title", per_group=3))),
                       ("MMR searches need a single-device index", (lambda d: d.search_mmr("q", 5), lambda d: d.search_mmr_vectors(vec, 5, allowed_ids=EVEN))),
                       ("search_threshold / count_above need a single-device index",
                        (lambda d: d.search_threshold("q", 0.3), lambda d: d.count_above("q", 0.3), lambda d: d.search_threshold_vectors(vec, 0.3, allowed_ids=EVEN))),
                       ("score_vectors / score_rows_batch / score_ids need a single-device index",
                        (lambda d: d.score_vectors(vec, [[1]]), lambda d: d.score_rows_batch(["q"], [[1]]), lambda d: d.score_ids("q", ["p1"]), lambda d: d.score_ids("q", [])))):
        for run in runs:
            with pytest.raises(_native.RqError, match="^" + text + "$"):
                run(di)
    assert di.search_threshold_vectors(vec, 0.3, 0) == [[]]      # (nothing asked for: answered before the index is looked at)
    # an index over several devices has every method: range and scoring refuse it here, the other calls reach it (the library refuses)
    multi, native = _dense(_Native(devices=(0, 1)))
    for text, run in (("search_threshold / count_above need a single-device index", lambda: multi.search_threshold("q", 0.3)),
                      ("search_threshold / count_above need a single-device index", lambda: multi.count_above("q", 0.3)),
                      ("score_vectors / score_rows_batch / score_ids need a single-device index", lambda: multi.score_vectors(vec, [[1]])),
                      ("score_vectors / score_rows_batch / score_ids need a single-device index", lambda: multi.score_ids("q", ["p1"]))):
        with pytest.raises(_native.RqError, match="^" + text + "$"):
            run()
    assert not native.calls
    multi.search("q", 5, allowed_ids=EVEN), multi.search("q", 5, distinct_by="title"), multi.search("q", 5, distinct_by="title", per_group=3), multi.search_mmr("q", 5)
    assert [c["fn"] for c in native.calls] == ["search", "search_grouped", "search_group_members", "search_mmr"]
    # per_group: who takes it, and who says so
    r = _hybrid(_dense()[0])
    r.bm25_index.add_documents([si.Document(id="p1", text="q w", title="t1")])
    for what, run in (("BM25Index.search", lambda **kw: r.bm25_index.search("q", 5, **kw)), ("bm25_search", lambda **kw: r.bm25_search("q", 5, **kw)),
                      ("hybrid_search", lambda **kw: r.hybrid_search("q", 5, **kw)), ("search_rows_batch", lambda **kw: r.dense_index.search_rows_batch(["q"], 5, **kw))):
        with pytest.raises(ValueError, match=rf"^{what} returns one passage per group: per_group=2 is not supported \(use DenseIndex.search\)$"):
            run(distinct_by="title", per_group=2)
        run(distinct_by="title", per_group=1)


class _Duck:
    """An index of someone else's: `search(query, top_k)` and only the keywords its caller was given."""

    def __init__(self):
        self.seen = []

    def search(self, query, top_k, **kw):
        self.seen.append((query, top_k, kw))
        return [("p1", 0.5, "text")]


class _StrictDuck:
    def search(self, query, top_k):
        return [("p1", 0.5, "text")]


def test_only_the_keywords_that_were_given_are_handed_on(monkeypatch):
    mine = _Filter([1])
    given = [({}, {}), (dict(allowed_ids=EVEN), dict(allowed_ids=EVEN)), (dict(allowed_ids=mine), dict(allowed_ids=mine)),
             (dict(distinct_by="title"), dict(distinct_by="title")), (dict(distinct_by="title", allowed_ids=EVEN), dict(distinct_by="title", allowed_ids=EVEN)),
             (dict(distinct_by="title", per_group=1), dict(distinct_by="title")), (dict(distinct_by="title", per_group=None), dict(distinct_by="title")),
             (dict(distinct_by="title", per_group=3), dict(distinct_by="title", per_group=3)),
             (dict(distinct_by="title", per_group=3, allowed_ids=EVEN), dict(distinct_by="title", per_group=3, allowed_ids=EVEN))]
    said = lambda kw: {k: v for k, v in kw.items() if v is not None}          # (a keyword handed on as None says nothing)
    r = _hybrid(_Duck())
    r.bm25_index = _Duck()
    for kw, want in given:
        assert r.dense_search("q", 7, **kw) == [("p1", 0.5)]
        query, top_k, got = r.dense_index.seen[-1]
        assert (query, top_k) == ("q", 7) and said(got) == want and (kw or got == {})
        if kw.get("per_group", 1) in (1, None):
            r.bm25_search("q", 7, **kw)
            query, top_k, got = r.bm25_index.seen[-1]
            assert (query, top_k) == ("q", 7) and said(got) == {k: v for k, v in want.items() if k != "per_group"} and (kw or got == {})
    strict = _hybrid(_StrictDuck())
    strict.bm25_index = _StrictDuck()
    assert strict.dense_search("q", 7) == [("p1", 0.5)] and strict.bm25_search("q", 7) == [("p1", 0.5, "text")]
    assert strict.dense_search_batch(["q", "q"], 7) == [[("p1", 0.5)]] * 2
    with pytest.raises(TypeError):
        strict.dense_search("q", 7, allowed_ids=EVEN)
    strict.dense_index = None                        # dense retrieval disabled: the keywords are still checked
    assert strict.dense_search("q", 7) == [] and strict.dense_search_mmr("q", 7) == [] and strict.dense_search_threshold("q", 0.3) == []
    with pytest.raises(ValueError, match="per_group needs distinct_by"):
        strict.dense_search("q", 7, per_group=2)
    # DenseIndex.search -> search_batch, the same way
    di = _dense()[0]
    seen = []
    monkeypatch.setattr(di, "search_batch", lambda queries, top_k, **kw: seen.append((queries, top_k, kw)) or [["answer"]])
    for kw, want in given:
        assert di.search("q", 7, **kw) == ["answer"]
        queries, top_k, got = seen[-1]
        assert (queries, top_k) == (["q"], 7) and said(got) == want and (kw or got == {})
