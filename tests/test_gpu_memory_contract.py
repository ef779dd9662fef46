"""What every device-form call does to memory OUTSIDE what it returns (include/rq.h "Caller buffers"): each output lies between guard
words (tests/guarded.py), each input's bits are remembered, and after ONE call

    * the guards in front of and behind every output hold, every slot of every output was written (padding included: -1, 0.0, key 0,
      count), every input is unchanged;
    * the results equal the route's oracle under the rule of the route's own GPU test module -- the comparison functions and their
      bounds are IMPORTED from those modules (test_gpu_select._same, test_gpu_filter_each._same, test_gpu_range.check,
      test_gpu_grouped.agrees, test_gpu_group_members.agrees, test_gpu_mmr.follows_oracle, test_gpu_score_rows.close_to,
      sparse_oracle.same, sparse_grouped_oracle.same, hybrid_oracle.same, test_gpu_router._gate_close, router_gate_oracle.same), no
      number is restated here;
    * the status is 0 where the route has one (after the route's fixup form, which is a guarded call like any other).

The views are 17 elements into their allocation: naturally aligned for their element type and no more, which is all the header asks.
Batches of 1, 65, 130 and 257 queries leave one or two real queries in a pass of 64, 128 or 256 slots; the back guard holds the row
of every pad slot, so a kernel that writes one fails an assertion here instead of writing memory nobody owns.  A refused call
(RQ_EINVAL) leaves every output, guards included, untouched.  Finite inputs only: the non-finite rules are pinned elsewhere.

`covers` records which methods of rag_uq_amd._native a test calls; tests/test_memory_contract.py (CPU) fails when a device-form method
with an output pointer has no case here."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import group_members_oracle as gmo  # noqa: E402
import group_oracle as gro  # noqa: E402
import hybrid_grouped_oracle as hgo  # noqa: E402
import hybrid_oracle as ho  # noqa: E402
import mmr_oracle as mo  # noqa: E402,F401  (the oracle behind test_gpu_mmr.follows_oracle)
import nonfinite_oracle as nfo  # noqa: E402
import range_oracle as ro  # noqa: E402
import router_gate_oracle as rgo  # noqa: E402
import score_oracle as sco  # noqa: E402
import sparse_grouped_oracle as sgo  # noqa: E402
import sparse_masked_oracle as smo  # noqa: E402
import sparse_oracle as so  # noqa: E402
import test_gpu_filter_each as t_each  # noqa: E402
import test_gpu_group_members as t_members  # noqa: E402
import test_gpu_grouped as t_grouped  # noqa: E402
import test_gpu_mmr as t_mmr  # noqa: E402
import test_gpu_range as t_range  # noqa: E402
import test_gpu_router as t_router  # noqa: E402
import test_gpu_score_rows as t_score  # noqa: E402
import test_gpu_select as t_select  # noqa: E402
from guarded import frozen, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
NONE = nat.GROUP_NONE
NQ = 257
N_WIDE, N_TINY = 4101, 70          # 65 bins with a ragged last one (the approximate route of test_gpu_blocking_forms.py); the exact route
OFFSET = 10 ** 6

COVERED = {}                       # "Class.method" -> the tests that call it


def covers(*methods):
    def mark(fn):
        for m in methods:
            COVERED.setdefault(m, []).append(fn.__name__)
        return fn
    return mark


# ---- one call's buffers ------------------------------------------------------------------------------------------------------------------
def _t():
    import torch
    return torch


def _dev(a):
    return _t().from_numpy(np.ascontiguousarray(a)).cuda()


class Call:
    """The buffers of one call: outputs between guard words, inputs with their bits remembered."""

    def __init__(self, what, side=None):
        self.what, self.outs, self.ins, self.side = what, {}, {}, side

    def out(self, name, shape, dtype, per_query=None):
        self.outs[name] = guarded(shape, dtype, "cuda", per_query)
        return self.outs[name]

    def inp(self, name, array):
        self.ins[name] = frozen(_dev(array))
        return self.ins[name]

    @property
    def stream(self):
        """The stream argument of the call; every buffer was filled on torch's stream, so that comes first."""
        _t().cuda.synchronize()
        return self.side.cuda_stream if self.side is not None else 0

    def check(self, stage=""):
        _t().cuda.synchronize()
        for name, g in self.outs.items():
            g.check(f"{self.what}{stage}: output {name}")
        self.unchanged(stage)

    def unchanged(self, stage=""):
        _t().cuda.synchronize()
        for name, f in self.ins.items():
            f.check(f"{self.what}{stage}: input {name}")

    def untouched(self):
        _t().cuda.synchronize()
        for name, g in self.outs.items():
            g.untouched(f"{self.what}: output {name}")
        self.unchanged()

    def host(self, *names):
        return tuple(self.outs[n].numpy() for n in names)

    def bits(self):
        """Every output's bytes, for "the other queries keep their bits" """
        _t().cuda.synchronize()
        return {n: g.numpy().copy().view(np.uint8).reshape(g.shape[0], -1) for n, g in self.outs.items()}


def _kept(before, after, rows, what):
    for n in before:
        assert np.array_equal(before[n][rows], after[n][rows]), f"{what}: output {n} of a query that was not flagged changed"


def refused(call, fn, match=None):
    with pytest.raises(nat.RqError, match=match):
        fn()
    call.untouched()


# ---- the dense indexes -------------------------------------------------------------------------------------------------------------------
def _groups(n, seed=3):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, max(n // 6, 2), size=n).astype(np.int64)
    g[rng.random(n) < 0.1] = NONE
    return g


class Shard:
    """One index with group ids, three filters, NQ queries and their canonical scores per metric (computed once, shared, read-only)."""

    def __init__(self, name, n, dim, seed, row_pad=None, scan8=0, row_offset=0, like=None):
        self.name, self.n, self.dim, self.row_offset = name, n, dim, row_offset
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed) if like is None else like.x16
        self.q = orc.synthetic_queries(NQ, dim, seed=seed + 1) if like is None else like.q
        self._scores = {} if like is None else like._scores
        self.idx = nat.NativeIndex(dim, 0)
        if row_pad:
            self.idx.set_option("row_pad", row_pad)
        self.idx.set_option("scan8", scan8)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self.groups = _groups(n)
        self.idx.set_groups(self.groups)
        rng = np.random.default_rng(11)
        self.masks = {"third": np.arange(n) % 3 == 0, "head": np.arange(n) < max(n // 40, 5), "half": rng.random(n) < 0.5}
        self.filters = {k: self.idx.make_filter(m) for k, m in self.masks.items()}

    def scores(self, metric=COS):
        if metric not in self._scores:
            s = nfo.scores(self.q, self.x16, metric)
            s.setflags(write=False)
            self._scores[metric] = s
        return self._scores[metric]

    def queries(self, call, B):
        return call.inp("queries", self.q[:B])

    def close(self, side):
        self.idx.stream_release(side.cuda_stream)
        for f in self.filters.values():
            f.close()
        self.idx.close()


@pytest.fixture(scope="module")
def side():
    return _t().cuda.Stream()


@pytest.fixture(scope="module")
def world(side):
    wide = Shard("wide", N_WIDE, 768, 1234)
    w = {"wide": wide, "tiny": Shard("tiny", N_TINY, 768, 70),
         "narrow": Shard("narrow", N_WIDE, 384, 21, row_pad=384, row_offset=OFFSET),
         "wide8": Shard("wide8", N_WIDE, 768, 1234, scan8=2, like=wide)}
    assert w["narrow"].idx.row_pad == 384 and w["wide"].idx.row_pad == 768
    yield w
    for sh in w.values():
        sh.close(side)


def _k(sh, k):
    return sh.n + 3 if k == "n+3" else k


def _keys_ok(keys, scores, rows, what):
    assert np.array_equal(keys.view(np.uint64), t_grouped.host_keys(scores, rows)), f"{what}: keys are not (score, row) of the outputs, 0 where there is none"


# ---- rq_search_device / rq_search_filtered_device and their fixups ---------------------------------------------------------------------
def _search_bufs(sh, what, B, k, keys, side):
    import torch
    c = Call(what, side)
    sh.queries(c, B)
    c.out("scores", (B, k), torch.float32)
    c.out("rows", (B, k), torch.int64)
    if keys:
        c.out("keys", (B, k), torch.int64)
    c.out("status", (B,), torch.int32)
    return c


def _search_args(c):
    return c.outs["scores"], c.outs["rows"], c.outs.get("keys"), c.outs["status"]


SEARCH = [("wide", 1, 10, True, None, True, COS), ("wide", 65, 1, False, "third", False, COS), ("wide", 130, 321, True, None, False, COS),
          ("wide", 257, 10, False, None, False, IP), ("wide", 257, 10, True, "third", True, COS), ("wide", 65, 321, True, "half", False, COS),
          ("tiny", 65, "n+3", True, None, False, COS), ("tiny", 1, "n+3", False, "third", False, COS), ("tiny", 257, 10, True, None, False, COS),
          ("narrow", 130, 10, True, None, True, COS), ("narrow", 65, 321, False, "third", False, COS), ("narrow", 1, 1, True, None, False, IP),
          ("wide8", 257, 10, True, None, False, COS), ("wide8", 130, 321, False, None, True, COS), ("wide8", 1, 1, True, None, False, COS)]


@covers("NativeIndex.search_device", "NativeIndex.search_fixup_device")
@pytest.mark.parametrize("shard,B,k,keys,mask,on_side,metric", SEARCH)
def test_search_and_its_fixup(world, side, shard, B, k, keys, mask, on_side, metric):
    sh = world[shard]
    k = _k(sh, k)
    what = f"search {shard} B={B} k={k} keys={keys} filter={mask} metric={metric}"
    c = _search_bufs(sh, what, B, k, keys, side if on_side else None)
    flt = sh.filters[mask] if mask else None
    sh.idx.search_device(c.ins["queries"], B, k, metric, *_search_args(c), c.stream, row_filter=flt)
    c.check()
    flagged = c.host("status")[0] != 0
    before = c.bits()
    n = sh.idx.search_fixup_device(c.ins["queries"], B, k, metric, *_search_args(c), c.stream, row_filter=flt)
    c.check(" after the fixup")
    assert n == int(flagged.sum())
    _kept(before, c.bits(), ~flagged, what)
    gs, gr, st = c.host("scores", "rows", "status")
    assert not st.any(), f"{what}: status {np.flatnonzero(st).tolist()}"
    s_all = sh.scores(metric)[:B]
    want = orc.topk_from_scores(s_all, k, sh.row_offset) if mask is None else fo.filtered_topk_from_scores(s_all, sh.masks[mask], k, sh.row_offset)
    t_select._same(gs, gr, want[0], want[1], what)
    if keys:
        _keys_ok(c.host("keys")[0], gs, gr, what)


@covers("NativeIndex.search_fixup_device")
@pytest.mark.parametrize("shard,B,k,keys,mask,on_side", [("wide", 65, 10, True, None, False), ("wide", 257, 10, False, "third", True),
                                                          ("narrow", 130, 10, True, None, False), ("tiny", 65, "n+3", True, "half", False),
                                                          ("wide", 130, 321, True, None, False), ("wide", 1, 1, False, None, False)])
def test_the_fixup_of_queries_flagged_by_hand(world, side, shard, B, k, keys, mask, on_side):
    """Queries 0 and B - 1 flagged on the device, garbage over their outputs (tests/test_gpu_select.py has the pattern): the fixup writes
    those two queries' rows and nothing else."""
    import torch
    sh = world[shard]
    k = _k(sh, k)
    what = f"fixup by hand {shard} B={B} k={k} keys={keys} filter={mask}"
    c = _search_bufs(sh, what, B, k, keys, side if on_side else None)
    flt = sh.filters[mask] if mask else None
    sh.idx.search_device(c.ins["queries"], B, k, COS, *_search_args(c), c.stream, row_filter=flt)
    sh.idx.search_fixup_device(c.ins["queries"], B, k, COS, *_search_args(c), c.stream, row_filter=flt)
    c.check()
    flagged = sorted({0, B - 1})
    sel = torch.tensor(flagged, device="cuda")
    c.outs["status"].view[sel] = 1
    c.outs["scores"].view[sel] = float("nan")
    c.outs["rows"].view[sel] = -7
    if keys:
        c.outs["keys"].view[sel] = -1
    before = c.bits()
    n = sh.idx.search_fixup_device(c.ins["queries"], B, k, COS, *_search_args(c), c.stream, row_filter=flt)
    c.check(" after the fixup")
    assert n == len(flagged), f"{what}: the fixup returned {n}"
    other = np.setdiff1d(np.arange(B), flagged)
    _kept(before, c.bits(), other, what)
    gs, gr, st = c.host("scores", "rows", "status")
    assert not st.any()
    s_all = sh.scores(COS)[:B]
    want = orc.topk_from_scores(s_all, k, sh.row_offset) if mask is None else fo.filtered_topk_from_scores(s_all, sh.masks[mask], k, sh.row_offset)
    t_select._same(gs, gr, want[0], want[1], what)
    if keys:
        _keys_ok(c.host("keys")[0], gs, gr, what)


# ---- rq_search_filtered_each_device and its fixup ----------------------------------------------------------------------------------------
def _mixed(sh, B, seed):
    """Three filters and "no filter" in one batch, in no order: the scatter back to the queries' own positions is not monotonic."""
    names = ["half", None, "third", "head"]
    pick = np.random.default_rng(seed).integers(0, 4, B)
    pick[:4] = [2, 0, 3, 1][:B] if B >= 4 else pick[:4]
    return [names[i] for i in pick]


def _each_want(sh, names, k, metric=COS):
    s_all = sh.scores(metric)
    ws, wr = np.zeros((len(names), k), np.float32), np.full((len(names), k), -1, np.int64)
    for i, nm in enumerate(names):
        mask = np.ones(sh.n, bool) if nm is None else sh.masks[nm]
        ws[i], wr[i] = (a[0] for a in fo.filtered_topk_from_scores(s_all[i:i + 1], mask, k, sh.row_offset))
    return ws, wr


EACH = [("wide", 65, 10, True, True), ("wide", 65, 321, False, False), ("wide", 130, 1, True, False), ("wide", 257, 10, False, False),
        ("wide", 1, 10, True, False), ("tiny", 65, "n+3", True, False), ("narrow", 65, 10, True, True), ("narrow", 130, 321, False, False)]


@covers("NativeIndex.search_filtered_each_device", "NativeIndex.search_filtered_each_fixup_device")
@pytest.mark.parametrize("shard,B,k,keys,on_side", EACH)
def test_per_query_filters_and_their_fixup(world, side, shard, B, k, keys, on_side):
    sh = world[shard]
    k = _k(sh, k)
    what = f"each {shard} B={B} k={k} keys={keys}"
    names = _mixed(sh, B, B + k)
    filters = [None if nm is None else sh.filters[nm] for nm in names]
    c = _search_bufs(sh, what, B, k, keys, side if on_side else None)
    sh.idx.search_filtered_each_device(c.ins["queries"], B, k, COS, *_search_args(c), filters, c.stream)
    c.check()
    flagged = c.host("status")[0] != 0
    before = c.bits()
    n = sh.idx.search_filtered_each_fixup_device(c.ins["queries"], B, k, COS, *_search_args(c), filters, c.stream)
    c.check(" after the fixup")
    assert n == int(flagged.sum())
    _kept(before, c.bits(), ~flagged, what)
    gs, gr, st = c.host("scores", "rows", "status")
    assert not st.any()
    t_each._same((gs, gr), _each_want(sh, names, k), what)
    if keys:
        _keys_ok(c.host("keys")[0], gs, gr, what)


@covers("NativeIndex.search_filtered_each_fixup_device")
@pytest.mark.parametrize("shard,B,k", [("wide", 65, 10), ("narrow", 130, 10)])
def test_the_each_fixup_of_queries_flagged_by_hand(world, shard, B, k):
    import torch
    sh = world[shard]
    what = f"each fixup by hand {shard} B={B} k={k}"
    names = _mixed(sh, B, 5)
    filters = [None if nm is None else sh.filters[nm] for nm in names]
    c = _search_bufs(sh, what, B, k, True, None)
    sh.idx.search_filtered_each_device(c.ins["queries"], B, k, COS, *_search_args(c), filters, c.stream)
    sh.idx.search_filtered_each_fixup_device(c.ins["queries"], B, k, COS, *_search_args(c), filters, c.stream)
    c.check()
    flagged = [0, B - 1]
    sel = torch.tensor(flagged, device="cuda")
    c.outs["status"].view[sel] = 1
    c.outs["scores"].view[sel] = float("nan")
    c.outs["rows"].view[sel] = -7
    c.outs["keys"].view[sel] = -1
    before = c.bits()
    n = sh.idx.search_filtered_each_fixup_device(c.ins["queries"], B, k, COS, *_search_args(c), filters, c.stream)
    c.check(" after the fixup")
    assert n == 2
    _kept(before, c.bits(), np.arange(1, B - 1), what)
    gs, gr, st = c.host("scores", "rows", "status")
    assert not st.any()
    t_each._same((gs, gr), _each_want(sh, names, k), what)
    _keys_ok(c.host("keys")[0], gs, gr, what)


# ---- rq_search_range_device and its fixup ------------------------------------------------------------------------------------------------
RANGE_TARGETS = [100, 0, 3]        # rows that clear the threshold, about: more than cap = 1 or 7 (also of every third row), none, fewer than 7


def _thresholds(sh, B):
    """One threshold per query, the targets in turn, each in a gap that a last-bit difference cannot cross (test_gpu_range.MIN_GAP)."""
    s = sh.scores(COS)
    thr = np.zeros(B, np.float32)
    for b in range(B):
        found = ro.threshold_for(np.sort(s[b])[::-1], min(RANGE_TARGETS[b % 3], sh.n // 2), t_range.MIN_GAP)
        assert found is not None, f"no gap for query {b}: change the seed, not the rule"
        thr[b] = found[0]
    return thr


RANGE = [("wide", 1, 1, True, None, True), ("wide", 65, 7, False, None, False), ("wide", 130, 7, True, "third", False), ("wide", 257, 1, False, None, False),
         ("wide", 257, 7, True, "half", True), ("tiny", 65, 7, True, None, False), ("narrow", 130, 7, True, None, False), ("narrow", 65, 1, False, "third", True)]


@covers("NativeIndex.search_range_device", "NativeIndex.search_range_fixup_device")
@pytest.mark.parametrize("shard,B,cap,keys,mask,on_side", RANGE)
def test_range_search_and_its_fixup(world, side, shard, B, cap, keys, mask, on_side):
    import torch
    sh = world[shard]
    what = f"range {shard} B={B} cap={cap} keys={keys} filter={mask}"
    thr = _thresholds(sh, B)
    c = Call(what, side if on_side else None)
    q, d_thr = sh.queries(c, B), c.inp("thresholds", thr)
    outs = [c.out("scores", (B, cap), torch.float32), c.out("rows", (B, cap), torch.int64), c.out("keys", (B, cap), torch.int64) if keys else None,
            c.out("count", (B,), torch.int64), c.out("status", (B,), torch.int32)]
    flt = sh.filters[mask] if mask else None
    sh.idx.search_range_device(q, B, d_thr, cap, COS, *outs, c.stream, row_filter=flt)
    c.check()
    flagged = c.host("status")[0] != 0
    before = c.bits()
    n = sh.idx.search_range_fixup_device(q, B, d_thr, cap, COS, *outs, c.stream, row_filter=flt)
    c.check(" after the fixup")
    assert n == int(flagged.sum())
    _kept(before, c.bits(), ~flagged, what)
    gs, gr, gc, st = c.host("scores", "rows", "count", "status")
    assert not st.any()
    want = ro.from_scores(sh.scores(COS)[:B], thr, cap, sh.row_offset, sh.masks[mask] if mask else None)
    t_range.check((gs, gr, gc), want, what)
    if B >= 3:
        assert want[2][0] > cap and want[2][1] == 0, "the cases are the ones the issue names: more than cap rows pass, none pass"
    if keys:
        _keys_ok(c.host("keys")[0], gs, gr, what)


# ---- grouped searches, the pure collapse ---------------------------------------------------------------------------------------------------
def _grouped_bufs(sh, what, B, k, keys, side):
    import torch
    c = Call(what, side)
    sh.queries(c, B)
    outs = [c.out("scores", (B, k), torch.float32), c.out("rows", (B, k), torch.int64), c.out("groups", (B, k), torch.int32),
            c.out("keys", (B, k), torch.int64) if keys else None, c.out("status", (B,), torch.int32)]
    return c, outs


GROUPED = [("wide", 1, 10, True, None, True), ("wide", 65, 1, False, None, False), ("wide", 130, 321, True, None, False), ("wide", 257, 10, True, "third", False),
           ("tiny", 65, "n+3", True, None, False), ("narrow", 130, 10, False, None, True), ("narrow", 65, 321, True, "half", False), ("wide8", 65, 10, True, None, False)]


@covers("NativeIndex.search_grouped_device", "NativeIndex.search_grouped_fixup_device")
@pytest.mark.parametrize("shard,B,k,keys,mask,on_side", GROUPED)
def test_grouped_search_and_its_fixup(world, side, shard, B, k, keys, mask, on_side):
    sh = world[shard]
    k = _k(sh, k)
    what = f"grouped {shard} B={B} k={k} keys={keys} filter={mask}"
    c, outs = _grouped_bufs(sh, what, B, k, keys, side if on_side else None)
    q = c.ins["queries"]
    flt = sh.filters[mask] if mask else None
    sh.idx.search_grouped_device(q, B, k, COS, *outs, c.stream, row_filter=flt)
    c.check()
    flagged = c.host("status")[0] != 0
    before = c.bits()
    n = sh.idx.search_grouped_fixup_device(q, B, k, COS, *outs, c.stream, row_filter=flt)
    c.check(" after the fixup")
    assert n == int(flagged.sum())
    _kept(before, c.bits(), ~flagged, what)
    got = c.host("scores", "rows", "groups")
    assert not c.host("status")[0].any()
    want = gro.grouped_from_scores(sh.scores(COS)[:B], sh.groups, k, sh.masks[mask] if mask else None, sh.row_offset)
    t_grouped.agrees(got, want, sh.scores(COS), what)
    if keys:
        _keys_ok(c.host("keys")[0], got[0], got[1], what)


@covers("NativeIndex.search_grouped_fixup_device")
def test_the_grouped_fixup_of_queries_flagged_by_hand(world):
    import torch
    sh, B, k = world["wide"], 65, 10
    what = "grouped fixup by hand"
    c, outs = _grouped_bufs(sh, what, B, k, True, None)
    q = c.ins["queries"]
    sh.idx.search_grouped_device(q, B, k, COS, *outs, c.stream)
    sh.idx.search_grouped_fixup_device(q, B, k, COS, *outs, c.stream)
    c.check()
    sel = torch.tensor([0, B - 1], device="cuda")
    c.outs["status"].view[sel] = 1
    c.outs["scores"].view[sel] = float("nan")
    for name in ("rows", "groups"):
        c.outs[name].view[sel] = -7
    c.outs["keys"].view[sel] = -1
    before = c.bits()
    assert sh.idx.search_grouped_fixup_device(q, B, k, COS, *outs, c.stream) == 2
    c.check(" after the fixup")
    _kept(before, c.bits(), np.arange(1, B - 1), what)
    got = c.host("scores", "rows", "groups")
    assert not c.host("status")[0].any()
    t_grouped.agrees(got, gro.grouped_from_scores(sh.scores(COS)[:B], sh.groups, k, None, sh.row_offset), sh.scores(COS), what)
    _keys_ok(c.host("keys")[0], got[0], got[1], what)


COLLAPSE = [("wide", 1, 1, 1, True, True, False), ("wide", 65, 65, 10, True, False, True), ("wide", 130, 20, 20, False, True, False),
            ("wide", 257, 64, 1, True, True, False), ("narrow", 65, 100, 10, False, True, True), ("tiny", 65, 70, 70, True, False, False),
            ("wide", 65, 1024, 321, True, True, False)]


@covers("NativeIndex.group_collapse_device")
@pytest.mark.parametrize("shard,B,m,k,explicit,keys,on_side", COLLAPSE)
def test_the_pure_collapse(world, side, shard, B, m, k, explicit, keys, on_side):
    """Distinct candidate rows in no order, -1 at the first position and a row just outside the shard at the last (m >= 3), with their
    own ids or the index's.  Bit for bit, status included, as tests/test_gpu_grouped.py::test_pure_collapse_equals_the_oracle has it."""
    import torch
    sh = world[shard]
    what = f"collapse {shard} B={B} m={m} k={k} explicit={explicit} keys={keys}"
    rng = np.random.default_rng(1000 * m + B)
    s_all = sh.scores(COS)[:B]
    local = np.stack([rng.permutation(sh.n)[:m] for _ in range(B)]).astype(np.int64)
    cs = np.take_along_axis(s_all, local, axis=1).astype(np.float32)
    cr = local + sh.row_offset
    if m >= 3:
        cr[:, 0], cr[:, m - 1] = -1, sh.row_offset + sh.n
    ids = rng.integers(0, max(m // 4, 2), size=(B, m)).astype(np.int64)
    ids[rng.random((B, m)) < 0.15] = NONE
    g_in = ids if explicit else gro.lookup_groups(cr, sh.groups, sh.row_offset)
    c = Call(what, side if on_side else None)
    ins = [c.inp("cand_rows", cr), c.inp("cand_scores", cs), c.inp("cand_groups", ids.astype(np.int32)) if explicit else None]
    outs = [c.out("scores", (B, k), torch.float32), c.out("rows", (B, k), torch.int64), c.out("groups", (B, k), torch.int32),
            c.out("keys", (B, k), torch.int64) if keys else None, c.out("status", (B,), torch.int32)]
    sh.idx.group_collapse_device(*ins, B, m, k, *outs, c.stream)
    c.check()
    ws, wr, wg, wst = gro.collapse_batch(cs, cr, g_in, k, sh.n, sh.row_offset)
    gs, gr, gg, gst = c.host("scores", "rows", "groups", "status")
    assert np.array_equal(gr, wr) and np.array_equal(gg, wg), what
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{what}: scores are passed through bit for bit"
    assert np.array_equal(gst, wst), f"{what}: status"
    if keys:
        _keys_ok(c.host("keys")[0], ws, wr, what)


# ---- group members, the pure fill ----------------------------------------------------------------------------------------------------------
def _members_bufs(sh, what, B, k, s, side, winners=None):
    import torch
    c = Call(what, side)
    sh.queries(c, B)
    c.out("scores", (B, k, s), torch.float32)
    c.out("rows", (B, k, s), torch.int64)
    if winners is None:
        c.out("groups", (B, k), torch.int32)
    c.out("count", (B, k), torch.int32)
    c.out("status", (B,), torch.int32)
    return c


MEMBERS = [("wide", 1, 3, 3, None, True), ("wide", 65, 10, 1, None, False), ("wide", 130, 7, 3, "third", False), ("wide", 257, 10, 3, None, False),
           ("wide", 65, 321, 3, None, False), ("tiny", 65, 24, 3, None, False), ("narrow", 130, 1, 1, None, True), ("narrow", 65, 10, 3, "half", False)]


@covers("NativeIndex.search_group_members_device", "NativeIndex.search_group_members_fixup_device")
@pytest.mark.parametrize("shard,B,k,s,mask,on_side", MEMBERS)
def test_group_members_and_their_fixup(world, side, shard, B, k, s, mask, on_side):
    """[B][k][s] blocks; k x s is odd at 3 x 3, 7 x 3, 321 x 3 and 1 x 1."""
    sh = world[shard]
    what = f"members {shard} B={B} k={k} s={s} filter={mask}"
    c = _members_bufs(sh, what, B, k, s, side if on_side else None)
    q = c.ins["queries"]
    outs = [c.outs[n] for n in ("scores", "rows", "groups", "count", "status")]
    flt = sh.filters[mask] if mask else None
    sh.idx.search_group_members_device(q, B, k, s, COS, *outs, c.stream, row_filter=flt)
    c.check()
    flagged = c.host("status")[0] != 0
    before = c.bits()
    n = sh.idx.search_group_members_fixup_device(q, B, k, s, COS, *outs, c.stream, row_filter=flt)
    c.check(" after the fixup")
    assert n == int(flagged.sum())
    _kept(before, c.bits(), ~flagged, what)
    assert not c.host("status")[0].any()
    want = gmo.members_from_scores(sh.scores(COS)[:B], sh.groups, k, s, sh.masks[mask] if mask else None, sh.row_offset)
    t_members.agrees(sh, c.host("scores", "rows", "groups", "count"), want, COS, what, q=sh.q[:B])


@covers("NativeIndex.search_group_members_fixup_device")
def test_the_member_fixup_of_queries_flagged_by_hand(world):
    import torch
    sh, B, k, s = world["wide"], 65, 5, 3
    what = "member fixup by hand"
    c = _members_bufs(sh, what, B, k, s, None)
    q = c.ins["queries"]
    outs = [c.outs[n] for n in ("scores", "rows", "groups", "count", "status")]
    sh.idx.search_group_members_device(q, B, k, s, COS, *outs, c.stream)
    sh.idx.search_group_members_fixup_device(q, B, k, s, COS, *outs, c.stream)
    c.check()
    sel = torch.tensor([0, B - 1], device="cuda")
    c.outs["status"].view[sel] = 1
    c.outs["scores"].view[sel] = float("nan")
    for name in ("rows", "groups", "count"):
        c.outs[name].view[sel] = -7
    before = c.bits()
    assert sh.idx.search_group_members_fixup_device(q, B, k, s, COS, *outs, c.stream) == 2
    c.check(" after the fixup")
    _kept(before, c.bits(), np.arange(1, B - 1), what)
    assert not c.host("status")[0].any()
    t_members.agrees(sh, c.host("scores", "rows", "groups", "count"), gmo.members_from_scores(sh.scores(COS)[:B], sh.groups, k, s, None, sh.row_offset), COS, what, q=sh.q[:B])


FILL = [("wide", 1, 3, 3, None, True), ("wide", 65, 10, 1, None, False), ("wide", 130, 7, 3, "third", False), ("wide", 257, 10, 3, None, False),
        ("tiny", 65, 24, 3, None, False), ("narrow", 130, 5, 3, None, False)]


@covers("NativeIndex.group_fill_device")
@pytest.mark.parametrize("shard,B,k,s,mask,on_side", FILL)
def test_the_pure_fill(world, side, shard, B, k, s, mask, on_side):
    """The winner lists are the oracle's own (best row and id of each of the k best groups, (-1, GROUP_NONE) beyond the distinct groups):
    the fill over them is the member search's answer."""
    sh = world[shard]
    what = f"fill {shard} B={B} k={k} s={s} filter={mask}"
    want = gmo.members_from_scores(sh.scores(COS)[:B], sh.groups, k, s, sh.masks[mask] if mask else None, sh.row_offset)
    win_rows, win_groups = np.ascontiguousarray(want[1][:, :, 0]), want[2].astype(np.int32)
    if shard == "tiny":
        assert (win_rows == -1).any(), "a slot with no group is among the cases"
    c = _members_bufs(sh, what, B, k, s, side if on_side else None, winners=True)
    d_wr, d_wg = c.inp("win_rows", win_rows), c.inp("win_groups", win_groups)
    sh.idx.group_fill_device(c.ins["queries"], B, k, s, COS, d_wr, d_wg, c.outs["scores"], c.outs["rows"], c.outs["count"], c.outs["status"], c.stream,
                             row_filter=sh.filters[mask] if mask else None)
    c.check()
    gs, gr, gc, st = c.host("scores", "rows", "count", "status")
    assert not st.any()
    t_members.agrees(sh, (gs, gr, win_groups, gc), want, COS, what, q=sh.q[:B])


# ---- MMR selection, row scoring --------------------------------------------------------------------------------------------------------------
MMR = [("wide", 1, 10, 10, True, True), ("wide", 65, 20, 10, False, False), ("wide", 130, 20, 1, True, False), ("wide", 257, 20, 10, True, False),
       ("narrow", 65, 20, 20, True, False), ("tiny", 65, 20, 10, False, True), ("wide", 65, 1, 1, True, False)]


@covers("NativeIndex.mmr_select_device")
@pytest.mark.parametrize("shard,B,m,k,with_mmr,on_side", MMR)
def test_mmr_selection(world, side, shard, B, m, k, with_mmr, on_side):
    """Candidates: the oracle's top m, the last two absent (-1, and a row just outside the shard) when m > 2: k_eff < k at m = k."""
    import torch
    sh, lam = world[shard], 0.5
    what = f"mmr {shard} B={B} m={m} k={k} d_mmr={with_mmr}"
    rel, rows = (a.copy() for a in orc.topk_from_scores(sh.scores(COS)[:B], m, sh.row_offset))
    if m > 2:
        rows[:, m - 2], rows[:, m - 1] = -1, sh.row_offset + sh.n
    c = Call(what, side if on_side else None)
    d_r, d_s = c.inp("cand_rows", rows), c.inp("cand_rel", rel)
    o_s, o_r = c.out("scores", (B, k), torch.float32), c.out("rows", (B, k), torch.int64)
    o_v = c.out("mmr", (B, k), torch.float32) if with_mmr else None
    sh.idx.mmr_select_device(d_r, d_s, B, m, k, lam, COS, o_s, o_r, o_v, c.stream)
    c.check()
    got = (o_s.numpy(), o_r.numpy(), o_v.numpy() if with_mmr else None)
    t_mmr.follows_oracle(sh.x16, rel, rows, got, k, lam, COS, sh.row_offset, what)


SCORE = [("wide", 1, 1, False), ("wide", 65, 100, True), ("wide", 130, 100, False), ("wide", 257, 1, False), ("wide", 257, 100, True),
         ("narrow", 130, 100, False), ("tiny", 65, 100, False), ("narrow", 1, 100, True)]


@covers("NativeIndex.score_rows_device")
@pytest.mark.parametrize("shard,B,m,on_side", SCORE)
def test_score_rows(world, side, shard, B, m, on_side):
    """-1 and rows outside the shard at the first and the last position (at m = 1 they are the same position: the queries take turns)."""
    import torch
    sh = world[shard]
    what = f"score_rows {shard} B={B} m={m}"
    rng = np.random.default_rng(B * 10007 + m)
    rows = rng.integers(0, sh.n, size=(B, m)).astype(np.int64) + sh.row_offset
    absent = np.array([-1, sh.row_offset + sh.n, sh.row_offset - 1, 2 ** 40], np.int64)
    rows[1::3, 0] = absent[np.arange(len(rows[1::3])) % 4]
    rows[0::3, m - 1] = absent[(1 + np.arange(len(rows[0::3]))) % 4]
    c = Call(what, side if on_side else None)
    q, d_r = sh.queries(c, B), c.inp("rows", rows)
    out = c.out("scores", (B, m), torch.float32)
    sh.idx.score_rows_device(q, B, d_r, m, COS, out, c.stream)
    c.check()
    t_score.close_to(out.numpy(), sco.pairs(sh.q[:B], sh.x16, rows, COS, sh.row_offset, scores=sh.scores(COS)[:B]), what)


# ---- sparse ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse():
    """sparse_oracle's tile64_n200 index (4 tiles of 64, the last ragged) and batch_index() (2 000 documents, tiles of 256), both with a
    group table."""
    out = {}
    for name, ix, tile in (("tile64", next(c for c in so.cases() if c["name"] == "tile64_n200")["ix"], 64), ("batch", so.batch_index(), 256)):
        sp = nat.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
        sp.set_option("tile_docs", tile)
        groups = np.random.default_rng(9).integers(-1, max(ix["n_docs"] // 7, 2), ix["n_docs"]).astype(np.int32)
        sp.set_groups(groups)
        rng = np.random.default_rng(4)
        masks = smo.table([rng.random(ix["n_docs"]) < 0.5, np.arange(ix["n_docs"]) % 7 == 0], dirty=True)
        out[name] = {"sp": sp, "ix": ix, "groups": groups, "masks": masks}
    yield out
    for w in out.values():
        w["sp"].close()


def _sparse_call(w, what, B, masked, side):
    ix = w["ix"]
    q_indptr, q_tokens = so.queries(np.random.default_rng(100 + B), ix["n_tokens"], B)
    c = Call(what, side)
    args = {"q": (q_indptr, q_tokens), "d_ptr": c.inp("q_indptr", q_indptr), "d_tok": c.inp("q_tokens", q_tokens), "n_tok": len(q_tokens), "kw": {},
            "masks": None, "mask_of": None}
    if masked:
        args["masks"] = w["masks"]
        args["mask_of"] = np.random.default_rng(B).integers(-1, 2, B).astype(np.int32)
        args["kw"] = {"d_masks": c.inp("masks", w["masks"].view(np.int32)), "n_masks": 2, "d_mask_of": c.inp("mask_of", args["mask_of"])}
    return c, args


SPARSE = [("tile64", 1, 1, False, False, 0), ("tile64", 70, 10, True, True, 0), ("tile64", 70, 1024, True, False, 0), ("batch", 70, 1024, False, False, 0),
          ("batch", 1, 10, True, False, 0), ("batch", 70, 1, False, True, 0), ("batch", 70, 20, False, False, 30 * 1920)]


@covers("SparseIndex.topk_device")
@pytest.mark.parametrize("index,B,k,masked,on_side,cand_cap", SPARSE)
def test_sparse_topk(sparse, side, index, B, k, masked, on_side, cand_cap):
    """cand_cap = 30 x 1 920 bytes cuts the 70 queries into three rounds (tests/sparse_oracle.py "batch70_three_rounds")."""
    import torch
    w = sparse[index]
    what = f"sparse topk {index} B={B} k={k} masked={masked} cand_cap={cand_cap}"
    c, a = _sparse_call(w, what, B, masked, side if on_side else None)
    d_rows, d_scores = c.out("rows", (B, k), torch.int32), c.out("scores", (B, k), torch.float64)
    w["sp"].set_option("cand_cap", cand_cap)
    try:
        w["sp"].topk_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], k, d_rows, d_scores, c.stream, **a["kw"])
        c.check()
        assert w["sp"].get_option("rounds_last") == (3 if cand_cap else 1)
    finally:
        w["sp"].set_option("cand_cap", 0)
    want = smo.topk(w["ix"], *a["q"], k, a["masks"], a["mask_of"]) if masked else so.topk(w["ix"], *a["q"], k)
    assert so.same((d_rows.numpy(), d_scores.numpy()), want), what


@covers("SparseIndex.topk_grouped_device")
@pytest.mark.parametrize("index,B,k,masked,on_side", [("tile64", 1, 1, False, False), ("tile64", 70, 10, True, True), ("batch", 70, 1024, False, False),
                                                      ("batch", 1, 10, True, False), ("batch", 70, 10, True, False), ("tile64", 70, 1024, False, True)])
def test_sparse_topk_grouped(sparse, side, index, B, k, masked, on_side):
    import torch
    w = sparse[index]
    what = f"sparse grouped {index} B={B} k={k} masked={masked}"
    c, a = _sparse_call(w, what, B, masked, side if on_side else None)
    d_rows, d_scores, d_count = c.out("rows", (B, k), torch.int32), c.out("scores", (B, k), torch.float64), c.out("count", (B,), torch.int32)
    w["sp"].topk_grouped_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], k, d_rows, d_scores, d_count, c.stream, **a["kw"])
    c.check()
    want = sgo.topk(w["ix"], *a["q"], k, w["groups"], a["masks"], a["mask_of"])
    assert sgo.same((d_rows.numpy(), d_scores.numpy(), d_count.numpy()), want), what


@covers("SparseIndex.score_rows_device")
@pytest.mark.parametrize("index,B,m,on_side", [("tile64", 1, 1, False), ("tile64", 70, 100, True), ("batch", 70, 100, False), ("batch", 1, 100, False),
                                               ("batch", 70, 1, True), ("tile64", 70, 1, False)])
def test_sparse_score_rows(sparse, side, index, B, m, on_side):
    import torch
    w = sparse[index]
    n = w["ix"]["n_docs"]
    what = f"sparse score_rows {index} B={B} m={m}"
    c, a = _sparse_call(w, what, B, False, side if on_side else None)
    rows = np.random.default_rng(B + m).integers(0, n, size=(B, m)).astype(np.int32)
    rows[1::3, 0] = -1
    rows[0::3, m - 1] = n
    d_r, out = c.inp("rows", rows), c.out("scores", (B, m), torch.float64)
    w["sp"].score_rows_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], d_r, m, out, c.stream)
    c.check()
    want = ho.sparse_score_rows(w["ix"], *a["q"], rows)
    assert np.array_equal(out.numpy().view(np.uint64), want.view(np.uint64)), what


# ---- hybrid --------------------------------------------------------------------------------------------------------------------------------------
HYBRID = ["n1_1x0_b3", "n1_0x1_b3", "n65_33x32_b3", "n2048_1024x1024_b3", "n200_100x100_b70"]        # K1 + K2 of 1, 65 and 2 048; a batch of 70
_HYBRID_CASES = {}


def _hybrid_case(name):
    if not _HYBRID_CASES:
        _HYBRID_CASES.update({c["name"]: c for c in ho.cases()})
    return _HYBRID_CASES[name]


@pytest.fixture(scope="module")
def hybrid():
    ks = _hybrid_case(HYBRID[0])["ks"]
    assert all(_hybrid_case(n)["ks"] is ks for n in HYBRID)
    key_group = (np.arange(ks["n_keys"]) % 37).astype(np.int32)
    key_group[::11] = -1
    hm = nat.HybridMap(ks["nb"], ks["dense_key"], ks["known"])
    hm.set_groups(key_group)
    yield {"hm": hm, "ks": ks, "key_group": key_group}
    hm.close()


def _pools(c, case):
    """The four pool arrays as frozen inputs (None for a pool of width 0, as the blocking forms pass them) and (B, K1, K2)."""
    sp_rows, sp_scores, de_rows, de_scores = case["pools"]
    B, K1, K2 = sp_rows.shape[0], sp_rows.shape[1], de_rows.shape[1]
    d = [c.inp(n, a) if a.shape[1] else None for n, a in (("sp_rows", sp_rows), ("sp_scores", sp_scores), ("de_rows", de_rows), ("de_scores", de_scores))]
    return d, B, K1, K2


def _top_ks(K1, K2):
    return sorted({1, min(K1 + K2, nat.MAX_K)})            # top_k of 1 and of K1 + K2, which the route admits up to RQ_MAX_K


def _fused_outs(c, B, k, with_pos):
    import torch
    return [c.out("keys", (B, k), torch.int32), c.out("b", (B, k), torch.float64), c.out("d", (B, k), torch.float64), c.out("h", (B, k), torch.float64),
            c.out("pos", (B, k), torch.int32) if with_pos else None, c.out("count", (B,), torch.int32)]


def _fused_got(c, with_pos):
    return c.host(*(["keys", "b", "d", "h"] + (["pos"] if with_pos else []) + ["count"]))


@covers("HybridMap.missing_device")
@pytest.mark.parametrize("name", HYBRID)
def test_hybrid_missing(hybrid, side, name):
    import torch
    case = _hybrid_case(name)
    c = Call(f"hybrid missing {name}", side if name.endswith("b70") else None)
    d, B, K1, K2 = _pools(c, case)
    md = c.out("miss_dense", (B, K1), torch.int64) if K1 else None
    ms = c.out("miss_sparse", (B, K2), torch.int32) if K2 else None
    hybrid["hm"].missing_device(d[0], d[2], B, K1, K2, md, ms, c.stream)
    c.check()
    want = ho.missing(hybrid["ks"], case["pools"][0], case["pools"][2])
    got = (md.numpy() if K1 else want[0], ms.numpy() if K2 else want[1])
    assert ho.same(got, want), c.what


@covers("HybridMap.fuse_device")
@pytest.mark.parametrize("extras,with_pos", [(False, True), (True, False), (True, True)])
@pytest.mark.parametrize("name", HYBRID)
def test_hybrid_fuse(hybrid, side, name, extras, with_pos):
    case = _hybrid_case(name)
    e = ho.extras_for(case) if extras else {}
    for top_k in _top_ks(case["pools"][0].shape[1], case["pools"][2].shape[1]):
        c = Call(f"hybrid fuse {name} top_k={top_k} extras={extras} d_pos={with_pos}", side if name.endswith("b70") else None)
        d, B, K1, K2 = _pools(c, case)
        kw = {f"d_{n}": c.inp(n, a) for n, a in e.items() if a.shape[1]}
        outs = _fused_outs(c, B, top_k, with_pos)
        hybrid["hm"].fuse_device(*d, B, K1, K2, top_k, *outs, c.stream, **kw)
        c.check()
        want = ho.fuse(hybrid["ks"], *case["pools"], top_k, **e)
        assert ho.same(_fused_got(c, with_pos), want if with_pos else want[:4] + (want[5],)), c.what


@covers("HybridMap.fuse_grouped_device")
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("name", HYBRID)
def test_hybrid_fuse_grouped(hybrid, side, name, with_pos):
    case = _hybrid_case(name)
    for top_k in _top_ks(case["pools"][0].shape[1], case["pools"][2].shape[1]):
        c = Call(f"hybrid fuse grouped {name} top_k={top_k} d_pos={with_pos}", side if name.endswith("b70") else None)
        d, B, K1, K2 = _pools(c, case)
        outs = _fused_outs(c, B, top_k, with_pos)
        hybrid["hm"].fuse_grouped_device(*d, B, K1, K2, top_k, *outs, c.stream)
        c.check()
        want = hgo.fuse(hybrid["ks"], hybrid["key_group"], *case["pools"], top_k)
        assert hgo.same(_fused_got(c, with_pos), want if with_pos else want[:4] + (want[5],)), c.what


# ---- router --------------------------------------------------------------------------------------------------------------------------------------
ROUTER = ["p1_b3_h16", "p65_b3_h16", "p1024_b3_h16", "p100_b70_h64"]


@covers("RouterGate.gate_device", "RouterGate.rerank_device")
@pytest.mark.parametrize("mode", t_router.MODES)
@pytest.mark.parametrize("name", ROUTER)
def test_router_gate_and_rerank(side, name, mode):
    """P of 1, 65 and 1 024 with top_r of 1 and P, in both normalisation modes; the rerank is compared bit for bit given the gate's own w,
    the gate within test_gpu_router's derived tolerance, as tests/test_gpu_router.py does."""
    import torch
    case = next(c for c in rgo.cases() if c["name"] == name)
    stats = case["stats"] if mode == rgo.STATS else None
    B, P = case["b"].shape
    on = side if name.endswith("h64") else None
    ng = t_router._native_gate(case["weights"])
    try:
        c = Call(f"router gate {name} {mode}", on)
        d_b, d_d = c.inp("b", case["b"]), c.inp("d", case["d"])
        d_w = c.out("w", (B, P), torch.float64)
        ng.gate_device(d_b, d_d, B, P, d_w, t_router.MODE_ID[mode], stats, c.stream)
        c.check()
        w = d_w.numpy()
        t_router._gate_close(w, t_router._oracle_w(case, mode))
        for top_r in sorted({1, P}):
            c = Call(f"router rerank {name} {mode} top_r={top_r}", on)
            ins = [c.inp(n, case[n]) for n in ("keys", "b", "d", "count")]
            outs = [c.out(n, (B, top_r), t) for n, t in (("keys", torch.int32), ("b", torch.float64), ("d", torch.float64), ("w", torch.float64),
                                                          ("h", torch.float64), ("pos", torch.int32))] + [c.out("count", (B,), torch.int32)]
            ng.rerank_device(*ins, B, P, top_r, *outs, t_router.MODE_ID[mode], stats, c.stream)
            c.check()
            got = c.host("keys", "b", "d", "w", "h", "pos", "count")
            assert rgo.same(got, rgo.rerank_given_w(case["keys"], case["b"], case["d"], w, case["count"], top_r)), c.what
    finally:
        ng.close()


# ---- refusals: RQ_EINVAL leaves every output, guards included, as it was --------------------------------------------------------------------------
@covers("NativeIndex.search_device", "NativeIndex.search_fixup_device", "NativeIndex.search_filtered_each_device", "NativeIndex.search_filtered_each_fixup_device")
def test_refused_searches_write_nothing(world):
    sh, B, k = world["wide"], 65, 10
    c = _search_bufs(sh, "refused search", B, k, True, None)
    q, outs = c.ins["queries"], _search_args(c)
    foreign = world["tiny"].filters["third"]
    refused(c, lambda: sh.idx.search_device(q, B, 0, COS, *outs, c.stream))
    refused(c, lambda: sh.idx.search_device(q, B, nat.MAX_K + 1, COS, *outs, c.stream, row_filter=sh.filters["third"]))
    refused(c, lambda: sh.idx.search_device(q, B, k, COS, *outs, c.stream, row_filter=foreign))
    refused(c, lambda: sh.idx.search_fixup_device(q, B, 0, COS, *outs, c.stream))
    refused(c, lambda: sh.idx.search_fixup_device(q, B, k, COS, *outs, c.stream, row_filter=foreign))
    each = [None] * (B - 1) + [foreign]                                  # one filter of another index ANYWHERE refuses the whole call
    refused(c, lambda: sh.idx.search_filtered_each_device(q, B, k, COS, *outs, each, c.stream))
    refused(c, lambda: sh.idx.search_filtered_each_device(q, B, 0, COS, *outs, [None] * B, c.stream))
    refused(c, lambda: sh.idx.search_filtered_each_fixup_device(q, B, k, COS, *outs, each, c.stream))


@covers("NativeIndex.search_range_device", "NativeIndex.search_range_fixup_device", "NativeIndex.search_grouped_device", "NativeIndex.search_grouped_fixup_device",
        "NativeIndex.group_collapse_device", "NativeIndex.search_group_members_device", "NativeIndex.search_group_members_fixup_device",
        "NativeIndex.group_fill_device", "NativeIndex.mmr_select_device", "NativeIndex.score_rows_device")
def test_refused_dense_calls_write_nothing(world):
    """The Python wrappers check sizes themselves, so these refusals are ones only the library can make: a filter of another index, an
    unknown metric where the wrapper passes it on, a null input pointer."""
    import torch
    sh, B, k = world["wide"], 65, 10
    foreign = world["tiny"].filters["third"]
    c = Call("refused range")
    q, thr = sh.queries(c, B), c.inp("thresholds", np.zeros(B, np.float32))
    outs = [c.out("scores", (B, 7), torch.float32), c.out("rows", (B, 7), torch.int64), c.out("keys", (B, 7), torch.int64), c.out("count", (B,), torch.int64),
            c.out("status", (B,), torch.int32)]
    refused(c, lambda: sh.idx.search_range_device(q, B, thr, 7, COS, *outs, c.stream, row_filter=foreign))
    refused(c, lambda: sh.idx.search_range_device(q, B, None, 7, COS, *outs, c.stream))
    refused(c, lambda: sh.idx.search_range_fixup_device(q, B, thr, 7, COS, *outs, c.stream, row_filter=foreign))
    c, outs = _grouped_bufs(sh, "refused grouped", B, k, True, None)
    q = c.ins["queries"]
    refused(c, lambda: sh.idx.search_grouped_device(q, B, k, COS, *outs, c.stream, row_filter=foreign))
    refused(c, lambda: sh.idx.search_grouped_fixup_device(q, B, k, COS, *outs, c.stream, row_filter=foreign))
    cand = c.inp("cand_rows", np.zeros((B, 20), np.int64))
    refused(c, lambda: sh.idx.group_collapse_device(cand, None, None, B, 20, k, *outs, c.stream))
    c = _members_bufs(sh, "refused members", B, 3, 3, None)
    q = c.ins["queries"]
    outs = [c.outs[n] for n in ("scores", "rows", "groups", "count", "status")]
    refused(c, lambda: sh.idx.search_group_members_device(q, B, 3, 3, COS, *outs, c.stream, row_filter=foreign))
    refused(c, lambda: sh.idx.search_group_members_fixup_device(q, B, 3, 3, COS, *outs, c.stream, row_filter=foreign))
    wr, wg = c.inp("win_rows", np.zeros((B, 3), np.int64)), c.inp("win_groups", np.zeros((B, 3), np.int32))
    refused(c, lambda: sh.idx.group_fill_device(q, B, 3, 3, COS, wr, wg, outs[0], outs[1], outs[3], outs[4], c.stream, row_filter=foreign))
    c = Call("refused mmr")
    d_r, d_s = c.inp("cand_rows", np.zeros((B, 20), np.int64)), c.inp("cand_rel", np.zeros((B, 20), np.float32))
    outs = [c.out("scores", (B, k), torch.float32), c.out("rows", (B, k), torch.int64), c.out("mmr", (B, k), torch.float32)]
    refused(c, lambda: sh.idx.mmr_select_device(d_r, d_s, B, 20, k, 0.5, 7, *outs, c.stream))            # an unknown metric
    c = Call("refused score_rows")
    q, out = sh.queries(c, B), c.out("scores", (B, 20), torch.float32)
    refused(c, lambda: sh.idx.score_rows_device(q, B, None, 20, COS, out, c.stream))


@covers("SparseIndex.topk_device", "SparseIndex.topk_grouped_device", "SparseIndex.score_rows_device")
def test_refused_sparse_calls_write_nothing(sparse):
    import torch
    w, B, k = sparse["tile64"], 70, 10
    c, a = _sparse_call(w, "refused sparse", B, True, None)
    d_rows, d_scores, d_count = c.out("rows", (B, k), torch.int32), c.out("scores", (B, k), torch.float64), c.out("count", (B,), torch.int32)
    sp = w["sp"]
    refused(c, lambda: sp.topk_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], 0, d_rows, d_scores, c.stream), "k ")
    refused(c, lambda: sp.topk_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], nat.SPARSE_MAX_K + 1, d_rows, d_scores, c.stream, **a["kw"]), "k ")
    refused(c, lambda: sp.topk_device(a["d_ptr"], a["d_tok"], 0, a["n_tok"], k, d_rows, d_scores, c.stream), "B ")
    refused(c, lambda: sp.topk_grouped_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], 0, d_rows, d_scores, d_count, c.stream, **a["kw"]), "k ")
    rows = c.inp("rows", np.zeros((B, k), np.int32))
    refused(c, lambda: sp.score_rows_device(a["d_ptr"], a["d_tok"], B, a["n_tok"], rows, 0, d_scores, c.stream), "m ")


@covers("HybridMap.missing_device", "HybridMap.fuse_device", "HybridMap.fuse_grouped_device")
def test_refused_hybrid_calls_write_nothing(hybrid):
    import torch
    case = _hybrid_case("n65_33x32_b3")
    hm = hybrid["hm"]
    c = Call("refused hybrid")
    d, B, K1, K2 = _pools(c, case)
    md, ms = c.out("miss_dense", (B, K1), torch.int64), c.out("miss_sparse", (B, K2), torch.int32)
    outs = _fused_outs(c, B, 5, True)
    extra = c.inp("extra_dense", np.zeros((B, K1), np.float32))
    refused(c, lambda: hm.missing_device(d[0], d[2], 0, K1, K2, md, ms, c.stream), "B ")
    refused(c, lambda: hm.missing_device(d[0], d[2], B, nat.MAX_K + 1, K2, md, ms, c.stream), "K1 ")
    refused(c, lambda: hm.fuse_device(*d, B, K1, K2, 0, *outs, c.stream), "top_k")
    refused(c, lambda: hm.fuse_device(*d, B, K1, K2, nat.MAX_K + 1, *outs, c.stream), "top_k")            # (why K1 + K2 = 2 048 is fused at top_k = RQ_MAX_K)
    refused(c, lambda: hm.fuse_device(*d, B, K1, K2, 5, *outs, c.stream, d_extra_dense=extra), "without its miss")
    refused(c, lambda: hm.fuse_grouped_device(*d, B, K1, K2, 0, *outs, c.stream), "top_k")


@covers("RouterGate.gate_device", "RouterGate.rerank_device")
def test_refused_router_calls_write_nothing():
    import torch
    case = next(c for c in rgo.cases() if c["name"] == "p65_b3_h16")
    B, P, r = 3, 65, 5
    ng = t_router._native_gate(case["weights"])
    try:
        c = Call("refused router")
        ins = [c.inp(n, case[n]) for n in ("keys", "b", "d", "count")]
        d_w = c.out("w", (B, P), torch.float64)
        outs = [c.out(n, (B, r), t) for n, t in (("keys", torch.int32), ("b", torch.float64), ("d", torch.float64), ("ow", torch.float64),
                                                  ("h", torch.float64), ("pos", torch.int32))] + [c.out("count", (B,), torch.int32)]
        refused(c, lambda: ng.gate_device(ins[1], ins[2], B, P, d_w, 2, None, c.stream), "mode")
        refused(c, lambda: ng.gate_device(ins[1], ins[2], B, P, d_w, nat.ROUTER_NORM_STATS, None, c.stream), "statistics")
        refused(c, lambda: ng.rerank_device(*ins, B, P, P + 1, *outs, nat.ROUTER_NORM_QUERY, None, c.stream), "top_r")
        refused(c, lambda: ng.rerank_device(*ins, B, P, 0, *outs, nat.ROUTER_NORM_QUERY, None, c.stream), "top_r")
    finally:
        ng.close()
