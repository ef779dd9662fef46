"""Searches with one filter per query on the MI355X (include/rq.h "per-query filters", csrc/rq_filter_each.hip): query q
of an each-call equals the oracle restricted to the rows of filters[q] -- rows identical, |score difference| <= 1e-6 (the bar of
tests/test_gpu_parity.py) -- and rows, keys and score bits equal the host loop of single-filter calls over the same groups, which
was the only way to get the result before.  The oracle is tests/filter_oracle.py (tests/nonfinite_oracle.py for the non-finite
cases).  Shapes are small and chosen for where the new kernels can go wrong: tenant lists of 256 and 257 rows (both sides of a
chunk edge), lists of 1 .. 513 rows, more queries than one pass, rounds cut by the key cap, both stored row lengths."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
N_BASE = 4101                      # 65 bins; row % 16 == t: 257 rows for t < 5, 256 otherwise
GATHER, SCAN, EXACT, NULL_BIT = 1, 2, 3, 4
ROUTES = [-1, GATHER, SCAN, EXACT]
MIXED = [f"t{t}" for t in range(16)] + ["five_rows", "none", "all", "random50", None]


def tenant_masks(n, tenants=16):
    return {f"t{t}": np.arange(n) % tenants == t for t in range(tenants)}


class World:
    """One index with its rows, 64 queries, their canonical scores (computed once), the shared masks and one filter per mask."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, options=(), x16=None, q=None, row_offset=0):
        self.n, self.dim = n, dim
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed) if x16 is None else x16
        self.q = orc.synthetic_queries(64, dim, seed=seed + 1) if q is None else q
        self.idx = nat.NativeIndex(dim, 0)
        for name, v in options:
            self.idx.set_option(name, v)
        self.idx.set_option("scan8", 0)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self.masks = {**fo.standard_masks(n), **tenant_masks(n)}
        self._filters, self._scores = {}, {}

    def scores(self, metric=COS):
        if metric not in self._scores:
            self._scores[metric] = orc.exact_scores(self.q, self.x16, metric)
        return self._scores[metric]

    def filter(self, name):
        if name is None:
            return None
        if name not in self._filters:
            self._filters[name] = self.idx.make_filter(self.masks[name])
            assert self._filters[name].count == int(self.masks[name].sum())
        return self._filters[name]

    def filters(self, names):
        return [self.filter(nm) for nm in names]

    def want(self, names, k, scores=None, row_offset=0):
        """The oracle of the each-call: query i ranked over the rows of masks[names[i]] (None: every row)."""
        scores = self.scores() if scores is None else scores
        s = np.zeros((len(names), k), np.float32); r = np.full((len(names), k), -1, np.int64)
        for nm in dict.fromkeys(names):
            pos = [i for i, x in enumerate(names) if x == nm]
            mask = np.ones(self.n, dtype=bool) if nm is None else self.masks[nm]
            s[pos], r[pos] = fo.filtered_topk_from_scores(scores[pos], mask, k, row_offset)
        return s, r

    def close(self):
        for f in self._filters.values():
            f.close()
        self.idx.close()


@pytest.fixture(scope="module")
def base():
    w = World()
    yield w
    w.close()


def deal(entries, B):
    return [entries[i % len(entries)] for i in range(B)]


def _same(got, want, what=""):
    (s, r), (gs, gr) = got, want
    assert np.array_equal(r, gr), f"{what}: rows differ at {np.argwhere(r != gr)[:4].tolist()}"
    err = float(np.abs(s - gs).max(initial=0.0))
    assert err <= SCORE_TOL, f"{what}: scores differ by {err}"


def _bits(a, b, what=""):
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: not bit for bit"


class Dev:
    """One device call on a stream with its own buffers (kept alive by the object); outputs start as 7s."""

    def __init__(self, q, k):
        import torch
        self.B, self.k = len(q), k
        self.q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        self.s = torch.full((self.B, k), 7.0, dtype=torch.float32, device="cuda")
        self.r = torch.full((self.B, k), 7, dtype=torch.int64, device="cuda")
        self.keys = torch.full((self.B, k), 7, dtype=torch.int64, device="cuda")       # (uint64 bit patterns)
        self.st = torch.full((self.B,), 7, dtype=torch.int32, device="cuda")

    def each(self, idx, filters, metric=COS, stream=0):
        idx.search_filtered_each_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, filters, stream)
        return self

    def each_fixup(self, idx, filters, metric=COS, stream=0):
        return idx.search_filtered_each_fixup_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, filters, stream)

    def single(self, idx, flt, metric=COS, stream=0):
        idx.search_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, stream, row_filter=flt)
        return self

    def single_fixup(self, idx, flt, metric=COS, stream=0):
        return idx.search_fixup_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, stream, row_filter=flt)

    def status(self):
        import torch
        torch.cuda.synchronize()
        return self.st.cpu().numpy().copy()

    def result(self):
        import torch
        torch.cuda.synchronize()
        return self.s.cpu().numpy(), self.r.cpu().numpy()

    def all(self):
        return (*self.result(), self.keys.cpu().numpy())


def host_loop(idx, q, k, filters, metric=COS):
    """Today's way: one single-filter device call (and its fixup) per distinct filter, over that filter's queries.  Returns
    (scores, rows, keys, status before the repairs, number repaired)."""
    B = len(filters)
    s = np.zeros((B, k), np.float32); r = np.zeros((B, k), np.int64); keys = np.zeros((B, k), np.int64); st = np.zeros(B, np.int32)
    repaired = 0
    groups = {}
    for i, f in enumerate(filters):
        groups.setdefault(id(f), (f, []))[1].append(i)
    for f, pos in groups.values():
        d = Dev(q[pos], k).single(idx, f, metric)
        st[pos] = d.status()
        repaired += d.single_fixup(idx, f, metric)
        s[pos], r[pos], keys[pos] = d.all()
    return s, r, keys, st, repaired


def each_call(idx, q, k, filters, metric=COS, route=-1):
    """The each-call and its fixup on the device; returns (scores, rows, keys, status before the repair, number repaired)."""
    idx.set_option("filter_route", route)
    try:
        d = Dev(q, k).each(idx, filters, metric)
        st = d.status()
        repaired = d.each_fixup(idx, filters, metric)
        assert repaired == int((st != 0).sum()), f"the fixup repaired {repaired} of {int((st != 0).sum())} flagged queries"
        assert not d.status().any()
        return (*d.all(), st, repaired)
    finally:
        idx.set_option("filter_route", -1)


def opt(idx, name):
    return int(idx.get_option(name))


# ---- 1. the mixed batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_mixed_batch_through_every_route(base, route):
    """Sixteen tenants (lists of 257 and 256 rows), five_rows, none, all, random50 and NULL, dealt to the 64 queries interleaved."""
    names = deal(MIXED, 64)
    filters = base.filters(names)
    calls = opt(base.idx, "filter_each_calls")
    t0 = base.idx.timing()
    s, r, keys, _, _ = each_call(base.idx, base.q, 10, filters, route=route)
    t1 = base.idx.timing()
    assert opt(base.idx, "filter_each_calls") == calls + 1 and opt(base.idx, "filter_each_groups_last") == len(MIXED)
    assert t1["searches"] - t0["searches"] == 1 and t1["queries"] - t0["queries"] == 64        # one search, not one per group
    routes, ragged, shared = opt(base.idx, "filter_each_routes_last"), opt(base.idx, "filter_each_ragged_last"), opt(base.idx, "filter_each_shared_exact_last")
    assert routes & 1 and routes & (1 << NULL_BIT)
    n_null, n_none = names.count(None), names.count("none")
    if route == GATHER:
        assert ragged == 64 - n_null - n_none and shared == 0 and routes == 1 | (1 << GATHER) | (1 << NULL_BIT)
    elif route == EXACT:
        assert shared == 64 - n_null - n_none and ragged == 0 and routes == 1 | (1 << EXACT) | (1 << NULL_BIT)
    elif route == SCAN:
        assert ragged == 0 and shared == 0
    else:
        assert ragged == sum(1 for nm in names if nm is not None and (nm.startswith("t") or nm == "five_rows")) and shared == 0
    _same((s, r), base.want(names, 10), f"route {route}")
    base.idx.set_option("filter_route", route)
    try:
        ls, lr, lkeys, _, _ = host_loop(base.idx, base.q, 10, filters)
    finally:
        base.idx.set_option("filter_route", -1)
    assert np.array_equal(r, lr) and np.array_equal(keys, lkeys), f"route {route}: rows or keys differ from the loop"
    gathered = [i for i, nm in enumerate(names) if nm is not None and (nm.startswith("t") or nm == "five_rows")]
    sel = slice(None) if route in (GATHER, EXACT) else gathered
    assert np.array_equal(s[sel].view(np.uint32), ls[sel].view(np.uint32)), f"route {route}: score bits differ from the loop"
    pad = [i for i, nm in enumerate(names) if nm == "none"]
    assert (r[pad] == -1).all() and not s[pad].any() and not keys[pad].any()
    five = [i for i, nm in enumerate(names) if nm == "five_rows"]
    assert (r[five][:, 5:] == -1).all() and (r[five][:, :5] >= 0).all() and not keys[five][:, 5:].any()


# ---- 2. list lengths and padding -------------------------------------------------------------------------------------------
LENGTHS = [1, 255, 256, 257, 511, 512, 513]


@pytest.fixture(scope="module")
def lengths(base):
    rng = np.random.default_rng(8)
    masks = {}
    for L in LENGTHS:
        m = np.zeros(N_BASE, dtype=bool)
        m[rng.choice(N_BASE, size=L, replace=False)] = True
        masks[f"len{L}"] = m
    base.masks.update(masks)
    return [f"len{L}" for L in LENGTHS]


@pytest.mark.parametrize("k", [10, 300])
def test_list_lengths_around_the_chunk_edges(base, lengths, k):
    """One query per list of 1, 255, 256, 257, 511, 512 and 513 rows; k = 300 pads every list shorter than that: k_eff = min(k, rows)."""
    filters = base.filters(lengths)
    q = base.q[:len(LENGTHS)]
    s, r, keys, st, _ = each_call(base.idx, q, k, filters)
    assert opt(base.idx, "filter_each_ragged_last") == len(LENGTHS) and not st.any()
    _same((s, r), base.want(lengths, k, base.scores()[:len(LENGTHS)]), f"k = {k}")
    for i, L in enumerate(LENGTHS):
        ke = min(k, L)
        assert (r[i, :ke] >= 0).all() and (r[i, ke:] == -1).all() and not s[i, ke:].any() and not keys[i, ke:].any(), f"list of {L} rows at k = {k}"
        assert base.masks[lengths[i]][r[i, :ke]].all()


def test_a_zero_norm_query_returns_the_first_rows_of_its_own_tenant(base):
    names = deal(MIXED, 64)
    q = base.q.copy()
    zero = [0, 5, 16, 19, 20]                              # t0 (257 rows), t5 (256), five_rows, random50, NULL
    q[zero] = 0
    scores = base.scores().copy()
    scores[zero] = 0
    for route in (-1, EXACT):
        s, r, _, _, _ = each_call(base.idx, q, 10, base.filters(names), route=route)
        _same((s, r), base.want(names, 10, scores), f"route {route}")
        assert r[0].tolist() == list(range(0, 160, 16)) and r[5].tolist() == list(range(5, 165, 16)) and not s[zero].any()
        assert r[16, :5].tolist() == np.flatnonzero(base.masks["five_rows"]).tolist() and (r[16, 5:] == -1).all()
        assert r[20].tolist() == list(range(10))


# ---- 3. one tenant per query ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [65, 130])
def test_one_tenant_per_query(base, B):
    """More distinct filters than one pass has queries: the rule gathers every one, in ONE ragged round."""
    masks = {f"own{B}_{t}": np.arange(N_BASE) % B == t for t in range(B)}
    base.masks.update(masks)
    names = list(masks)
    q = orc.synthetic_queries(B, 768, seed=B)
    scores = orc.exact_scores(q, base.x16, COS)
    s, r, keys, st, _ = each_call(base.idx, q, 10, base.filters(names))
    assert opt(base.idx, "filter_each_ragged_last") == B and opt(base.idx, "filter_each_rounds_last") == 1
    assert opt(base.idx, "filter_each_groups_last") == B and opt(base.idx, "filter_route_last") == GATHER and not st.any()
    _same((s, r), base.want(names, 10, scores), f"B = {B}")
    assert ((r % B) == np.arange(B)[:, None]).all()


# ---- 4. rounds -------------------------------------------------------------------------------------------------------------
def test_rounds_cut_by_the_key_cap(base):
    """16 tenants x 4 queries: 16 404 keys.  A cap of 1000 keys cuts rounds of three queries; a cap of 100 is below every list, so
    every query gets a round of its own and is still answered."""
    names = deal([f"t{t}" for t in range(16)], 64)
    filters = base.filters(names)
    whole = each_call(base.idx, base.q, 10, filters)
    assert opt(base.idx, "filter_each_rounds_last") == 1
    try:
        for cap, rounds in ((1000, 22), (100, 64)):
            base.idx.set_option("filter_each_key_cap", cap)
            cut = each_call(base.idx, base.q, 10, filters)
            assert opt(base.idx, "filter_each_rounds_last") == rounds and opt(base.idx, "filter_each_ragged_last") == 64
            assert np.array_equal(cut[1], whole[1]) and np.array_equal(cut[2], whole[2]) and np.array_equal(cut[0].view(np.uint32), whole[0].view(np.uint32)), cap
    finally:
        base.idx.set_option("filter_each_key_cap", 0)
    _same(whole[:2], base.want(names, 10))


# ---- 5. the shared exact route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [12, 13, 20])
def test_many_broad_masks_share_one_exact_scan(base, nf):
    masks = {f"half{j}": np.random.default_rng(100 + j).random(N_BASE) < 0.5 for j in range(nf)}
    base.masks.update(masks)
    names = deal(list(masks), 64)
    s, r, _, _, _ = each_call(base.idx, base.q, 10, base.filters(names))
    shared = opt(base.idx, "filter_each_shared_exact_last")
    assert shared == (64 if nf > 12 else 0), f"{nf} masks: {shared} queries took the shared exact route"
    assert opt(base.idx, "filter_each_routes_last") == (1 << (EXACT if nf > 12 else SCAN))
    _same((s, r), base.want(names, 10), f"{nf} masks")


# ---- 6. inner product, row_offset, two shards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [-1, EXACT])
def test_inner_product_row_offset_and_merged_shards(base, route):
    import torch
    cut, k = 2000, 10
    names = deal(MIXED, 64)
    q = 3.0 * base.q
    parts = []
    for lo, hi in ((0, cut), (cut, N_BASE)):
        w = World(hi - lo, x16=base.x16[lo:hi], q=q, row_offset=10 ** 6 + lo)
        w.masks = {nm: m[lo:hi] for nm, m in base.masks.items() if nm in MIXED}
        w.idx.set_option("filter_route", route)
        filters = w.filters(names)
        d = Dev(q, k).each(w.idx, filters, IP)
        d.each_fixup(w.idx, filters, IP)
        s, r, keys = d.all()
        _same((s, r), w.want(names, k, orc.exact_scores(q, w.x16, IP), row_offset=10 ** 6 + lo), f"shard at {lo}")
        parts.append(d.keys.clone())
        w.close()
    keys = torch.cat(parts, dim=1).contiguous()
    out = Dev(q, k)
    nat.merge_keys_device(keys, 2 * k, 64, k, out.s, out.r)
    _same(out.result(), base.want(names, k, orc.exact_scores(q, base.x16, IP), row_offset=10 ** 6), f"route {route}")


# ---- 7. layouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [384, 32])
def test_the_narrow_layout_and_its_row_pad_twin(dim):
    narrow = World(dim=dim, seed=21)
    twin = World(dim=dim, seed=21, options=(("row_pad", 768),))
    assert narrow.idx.row_pad == 384 and twin.idx.row_pad == 768
    names = deal(MIXED, 64)
    want = narrow.want(names, 10)
    for route in (-1, EXACT):
        a = each_call(narrow.idx, narrow.q, 10, narrow.filters(names), route=route)
        b = each_call(twin.idx, twin.q, 10, twin.filters(names), route=route)
        _same(a[:2], want, f"dim {dim} route {route}")
        _bits(a, b, f"dim {dim} route {route}")
        assert np.array_equal(a[2], b[2])
    narrow.close(); twin.close()


# ---- 8. non-finite values --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [-1, SCAN])
@pytest.mark.parametrize("metric", [COS, IP])
def test_nonfinite_rows_and_queries(route, metric):
    """Shard A of tests/nonfinite_oracle.py: a NaN bin, NaN and infinite rows inside the tenants' slices; NaN, infinite, subnormal,
    huge and zero queries.  The statuses are those of the single-filter calls (a route that re-scores every allowed row certifies
    every query; the scan route flags what its certificate cannot cover), the fixup returns exactly the number flagged, and the
    repaired answers match the oracle per filter."""
    q = nfo.queries(768)
    x16 = nfo.shard_a(768, q)
    w = World(x16=x16, q=q)
    names = deal([f"t{t}" for t in range(16)] + ["random50", "all", None], 64)
    filters = w.filters(names)
    try:
        s, r, keys, st, repaired = each_call(w.idx, q, 10, filters, metric, route)
        w.idx.set_option("filter_route", route)
        ls, lr, lkeys, lst, lrep = host_loop(w.idx, q, 10, filters, metric)
        assert np.array_equal(st, lst), f"statuses differ from the single-filter calls at {np.flatnonzero(st != lst).tolist()}"
        assert repaired == lrep == int((lst != 0).sum())
        for nm in dict.fromkeys(names):
            pos = [i for i, x in enumerate(names) if x == nm]
            ws, wr = nfo.topk(q[pos], x16, 10, metric, mask=None if nm is None else w.masks[nm])
            nfo.assert_matches(s[pos], r[pos], ws, wr, SCORE_TOL, f"{nm} route {route} metric {metric}")
        assert np.array_equal(r, lr) and np.array_equal(keys, lkeys)
    finally:
        w.idx.set_option("filter_route", -1)
        w.close()


def test_the_each_fixup_repairs_every_flagged_query_under_its_own_filter(base):
    """eps = 10 on the forced scan route: no certificate can hold, so every query of a group that scans comes back flagged --
    groups whose queries are scattered over the batch, the NULL group among them -- and climbs the ladder with ITS filter."""
    idx = base.idx
    names = deal(MIXED, 64)
    filters = base.filters(names)
    idx.set_option("eps", 10)
    try:
        before = opt(idx, "filter_repaired")
        s, r, keys, st, repaired = each_call(idx, base.q, 10, filters, route=SCAN)
        broad = [i for i, nm in enumerate(names) if nm in (None, "all", "random50")]      # a bound of 10 on scores within [-1, 1]
        empty = [i for i, nm in enumerate(names) if nm == "none"]                        # padding: certified
        assert st[broad].all() and not st[empty].any() and repaired == int(st.sum()) >= len(broad)
        assert opt(idx, "filter_repaired") == before + repaired
        _same((s, r), base.want(names, 10), "repaired")
        # contiguous groups take the ladder through pointer offsets
        names = sorted(names, key=str)
        s, r, keys, st, repaired = each_call(idx, base.q, 10, base.filters(names), route=SCAN)
        assert repaired == int(st.sum()) >= len(broad)
        _same((s, r), base.want(names, 10), "repaired, arranged by filter")
    finally:
        idx.set_option("eps", -1)


# ---- 9. ordering -------------------------------------------------------------------------------------------------------------
def test_an_each_call_completes_what_the_stream_deferred(base):
    """pipeline = 2: a hinted fused call leaves its tail pending; the each-call behind it completes it first and defers nothing."""
    idx = base.idx
    names = deal(MIXED, 64)
    filters = base.filters(names)
    q2 = orc.synthetic_queries(64, 768, seed=99)
    idx.set_option("pipeline", 2)
    try:
        a, b = Dev(base.q, 10), Dev(q2, 10)
        idx.search_hint_next_device(b.q, 64)
        a.single(idx, None)
        b.each(idx, filters)
        got_a, got_b = a.result(), b.result()           # complete in stream order: no flush needed after an each-call
        idx.search_flush_device(0)
        a.single_fixup(idx, None); b.each_fixup(idx, filters)
        _same(a.result(), got_a)
        _same(got_a, orc.topk_from_scores(base.scores(), 10), "the fused call")
        _same(b.result(), got_b)
        _same(got_b, base.want(names, 10, orc.exact_scores(q2, base.x16, COS)), "the each-call")
    finally:
        idx.set_option("pipeline", 0)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import torch
    x16 = orc.synthetic_corpus(300, 768, seed=3)
    q = orc.synthetic_queries(3, 768)
    idx, other = nat.NativeIndex(768, 0), nat.NativeIndex(768, 0)
    idx.add_f16(x16); other.add_f16(x16)
    good, foreign = idx.make_filter(np.arange(0, 300, 3)), other.make_filter(np.arange(0, 300, 3))
    d = Dev(q, 5).each(idx, [good, None, good])
    d.each_fixup(idx, [good, None, good])
    assert (d.result()[1][[0, 2]] % 3 == 0).all()
    state = lambda: (opt(idx, "filter_each_calls"), idx.timing()["searches"], idx.timing()["queries"])
    before = state()

    def refused(match, call):
        d = Dev(q, 5)
        with pytest.raises((nat.RqError, ValueError), match=match):
            call(d)
        torch.cuda.synchronize()
        assert (d.s == 7).all() and (d.r == 7).all() and (d.keys == 7).all() and (d.st == 7).all() and state() == before, match

    refused("another index", lambda d: d.each(idx, [good, foreign, None]))
    refused("another index", lambda d: d.each_fixup(idx, [good, foreign, None]))
    with pytest.raises(nat.RqError, match="another index"):
        idx.search_filtered_each(q, 5, [None, foreign, good])
    lib = idx._lib
    null_array = lambda d: nat._check(lib.rq_search_filtered_each_device(idx._h, None, nat._ptr(d.q), 3, 5, 0, nat._ptr(d.s), nat._ptr(d.r), nat._ptr(d.keys),
                                                                         nat._ptr(d.st), None), "rq_search_filtered_each_device")
    refused("null filter array", null_array)
    arr3 = (nat.C.c_void_p * 3)(None, None, None)
    refused("B 0 outside", lambda d: nat._check(lib.rq_search_filtered_each_device(idx._h, arr3, nat._ptr(d.q), 0, 5, 0, nat._ptr(d.s), nat._ptr(d.r), None,
                                                                                   nat._ptr(d.st), None), "rq_search_filtered_each_device"))
    refused("outside 1..", lambda d: nat._check(lib.rq_search_filtered_each_device(idx._h, arr3, nat._ptr(d.q), 3, nat.MAX_K + 1, 0, nat._ptr(d.s), nat._ptr(d.r), None,
                                                                                   nat._ptr(d.st), None), "rq_search_filtered_each_device"))
    refused("d_status is required", lambda d: nat._check(lib.rq_search_filtered_each_device(idx._h, arr3, nat._ptr(d.q), 3, 5, 0, nat._ptr(d.s), nat._ptr(d.r), None,
                                                                                            None, None), "rq_search_filtered_each_device"))
    refused("one filter", lambda d: d.each(idx, [good, None]))                     # the binding: one entry per query
    multi = nat.NativeIndex(768, devices=[0, 0])
    multi.add_f16(x16)
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_filtered_each(q, 5, [None, None, None])
    multi.close()
    idx.add_f16(x16[:10])                                                             # `good` is stale now, in the middle of the array
    before = state()
    refused("stale filter", lambda d: d.each(idx, [None, good, None]))
    refused("stale filter", lambda d: d.each_fixup(idx, [None, good, None]))
    with pytest.raises(nat.RqError, match="stale filter"):
        idx.search_filtered_each(q, 5, [None, good, None])
    for f in (good, foreign):
        f.close()
    idx.close(); other.close()


# ---- 11. degenerate batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["t3", "random50", "none"])
def test_one_filter_for_the_whole_batch_is_the_existing_call(base, mask):
    flt = base.filter(mask)
    d = Dev(base.q, 10).each(base.idx, [flt] * 64)
    route = opt(base.idx, "filter_route_last")
    e = Dev(base.q, 10).single(base.idx, flt)
    assert opt(base.idx, "filter_each_groups_last") == 1 and opt(base.idx, "filter_route_last") == route
    assert opt(base.idx, "filter_each_ragged_last") == 0 and opt(base.idx, "filter_each_shared_exact_last") == 0
    assert np.array_equal(d.status(), e.status())
    a, b = d.all(), e.all()
    _bits(a, b, mask)
    assert np.array_equal(a[2], b[2])
    _same(base.idx.search_filtered_each(base.q, 10, [flt] * 64), fo.filtered_topk_from_scores(base.scores(), base.masks[mask], 10), mask)


def test_a_batch_of_null_entries_is_the_unfiltered_search(base):
    got = base.idx.search_filtered_each(base.q, 10, [None] * 64)
    assert opt(base.idx, "filter_each_groups_last") == 1 and opt(base.idx, "filter_each_routes_last") == 1 << NULL_BIT
    _bits(got, base.idx.search(base.q, 10), "all NULL")
    _same(got, orc.topk_from_scores(base.scores(), 10))


# ---- 12. end to end ------------------------------------------------------------------------------------------------------------
def test_allowed_ids_each_end_to_end(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    docs = [si.Document(id=f"p{i}", text=f"passage {i} about topic {i % 7} and item {i * 31 % 101}", title=f"T{i}") for i in range(300)]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs)
    emb = HashEmbedder()
    x16 = orc.prepare_rows_f32(emb.embed([d.text for d in docs]), True)
    tenants = [[f"p{i}" for i in range(t, 300, 5)] for t in range(5)]
    reusable = r.dense_index.make_filter(tenants[4])
    queries = ["passage 3 about topic 3", "item 17", docs[42].text, docs[44].text, "topic 5", docs[7].text]
    each = [tenants[0], tenants[1], tenants[2], reusable, None, tenants[0] + ["no such id"]]
    calls = int(r.dense_index._index.get_option("filter_each_calls"))
    got = r.dense_index.search_batch(queries, 20, allowed_ids_each=each)
    assert int(r.dense_index._index.get_option("filter_each_calls")) == calls + 1
    assert int(r.dense_index._index.get_option("filter_each_groups_last")) == 6
    rows = r.dense_index.search_rows_batch(queries, 20, allowed_ids_each=each)[1]
    for i, (qtext, entry) in enumerate(zip(queries, each)):
        mask = np.ones(300, dtype=bool)
        if entry is not None:
            mask = np.zeros(300, dtype=bool)
            mask[(4 if entry is reusable else i if i < 3 else 0)::5] = True
        gs, gr = fo.filtered_topk(emb.embed([qtext]), x16, mask, 20)
        assert [d for d, _, _ in got[i]] == [f"p{j}" for j in gr[0]], i
        np.testing.assert_allclose([s for _, s, _ in got[i]], gs[0], atol=SCORE_TOL)
        assert rows[i].tolist() == gr[0].tolist()
        single = r.dense_index.search(qtext, 20) if entry is None else r.dense_index.search(qtext, 20, allowed_ids=entry)
        assert got[i] == single
    assert got[2][0][0] == "p42" and got[3][0][0] == "p44"
    reusable.close()
    r.close()
