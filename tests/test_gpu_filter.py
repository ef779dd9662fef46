"""Filtered searches on the MI355X (include/rq.h rq_filter / rq_search_filtered*, csrc/rq_filter.hip): the top-k over
an allowed set of rows equals the oracle restricted to those rows -- rows identical, |score difference| <= 1e-6 (the bar of
tests/test_gpu_parity.py) -- whatever route the call takes (gather, masked scan, exact), and bit for bit the unfiltered
search when every row is allowed.  The oracle is tests/filter_oracle.py."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bin_records as br  # noqa: E402
import filter_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
N_BASE = 4101                      # 65 bins, N mod 64 = 5: at k = 10 nb = 18 and 2 nb < 65, the approximate route is the planned one
N_LARGE = 70_000                   # 1 094 quads over 512 workgroups: partitions hold several quads, all 512 maxima in play
GATHER, SCAN, EXACT = 1, 2, 3
ROUTES = [-1, GATHER, SCAN, EXACT]
MASK_NAMES = ["random50", "one_per_bin", "rotation", "top3_excluded", "contiguous10", "five_rows", "none", "all"]


class Shape:
    """One index with its rows, 64 base queries, their canonical scores (computed once) and the shared masks."""

    def __init__(self, n, dim=768, seed=1234, options=()):
        self.n, self.dim = n, dim
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed)
        self.q = orc.synthetic_queries(64, dim, seed=seed + 1)
        self.idx = nat.NativeIndex(dim, 0)
        for name, v in options:
            self.idx.set_option(name, v)
        self.idx.set_option("scan8", 0)
        self.idx.add_f16(self.x16)
        self.scores = orc.exact_scores(self.q, self.x16, COS)
        _, top = orc.topk_from_scores(self.scores, 3)
        self.masks = fo.standard_masks(n, top)
        self._filters = {}

    def filter(self, name):
        if name not in self._filters:
            self._filters[name] = self.idx.make_filter(self.masks[name])
            assert self._filters[name].count == int(self.masks[name].sum())
        return self._filters[name]

    def close(self):
        for f in self._filters.values():
            f.close()
        self.idx.close()


@pytest.fixture(scope="module")
def base():
    sh = Shape(N_BASE)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def large():
    sh = Shape(N_LARGE, seed=77)
    yield sh
    sh.close()


def _same(got, want, what=""):
    (s, r), (gs, gr) = got, want
    assert np.array_equal(r, gr), f"{what}: rows differ at {np.argwhere(r != gr)[:4].tolist()}"
    err = float(np.abs(s - gs).max(initial=0.0))
    assert err <= SCORE_TOL, f"{what}: scores differ by {err}"


def _routed(idx, route, call):
    idx.set_option("filter_route", route)
    try:
        out = call()
        return out, int(idx.get_option("filter_route_last"))
    finally:
        idx.set_option("filter_route", -1)


class Dev:
    """One device call on the null stream with its own buffers (kept alive by the object)."""

    def __init__(self, q, k):
        import torch
        self.B, self.k = len(q), k
        self.q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        self.s = torch.full((self.B, k), 7.0, dtype=torch.float32, device="cuda")
        self.r = torch.full((self.B, k), 7, dtype=torch.int64, device="cuda")
        self.keys = torch.zeros((self.B, k), dtype=torch.int64, device="cuda")       # (uint64 bit patterns)
        self.st = torch.full((self.B,), 7, dtype=torch.int32, device="cuda")

    def search(self, idx, metric=COS, flt=None, stream=0):
        idx.search_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, stream, row_filter=flt)
        return self

    def fixup(self, idx, metric=COS, flt=None, stream=0):
        return idx.search_fixup_device(self.q, self.B, self.k, metric, self.s, self.r, self.keys, self.st, stream, row_filter=flt)

    def result(self):
        import torch
        torch.cuda.synchronize()
        return self.s.cpu().numpy(), self.r.cpu().numpy()


# ---- masks x routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mask", MASK_NAMES)
def test_every_mask_through_every_route(base, mask, route):
    flt = base.filter(mask)
    want = fo.filtered_topk_from_scores(base.scores, base.masks[mask], 10)
    got, took = _routed(base.idx, route, lambda: base.idx.search(base.q, 10, row_filter=flt))
    _same(got, want, f"{mask} route {route} (took {took})")
    na = int(base.masks[mask].sum())
    assert took == (0 if na == 0 else (route if route > 0 else took))
    if na < 10:
        assert (got[1][:, na:] == -1).all() and not got[0][:, na:].any()


def test_all_rows_allowed_is_the_unfiltered_search_bit_for_bit(base):
    """The same kernels over an equal row-scale array: pipeline = 0, scan8 = 0, scan route."""
    flt = base.filter("all")
    for k in (10, 100):
        plain = base.idx.search(base.q, k)
        got, took = _routed(base.idx, SCAN, lambda: base.idx.search(base.q, k, row_filter=flt))
        assert took in (SCAN, EXACT)
        assert np.array_equal(got[1], plain[1]) and np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32)), k


@pytest.mark.parametrize("shape", ["base", "large"])
def test_a_contiguous_range_is_not_scanned_at_k_100(shape, base, large):
    """One source appended together: too few of the tail's partitions hold an allowed row for its threshold to mean anything."""
    sh = base if shape == "base" else large
    flt = sh.filter("contiguous10")
    want = fo.filtered_topk_from_scores(sh.scores, sh.masks["contiguous10"], 100)
    got, took = _routed(sh.idx, -1, lambda: sh.idx.search(sh.q, 100, row_filter=flt))
    _same(got, want, shape)
    assert took in (GATHER, EXACT), took


# ---- data and argument cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_a_zero_norm_query_returns_the_first_allowed_rows(base, route):
    q = base.q.copy()
    q[5] = 0
    scores = base.scores.copy()
    scores[5] = 0
    for mask in ("random50", "five_rows"):
        want = fo.filtered_topk_from_scores(scores, base.masks[mask], 10)
        got, _ = _routed(base.idx, route, lambda: base.idx.search(q, 10, row_filter=base.filter(mask)))
        _same(got, want, f"{mask} route {route}")
        first = np.flatnonzero(base.masks[mask])[:10]
        assert got[1][5, :first.size].tolist() == first.tolist() and not got[0][5].any()


@pytest.mark.parametrize("route", ROUTES)
def test_ties_among_allowed_duplicates_order_by_row(route):
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=5)
    x16[100:401] = x16[7]                                  # 301 identical rows (and row 7)
    mask = np.ones(N_BASE, dtype=bool)
    mask[101:401:2] = False                                # half of the copies excluded
    q = orc.synthetic_queries(4, 768, 13)
    q[1] = x16[7].astype(np.float32)
    idx = nat.NativeIndex(768, 0)
    idx.add_f16(x16)
    flt = idx.make_filter(mask)
    for k in (10, 200):
        want = fo.filtered_topk(q, x16, mask, k)
        got, _ = _routed(idx, route, lambda: idx.search(q, k, row_filter=flt))
        _same(got, want, f"k={k} route {route}")
        assert got[1][1, :3].tolist() == [7, 100, 102]
    flt.close(); idx.close()


@pytest.mark.parametrize("route", ROUTES)
def test_inner_product(base, route):
    q = 3.0 * base.q[:9]
    want = fo.filtered_topk(q, base.x16, base.masks["random50"], 10, IP)
    got, _ = _routed(base.idx, route, lambda: base.idx.search(q, 10, IP, row_filter=base.filter("random50")))
    _same(got, want, f"route {route}")


@pytest.mark.parametrize("route", ROUTES)
def test_row_offset_is_added_to_local_rows(route):
    sh = Shape(1000, seed=9)
    sh.idx.set_row_offset(10 ** 6)
    want = fo.filtered_topk_from_scores(sh.scores, sh.masks["random50"], 10, row_offset=10 ** 6)
    got, _ = _routed(sh.idx, route, lambda: sh.idx.search(sh.q, 10, row_filter=sh.filter("random50")))
    _same(got, want, f"route {route}")
    assert got[1].min() >= 10 ** 6
    sh.close()


@pytest.mark.parametrize("route", ROUTES)
def test_keys_of_two_filtered_shards_merge(base, route):
    import torch
    cut, k = 2000, 10
    mask = base.masks["random50"]
    parts = []
    for lo, hi in ((0, cut), (cut, N_BASE)):
        idx = nat.NativeIndex(768, 0)
        idx.add_f16(base.x16[lo:hi])
        idx.set_row_offset(lo)
        flt = idx.make_filter(mask[lo:hi])
        idx.set_option("filter_route", route)
        d = Dev(base.q, k).search(idx, flt=flt)
        d.fixup(idx, flt=flt)
        torch.cuda.synchronize()
        parts.append(d.keys.clone())
        flt.close(); idx.close()
    keys = torch.cat(parts, dim=1).contiguous()
    out = Dev(base.q, k)
    nat.merge_keys_device(keys, 2 * k, 64, k, out.s, out.r)
    _same(out.result(), fo.filtered_topk_from_scores(base.scores, mask, k), f"route {route}")


# ---- rungs ---------------------------------------------------------------------------------------------------------------
def test_the_exact_rung_through_the_filtered_fixup(large):
    """eps = 10: no certificate can hold, every query climbs the ladder -- fast tail, wider generic pass, fp64 scan -- with the
    filter at every rung.  (The large shape: on the base shape the wider pass would already be planned exact.)"""
    idx, flt = large.idx, large.filter("random50")
    idx.set_option("eps", 10)
    idx.set_option("filter_route", SCAN)
    try:
        t0 = idx.timing()
        before = t0["exact_scans"], t0["widened"], int(idx.get_option("filter_repaired")), int(idx.get_option("scan8_used"))
        d = Dev(large.q, 10).search(idx, flt=flt)
        repaired = d.fixup(idx, flt=flt)
        got = d.result()
        assert repaired == 64 and not d.st.cpu().numpy().any()
        t1 = idx.timing()
        assert t1["exact_scans"] == before[0] + 64 and t1["widened"] == before[1] + 64
        assert int(idx.get_option("filter_repaired")) == before[2] + 64 and int(idx.get_option("scan8_used")) == before[3]
        _same(got, fo.filtered_topk_from_scores(large.scores, large.masks["random50"], 10))
    finally:
        idx.set_option("eps", -1)
        idx.set_option("filter_route", -1)


@pytest.mark.parametrize("mask", ["random50", "rotation", "five_rows"])
def test_the_generic_tail_masks_its_keys(base, large, mask):
    """fast_tail = 0 (base shape) and k = 400 (beyond the fast tail; large shape): select / re-score / mask keys / final."""
    base.idx.set_option("fast_tail", 0)
    try:
        got, took = _routed(base.idx, SCAN, lambda: base.idx.search(base.q, 10, row_filter=base.filter(mask)))
    finally:
        base.idx.set_option("fast_tail", 1)
    assert took == SCAN
    _same(got, fo.filtered_topk_from_scores(base.scores, base.masks[mask], 10), "fast_tail = 0")
    got, took = _routed(large.idx, SCAN, lambda: large.idx.search(large.q[:8], 400, row_filter=large.filter(mask)))
    assert took == SCAN
    _same(got, fo.filtered_topk_from_scores(large.scores[:8], large.masks[mask], 400), "k = 400")


# ---- passes and layouts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [100, 130, 300])
def test_wide_passes_over_the_masked_scale(base, B):
    """B = 100: one pass of 128; 130: one of 256; 300: 256 + 64 (two scan grids in one call)."""
    q = orc.synthetic_queries(B, 768, seed=B)
    for mask in ("random50", "one_per_bin"):
        want = fo.filtered_topk(q, base.x16, base.masks[mask], 10)
        got, took = _routed(base.idx, SCAN, lambda: base.idx.search(q, 10, row_filter=base.filter(mask)))
        assert took == SCAN
        _same(got, want, f"B={B} {mask}")


@pytest.mark.parametrize("dim", [384, 96])
def test_the_narrow_layout_and_its_row_pad_twin(dim):
    narrow = Shape(N_BASE, dim=dim, seed=21)
    twin = Shape(N_BASE, dim=dim, seed=21, options=(("row_pad", 768),))
    assert narrow.idx.row_pad == 384 and twin.idx.row_pad == 768
    for B in (64, 130):
        q = orc.synthetic_queries(B, dim, seed=B + dim)
        for mask in ("random50", "rotation"):
            want = fo.filtered_topk(q, narrow.x16, narrow.masks[mask], 10)
            for route in (-1, SCAN):
                a, _ = _routed(narrow.idx, route, lambda: narrow.idx.search(q, 10, row_filter=narrow.filter(mask)))
                b, _ = _routed(twin.idx, route, lambda: twin.idx.search(q, 10, row_filter=twin.filter(mask)))
                _same(a, want, f"dim {dim} B={B} {mask} route {route}")
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    narrow.close(); twin.close()


# ---- evidence that the scan route really ran ---------------------------------------------------------------------------
def test_the_rule_takes_the_scan_route_and_certifies_without_repair(large):
    idx, flt = large.idx, large.filter("random50")
    idx.set_option("profile", 1)
    try:
        idx.reset_timing()
        before = int(idx.get_option("filter_repaired")), int(idx.get_option("repaired_queries"))
        d = Dev(large.q, 10).search(idx, flt=flt)
        got = d.result()
        status = d.st.cpu().numpy()
        t = idx.timing()
        assert int(idx.get_option("filter_route_last")) == SCAN
        assert t["scan_launches"] == 1 and t["exact_scans"] == 0 and t["widened"] == 0      # one pass of 64 queries
        assert not status.any()                                                                   # certified by construction
        assert d.fixup(idx, flt=flt) == 0
        assert (int(idx.get_option("filter_repaired")), int(idx.get_option("repaired_queries"))) == before
        _same(got, fo.filtered_topk_from_scores(large.scores, large.masks["random50"], 10))
    finally:
        idx.set_option("profile", 0)
        idx.reset_timing()


# ---- bin records of a masked scan -----------------------------------------------------------------------------------------
def _sub_bins(rec, exact, n, bins):
    """Records and exact scores of the chosen bins alone, as a shard of their own (a ragged last bin stays last)."""
    bins = np.asarray(bins)
    rows = np.concatenate([np.arange(64 * b, min(64 * b + 64, n)) for b in bins]) if bins.size else np.zeros(0, np.int64)
    return rec[:, bins], exact[:, rows], int(rows.size)


def _check_masked_records(idx, rec, exact_cos, mask, B, what):
    """tests/bin_records.check_records with -inf at excluded rows.  I1, I2, I6, I7, I8 on every bin; I3 and I4 on bins with an
    allowed row; I5 on bins with two; a bin with none: m1 not NaN and below -1 - beta, so that it never reaches a threshold."""
    n = mask.size
    beta = idx.get_option("eps_cosine")
    exact = np.where(mask[None, :], exact_cos, -np.inf)
    nbins = (n + 63) // 64
    per_bin = np.bincount(np.flatnonzero(mask) // 64, minlength=nbins)
    rep = br.check_records(rec, exact, n, beta, B)
    bad = [f for f in br.failures({k: rep[k] for k in ("I1", "I2", "I6", "I7", "I8")})]
    assert not bad, f"{what}: " + "; ".join(bad)
    r1, e1, n1 = _sub_bins(rec[:B], exact, n, np.flatnonzero(per_bin >= 1))
    rep1 = br.check_records(r1, e1, n1, beta, B)
    bad = br.failures({k: rep1[k] for k in ("I3", "I4")})
    assert not bad, f"{what} (bins with an allowed row): " + "; ".join(bad)
    # I5 speaks of VALID rows; under a filter the second position must be an allowed row wherever the bin has two
    f = br.decode(rec[:B])
    two = np.flatnonzero(per_bin >= 2)
    p1, p2 = f["p1"][:, two], f["p2"][:, two]
    rows2 = 64 * two[None, :] + p2
    assert (p1 != p2).all() and (rows2 < n).all() and mask[np.minimum(rows2, n - 1)].all(), f"{what}: I5 on bins with two allowed rows"
    empty = np.flatnonzero(per_bin == 0)
    m1 = f["m1"][:, empty]
    assert not np.isnan(m1).any() and (m1 < -1.0 - beta).all(), f"{what}: empty bins record {m1.max(initial=-np.inf)}"


@pytest.mark.parametrize("mask", ["one_per_bin", "rotation"])
@pytest.mark.parametrize("dim,B,slots", [(768, 64, 64), (768, 100, 128), (768, 200, 256), (384, 64, 64), (384, 100, 128)])
def test_bin_records_of_a_masked_scan(base, mask, dim, B, slots):
    """The 64-query form, the 128- and 256-query fp16 passes and the two narrow forms, over row scales with NaN at excluded rows."""
    import torch
    sh = base if dim == 768 else Shape(N_BASE, dim=dim, seed=21)
    idx = sh.idx
    q = orc.synthetic_queries(B, dim, seed=1000 + B)
    exact = orc.exact_scores(q, sh.x16, COS)
    idx.set_option("poison_bins", 1)
    idx.set_option("filter_route", SCAN)
    try:
        d = Dev(q, 10).search(idx, flt=sh.filter(mask))
        torch.cuda.synchronize()
        assert int(idx.get_option("filter_route_last")) == SCAN
        rec = idx.debug_bin_records(0, slots)
        with pytest.raises(nat.RqError):
            idx.debug_bin_records(0, slots + 1)
        _check_masked_records(idx, rec, exact, sh.masks[mask], B, f"dim {dim} B={B} {mask}")
        d.fixup(idx, flt=sh.filter(mask))
        _same(d.result(), fo.filtered_topk_from_scores(exact, sh.masks[mask], 10))
    finally:
        idx.set_option("poison_bins", 0)
        idx.set_option("filter_route", -1)
        if sh is not base:
            sh.close()


# ---- ordering and refusals ---------------------------------------------------------------------------------------------
def test_a_filtered_call_completes_what_the_stream_deferred(base):
    """pipeline = 2: a hinted fused call leaves its tail pending; the filtered call behind it completes it first."""
    idx, flt = base.idx, base.filter("random50")
    q1, q2 = base.q, orc.synthetic_queries(64, 768, seed=99)
    idx.set_option("pipeline", 2)
    try:
        a, b = Dev(q1, 10), Dev(q2, 10)
        idx.search_hint_next_device(b.q, 64)
        a.search(idx)
        b.search(idx, flt=flt)
        got_a = a.result()                      # complete in stream order: no flush needed after a filtered call
        idx.search_flush_device(0)
        a.fixup(idx); b.fixup(idx, flt=flt)
        _same(a.result(), got_a)
        _same(got_a, orc.topk_from_scores(base.scores, 10), "the fused call")
        _same(b.result(), fo.filtered_topk(q2, base.x16, base.masks["random50"], 10), "the filtered call")
    finally:
        idx.set_option("pipeline", 0)


def test_first_filtered_calls_on_two_streams():
    """A filter belongs to its index, not to a stream: the masked row scale its first scan builds must be complete before a call on
    ANOTHER stream can find it.  Stream A has work queued in front of the first filtered call; stream B calls right behind it.  The
    same after a reservation, which makes the filter rebuild its array for the new capacity."""
    import torch
    sh = Shape(N_BASE, seed=31)
    idx = sh.idx
    want = fo.filtered_topk_from_scores(sh.scores, sh.masks["random50"], 10)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn((4096, 4096), device="cuda")
    idx.set_option("filter_route", SCAN)
    try:
        for round_ in range(2):
            flt = sh.filter("random50")                      # (no search has used it yet in round 0; stale capacity in round 1)
            a, b = Dev(sh.q, 10), Dev(sh.q, 10)
            torch.cuda.synchronize()
            with torch.cuda.stream(sa):
                for _ in range(40):
                    big = torch.mm(big, big).clamp_(-1, 1)   # queued in front of the first filtered call of stream A
            a.search(idx, flt=flt, stream=sa.cuda_stream)
            b.search(idx, flt=flt, stream=sb.cuda_stream)
            assert int(idx.get_option("filter_route_last")) == SCAN
            torch.cuda.synchronize()
            assert not a.st.cpu().numpy().any() and not b.st.cpu().numpy().any()
            _same(b.result(), want, f"stream B, round {round_}")
            _same(a.result(), want, f"stream A, round {round_}")
            idx.reserve(3 * N_BASE + 5000 * round_)          # a new capacity: the next call rebuilds the filter's array
    finally:
        idx.set_option("filter_route", -1)
        for s in (sa, sb):
            idx.stream_release(s.cuda_stream)
        sh.close()


def test_refusals():
    x16 = orc.synthetic_corpus(300, 768, seed=3)
    q = orc.synthetic_queries(2, 768)
    idx, other = nat.NativeIndex(768, 0), nat.NativeIndex(768, 0)
    idx.add_f16(x16); other.add_f16(x16)
    flt = idx.make_filter(np.arange(0, 300, 3))
    assert flt.count == 100 and len(flt) == 100
    with pytest.raises(nat.RqError, match="another index"):
        other.search(q, 5, row_filter=flt)
    with pytest.raises(ValueError):
        idx.make_filter(np.ones(299, dtype=bool))
    with pytest.raises(ValueError):
        idx.make_filter([300])
    idx.search(q, 5, row_filter=flt)
    idx.add_f16(x16[:10])
    with pytest.raises(nat.RqError, match="stale filter"):
        idx.search(q, 5, row_filter=flt)
    d = Dev(q, 5)
    with pytest.raises(nat.RqError, match="stale filter"):
        d.search(idx, flt=flt)
    with pytest.raises(nat.RqError, match="stale filter"):
        d.fixup(idx, flt=flt)
    multi = nat.NativeIndex(768, devices=[0, 0])
    multi.add_f16(x16)
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.make_filter(np.ones(300, dtype=bool))
    multi.close()
    # destroying the index before the filter is safe from Python: the index has freed it, close() only forgets the handle
    keep = other.make_filter([1, 2, 3])
    other.close()
    keep.close(); keep.close()
    idx.close()
    flt.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_allowed_ids_end_to_end(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    docs = [si.Document(id=f"p{i}", text=f"passage {i} about topic {i % 7} and item {i * 31 % 101}", title=f"T{i}") for i in range(300)]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs)
    emb = HashEmbedder()
    x16 = orc.prepare_rows_f32(emb.embed([d.text for d in docs]), True)
    allowed = [f"p{i}" for i in range(0, 300, 7)] + ["no such id"]
    mask = np.zeros(300, dtype=bool)
    mask[::7] = True
    reusable = r.dense_index.make_filter(allowed)
    for qtext in ("passage 3 about topic 3", "item 17", docs[42].text):
        gs, gr = fo.filtered_topk(emb.embed([qtext]), x16, mask, 20)
        for arg in (allowed, reusable):
            got = r.dense_index.search(qtext, 20, allowed_ids=arg)
            assert [d for d, _, _ in got] == [f"p{i}" for i in gr[0]] and set(d for d, _, _ in got) <= set(allowed)
            np.testing.assert_allclose([s for _, s, _ in got], gs[0], atol=SCORE_TOL)
        assert r.dense_index.search_batch([qtext], 20, allowed_ids=allowed)[0] == got
        rows = r.dense_index.search_rows_batch([qtext], 20, allowed_ids=allowed)[1]
        assert rows[0].tolist() == gr[0].tolist()
        # the hybrid search over the same allowed set: a brute-force restatement of reference :485-523 on masked pools
        bm = r.bm25_index.get_scores(r.bm25_index._tokenize(qtext))
        bm = np.where(mask, bm, 0.0)
        order = [i for i in np.lexsort((-np.arange(300), -bm)) if bm[i] > 0][:50]
        sparse = {f"p{i}": float(bm[i]) for i in order}
        ds, dr = fo.filtered_topk(emb.embed([qtext]), x16, mask, 50)
        dense = {f"p{i}": float(s) for s, i in zip(ds[0], dr[0]) if i >= 0}
        ids = list(dict.fromkeys(list(sparse) + list(dense)))
        mb, md = max(sparse.values(), default=0) or 1, max(dense.values(), default=0) or 1
        hyb = {d: (sparse.get(d, 0.0) / mb + dense.get(d, 0.0) / md) / 2 for d in ids}
        want = sorted(ids, key=lambda d: hyb[d], reverse=True)[:10]
        res = r.hybrid_search(qtext, top_k=10, allowed_ids=allowed)
        assert [x.doc_id for x in res] == want and set(want) <= set(allowed)
        np.testing.assert_allclose([x.hybrid_score for x in res], [hyb[d] for d in want], atol=2e-6)
        routed = r.get_scores_for_router(qtext, num_passages=10, allowed_ids=allowed)
        assert routed[2] == want + [""] * (10 - len(want))
    assert [d for d, _ in r.dense_search(docs[42].text, 1, allowed_ids=allowed)] == ["p42"]      # 42 = 6 x 7 is allowed
    assert r.dense_search(docs[43].text, 1, allowed_ids=allowed)[0][0] != "p43"
    assert r.dense_index.search("item 17", 5, allowed_ids=["no such id"]) == []
    reusable.close()
    r.close()
