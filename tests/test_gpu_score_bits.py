"""Every route's returned scores, held to the fp64 definition BIT FOR BIT on an MI355X (tests/score_bits.py states the rule).

The other GPU tests compare scores with the oracle within SCORE_TOL = 1e-6 and routes with each other bit for bit: a re-score that
drifted to an fp32 accumulation or to a second rounding would move every route together and stay inside that bar
(tests/test_score_bits.py measures it).  Here each route is forced by the options that exist, confirmed from the counters that
exist, and its (query, row, score) triples go through score_bits.assert_score_bits; rows are compared exactly with
score_bits.canonical_topk, whose order near position k depends on the fp32 bits of the planted twins.

One index per layout and metric, 4101 rows (65 bins, a ragged last one), the 8 queries of score_bits.make_case.  Every device
form is followed by its fixup form and every status must be 0 afterwards.  Each test prints the pairs it checked and how many of
them the definition leaves undecided; the totals per layout are printed when the layout's index is closed."""
import numpy as np
import pytest

from rag_uq_amd import _native as nat

import group_members_oracle as gmo
import score_bits as sb
from score_bits import COS, IP, B, K

pytestmark = pytest.mark.gpu

LAYOUTS = [(768, 768), (384, 768), (384, 384), (300, 384)]              # (dim, row_pad)
PARAMS = [(d, p, m) for d, p in LAYOUTS for m in (COS, IP)]
SCAN, GATHER, EXACT = 1, 2, 3                                            # "range_route"; "filter_route" is 1 gather, 2 scan, 3 exact
TOTALS = {}


def new_index(dim, row_pad, x16, devices=None):
    idx = nat.NativeIndex(dim, devices=devices) if devices else nat.NativeIndex(dim, 0)
    if devices:
        idx.set_option("stripe_rows", 64)
    if idx.row_pad != row_pad:
        idx.set_option("row_pad", row_pad)
    idx.add_f16(x16)
    idx.set_option("scan8", 0)                                           # the fp16 scan unless a test asks for the image
    assert idx.row_pad == row_pad and len(idx) == len(x16)
    return idx


class Layout:
    def __init__(self, dim, row_pad, metric):
        self.dim, self.row_pad, self.metric = dim, row_pad, metric
        self.name = f"dim {dim} row_pad {row_pad} {'cosine' if metric == COS else 'inner product'}"
        self.case = sb.make_case(dim, metric)
        self.ref, self.q, self.x16 = self.case.ref, self.case.q, self.case.x16
        self.idx = new_index(dim, row_pad, self.x16)
        self.third = np.arange(sb.N) % 3 == 0

    def bits(self, scores, rows, what, ref=None, cap=sb.CAP):
        checked, und = sb.assert_score_bits(scores, rows, self.ref if ref is None else ref, f"{self.name}: {what}", cap)
        t = TOTALS.setdefault(self.name, [0, 0])
        t[0] += checked
        t[1] += und

    def rows_equal(self, got_rows, want_rows, flagged, what):
        assert not flagged.any(), f"{self.name}: {what}: an undecided pair near the cut (tests/test_score_bits.py keeps the inputs clear of that)"
        got_rows, want_rows = np.asarray(got_rows), np.asarray(want_rows)
        assert np.array_equal(got_rows, want_rows), \
            f"{self.name}: {what}: rows differ at (query, rank) {np.argwhere(got_rows != want_rows)[:4].tolist()}"


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"dim{p[0]}-pad{p[1]}-{'cos' if p[2] == COS else 'ip'}")
def lay(request):
    layout = Layout(*request.param)
    yield layout
    layout.idx.close()
    t = TOTALS.get(layout.name, [0, 0])
    print(f"\nscore bits total [{layout.name}]: {t[0]} pairs checked, {t[1]} undecided")


def device_search(idx, q, k, metric, flt=None, filters=None):
    """The device form, then its fixup, on the null stream -> host (scores, rows), the status before and after the repair."""
    import torch
    nq = len(q)
    d_q = torch.from_numpy(np.array(q, dtype=np.float32)).cuda()
    d_s = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    d_st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if filters is not None:
        idx.search_filtered_each_device(d_q, nq, k, metric, d_s, d_r, None, d_st, filters, 0)
    else:
        idx.search_device(d_q, nq, k, metric, d_s, d_r, None, d_st, 0, row_filter=flt)
    torch.cuda.synchronize()
    before = d_st.cpu().numpy().copy()
    if filters is not None:
        idx.search_filtered_each_fixup_device(d_q, nq, k, metric, d_s, d_r, None, d_st, filters, 0)
    else:
        idx.search_fixup_device(d_q, nq, k, metric, d_s, d_r, None, d_st, 0, row_filter=flt)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_r.cpu().numpy(), before, d_st.cpu().numpy()


def launches(idx, profile, call):
    """call() with "profile" = 1 (every scan pass is counted) or 2 (every fast tail is): (its result, launches counted, timing)"""
    idx.set_option("profile", profile)
    try:
        idx.reset_timing()
        out = call()
        t = idx.timing()
        return out, int(t["scan_launches"]), t
    finally:
        idx.set_option("profile", 0)
        idx.reset_timing()


# ---- the plain search: scan + fast tail, scan + generic tail, int8 image, exact rung, wide passes -------------------------------
@pytest.mark.parametrize("fast_tail", [1, 0])
def test_fp16_scan_with_the_fast_and_the_generic_tail(lay, fast_tail):
    idx = lay.idx
    ws, wr, flagged = sb.canonical_topk(lay.ref, K)
    idx.set_option("fast_tail", fast_tail)
    try:
        assert int(idx.get_option("scan8")) == 0 and int(idx.get_option("fast_tail")) == fast_tail
        used8 = int(idx.get_option("scan8_used"))
        for profile, want in ((1, 1), (2, fast_tail)):                   # one scan pass; one fast tail launch or none (the generic tail)
            (gs, gr, before, after), n, t = launches(idx, profile, lambda: device_search(idx, lay.q, K, lay.metric))
            what = f"fp16 scan, {'fast' if fast_tail else 'generic'} tail"
            assert n == want and t["exact_scans"] == 0 and t["widened"] == 0, (what, profile, n, t)
            assert not before.any() and not after.any(), what                       # certified by that tail, nothing repaired
            lay.rows_equal(gr, wr, flagged, what)
            lay.bits(gs, gr, what)
        assert int(idx.get_option("scan8_used")) == used8
    finally:
        idx.set_option("fast_tail", 1)


def test_int8_image_and_tail(lay):
    idx = lay.idx
    if lay.row_pad != 768:
        idx.set_option("scan8", 2)                                       # the narrow layout builds no image: "scan8" is treated as 0
        try:
            gs, gr, _, after = device_search(idx, lay.q, K, lay.metric)
            assert int(idx.get_option("scan8_used")) == 0 and not after.any()
        finally:
            idx.set_option("scan8", 0)
        lay.bits(gs, gr, "scan8 = 2 on the narrow layout (fp16 scan)")
        return
    ws, wr, flagged = sb.canonical_topk(lay.ref, K)
    used8 = int(idx.get_option("scan8_used"))
    idx.set_option("scan8", 2)
    try:
        gs, gr, _, after = device_search(idx, lay.q, K, lay.metric)
        assert int(idx.get_option("scan8_used")) == used8 + 1, "the int8 image was not scanned"
        assert not after.any()
    finally:
        idx.set_option("scan8", 0)
    lay.rows_equal(gr, wr, flagged, "int8 image")
    lay.bits(gs, gr, "int8 image + tail")


@pytest.mark.parametrize("exact_mfma", [1, 0])
def test_exact_rung_with_both_kernels(lay, exact_mfma):
    idx = lay.idx
    kernel = "rq_exact_scan_kernel" if exact_mfma else "rq_rescore_kernel"
    idx.set_option("exact_mfma", exact_mfma)
    try:
        # k = 64: nb = 72 bins of 65, the plan is the exact scan -- no corpus pass is launched
        ws, wr, flagged = sb.canonical_topk(lay.ref, 64)
        (gs, gr, before, after), n, t = launches(idx, 1, lambda: device_search(idx, lay.q, 64, lay.metric))
        assert n == 0 and t["widened"] == 0 and not before.any() and not after.any(), (kernel, n, t)
        lay.rows_equal(gr, wr, flagged, f"exact rung ({kernel})")
        lay.bits(gs, gr, f"exact rung, k = 64 ({kernel})")
        # 130 rows, k = 130: the whole order comes back, negative scores and the zero row's +0.0 included
        small = sb.make_small(lay.dim, lay.metric)
        sidx = new_index(lay.dim, lay.row_pad, small.x16)
        try:
            sidx.set_option("exact_mfma", exact_mfma)
            ws, wr, flagged = sb.canonical_topk(small.ref, sb.N_SMALL)
            gs, gr, before, after = device_search(sidx, small.q, sb.N_SMALL, lay.metric)
            assert not before.any() and not after.any()
            lay.rows_equal(gr, wr, flagged, f"130 rows ({kernel})")
            assert (gs < 0).any() and not sb.bits(gs[gr == 9]).any()
            lay.bits(gs, gr, f"130 rows, k = 130 ({kernel})", ref=small.ref)
        finally:
            sidx.close()
    finally:
        idx.set_option("exact_mfma", 1)


def test_wide_passes(lay):
    idx = lay.idx
    q = np.concatenate([lay.q, sb.queries(122, lay.dim, lay.metric, seed=66)])          # B = 130: the module's 8 queries first
    ws, wr, flagged = sb.canonical_topk(lay.ref, K)
    (gs, gr, before, after), n, t = launches(idx, 1, lambda: device_search(idx, q, K, lay.metric))
    assert n == (1 if lay.row_pad == 768 else 2), (n, t)                 # one pass of 256 queries; narrow rows: 128, then 64
    assert t["exact_scans"] == 0 and not after.any()
    lay.rows_equal(gr[:B], wr, flagged, "wide passes")
    lay.bits(gs[:B], gr[:B], "wide passes, B = 130")


# ---- filtered searches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2, 3])
def test_filtered_routes(lay, route):
    idx = lay.idx
    flt = idx.make_filter(lay.third)
    ws, wr, flagged = sb.canonical_topk(lay.ref, K, lay.third)
    idx.set_option("filter_route", route)
    try:
        gs, gr, _, after = device_search(idx, lay.q, K, lay.metric, flt=flt)
        assert int(idx.get_option("filter_route_last")) == route and not after.any()
    finally:
        idx.set_option("filter_route", -1)
        flt.close()
    lay.rows_equal(gr, wr, flagged, f"filter route {route}")
    lay.bits(gs, gr, f"filtered, route {route}")


@pytest.mark.parametrize("route", [-1, 1, 2, 3])
def test_per_query_filters(lay, route):
    idx = lay.idx
    masks = [lay.third, ~lay.third, None]
    flts = [idx.make_filter(m) if m is not None else None for m in masks]
    want = [sb.canonical_topk(lay.ref, K, m) for m in masks]
    deal = [b % 3 for b in range(B)]                                     # two different filters and a NULL entry in one call
    wr = np.stack([want[g][1][b] for b, g in enumerate(deal)])
    flagged = np.array([want[g][2][b] for b, g in enumerate(deal)])
    idx.set_option("filter_route", route)
    try:
        gs, gr, _, after = device_search(idx, lay.q, K, lay.metric, filters=[flts[g] for g in deal])
        routes = int(idx.get_option("filter_each_routes_last"))
        assert not after.any()
        assert routes & 16 and routes & 14 and not routes & 1, routes    # the NULL entry and at least one filtered route
        if route > 0:
            assert routes == 16 | (1 << route), routes
    finally:
        idx.set_option("filter_route", -1)
        for f in flts:
            if f is not None:
                f.close()
    lay.rows_equal(gr, wr, flagged, f"per-query filters (route {route})")
    lay.bits(gs, gr, f"per-query filters, route {route}")


# ---- scoring given rows: the widest net --------------------------------------------------------------------------------------
def test_score_rows_host_and_device_form(lay):
    import torch
    idx = lay.idx
    rows = np.ascontiguousarray(np.broadcast_to(np.arange(sb.N, dtype=np.int64), (B, sb.N)))
    calls, pairs = int(idx.get_option("score_calls")), int(idx.get_option("score_pairs"))
    host = idx.score_rows(lay.q, rows, lay.metric)
    d_q, d_r = torch.from_numpy(np.array(lay.q, dtype=np.float32)).cuda(), torch.from_numpy(rows).cuda()
    d_s = torch.full((B, sb.N), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.score_rows_device(d_q, B, d_r, sb.N, lay.metric, d_s, 0)
    torch.cuda.synchronize()
    assert int(idx.get_option("score_calls")) == calls + 2 and int(idx.get_option("score_pairs")) == pairs + 2 * B * sb.N
    lay.bits(host, rows, "rq_score_rows, every row")
    lay.bits(d_s.cpu().numpy(), rows, "rq_score_rows_device, every row")
    # the cancelling rows against their query under their own cap, then the planted rows alone
    cq = sb.CANCEL_QUERY
    one = sb.Ref(*(a[cq:cq + 1] for a in lay.ref))
    lay.bits(host[cq:cq + 1, sb.CANCEL_ROWS], sb.CANCEL_ROWS[None, :], "rq_score_rows, cancelling rows", ref=one, cap=sb.CAP_CANCEL)
    planted = sb.planted_rows(lay.case)
    listed = np.ascontiguousarray(np.broadcast_to(planted, (B, len(planted))))
    lay.bits(idx.score_rows(lay.q, listed, lay.metric), listed, "rq_score_rows, cancelling rows and twins")


# ---- range searches ----------------------------------------------------------------------------------------------------------
def range_device(idx, q, thr, cap, metric, flt=None):
    import torch
    nq = len(q)
    d_q = torch.from_numpy(np.array(q, dtype=np.float32)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(thr, np.float32)).cuda()
    d_s = torch.full((nq, cap), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((nq, cap), 7, dtype=torch.int64, device="cuda")
    d_c = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    d_st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_range_device(d_q, nq, d_t, cap, metric, d_s, d_r, None, d_c, d_st, 0, row_filter=flt)
    idx.search_range_fixup_device(d_q, nq, d_t, cap, metric, d_s, d_r, None, d_c, d_st, 0, row_filter=flt)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_r.cpu().numpy(), d_c.cpu().numpy(), d_st.cpu().numpy()


@pytest.mark.parametrize("route,filtered", [(SCAN, False), (EXACT, False), (GATHER, True)])
def test_range_routes(lay, route, filtered):
    idx = lay.idx
    allowed = lay.third if filtered else None
    thr, flagged = sb.range_thresholds(lay.ref, 40, allowed)             # between the 40th and the 41st score of every query
    ws, wr, wc = sb.range_want(lay.ref, thr, 64, allowed)
    assert (wc == 40).all()
    flt = idx.make_filter(allowed) if filtered else None
    idx.set_option("range_route", route)
    try:
        gs, gr, gc, st = range_device(idx, lay.q, thr, 64, lay.metric, flt)
        assert int(idx.get_option("range_route_last")) == route and not st.any()
        host = idx.search_range(lay.q, thr, 64, lay.metric, row_filter=flt)
    finally:
        idx.set_option("range_route", -1)
        if flt is not None:
            flt.close()
    assert np.array_equal(gc, wc) and np.array_equal(host[2], wc)
    for what, s, r in ((f"range route {route}, device form", gs, gr), (f"range route {route}, host form", host[0], host[1])):
        lay.rows_equal(r, wr, flagged, what)
        lay.bits(s, r, what)


def test_range_returns_the_cancelling_rows_of_a_filter_that_allows_only_them(lay):
    idx = lay.idx
    allowed = np.isin(np.arange(sb.N), sb.CANCEL_ROWS)
    thr = np.full(B, -1.0 if lay.metric == COS else -100.0, np.float32)  # below every score: all 64 rows, in the canonical order
    ws, wr, wc = sb.range_want(lay.ref, thr, 64, allowed)
    _, _, flagged = sb.canonical_topk(lay.ref, 64, allowed)
    assert (wc == 64).all()
    flt = idx.make_filter(allowed)
    idx.set_option("range_route", GATHER)
    try:
        gs, gr, gc, st = range_device(idx, lay.q, thr, 64, lay.metric, flt)
        assert int(idx.get_option("range_route_last")) == GATHER and not st.any()
    finally:
        idx.set_option("range_route", -1)
        flt.close()
    assert np.array_equal(gc, wc)
    lay.rows_equal(gr, wr, flagged, "range over the cancelling rows")
    lay.bits(gs, gr, "range over the cancelling rows")
    cq = sb.CANCEL_QUERY
    lay.bits(gs[cq:cq + 1], gr[cq:cq + 1], "range, cancelling rows against their query", ref=sb.Ref(*(a[cq:cq + 1] for a in lay.ref)), cap=sb.CAP_CANCEL)


# ---- grouped searches and group members ----------------------------------------------------------------------------------------
def grouped_device(idx, q, k, metric):
    import torch
    nq = len(q)
    d_q = torch.from_numpy(np.array(q, dtype=np.float32)).cuda()
    d_s = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    d_g = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    d_k = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    d_st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_grouped_device(d_q, nq, k, metric, d_s, d_r, d_g, d_k, d_st, 0)
    idx.search_grouped_fixup_device(d_q, nq, k, metric, d_s, d_r, d_g, d_k, d_st, 0)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_r.cpu().numpy(), d_g.cpu().numpy(), d_st.cpu().numpy()


def members_device(idx, q, k, s, metric):
    import torch
    nq = len(q)
    d_q = torch.from_numpy(np.array(q, dtype=np.float32)).cuda()
    d_s = torch.full((nq, k, s), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((nq, k, s), 7, dtype=torch.int64, device="cuda")
    d_g = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    d_c = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    d_st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_group_members_device(d_q, nq, k, s, metric, d_s, d_r, d_g, d_c, d_st, 0)
    idx.search_group_members_fixup_device(d_q, nq, k, s, metric, d_s, d_r, d_g, d_c, d_st, 0)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_r.cpu().numpy(), d_g.cpu().numpy(), d_c.cpu().numpy(), d_st.cpu().numpy()


@pytest.mark.parametrize("shared", [True, False], ids=["twins-share-a-group", "twins-in-two-groups"])
def test_grouped_and_group_members(lay, shared):
    idx = lay.idx
    groups = sb.twin_groups(lay.case, shared)
    idx.set_groups(groups)
    try:
        for s in (1, 3):
            (ws, wr, wg, wc), hi = (gmo.members_from_scores(v, groups, K, s) for v in (lay.ref.lo, lay.ref.hi))
            assert np.array_equal(wr, hi[1])                             # (no undecided pair has a say: tests/test_score_bits.py)
            calls, fills = int(idx.get_option("group_calls")), int(idx.get_option("group_fill_calls"))
            if s == 1:
                gs, gr, gg, st = grouped_device(idx, lay.q, K, lay.metric)
                what = f"grouped, twins {'share a group' if shared else 'in two groups'}"
                assert int(idx.get_option("group_calls")) > calls
                wr, wg2 = wr[:, :, 0], wg
            else:
                gs, gr, gg, gc, st = members_device(idx, lay.q, K, s, lay.metric)
                what = f"group members, twins {'share a group' if shared else 'in two groups'}"
                assert int(idx.get_option("group_fill_calls")) > fills and np.array_equal(gc, wc)
                wg2 = wg
            assert not st.any() and np.array_equal(gg, wg2), what
            lay.rows_equal(gr, wr, np.zeros(B, bool), what)
            lay.bits(gs, gr, what)
    finally:
        idx.set_groups(np.full(sb.N, nat.GROUP_NONE, np.int32))


# ---- MMR's returned relevances, the multi-device parent's key merge -----------------------------------------------------------------
def test_mmr_returns_the_relevances(lay):
    idx = lay.idx
    ws, wr, _ = sb.canonical_topk(lay.ref, K)
    _, _, flagged = sb.canonical_topk(lay.ref, 20)
    calls = int(idx.get_option("mmr_calls"))
    gs, gr = idx.search_mmr(lay.q, K, 20, 1.0, lay.metric)               # lambda 1: v is the relevance, picks follow the canonical order
    assert int(idx.get_option("mmr_calls")) == calls + 1
    lay.rows_equal(gr, wr, flagged, "MMR, lambda 1")
    lay.bits(gs, gr, "MMR relevances")


def test_multi_device_parent_keeps_the_bits_through_the_key_merge(lay):
    ws, wr, flagged = sb.canonical_topk(lay.ref, K)
    multi = new_index(lay.dim, lay.row_pad, lay.x16, devices=[0, 0])     # the same GPU named twice, stripes of 64 rows
    try:
        assert int(multi.get_option("stripe_rows")) == 64
        gs, gr = multi.search(lay.q, K, lay.metric)
    finally:
        multi.close()
    lay.rows_equal(gr, wr, flagged, "multi-device parent")
    lay.bits(gs, gr, "multi-device parent")
