"""Range searches on the MI355X (include/rq.h rq_search_range*, csrc/rq_range.hip): the count and the rows of every
call equal the oracle (tests/range_oracle.py) -- counts and rows exactly, scores within 1e-6, the SCORE_TOL of the parity tests --
on every route, form, layout and batch size; a threshold equal to a row's own score includes the row and one ulp above excludes it.

Thresholds that "about r rows clear" are midpoints of a gap of at least 4 x SCORE_TOL between neighbouring oracle scores, found within
8 ranks of r (range_oracle.threshold_for), so that a last-bit difference between the oracle's summation order and the kernels' cannot
move a row across the threshold.  For Gaussian rows at these sizes neighbouring gaps near those ranks average about 1e-4 (the
scores of 4 101 rows spread over +-0.13), so 16 consecutive gaps all below 4e-6 does not happen; the tests assert that a gap was
found for every (query, target) and leave none out."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_oracle as nfo  # noqa: E402
import range_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
MIN_GAP = 4 * SCORE_TOL
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
SCAN, GATHER, EXACT = 1, 2, 3
N_BASE = 4101                      # 65 bins, a ragged last bin
NQ = 130
BATCHES = [1, 3, 64, 70, 130]      # pad slots of a 128-query pass, more than one pass
TARGETS = [0, 1, 10, 300, 1500]    # rows that clear the threshold, about: none, one, a few, more than cap = 128, far more


class Shape:
    """One index with its rows, NQ queries, their oracle scores and thresholds per metric (computed once, shared, never changed)."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, row_offset=0, targets=TARGETS):
        self.n, self.dim, self.row_offset, self.targets = n, dim, row_offset, targets
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed)
        self.q = orc.synthetic_queries(NQ, dim, seed=seed + 1)
        self.idx = nat.NativeIndex(dim, 0)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self._full, self._thr = {}, {}

    def full(self, metric=COS):
        if metric not in self._full:
            s = nfo.scores(self.q, self.x16, metric)
            s.setflags(write=False)
            self._full[metric] = s
        return self._full[metric]

    def thresholds(self, metric=COS):
        """thr[q][t]: the threshold of query q that about targets[t] rows clear; asserts that every one was found."""
        if metric not in self._thr:
            s = self.full(metric)
            thr = np.zeros((NQ, len(self.targets)), np.float32)
            for b in range(NQ):
                srt = np.sort(s[b])[::-1]
                for t, target in enumerate(self.targets):
                    found = ro.threshold_for(srt, target, MIN_GAP)
                    assert found is not None, f"no gap of {MIN_GAP} within 8 ranks of {target} for query {b}, metric {metric}: change the seed, not the rule"
                    thr[b, t] = found[0]
            thr.setflags(write=False)
            self._thr[metric] = thr
        return self._thr[metric]

    def mixed(self, B, metric=COS, rot=0):
        """One threshold per query, the targets in turn."""
        t = self.thresholds(metric)
        return np.ascontiguousarray(t[np.arange(B), (np.arange(B) + rot) % len(self.targets)])

    def want(self, B, thr, cap, metric=COS, mask=None):
        return ro.from_scores(self.full(metric)[:B], thr, cap, self.row_offset, mask)

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def wide():
    sh = Shape()
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def narrow():
    sh = Shape(dim=384, seed=21)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def dim33():
    sh = Shape(dim=33, seed=33)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shifted():
    sh = Shape(seed=9, row_offset=10 ** 6)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def tiny():
    sh = Shape(n=70, seed=70, targets=[0, 1, 10, 30, 60])          # 2 bins, ragged
    yield sh
    sh.close()


def check(got, want, what=""):
    """Counts and rows exactly, scores within SCORE_TOL (non-finite ones bit for bit), padding (0.0, -1)."""
    (gs, gr, gc), (ws, wr, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.argwhere(gc != wc)[:4].tolist()}: {gc[gc != wc][:4]} != {wc[gc != wc][:4]}"
    nfo.assert_matches(gs, gr, ws, wr, SCORE_TOL, what)
    assert not gs[gr < 0].any()


def routed(idx, route, call):
    idx.set_option("range_route", route)
    try:
        out = call()
        return out, int(idx.get_option("range_route_last"))
    finally:
        idx.set_option("range_route", -1)


def range_device(idx, q, thr, cap, metric=COS, stream=None, row_filter=None, fixup=True, keys=False):
    """One rq_search_range_device call over host inputs (then, with fixup, the repair) -> host arrays + the status BEFORE the repair."""
    import torch
    B = q.shape[0]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        d_t = torch.from_numpy(np.broadcast_to(np.asarray(thr, np.float32), (B,)).copy()).cuda()
        sc = torch.full((B, cap), 7.0, dtype=torch.float32, device="cuda")
        rw = torch.full((B, cap), 7, dtype=torch.int64, device="cuda")
        ky = torch.full((B, cap), 7, dtype=torch.int64, device="cuda") if keys else None
        cn = torch.full((B,), 7, dtype=torch.int64, device="cuda")
        st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = stream.cuda_stream if stream is not None else 0
        idx.search_range_device(d_q, B, d_t, cap, metric, sc, rw, ky, cn, st, s, row_filter=row_filter)
        (stream or torch.cuda.current_stream()).synchronize()
        status, count0 = st.cpu().numpy().copy(), cn.cpu().numpy().copy()
        repaired = idx.search_range_fixup_device(d_q, B, d_t, cap, metric, sc, rw, ky, cn, st, s, row_filter=row_filter) if fixup else 0
        torch.cuda.synchronize()
        out = (sc.cpu().numpy(), rw.cpu().numpy(), cn.cpu().numpy())
        return out, status, count0, repaired, (ky.cpu().numpy() if keys else None), st.cpu().numpy()


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "dim33", "shifted", "tiny"])
@pytest.mark.parametrize("metric", [COS, IP])
def test_counts_rows_and_scores_equal_the_oracle(request, shape, metric):
    sh = request.getfixturevalue(shape)
    for B in BATCHES:
        for rot in (range(len(sh.targets)) if B < len(sh.targets) else (0, 3)):
            thr = sh.mixed(B, metric, rot)
            for cap in ((128, 1024) if B == 3 else (128,)):
                got = sh.idx.search_range(sh.q[:B], thr, cap, metric)
                assert int(sh.idx.get_option("range_route_last")) == SCAN
                want = sh.want(B, thr, cap, metric)
                check(got, want, f"{shape} metric {metric} B={B} rot={rot} cap={cap}")
    # (the cases really are the ones the docstring names)
    wc = sh.want(NQ, sh.mixed(NQ, metric), 128, metric)[2]
    assert (wc[0::5] == 0).all() and (np.abs(wc[1::5] - sh.targets[1]) <= 8).all() and (np.abs(wc[3::5] - sh.targets[3]) <= 8).all()
    if sh.n > 1024:
        assert (wc[3::5] > 128).all() and (wc[4::5] > 1024).all()
    one = sh.idx.search_range(sh.q[:3], float(sh.thresholds(metric)[0, 2]), 64, metric)                        # a scalar threshold
    check(one, sh.want(3, sh.thresholds(metric)[0, 2], 64, metric), f"{shape} scalar threshold")


# ---- 2. the boundary, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "shifted"])
@pytest.mark.parametrize("metric", [COS, IP])
def test_a_rows_own_score_includes_it_and_the_next_float_excludes_it(request, shape, metric):
    """thr = the score rq_score_rows returns for (query, row): the row qualifies; nextafter(thr, +inf): it does not -- on the scan
    route and, filtered, on the gather route (both re-score with csrc/rq_rowdot.h)."""
    sh = request.getfixturevalue(shape)
    B = 70
    s = sh.full(metric)[:B]
    rank = np.argsort(-s.astype(np.float64), axis=1, kind="stable")
    rows = rank[:, [0, 5, 40]]                                                    # the best row, the 6th, the 41st
    mine = sh.idx.score_rows(sh.q[:B], rows + sh.row_offset, metric)
    allowed = np.unique(np.concatenate([rows.ravel(), np.arange(0, sh.n, 97)]))
    flt = sh.idx.make_filter(allowed)
    try:
        for j in range(3):
            thr = np.ascontiguousarray(mine[:, j])
            up = np.nextafter(thr, np.float32(np.inf))
            for route, f in ((SCAN, None), (GATHER, flt)):
                (gs, gr, gc), took = routed(sh.idx, route, lambda: sh.idx.search_range(sh.q[:B], thr, 64, metric, row_filter=f))
                (_, hr, hc), _ = routed(sh.idx, route, lambda: sh.idx.search_range(sh.q[:B], up, 64, metric, row_filter=f))
                assert took == route
                for b in range(B):
                    g = rows[b, j] + sh.row_offset
                    assert g in gr[b], (shape, metric, route, b, j)
                    assert gs[b][gr[b] == g].view(np.uint32)[0] == thr[b:b + 1].view(np.uint32)[0]          # ... with exactly those bits
                    assert g not in hr[b] and hc[b] < gc[b], (shape, metric, route, b, j)
    finally:
        flt.close()


# ---- 3. routes and forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "dim33", "tiny"])
@pytest.mark.parametrize("metric", [COS, IP])
def test_routes_agree_bit_for_bit(request, shape, metric):
    sh = request.getfixturevalue(shape)
    B, cap = 70, 128
    thr = sh.mixed(B, metric, 1)
    mask = np.zeros(sh.n, bool)
    mask[np.random.default_rng(5).choice(sh.n, size=sh.n // 5, replace=False)] = True
    flt = sh.idx.make_filter(mask)
    try:
        for f, routes in ((None, (SCAN, EXACT)), (flt, (SCAN, GATHER, EXACT))):
            outs = []
            for route in routes:
                out, took = routed(sh.idx, route, lambda: sh.idx.search_range(sh.q[:B], thr, cap, metric, row_filter=f))
                assert took == route
                outs.append(out)
            check(outs[0], sh.want(B, thr, cap, metric, mask if f is not None else None), f"{shape} route {routes[0]} filtered={f is not None}")
            for route, o in zip(routes[1:], outs[1:]):
                assert np.array_equal(o[2], outs[0][2]) and np.array_equal(o[1], outs[0][1]), (shape, metric, route)
                assert np.array_equal(o[0].view(np.uint32), outs[0][0].view(np.uint32)), (shape, metric, route)
    finally:
        flt.close()


@pytest.mark.parametrize("shape", ["wide", "dim33", "shifted"])
def test_device_form_equals_the_host_form_also_on_another_stream(request, shape):
    import torch
    sh = request.getfixturevalue(shape)
    side = torch.cuda.Stream()
    for B, cap in ((1, 16), (70, 128), (130, 1024)):
        thr = sh.mixed(B, COS, 2)
        host = sh.idx.search_range(sh.q[:B], thr, cap)
        for stream in (None, side):
            dev, status, _, repaired, keys, st_after = range_device(sh.idx, sh.q[:B], thr, cap, stream=stream, keys=True)
            assert not status.any() and repaired == 0 and not st_after.any()
            for a, b in zip(dev, host):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (shape, B, cap)
            # keys: (score, global row) sortable, 0 where there is no row
            assert not keys[dev[1] < 0].any() and (keys[dev[1] >= 0] != 0).all()
            assert np.array_equal(0xffffffff - (keys[dev[1] >= 0] & 0xffffffff), dev[1][dev[1] >= 0] & 0xffffffff)
    sh.idx.stream_release(side.cuda_stream)


# ---- 4. ties, overflow ---------------------------------------------------------------------------------------------------------------
def test_duplicate_rows_at_the_threshold_all_count_and_the_cap_cuts_by_row():
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=77)
    dup = [37, 100, 2000, 2049, 4100]
    for r in dup[1:]:
        x16[r] = x16[37]
    q = orc.synthetic_queries(3, 768, seed=78)
    q[0] = x16[37].astype(np.float32)
    idx = nat.NativeIndex(768, 0)
    idx.add_f16(x16)
    for metric in (COS, IP):
        s = nfo.scores(q, x16, metric)
        t = idx.score_rows(q[:1], np.array([[37]], np.int64), metric)[0, 0]
        assert abs(float(t) - float(s[0, 37])) <= SCORE_TOL
        thr = np.array([t, s[1].max(), s[2].max()], np.float32) - np.array([0, 1e-4, 1e-4], np.float32)
        for route in (SCAN, EXACT):
            (gs, gr, gc), _ = routed(idx, route, lambda: idx.search_range(q, thr, 8, metric))
            assert gc[0] == 5 and gr[0, :5].tolist() == dup and (gr[0, 5:] == -1).all() and (gs[0, :5].view(np.uint32) == t.view(np.uint32)).all(), (metric, route)
            (gs, gr, gc), _ = routed(idx, route, lambda: idx.search_range(q, thr, 2, metric))
            assert gc[0] == 5 and gr[0].tolist() == dup[:2], (metric, route)                                  # count > cap, exactly; cut by row ascending
            check((gs, gr, gc), ro.from_scores(s, thr, 2), f"ties metric {metric} route {route}")
    idx.close()


def test_overflow_is_reported_counted_exactly_and_repaired(wide):
    sh, idx = wide, wide.idx
    B, cap = 70, 16
    thr = sh.mixed(B, COS, 0)                                                     # targets 0, 1, 10, 300, 1500 in turn
    want = sh.want(B, thr, cap)
    before = int(idx.get_option("range_repaired"))
    idx.set_option("range_cand_cap", cap)
    try:
        assert int(idx.get_option("range_cand_cap")) == cap
        dev, status, count0, repaired, _, st_after = range_device(idx, sh.q[:B], thr, cap)
        over = want[2] > cap
        assert over.sum() == 2 * B // 5 and np.array_equal(status, over.astype(np.int32))                     # status 1 exactly where the list overflowed
        assert np.array_equal(count0, want[2])                                                               # ... and the count is already exact
        assert repaired == int(over.sum()) and not st_after.any()
        check(dev, want, "overflow, repaired")
        assert int(idx.get_option("range_repaired")) == before + repaired
        check(idx.search_range(sh.q[:B], thr, cap), want, "overflow, host form")
        assert int(idx.get_option("range_repaired")) == before + 2 * repaired
        idx.set_option("range_cand_cap", 4)                                       # never below cap: cap rows still fit
        dev, status, _, _, _, _ = range_device(idx, sh.q[:B], thr, cap, fixup=False)
        assert np.array_equal(status, over.astype(np.int32))
        assert np.array_equal(dev[1][~over], want[1][~over])
    finally:
        idx.set_option("range_cand_cap", 0)
    dev, status, _, repaired, _, _ = range_device(idx, sh.q[:B], thr, cap)
    assert not status.any() and repaired == 0                                     # the default capacity holds 1 500 rows
    check(dev, want, "default capacity")


@pytest.fixture(scope="module")
def small():
    sh = Shape(n=2000, seed=57)                                                   # 32 bins, the last one ragged
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def small_narrow():
    sh = Shape(n=2000, dim=384, seed=58)
    yield sh
    sh.close()


@pytest.mark.parametrize("B,flagged", [(5, [0, 3, 4]), (70, [0, 63, 64, 69])])
@pytest.mark.parametrize("shape,metric", [("small", COS), ("small", IP), ("small_narrow", COS)])
def test_the_fixup_repairs_exactly_the_queries_flagged_by_hand(request, shape, metric, B, flagged):
    """rq_search_range_device without a fixup, then on the device: status 1 for a chosen subset and garbage over those queries' outputs
    (count included), then rq_search_range_fixup_device.  It returns the size of the subset, the flagged queries equal the oracle -- their
    counts exactly, keys made of score and row --, every other query keeps the first call's bits, every status is 0 and "range_repaired"
    rose by the size of the subset.  With and without d_keys."""
    import torch
    from rag_uq_amd import distributed as dist
    sh = request.getfixturevalue(shape)
    idx, cap = sh.idx, 16
    thr = sh.mixed(B, metric)
    want = sh.want(B, thr, cap, metric)
    d_q = torch.from_numpy(np.ascontiguousarray(sh.q[:B], np.float32)).cuda()
    d_t = torch.from_numpy(thr).cuda()
    for with_keys in (True, False):
        what = f"by hand: {shape}, metric {metric}, B {B}, keys {with_keys}"
        sc = torch.full((B, cap), 7.0, dtype=torch.float32, device="cuda")
        rw = torch.full((B, cap), 7, dtype=torch.int64, device="cuda")
        ky = torch.full((B, cap), 7, dtype=torch.int64, device="cuda") if with_keys else None
        cn = torch.full((B,), 7, dtype=torch.int64, device="cuda")
        st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        bufs = (sc, rw, cn, st) + ((ky,) if with_keys else ())
        idx.search_range_device(d_q, B, d_t, cap, metric, sc, rw, ky, cn, st, 0)
        torch.cuda.synchronize()
        first = [t.cpu().numpy().copy() for t in bufs]
        assert not first[3].any(), f"{what}: the first call flagged {np.nonzero(first[3])[0].tolist()} itself"
        sel = torch.tensor(flagged, device="cuda")
        st[sel] = 1
        sc[sel] = float("nan")
        rw[sel] = -7
        cn[sel] = -1
        if with_keys:
            ky[sel] = -1                                                          # all ones
        before = int(idx.get_option("range_repaired"))
        n = idx.search_range_fixup_device(d_q, B, d_t, cap, metric, sc, rw, ky, cn, st, 0)
        torch.cuda.synchronize()
        after = [t.cpu().numpy() for t in bufs]
        assert n == len(flagged), f"{what}: the fixup returned {n}"
        assert not after[3].any(), f"{what}: status after the fixup {after[3].tolist()}"
        check([a[flagged] for a in after[:3]], [w[flagged] for w in want], f"{what}, flagged queries")
        if with_keys:
            assert np.array_equal(after[4].view(np.uint64)[flagged], dist.pack_keys(after[0][flagged].reshape(-1), after[1][flagged].reshape(-1)).reshape(-1, cap)), \
                f"{what}: keys of the flagged queries"
        other = np.setdiff1d(np.arange(B), flagged)
        for a, b in zip(first, after):
            assert np.array_equal(a[other].view(np.uint8), b[other].view(np.uint8)), f"{what}: an unflagged query changed"
        assert int(idx.get_option("range_repaired")) == before + len(flagged), what


# ---- 5. filters ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "shifted"])
def test_filtered_calls_equal_the_oracle(request, shape):
    sh = request.getfixturevalue(shape)
    rng = np.random.default_rng(11)
    sparse = np.zeros(sh.n, bool)
    sparse[rng.choice(sh.n, size=30, replace=False)] = True
    dense = rng.random(sh.n) < 0.9
    last = np.zeros(sh.n, bool)
    last[sh.n - 3:] = True                                                        # only rows of the ragged last bin
    for name, mask, rule in (("sparse", sparse, GATHER), ("dense", dense, SCAN), ("last", last, GATHER), ("empty", np.zeros(sh.n, bool), 0)):
        flt = sh.idx.make_filter(mask)
        try:
            for metric in (COS, IP):
                for B in (3, 70):
                    thr = sh.mixed(B, metric, 2)
                    thr[0] = -3.0e38                                              # every allowed row with a finite score
                    got = sh.idx.search_range(sh.q[:B], thr, 128, metric, row_filter=flt)
                    assert int(sh.idx.get_option("range_route_last")) == rule, (name, B)
                    check(got, sh.want(B, thr, 128, metric, mask), f"{shape} filter {name} metric {metric} B={B}")
                    assert got[2][0] == mask.sum()
                    if rule:
                        for route in (SCAN, GATHER, EXACT):
                            out, took = routed(sh.idx, route, lambda: sh.idx.search_range(sh.q[:B], thr, 128, metric, row_filter=flt))
                            assert took == route
                            check(out, sh.want(B, thr, 128, metric, mask), f"{shape} filter {name} metric {metric} B={B} route {route}")
            dev, status, _, _, _, _ = range_device(sh.idx, sh.q[:3], sh.mixed(3, COS, 2), 16, row_filter=flt)
            check(dev, sh.want(3, sh.mixed(3, COS, 2), 16, COS, mask), f"{shape} filter {name}, device form")
        finally:
            flt.close()


def test_stale_and_foreign_filters_are_refused():
    x16 = orc.synthetic_corpus(300, 768, seed=6)
    q = orc.synthetic_queries(2, 768, seed=7)
    a, b = nat.NativeIndex(768, 0), nat.NativeIndex(768, 0)
    a.add_f16(x16[:200])
    b.add_f16(x16[:200])
    fa = a.make_filter(np.arange(0, 200, 2))
    assert a.search_range(q, -1.0, 4, row_filter=fa)[2].tolist() == [100, 100]
    with pytest.raises(nat.RqError, match="another index"):
        b.search_range(q, -1.0, 4, row_filter=fa)
    a.add_f16(x16[200:])
    with pytest.raises(nat.RqError, match="stale filter"):
        a.search_range(q, -1.0, 4, row_filter=fa)
    with pytest.raises(nat.RqError, match="stale filter"):
        a.search_range_device(8, 2, 16, 4, COS, 24, 32, None, 40, 48, row_filter=fa)
    assert a.search_range(q, -1.0, 4)[2].tolist() == [300, 300]
    fa.close()
    a.close()
    b.close()


# ---- 6. non-finite and extreme values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 384])
def test_non_finite_and_extreme_values_follow_the_rules(dim):
    q = nfo.queries(dim)
    shards = {"A": nfo.shard_a(dim, q), "C70": nfo.shard_c(dim, q)[:70]}
    shards["A"][3000] = 0                                                         # an all-zero row
    for name, x16 in shards.items():
        idx = nat.NativeIndex(dim, 0)
        idx.add_f16(x16)
        mask = np.arange(x16.shape[0]) % 3 != 1
        flt = idx.make_filter(mask)
        for metric in (COS, IP):
            s = nfo.scores(q, x16, metric)
            B = q.shape[0]
            assert not s[5].any() and np.isneginf(s[1]).all()                     # the zero-norm query, the NaN query
            if name == "A" and metric == IP:
                assert np.isposinf(s[:, 5]).any()                                 # inner product with a +inf score
            thr10 = np.zeros(B, np.float32)
            for b in range(B):
                fin = np.sort(s[b][np.isfinite(s[b])])[::-1]
                found = ro.threshold_for(fin, 10, MIN_GAP) if fin.size > 20 and fin[0] > fin[-1] else None
                thr10[b] = found[0] if found is not None else np.float32(0.0)
            thr10[5] = 0.0                                                        # the zero-norm query at thr <= 0: every row
            pos = thr10.copy()
            pos[5] = np.float32(1e-38)                                            # ... and at thr > 0: none
            low = np.full(B, -3.0e38, np.float32)                                 # everything but -inf
            for tname, thr in (("thr10", thr10), ("pos", pos), ("low", low)):
                for f, m in ((None, None), (flt, mask)):
                    for route in (SCAN, EXACT):
                        got, _ = routed(idx, route, lambda: idx.search_range(q, thr, 64, metric, row_filter=f))
                        check(got, ro.from_scores(s, thr, 64, mask=m), f"non-finite {name} dim {dim} metric {metric} {tname} filtered={f is not None} route {route}")
            assert idx.search_range(q, thr10, 64, metric)[2][5] == x16.shape[0] and idx.search_range(q, pos, 64, metric)[2][5] == 0
            # the device form: NaN / inf queries come back with status 1 and are repaired; a non-finite threshold returns nothing
            bad_thr = thr10.copy()
            bad_thr[[0, 6, 9]] = [np.nan, np.inf, -np.inf]
            dev, status, _, repaired, _, st_after = range_device(idx, q, bad_thr, 64, metric)
            nonfinite_q = ~np.isfinite(q.astype(np.float64) @ np.ones(dim))
            assert np.array_equal(status != 0, nonfinite_q) and repaired == int(nonfinite_q.sum()) and not st_after.any()
            check(dev, ro.from_scores(s, bad_thr, 64), f"non-finite {name} dim {dim} metric {metric}, device form")
            assert not dev[2][[0, 6, 9]].any() and (dev[1][[0, 6, 9]] == -1).all()
        flt.close()
        idx.close()


# ---- 7. deferred work, counters, refusals ---------------------------------------------------------------------------------------------------
def test_a_range_call_completes_what_the_stream_deferred(wide):
    """pipeline = 2: a fused search leaves its tail pending on the stream; the range call behind it completes it first, so that
    search's outputs are complete in stream order -- no flush -- and equal the oracle."""
    import torch
    idx = wide.idx
    B, k, cap = 64, 10, 32
    d_q = torch.from_numpy(wide.q[:B]).cuda()
    sc = torch.full((B, k), 7.0, device="cuda")
    rw = torch.full((B, k), 7, device="cuda", dtype=torch.int64)
    st = torch.full((B,), 7, device="cuda", dtype=torch.int32)
    thr = wide.mixed(B, COS, 1)
    d_t = torch.from_numpy(thr).cuda()
    rs = torch.full((B, cap), 7.0, device="cuda")
    rr = torch.full((B, cap), 7, device="cuda", dtype=torch.int64)
    rc = torch.full((B,), 7, device="cuda", dtype=torch.int64)
    rst = torch.full((B,), 7, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    idx.set_option("pipeline", 2)
    idx.set_option("scan8", 0)
    try:
        idx.search_device(d_q, B, k, COS, sc, rw, None, st, 0)
        idx.search_range_device(d_q, B, d_t, cap, COS, rs, rr, None, rc, rst, 0)
        torch.cuda.synchronize()
        got_s, got_r, got_st = sc.cpu().numpy(), rw.cpu().numpy(), st.cpu().numpy()
        idx.search_flush_device(0)
        torch.cuda.synchronize()
        assert np.array_equal(rw.cpu().numpy(), got_r) and np.array_equal(sc.cpu().numpy(), got_s)          # nothing was left to flush
    finally:
        idx.set_option("pipeline", 0)
        idx.set_option("scan8", 1)
    assert not got_st.any() and not rst.cpu().numpy().any()
    ws, wr = orc.topk_from_scores(wide.full(COS)[:B], k)
    assert np.array_equal(got_r, wr) and float(np.abs(got_s - ws).max()) <= SCORE_TOL
    check((rs.cpu().numpy(), rr.cpu().numpy(), rc.cpu().numpy()), wide.want(B, thr, cap), "behind a deferred tail")


def test_counters_count_and_bad_arguments_are_refused_by_the_library():
    x16 = orc.synthetic_corpus(130, 100, seed=3)
    q = orc.synthetic_queries(3, 100, seed=4)
    idx = nat.NativeIndex(100, 0)
    assert idx.search_range(q, -1.0, 4)[2].tolist() == [0, 0, 0] and int(idx.get_option("range_route_last")) == 0       # an empty index: padding
    assert (idx.search_range(q, -1.0, 4)[1] == -1).all() and int(idx.get_option("range_bins_last")) == -1
    idx.add_f16(x16)
    t0 = idx.timing()
    assert int(idx.get_option("range_calls")) == 2 and int(idx.get_option("range_route")) == -1
    check(idx.search_range(q, 0.0, 8), ro.search_range(q, x16, 0.0, 8), "130 x 100")
    dev, status, _, _, _, _ = range_device(idx, q, 0.0, 8)
    assert int(idx.get_option("range_calls")) == 4 and int(idx.get_option("range_route_last")) == SCAN
    t1 = idx.timing()
    assert (t1["searches"], t1["queries"]) == (t0["searches"] + 2, t0["queries"] + 6)                                    # rq_timing counts it as a search
    out_s, out_r, out_c, st = np.zeros(12, np.float32), np.zeros(12, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int32)
    thr = np.zeros(3, np.float32)
    p = nat._ptr
    for B, cap, metric in ((3, 4, 5), (0, 4, 0), (3, 0, 0), (3, nat.MAX_K + 1, 0), (65536, 4, 0)):                        # the library's own checks: RQ_EINVAL
        assert idx._lib.rq_search_range(idx._h, None, p(q), B, p(thr), cap, metric, p(out_s), p(out_r), p(out_c)) == -1
        assert idx._lib.rq_search_range_device(idx._h, None, p(q), B, p(thr), cap, metric, p(out_s), p(out_r), None, p(out_c), p(st), None) == -1
        assert idx._lib.rq_search_range_fixup_device(idx._h, None, p(q), B, p(thr), cap, metric, p(out_s), p(out_r), None, p(out_c), p(st), None) == -1
    assert idx._lib.rq_search_range(idx._h, None, p(q), 3, None, 4, 0, p(out_s), p(out_r), p(out_c)) == -1 and "null" in nat.last_error()
    assert idx._lib.rq_search_range_device(idx._h, None, p(q), 3, p(thr), 4, 0, p(out_s), p(out_r), None, p(out_c), None, None) == -1 and "d_status" in nat.last_error()
    thr[1] = np.inf
    assert idx._lib.rq_search_range(idx._h, None, p(q), 3, p(thr), 4, 0, p(out_s), p(out_r), p(out_c)) == -1 and "finite" in nat.last_error()
    assert int(idx.get_option("range_calls")) == 4                                                                        # a refused call counts nothing
    for bad in (0, 4, -2):
        with pytest.raises(nat.RqError):
            idx.set_option("range_route", bad)
    idx.close()


def test_a_multi_device_index_is_refused():
    x16 = orc.synthetic_corpus(300, 768, seed=6)
    multi = nat.NativeIndex(768, devices=[0, 0])
    multi.add_f16(x16)
    q = orc.synthetic_queries(2, 768, seed=7)
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_range(q, 0.5, 3)
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_range_device(8, 2, 16, 3, COS, 24, 32, None, 40, 48)          # (refused before a pointer is looked at)
    multi.close()


# ---- 8. the scan route skips --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow"])
def test_the_scan_route_rescores_fewer_bins_than_the_shard_has(request, shape):
    sh = request.getfixturevalue(shape)
    B, nbins = 64, (sh.n + 63) // 64
    for metric in (COS, IP):
        thr = np.ascontiguousarray(sh.thresholds(metric)[:B, 1])                  # one row clears it, about
        (gs, gr, gc), took = routed(sh.idx, SCAN, lambda: sh.idx.search_range(sh.q[:B], thr, 16, metric))
        check((gs, gr, gc), sh.want(B, thr, 16, metric), f"{shape} one row clears")
        bins = int(sh.idx.get_option("range_bins_last"))
        print(f"{shape} metric {metric}: {bins} of {B * nbins} (query, bin) pairs re-scored, {int(gc.sum())} rows qualified")
        assert took == SCAN and int(gc.sum()) >= 1 and 1 <= bins < B * nbins
        low = np.full(B, -3.0e38, np.float32)                                     # every bin clears it: the whole shard is re-scored
        routed(sh.idx, SCAN, lambda: sh.idx.search_range(sh.q[:B], low, 16, metric))
        assert int(sh.idx.get_option("range_bins_last")) == B * nbins
        routed(sh.idx, EXACT, lambda: sh.idx.search_range(sh.q[:B], thr, 16, metric))
        assert int(sh.idx.get_option("range_bins_last")) == -1                    # (not the scan route)
