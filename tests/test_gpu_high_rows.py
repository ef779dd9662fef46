"""Global rows with bit 31 set through every route (MI355X).  Keys carry the global row in 32 bits and rq_index_set_row_offset accepts
any offset with row_offset + rows < 2^32 - 1, yet the suite's largest offset was 5 000 000: a signed 32-bit slip in any of the casts
between a key's row field and the int64 rows a caller sees would have gone unnoticed.  One 4 101-row index (Gaussian rows, dim 768,
groups of eight consecutive rows, the 40 best rows of query 0 in a group of their own) is re-offset to
  2^31 - 2050        the shard straddles the boundary: rows below and above 2^31 in one answer;
  2^32 - 2 - 4101    the largest offset accepted: the last row is 2^32 - 3;
and at each offset one call of every route is compared with the oracles of the other test files given the same row_offset: rows
exactly, scores within SCORE_TOL (times the largest |score| under the inner product, the bar of tests/test_gpu_parity.py), keys
exactly.  The host side of the key codec is tests/test_high_rows.py."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat
from rag_uq_amd import distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import group_members_oracle as gmo  # noqa: E402
import group_oracle as gro  # noqa: E402
import mmr_oracle as mmo  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402
import range_oracle as ro  # noqa: E402
import score_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
METRICS = [COS, IP]
N, B, K = 4101, 16, 10
ZERO_Q = B - 1                                        # the last query is zero: every score ties, rows come out in row order
STRADDLE = 2 ** 31 - 2050
LARGEST = 2 ** 32 - 2 - N
OFFSETS = [STRADDLE, LARGEST]
EUNSUPPORTED = -6


class World:
    def __init__(self):
        self.x16 = orc.synthetic_corpus(N, 768, seed=3131)
        self.q = orc.synthetic_queries(B, 768, seed=3132)
        self.q[ZERO_Q] = 0.0
        self.idx = nat.NativeIndex(768, 0)
        self.idx.set_option("scan8", 0)
        self.idx.add_f16(self.x16)
        self.s = {m: nfo.scores(self.q, self.x16, m) for m in METRICS}
        self.groups = np.arange(N, dtype=np.int64) // 8
        self.groups[orc.topk_from_scores(self.s[COS][:1], 40)[1][0]] = 9999      # query 0: a first list of 16 rows holds one group
        self.idx.set_groups(self.groups)
        self.mask = np.random.default_rng(5).random(N) < 0.5
        for a in (self.x16, self.q, self.groups, self.mask, *self.s.values()):
            a.setflags(write=False)

    def tol(self, metric):
        return SCORE_TOL * max(1.0, float(np.abs(self.s[metric]).max()))

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def _same(got_s, got_r, want_s, want_r, tol, what):
    assert got_r.dtype == np.int64 and np.array_equal(got_r, want_r), f"{what}: rows differ at {np.argwhere(got_r != want_r)[:4].tolist()}: {got_r.ravel()[:3].tolist()} against {want_r.ravel()[:3].tolist()}"
    err = float(np.abs(got_s.astype(np.float64) - want_s.astype(np.float64)).max(initial=0.0))
    assert err <= tol, f"{what}: scores differ by {err}"


def _high(rows, off):
    """The answer holds rows with bit 31 set -- and, on the straddling shard, rows without."""
    live = rows[rows >= 0]
    assert (live >= off).all() and (live < off + N).all() and (live >= 2 ** 31).any()
    if off == STRADDLE:
        assert (live < 2 ** 31).any()


@pytest.mark.parametrize("off", OFFSETS, ids=["straddle", "largest"])
def test_search_keys_and_their_merge(world, off):
    import torch
    idx, q = world.idx, world.q
    idx.set_row_offset(off)
    dq = torch.from_numpy(np.array(q, order="C")).cuda()
    for metric in METRICS:
        what = f"offset {off} metric {metric}"
        want20 = orc.topk_from_scores(world.s[metric], 20, off)
        want = (want20[0][:, :K], want20[1][:, :K])
        _high(want[1], off)
        _same(*idx.search(q, K, metric), *want, world.tol(metric), f"search {what}")
        sc = torch.full((B, 20), -7.0, device="cuda"); rw = torch.full((B, 20), -7, device="cuda", dtype=torch.int64)
        ky = torch.zeros((B, 20), device="cuda", dtype=torch.int64); st = torch.full((B,), 9, device="cuda", dtype=torch.int32)
        torch.cuda.synchronize()
        idx.search_device(dq, B, 20, metric, sc, rw, ky, st)
        idx.search_fixup_device(dq, B, 20, metric, sc, rw, ky, st)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        gs, gr, gk = sc.cpu().numpy(), rw.cpu().numpy(), ky.cpu().numpy().view(np.uint64)
        _same(gs, gr, *want20, world.tol(metric), f"search_device {what}")
        assert np.array_equal(gk, dist.pack_keys(gs, gr)), f"{what}: the device's keys are not the host codec's"
        us, ur = dist.unpack_keys(gk)
        assert np.array_equal(ur, gr) and np.array_equal(us.view(np.uint32), gs.view(np.uint32)), f"{what}: unpack_keys"
        # the keys as two halves of ten, the worse half first: merged on the device and on the host
        halves = torch.cat([ky[:, K:], ky[:, :K]], dim=1).contiguous()
        ms = torch.empty((B, K), device="cuda"); mr = torch.empty((B, K), device="cuda", dtype=torch.int64)
        mk = torch.zeros((B, K), device="cuda", dtype=torch.int64)
        nat.merge_keys_device(halves, 20, B, K, ms, mr, mk)
        torch.cuda.synchronize()
        assert np.array_equal(mr.cpu().numpy(), gr[:, :K]) and np.array_equal(ms.cpu().numpy().view(np.uint32), gs[:, :K].view(np.uint32)), f"{what}: merge_keys_device"
        assert np.array_equal(mk.cpu().numpy().view(np.uint64), gk[:, :K]), f"{what}: merged keys"
        hs, hr = dist.merge_keys_host(halves.cpu().numpy().view(np.uint64), K)
        assert np.array_equal(hr, gr[:, :K]) and np.array_equal(hs.view(np.uint32), gs[:, :K].view(np.uint32)), f"{what}: merge_keys_host"
        assert gr[ZERO_Q].tolist() == list(range(off, off + 20))


@pytest.mark.parametrize("off", OFFSETS, ids=["straddle", "largest"])
def test_filtered_range_scored_and_diversified(world, off):
    idx, q = world.idx, world.q
    idx.set_row_offset(off)
    flt = idx.make_filter(world.mask)
    try:
        for metric in METRICS:
            what = f"offset {off} metric {metric}"
            s_all, tol = world.s[metric], world.tol(metric)
            want = fo.filtered_topk_from_scores(s_all, world.mask, K, off)
            _high(want[1], off)
            for route in (1, 2):
                idx.set_option("filter_route", route)
                _same(*idx.search(q, K, metric, row_filter=flt), *want, tol, f"filter route {route} {what}")
                assert int(idx.get_option("filter_route_last")) == route
            idx.set_option("filter_route", -1)
            # a threshold per query in a gap of the ranking near rank 20 (the zero query: every row clears -1)
            thr = np.full(B, -1.0, np.float32)
            for b in range(B - 1):
                t = ro.threshold_for(np.sort(s_all[b])[::-1], 20, 1e-5 * max(1.0, tol / SCORE_TOL))
                assert t is not None
                thr[b] = t[0]
            ws, wr, wc = ro.from_scores(s_all, thr, 32, off)
            gs, gr, gc = idx.search_range(q, thr, 32, metric)
            assert np.array_equal(gc, wc) and wc[ZERO_Q] == N and 12 <= wc[:B - 1].min() and wc[:B - 1].max() <= 28, f"range counts {what}"
            _same(gs, gr, ws, wr, tol, f"range {what}")
            _high(gr, off)
            # score_rows over the search's own rows, one entry just below the shard and one at 2^40: absent, 0.0
            top_s, top_r = idx.search(q, K, metric)
            rows = np.concatenate([top_r, np.full((B, 1), off - 1), np.full((B, 1), 2 ** 40), np.full((B, 1), off + N), np.full((B, 1), off + N - 1)], axis=1)
            got = idx.score_rows(q, rows, metric)
            assert np.array_equal(got[:, :K].view(np.uint32), top_s.view(np.uint32)), f"score_rows {what}: not the search's bits"
            assert not got[:, K:K + 3].view(np.uint32).any(), f"score_rows {what}: an absent entry scored"
            _same(got, rows, so.pairs(q, world.x16, rows, metric, off, s_all), rows, tol, f"score_rows {what}")
            if off == LARGEST:
                assert rows[0, -1] == 2 ** 32 - 3
            # MMR (the zero query aside: its candidates all tie)
            with np.errstate(all="ignore"):
                ms, mr, mv = mmo.mmr_topk(q[:8], world.x16, 5, 20, 0.5, metric, None, off)
            gs, gr, gv = idx.search_mmr(q[:8], 5, 20, 0.5, metric, return_mmr=True)
            _same(gs, gr, ms, mr, tol, f"mmr {what}")
            assert float(np.abs(gv.astype(np.float64) - mv).max()) <= tol, f"mmr values {what}"
            _high(gr, off)
    finally:
        idx.set_option("filter_route", -1)
        flt.close()


@pytest.mark.parametrize("off", OFFSETS, ids=["straddle", "largest"])
def test_grouped_and_group_members(world, off):
    idx, q = world.idx, world.q
    idx.set_row_offset(off)
    try:
        for metric in METRICS:
            what = f"offset {off} metric {metric}"
            s_all, tol = world.s[metric], world.tol(metric)
            ws, wr, wg = gro.grouped_from_scores(s_all, world.groups, K, None, off)
            _high(wr, off)
            assert wr[ZERO_Q, 0] == off and (np.diff(wr[ZERO_Q]) > 0).all() and wr[ZERO_Q, -1] < off + 8 * (K + 1)      # the zero query: the first groups, in row order
            for cap in (0, 16):                                               # 16: rung 2 holds 16 rows, the exclusion loop subtracts the offset from its winners
                idx.set_option("group_fetch_cap", cap)
                gs, gr, gg = idx.search_grouped(q, K, metric)
                _same(gs, gr, ws, wr, tol, f"grouped cap {cap} {what}")
                assert np.array_equal(gg, wg), f"grouped cap {cap} {what}: group ids"
                if cap == 16:
                    assert int(idx.get_option("group_rounds_last")) >= 1, f"{what}: the exclusion loop did not run"
                    if metric == COS:
                        assert gg[0, 0] == 9999
                ms, mr, mg, mc = idx.search_group_members(q, K, 3, metric)
                xs, xr, xg, xc = gmo.members_from_scores(s_all, world.groups, K, 3, None, off)
                _same(ms.reshape(B, -1), mr.reshape(B, -1), xs.reshape(B, -1), xr.reshape(B, -1), tol, f"members cap {cap} {what}")
                assert np.array_equal(mg, xg) and np.array_equal(mc, xc), f"members cap {cap} {what}: ids or counts"
                assert np.array_equal(idx.score_rows(q, mr.reshape(B, -1), metric).view(np.uint32), ms.reshape(B, -1).view(np.uint32)), f"members cap {cap} {what}: score_rows bits"
    finally:
        idx.set_option("group_fetch_cap", 0)


def test_refusals_leave_the_index_unchanged(world):
    idx, q = world.idx, world.q
    lib = nat.load_library()
    idx.set_row_offset(STRADDLE)
    before = idx.search(q, K)
    assert lib.rq_index_set_row_offset(idx._h, 2 ** 32 - 1 - N) == EUNSUPPORTED and "2^32-1" in nat.last_error()
    with pytest.raises(nat.RqError):
        idx.set_row_offset(2 ** 32 - 1 - N)
    with pytest.raises(nat.RqError):
        idx.set_row_offset(2 ** 33)
    after = idx.search(q, K)
    assert np.array_equal(after[1], before[1]) and after[0].tobytes() == before[0].tobytes() and after[1].min() >= STRADDLE
    idx.set_row_offset(LARGEST)
    before = idx.search(q, K)
    one = np.ascontiguousarray(world.x16[:1]).view(np.uint16)
    assert lib.rq_index_add_f16(idx._h, nat._ptr(one), 1) == EUNSUPPORTED
    with pytest.raises(nat.RqError):
        idx.add_f16(world.x16[:1])
    with pytest.raises(nat.RqError):
        idx.add_f32(world.x16[:1].astype(np.float32))
    assert len(idx) == N
    after = idx.search(q, K)
    assert np.array_equal(after[1], before[1]) and after[0].tobytes() == before[0].tobytes() and after[1].max() <= 2 ** 32 - 3
    assert after[1][ZERO_Q].tolist() == list(range(LARGEST, LARGEST + K))
