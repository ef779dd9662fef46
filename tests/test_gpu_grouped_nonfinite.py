"""Non-finite and extreme values through the grouped and group-member calls (MI355X): rq_search_grouped*, rq_group_collapse_device,
rq_search_group_members*, rq_group_fill_device against tests/group_oracle.py and tests/group_members_oracle.py run over
tests/nonfinite_oracle.py's score matrices -- include/rq.h's rules (a NaN score counts as -inf, a zero-norm query scores every row
0.0, +-inf scores order like any other, a -inf row is still a row, -0.0 leaves as +0.0) for the two newest routes.

The world is tests/test_gpu_nonfinite.py's shard A (4 101 rows: row 5 one +inf element, rows 64..127 all NaN, row 200 +inf and -inf,
row 300 all 65 504, rows 1000..1009 zero, row 2049 NaN, row 2050 the direction of query 0, row 4099 the direction of query 6, row
4100 one -inf element) at dim 768 and at dim 384 (the narrow layout), and 70 queries: 0 and 6 planted matches, 1 all NaN, 2 one +inf
element, 3 fp32-subnormal, 4 x 1e36, 5 zero, 7 one -inf element, and the same eight again at positions 62..69, the ragged second pass.

Everything is compared as nfo.assert_matches compares: rows, group ids and counts exactly, non-finite scores bit for bit, finite
scores within SCORE_TOL, no -0.0; padding is (0.0, -1, GROUP_NONE, count 0).

Which rung answers: at 65 bins a first rung of m1 = 8 x 10 = 80 rows re-scores every bin (2 x 90 >= 65: csrc/rq_plan.h), which proves
every query, a NaN query included; a first rung of m1 <= 20 rows takes the approximate pass, which never certifies a non-finite
query.  The device-form test therefore runs "group_fetch" at its default and at 2, and the rung test at 1 with "group_fetch_cap"
16 and 64."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native as nat
from rag_uq_amd import distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_members_oracle as gmo  # noqa: E402
import group_oracle as gro  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
METRICS = [COS, IP]
NONE = nat.GROUP_NONE
N = nfo.N_A
B, K = 70, 10
DIMS = [768, 384]                                    # (dim, row_pad) = (768, 768) and (384, 384)
PATTERNS = ["runs8", "sparse", "mixed", "one", "bad_groups"]
NAN_Q, INF_Q, TINY_Q, HUGE_Q, ZERO_Q, NEG_INF_Q = 1, 2, 3, 4, 5, 7
AGAIN = 62                                           # q[62:70] = q[:8]
NONFINITE_AT = [p + o for o in (0, AGAIN) for p in (NAN_Q, INF_Q, NEG_INF_Q)]


def group_patterns():
    row = np.arange(N, dtype=np.int64)
    mixed = row // 8
    mixed[::3] = NONE
    bad = np.full(N, NONE, np.int64)
    bad[nfo.NAN_BIN[0]:nfo.NAN_BIN[1]] = 5           # a group whose every row scores -inf
    bad[1000:1010] = 6                               # the zero rows
    return {"runs8": row // 8, "sparse": (row // 8) * 1000 + 7, "mixed": mixed, "one": np.zeros(N, np.int64), "bad_groups": bad}


def row_masks():
    row = np.arange(N)
    holes = np.ones(N, bool)
    holes[2050] = False                              # the planted match of query 0
    holes[nfo.NAN_BIN[0]:nfo.NAN_BIN[1]:2] = False   # half of the NaN bin
    return {"mod3": row % 3 != 1, "holes": holes}


def first_group_rows(groups, k, mask=None):
    """The lowest row in play of each of the first k groups in row order (what an all-tie query returns), -1 padded."""
    seen, out = set(), []
    for r in range(N):
        if mask is not None and not mask[r]:
            continue
        g = int(groups[r])
        if g >= 0:
            if g in seen:
                continue
            seen.add(g)
        out.append(r)
        if len(out) == k:
            break
    return out + [-1] * (k - len(out))


class World:
    """Queries, shard A and one index per dim, the score matrices and the oracle's answers, each made once and left unchanged."""

    def __init__(self):
        self._q, self._x, self._idx, self._s, self._want = {}, {}, {}, {}, {}
        self.groups = group_patterns()
        self.masks = row_masks()
        for a in list(self.groups.values()) + list(self.masks.values()):
            a.setflags(write=False)

    def q(self, dim):
        if dim not in self._q:
            q = nfo.queries(dim, B)
            q[AGAIN:AGAIN + 8] = q[:8]
            q.setflags(write=False)
            self._q[dim] = q
        return self._q[dim]

    def x(self, dim):
        if dim not in self._x:
            x = nfo.shard_a(dim, self.q(dim))
            x.setflags(write=False)
            self._x[dim] = x
        return self._x[dim]

    def idx(self, dim):
        if dim not in self._idx:
            idx = nat.NativeIndex(dim, 0)
            assert idx.row_pad == dim
            idx.add_f16(self.x(dim)[:2000]); idx.add_f16(self.x(dim)[2000:])
            self._idx[dim] = idx
        return self._idx[dim]

    def scores(self, dim, metric):
        if (dim, metric) not in self._s:
            s = nfo.scores(self.q(dim), self.x(dim), metric)
            assert not np.isnan(s).any()
            s.setflags(write=False)
            self._s[(dim, metric)] = s
        return self._s[(dim, metric)]

    def grouped(self, dim, metric, pattern, mask=None, k=K):
        key = ("g", dim, metric, pattern, mask, k)
        if key not in self._want:
            self._want[key] = gro.grouped_from_scores(self.scores(dim, metric), self.groups[pattern], k, None if mask is None else self.masks[mask])
        return self._want[key]

    def members(self, dim, metric, pattern, s, mask=None, k=K):
        key = ("m", dim, metric, pattern, mask, k, s)
        if key not in self._want:
            self._want[key] = gmo.members_from_scores(self.scores(dim, metric), self.groups[pattern], k, s, None if mask is None else self.masks[mask])
        return self._want[key]

    def close(self):
        for i in self._idx.values():
            i.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def same_grouped(got, want, what):
    gs, gr, gg = got[:3]
    ws, wr, wg = want
    nfo.assert_matches(gs, gr, ws, wr, SCORE_TOL, what)
    assert np.array_equal(gg, wg), f"{what}: group ids differ at {np.argwhere(gg != wg)[:4].tolist()}"
    pad = wr < 0
    assert not gs[pad].view(np.uint32).any() and (gg[pad] == NONE).all(), f"{what}: padding is not (0.0, -1, GROUP_NONE)"


def same_members(got, want, what):
    gs, gr, gg, gc = got[:4]
    ws, wr, wg, wc = want
    b, k, s = wr.shape
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.argwhere(gc != wc)[:4].tolist()}"
    assert np.array_equal(gg, wg), f"{what}: group ids differ at {np.argwhere(gg != wg)[:4].tolist()}"
    nfo.assert_matches(gs.reshape(b, k * s), gr.reshape(b, k * s), ws.reshape(b, k * s), wr.reshape(b, k * s), SCORE_TOL, what)
    pad = wr < 0
    assert not gs[pad].view(np.uint32).any(), f"{what}: a score beyond a slot's count is not 0.0"
    assert (gg[wc == 0] == NONE).all(), f"{what}: a slot beyond k_eff carries a group id"


def test_the_world_holds_the_cases_it_is_meant_to_hold(world):
    """On the oracle alone (no device): what the cases below rely on."""
    w = world
    g8 = w.groups["runs8"]
    for dim in DIMS:
        cos, ip = w.scores(dim, COS), w.scores(dim, IP)
        for s_all in (cos, ip):
            for at in (0, AGAIN):
                assert np.isneginf(s_all[NAN_Q + at]).all() and not s_all[ZERO_Q + at].any()
        assert np.isneginf(cos[INF_Q]).all() and np.isneginf(cos[NEG_INF_Q]).all()           # an infinite norm: every cosine is NaN
        assert np.isposinf(ip[INF_Q]).sum() > 1000 and np.isneginf(ip[INF_Q]).sum() > 1000
        assert np.isfinite(cos[TINY_Q]).sum() > 4000 and np.abs(ip[HUGE_Q][np.isfinite(ip[HUGE_Q])]).max() > 1e34
        ws, wr, wg, wc = w.members(dim, COS, "runs8", 8)
        assert wg[0, 0] == 2050 // 8 and wr[0, 0].tolist() == [2050] + [r for r in wr[0, 0, 1:7].tolist()] + [2049] and wc[0, 0] == 8
        assert sorted(wr[0, 0].tolist()) == list(range(2048, 2056)) and np.isneginf(ws[0, 0, 7]) and np.isfinite(ws[0, 0, :7]).all()
        for metric in METRICS:
            for pattern in PATTERNS:
                groups = w.groups[pattern]
                ws, wr, wg = w.grouped(dim, metric, pattern)
                first = first_group_rows(groups, K)
                for at in (0, AGAIN):
                    assert wr[NAN_Q + at].tolist() == first and wr[ZERO_Q + at].tolist() == first, (pattern, metric)
                    have = np.array(first) >= 0
                    assert np.isneginf(ws[NAN_Q + at][have]).all() and not ws[ZERO_Q + at].any()
        # under the inner product the +inf-element query's winners are +inf rows ranked by row: the lowest +inf row of each of the
        # first ten groups that hold one (the groups of the NaN bin hold none)
        ws, wr, wg = w.grouped(dim, IP, "runs8")
        want = first_group_rows(g8, K, np.isposinf(ip[INF_Q]))
        assert wr[INF_Q].tolist() == want and np.isposinf(ws[INF_Q]).all() and wg[INF_Q].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17]
    assert w.grouped(768, COS, "one")[1][NAN_Q].tolist() == [0] + [-1] * 9
    bad = w.groups["bad_groups"]
    assert np.isneginf(w.scores(768, COS)[:, bad == 5][[0, 8, 20]]).all()                    # group 5: every row -inf, whatever the query
    h = w.masks["holes"]
    assert not h[2050] and h[2049] and h[nfo.NAN_BIN[0]:nfo.NAN_BIN[1]].sum() == 32
    # a first list of 16 rows of the NaN query holds 2 groups of runs8 / sparse: 8 more must come from the exclusion loop
    assert len({int(g) for g in g8[:16]}) == 2


# ---- 1. every pattern, blocking forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_blocking_forms_over_every_group_pattern(world, pattern, dim, metric):
    idx, q = world.idx(dim), world.q(dim)
    groups = world.groups[pattern]
    idx.set_groups(groups)
    what = f"{pattern} dim {dim} metric {metric}"
    got = idx.search_grouped(q, K, metric)
    same_grouped(got, world.grouped(dim, metric, pattern), f"grouped {what}")
    first = first_group_rows(groups, K)
    have = np.array(first) >= 0
    for at in (0, AGAIN):
        assert got[1][NAN_Q + at].tolist() == first and np.isneginf(got[0][NAN_Q + at][have]).all(), f"{what}: the NaN query"
        assert got[1][ZERO_Q + at].tolist() == first and not got[0][ZERO_Q + at].view(np.uint32).any(), f"{what}: the zero query"
    if metric == IP and pattern in ("runs8", "sparse"):
        s, r = got[0][INF_Q], got[1][INF_Q]
        assert np.isposinf(s).all() and r.tolist() == first_group_rows(groups, K, np.isposinf(world.scores(dim, IP)[INF_Q])), f"{what}: +inf winners rank by row"
    for s in (1, 3, 8):
        mem = idx.search_group_members(q, K, s, metric)
        same_members(mem, world.members(dim, metric, pattern, s), f"members s={s} {what}")
        if s == 8 and pattern == "runs8" and metric == COS:
            assert mem[1][0, 0, 0] == 2050 and mem[1][0, 0, 7] == 2049 and np.isneginf(mem[0][0, 0, 7]) and mem[3][0, 0] == 8, \
                f"{what}: the NaN row is the last member of query 0's winning group"
    idx.set_groups(np.full(N, NONE))


# ---- 2. device forms and their fixups -----------------------------------------------------------------------------------------------
def _grouped_dev(idx, dq, metric, stream, row_filter=None):
    import torch
    bufs = {"q": dq, "s": torch.full((B, K), 7.0, dtype=torch.float32, device="cuda"), "r": torch.full((B, K), 7, dtype=torch.int64, device="cuda"),
            "g": torch.full((B, K), 7, dtype=torch.int32, device="cuda"), "k": torch.full((B, K), 7, dtype=torch.int64, device="cuda"),
            "st": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    idx.search_grouped_device(dq, B, K, metric, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"], stream, row_filter=row_filter)
    return bufs


def _members_dev(idx, dq, s, metric, stream, row_filter=None):
    import torch
    bufs = {"q": dq, "s": torch.full((B, K, s), 7.0, dtype=torch.float32, device="cuda"), "r": torch.full((B, K, s), 7, dtype=torch.int64, device="cuda"),
            "g": torch.full((B, K), 7, dtype=torch.int32, device="cuda"), "c": torch.full((B, K), 7, dtype=torch.int32, device="cuda"),
            "st": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    idx.search_group_members_device(dq, B, K, s, metric, bufs["s"], bufs["r"], bufs["g"], bufs["c"], bufs["st"], stream, row_filter=row_filter)
    return bufs


def _host(bufs, *names):
    return tuple(bufs[n].cpu().numpy() for n in names)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fetch", [8, 2], ids=["default", "fetch2"])
def test_device_forms_flag_the_nonfinite_queries_and_their_fixups_repair_them(world, fetch, dim, metric):
    """On a non-default stream, keys asked of the grouped call.  The fixup returns the number of flagged queries; afterwards every
    status is 0 and the outputs are the oracle's.  With "group_fetch" = 2 the first rung is an approximate pass (m1 = 20: 2 x 28 < 65
    bins), which cannot certify a query with a NaN or infinite element: those are flagged wherever they stand in the batch.  At the
    default the first rung re-scores every bin and proves them (module docstring), so what it flags is not asserted."""
    import torch
    idx = world.idx(dim)
    dq = torch.from_numpy(np.array(world.q(dim), dtype=np.float32, order="C")).cuda()
    st = torch.cuda.Stream()
    s = 3
    assert int(idx.get_option("group_fetch")) == 8
    idx.set_option("group_fetch", fetch)
    try:
        for pattern in PATTERNS:
            idx.set_groups(world.groups[pattern])
            what = f"{pattern} dim {dim} metric {metric} group_fetch {fetch}"
            bufs = _grouped_dev(idx, dq, metric, st.cuda_stream)
            st.synchronize()
            status = _host(bufs, "st")[0]
            print(f"{what}: the grouped call flagged {int(np.count_nonzero(status))} of {B} queries")
            assert set(np.unique(status).tolist()) <= {0, 1}
            if fetch == 2:
                assert status[NONFINITE_AT].all(), f"{what}: a non-finite query was certified by an approximate pass: status {status[NONFINITE_AT].tolist()}"
            n = idx.search_grouped_fixup_device(dq, B, K, metric, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"], st.cuda_stream)
            assert n == int(np.count_nonzero(status)), f"{what}: the grouped fixup returned {n}"
            st.synchronize()
            gs, gr, gg, gk, gst = _host(bufs, "s", "r", "g", "k", "st")
            assert not gst.any(), f"{what}: status after the fixup {np.flatnonzero(gst).tolist()}"
            want = world.grouped(dim, metric, pattern)
            same_grouped((gs, gr, gg), want, f"grouped device form {what}")
            assert np.array_equal(gk.view(np.uint64), dist.pack_keys(gs, gr)), f"{what}: keys"      # (pack_keys: key 0 where the row is -1)
            assert not gk[gr < 0].any()
            assert idx.search_grouped_fixup_device(dq, B, K, metric, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"], st.cuda_stream) == 0

            bufs = _members_dev(idx, dq, s, metric, st.cuda_stream)
            st.synchronize()
            status = _host(bufs, "st")[0]
            print(f"{what}: the members call flagged {int(np.count_nonzero(status))} of {B} queries")
            if fetch == 2:
                assert status[NONFINITE_AT].all(), f"{what}: members: a non-finite query was certified by an approximate pass"
            n = idx.search_group_members_fixup_device(dq, B, K, s, metric, bufs["s"], bufs["r"], bufs["g"], bufs["c"], bufs["st"], st.cuda_stream)
            assert n == int(np.count_nonzero(status)), f"{what}: the members fixup returned {n}"
            st.synchronize()
            got = _host(bufs, "s", "r", "g", "c", "st")
            assert not got[4].any(), f"{what}: members status after the fixup {np.flatnonzero(got[4]).tolist()}"
            same_members(got, world.members(dim, metric, pattern, s), f"members device form {what}")
    finally:
        idx.set_option("group_fetch", 8)
        idx.stream_release(st.cuda_stream)
        idx.set_groups(np.full(N, NONE))


# ---- 3. every rung ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("cap", [16, 64])
def test_every_rung_gives_the_same_answers(world, cap, dim, metric):
    """"group_fetch" = 1: the first list holds just k rows (an approximate pass at this size); "group_fetch_cap" 16 and 64: rung 2 asks for
    16 rows (approximate pass, then the ladder) or 64 (every bin re-scored), and whoever is still short of k groups goes through
    the exclusion loop -- the NaN and the zero query (16 rows = 2 groups of eight) among them, over all-tie lists."""
    idx, q = world.idx(dim), world.q(dim)
    assert int(idx.get_option("group_fetch")) == 8 and int(idx.get_option("group_fetch_cap")) == 0
    idx.set_option("group_fetch", 1)
    idx.set_option("group_fetch_cap", cap)
    try:
        for pattern in ("runs8", "sparse"):
            idx.set_groups(world.groups[pattern])
            what = f"{pattern} dim {dim} metric {metric} cap {cap}"
            repaired = int(idx.get_option("group_repaired"))
            same_grouped(idx.search_grouped(q, K, metric), world.grouped(dim, metric, pattern), f"grouped {what}")
            assert int(idx.get_option("group_repaired")) >= repaired + len(NONFINITE_AT), f"{what}: the non-finite queries were not repaired"
            rounds = int(idx.get_option("group_rounds_last"))
            print(f"{what}: {int(idx.get_option('group_repaired')) - repaired} queries repaired, {rounds} exclusion rounds")
            if cap == 16:
                assert rounds >= 1, f"{what}: the exclusion loop did not run"
            same_members(idx.search_group_members(q, K, 3, metric), world.members(dim, metric, pattern, 3), f"members {what}")
    finally:
        idx.set_option("group_fetch", 8)
        idx.set_option("group_fetch_cap", 0)
        idx.set_groups(np.full(N, NONE))


# ---- 4. filters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mask", ["mod3", "holes"])
def test_filtered_grouped_and_member_searches_on_every_filter_route(world, mask, dim, metric):
    idx, q = world.idx(dim), world.q(dim)
    flt = idx.make_filter(world.masks[mask])
    try:
        for pattern in ("runs8", "bad_groups"):
            groups = world.groups[pattern]
            idx.set_groups(groups)
            first = first_group_rows(groups, K, world.masks[mask])
            for route in (-1, 1, 2, 3):
                idx.set_option("filter_route", route)
                what = f"{pattern} mask {mask} route {route} dim {dim} metric {metric}"
                got = idx.search_grouped(q, K, metric, row_filter=flt)
                same_grouped(got, world.grouped(dim, metric, pattern, mask), f"grouped {what}")
                for at in (0, AGAIN):
                    assert got[1][NAN_Q + at].tolist() == first and np.isneginf(got[0][NAN_Q + at]).all(), f"{what}: the NaN query"
                    assert got[1][ZERO_Q + at].tolist() == first and not got[0][ZERO_Q + at].view(np.uint32).any(), f"{what}: the zero query"
                mem = idx.search_group_members(q, K, 3, metric, row_filter=flt)
                same_members(mem, world.members(dim, metric, pattern, 3, mask), f"members {what}")
                assert world.masks[mask][mem[1][mem[1] >= 0]].all(), f"{what}: a row outside the filter came back"
    finally:
        idx.set_option("filter_route", -1)
        flt.close()
        idx.set_groups(np.full(N, NONE))


# ---- 5. the identities of include/rq.h ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_members_are_the_grouped_answer_and_score_rows_bit_for_bit(world, dim, metric):
    idx, q = world.idx(dim), world.q(dim)
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
    try:
        for pattern in ("runs8", "mixed", "bad_groups"):
            idx.set_groups(world.groups[pattern])
            what = f"{pattern} dim {dim} metric {metric}"
            gs, gr, gg = idx.search_grouped(q, K, metric)
            ms, mr, mg, mc = idx.search_group_members(q, K, 1, metric)
            assert np.array_equal(mr[:, :, 0], gr) and np.array_equal(mg, gg) and np.array_equal(u32(ms[:, :, 0]), u32(gs)), f"{what}: s = 1 is not the grouped answer"
            assert np.array_equal(mc, (gr >= 0).astype(np.int32))
            for s in (3, 8):
                ms, mr, mg, mc = idx.search_group_members(q, K, s, metric)
                assert np.array_equal(mr[:, :, 0], gr) and np.array_equal(mg, gg) and np.array_equal(u32(ms[:, :, 0]), u32(gs)), f"{what} s={s}: member 0 is not the winner"
                again = idx.score_rows(q, mr.reshape(B, K * s), metric)
                diff = np.argwhere(u32(again) != u32(ms.reshape(B, K * s)))
                assert diff.size == 0, f"{what} s={s}: scores are not score_rows's bit for bit at (query, entry) {diff[:4].tolist()}"
                for b in (TINY_Q, HUGE_Q, INF_Q, NEG_INF_Q):
                    assert (mr[b] >= 0).sum() >= K, what                # (the special queries take part: their slots hold rows)
    finally:
        idx.set_groups(np.full(N, NONE))


# ---- 6. the pure collapse -----------------------------------------------------------------------------------------------------------
def _hand_made_lists(m, nb, seed):
    """[nb][m] candidates in shuffled order: four +inf rows in three groups (rows 800, 801 of one, 808 of the next, 2000 on its own: the
    groups tie at +inf and rank by row), three -inf rows, -0.0, +0.0, NaN scores (absent), rows -1 and beyond the shard (absent);
    explicit ids with the same structure."""
    rng = np.random.default_rng(seed)
    hand_rows = [800, 801, 808, 2000, 8, 9, 3000, 3001]
    hand_scores = [np.inf, np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf, np.nan]
    hand_ids = [3, 3, 4, NONE, 5, 5, NONE, 3]
    rows, scores, ids = [], [], []
    for b in range(nb):
        free = np.flatnonzero(~np.isin(np.arange(N) // 8, np.array(hand_rows) // 8))      # no drawn row shares a run of eight with a hand-made one
        others = rng.choice(free, size=m - len(hand_rows), replace=False)
        r = np.concatenate([hand_rows, others]).astype(np.int64)
        s = np.concatenate([hand_scores, rng.standard_normal(others.size)]).astype(np.float32)
        g = np.concatenate([hand_ids, rng.integers(6, max(m // 4, 8), size=others.size)]).astype(np.int64)
        g[rng.random(m) < 0.15] = NONE
        g[:7] = hand_ids[:7]
        s[8], s[9], s[10] = -0.0, 0.0, np.nan
        r[11], r[12] = -1, N + 5
        p = rng.permutation(m)
        rows.append(r[p]); scores.append(s[p]); ids.append(g[p])
    return np.stack(scores), np.stack(rows), np.stack(ids)


@pytest.mark.parametrize("m", [64, 257])
def test_pure_collapse_of_hand_made_lists_with_infinite_scores(world, m):
    import torch
    idx = world.idx(768)
    index_groups = world.groups["sparse"]
    idx.set_groups(index_groups)
    nb = 5
    cs, cr, cg = _hand_made_lists(m, nb, seed=m)
    d_r, d_s, d_g = torch.from_numpy(cr).cuda(), torch.from_numpy(cs).cuda(), torch.from_numpy(cg.astype(np.int32)).cuda()
    try:
        for k in (1, 10, 40, m):
            for explicit in (False, True):
                g_in = cg if explicit else gro.lookup_groups(cr, index_groups)
                ws, wr, wg, wst = gro.collapse_batch(cs, cr, g_in, k, N)
                if k == m:                                              # every winner is listed: the -inf rows 8 (for its group) and 3000 come last
                    assert wst.all() and all(wr[b][wr[b] >= 0][-2:].tolist() == [8, 3000] for b in range(nb)) and (np.isneginf(ws).sum(axis=1) == 2).all()
                assert wr[:, 0].tolist() == [800] * nb and (k == 1 or wr[:, 1:3].tolist() == [[808, 2000]] * nb), "three groups tie at +inf: they rank by row"
                o_s = torch.full((nb, k), 7.0, dtype=torch.float32, device="cuda")
                o_r = torch.full((nb, k), 7, dtype=torch.int64, device="cuda")
                o_g = torch.full((nb, k), 7, dtype=torch.int32, device="cuda")
                o_k = torch.full((nb, k), 7, dtype=torch.int64, device="cuda")
                o_st = torch.full((nb,), 7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                idx.group_collapse_device(d_r, d_s, d_g if explicit else None, nb, m, k, o_s, o_r, o_g, o_k, o_st)
                torch.cuda.synchronize()
                gs, gr, gg, gk, gst = o_s.cpu().numpy(), o_r.cpu().numpy(), o_g.cpu().numpy(), o_k.cpu().numpy().view(np.uint64), o_st.cpu().numpy()
                what = f"m={m} k={k} {'explicit ids' if explicit else 'ids looked up'}"
                assert np.array_equal(gr, wr), f"{what}: rows differ at {np.argwhere(gr != wr)[:4].tolist()}"
                assert np.array_equal(gg, wg), f"{what}: group ids"
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{what}: scores are passed through bit for bit, -0.0 as +0.0"
                assert np.array_equal(gst, wst), f"{what}: status {gst.tolist()} against {wst.tolist()}"
                assert np.array_equal(gk, dist.pack_keys(ws, wr)), f"{what}: keys"
                assert not np.isin(gr, [3001, N + 5]).any() and not np.isnan(gs).any()
    finally:
        idx.set_groups(np.full(N, NONE))


# ---- 7. the pure fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_pure_fill_over_hand_made_winner_lists_under_the_nonfinite_queries(world, dim, metric):
    import torch
    idx = world.idx(dim)
    groups = world.groups["bad_groups"]
    idx.set_groups(groups)
    nb, k, s = 8, 5, 4
    q = np.array(world.q(dim)[:nb], dtype=np.float32, order="C")
    s_all = world.scores(dim, metric)[:nb]
    #        absent slot    a row on its own: NaN   group 5: all -inf   the same group again   the zero rows
    rows = [[-1,            2049,                   64,                 100,                   1000]] * nb
    ids = [[5,              NONE,                   5,                  5,                     6]] * nb
    mask = world.masks["holes"].copy()
    mask[[65, 1003]] = False
    flt = idx.make_filter(mask)
    d_q = torch.from_numpy(q).cuda()
    d_wr, d_wg = torch.tensor(rows, dtype=torch.int64, device="cuda"), torch.tensor(ids, dtype=torch.int32, device="cuda")
    try:
        for f, in_play in ((None, np.ones(N, bool)), (flt, mask)):
            o_s = torch.full((nb, k, s), 7.0, dtype=torch.float32, device="cuda")
            o_r = torch.full((nb, k, s), 7, dtype=torch.int64, device="cuda")
            o_c = torch.full((nb, k), 7, dtype=torch.int32, device="cuda")
            o_st = torch.full((nb,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            idx.group_fill_device(d_q, nb, k, s, metric, d_wr, d_wg, o_s, o_r, o_c, o_st, row_filter=f)
            torch.cuda.synchronize()
            gs, gr, gc, gst = o_s.cpu().numpy(), o_r.cpu().numpy(), o_c.cpu().numpy(), o_st.cpu().numpy()
            what = f"dim {dim} metric {metric} {'filtered' if f else 'unfiltered'}"
            assert not gst.any(), what
            ws, wr, wc = np.zeros((nb, k, s), np.float32), np.full((nb, k, s), -1, np.int64), np.zeros((nb, k), np.int32)
            for b in range(nb):
                for j in range(1, k):
                    own = np.array([rows[b][j]]) if ids[b][j] < 0 else np.flatnonzero(groups == ids[b][j])
                    own = own[in_play[own]]
                    if own.size:                                        # the slot's rows in play, as the one group of a world of their own
                        ms, mr, _, mc = gmo.members(s_all[b, own], own, groups[own], 1, s)
                        ws[b, j], wr[b, j], wc[b, j] = ms[0], mr[0], mc[0]
            assert wc[0].tolist() == [0, 1, 4, 4, 4] and np.array_equal(wr[:, 2], wr[:, 3])
            assert wr[NAN_Q, 2].tolist() == ([64, 65, 66, 67] if f is None else [67, 69, 71, 73]) and wr[ZERO_Q, 4].tolist() == ([1000, 1001, 1002, 1003] if f is None else [1000, 1001, 1002, 1004])
            assert np.array_equal(gc, wc), f"{what}: counts {gc[:2].tolist()}"
            nfo.assert_matches(gs.reshape(nb, k * s), gr.reshape(nb, k * s), ws.reshape(nb, k * s), wr.reshape(nb, k * s), SCORE_TOL, what)
            assert not gs[wr < 0].view(np.uint32).any()
            assert np.isneginf(gs[[0, 3, 4, 6], 2]).all() and not gs[ZERO_Q].view(np.uint32).any(), f"{what}: group 5 scores -inf for every query but the zero one"
            again = idx.score_rows(q, gr.reshape(nb, k * s), metric)
            assert np.array_equal(again.view(np.uint32), gs.reshape(nb, k * s).view(np.uint32)), f"{what}: scores are not score_rows's bit for bit"
    finally:
        flt.close()
        idx.set_groups(np.full(N, NONE))
