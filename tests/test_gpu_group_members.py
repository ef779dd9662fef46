"""Group members on the MI355X (include/rq.h "group members", csrc/rq_group_members.hip): rows, group ids and counts
equal the oracle's (tests/group_members_oracle.py: one walk down the FULL exact ranking of oracle/dense_oracle.py), and every
score has the bits rq_score_rows returns for that (query, row) pair."""
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
import nonfinite_oracle as nfo  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6                   # against the oracle's own scores (the bar of tests/test_gpu_parity.py); the bits are score_rows's
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
NONE = nat.GROUP_NONE
N_BASE = 4101                      # 65 bins, a ragged last bin
NQ = 70
BIG_ID = 2 ** 31 - 1
FILL_MAX = 4096
# group sizes in the member table: 1, s - 1, s, s + 1 for s = 2, 3, 8; the lane-group round boundaries 15 / 16 / 17 / 32 / 33; the
# sort-size boundaries 63 / 64 / 65
SIZES = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65]


class Shape:
    """One index with its rows, NQ queries and their canonical score matrix per metric (computed once, shared, never changed)."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, nq=NQ, options=(("scan8", 0),), row_offset=0, x16=None, q=None):
        self.n, self.dim, self.row_offset = n, dim, row_offset
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed) if x16 is None else x16
        self.q = orc.synthetic_queries(nq, dim, seed=seed + 1) if q is None else q
        self.idx = nat.NativeIndex(dim, 0)
        for name, v in options:
            self.idx.set_option(name, v)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self._scores = {}

    def scores(self, metric=COS):
        if metric not in self._scores:
            s = nfo.scores(self.q, self.x16, metric)
            s.setflags(write=False)
            self._scores[metric] = s
        return self._scores[metric]

    def want(self, groups, k, s, metric=COS, B=16, mask=None):
        return gmo.members_from_scores(self.scores(metric)[:B], groups, k, s, mask, self.row_offset)

    def close(self):
        self.idx.close()


def agrees(sh, got, want, metric=COS, what="", q=None, scores_all=None):
    """(scores, rows, groups, counts) against the oracle's: rows, ids and counts identical; the scores bit for bit those of
    score_rows for the returned rows (0.0 where there is none), and within the parity bar of the oracle's own."""
    gs, gr, gg, gc = got[:4]
    ws, wr, wg, wc = want
    B, k, s = gr.shape
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.argwhere(gc != wc)[:4].tolist()}\n{gc[:2]}\n{wc[:2]}"
    assert np.array_equal(gg, wg), f"{what}: group ids differ"
    assert np.array_equal(gr, wr), f"{what}: rows differ at {np.argwhere(gr != wr)[:4].tolist()}"
    q = sh.q[:B] if q is None else q
    sr = sh.idx.score_rows(q, gr.reshape(B, k * s), metric)
    assert np.array_equal(gs.reshape(B, k * s).view(np.uint32), sr.view(np.uint32)), f"{what}: scores are not score_rows's bit for bit"
    scores_all = sh.scores(metric) if scores_all is None else scores_all
    fin = np.isfinite(ws)
    assert np.array_equal(gs[~fin], ws[~fin]), f"{what}: non-finite scores differ"
    tol = SCORE_TOL * max(1.0, float(np.abs(scores_all[np.isfinite(scores_all)]).max()))
    err = float(np.abs(gs[fin].astype(np.float64) - ws[fin].astype(np.float64)).max(initial=0.0))
    print(f"{what}: largest score difference to the oracle {err} (bar {tol})")
    assert err <= tol, f"{what}: scores differ from the oracle's by {err}"
    assert not np.signbit(gs[gs == 0]).any(), f"{what}: -0.0 returned"


def sized_groups(n, seed=3):
    """Every size of SIZES again and again until the rows run out, ids sparse, the members of a group scattered over the shard."""
    rng = np.random.default_rng(seed)
    ids = np.empty(n, np.int64)
    at, g = 0, 0
    while at < n:
        size = SIZES[g % len(SIZES)]
        ids[at:at + size] = 1000 + 37 * g
        at += size
        g += 1
    out = np.empty(n, np.int64)
    out[rng.permutation(n)] = ids
    return out


def patterns(n, seed=3):
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, max(n // 6, 2), size=n).astype(np.int64)
    rand[rng.random(n) < 0.1] = NONE
    rand[0], rand[1], rand[n - 1] = 0, BIG_ID, BIG_ID
    one = np.full(n, 5, np.int64)
    one[FILL_MAX:] = NONE                                   # one group of exactly RQ_GROUP_FILL_MAX rows: the largest the kernel fills
    return {"none": np.full(n, NONE, np.int64), "one": one, "runs8": np.arange(n, dtype=np.int64) // 8, "random": rand, "sized": sized_groups(n, seed)}


def test_the_shapes_keep_every_group_within_the_default_cap():
    """Verified on the CPU from the group arrays: no pattern of this file holds a group of more than RQ_GROUP_FILL_MAX rows, so with
    the cap at its default nothing may be repaired; and "sized" holds every size of SIZES."""
    for n in (N_BASE, 2000):
        for name, g in patterns(n).items():
            sizes = gmo.table_sizes(g)
            assert max(sizes.values(), default=0) <= FILL_MAX, name
        assert set(SIZES) <= set(gmo.table_sizes(patterns(n)["sized"]).values())
    assert max(gmo.table_sizes(patterns(N_BASE)["one"]).values()) == FILL_MAX


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


# ---- 1. group patterns, sizes, identities --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["none", "one", "runs8", "random", "sized"])
def test_group_patterns_equal_the_oracle(wide, pattern):
    groups = patterns(N_BASE)[pattern]
    wide.idx.set_groups(groups)
    q = wide.q[:16]
    repaired = int(wide.idx.get_option("group_fill_repaired"))
    for metric in (COS, IP):
        gs1, gr1, gg1 = wide.idx.search_grouped(q, 10, metric)
        for s in (1, 2, 3, 8):
            got = wide.idx.search_group_members(q, 10, s, metric)
            agrees(wide, got, wide.want(groups, 10, s, metric), metric, f"{pattern} s={s} metric {metric}")
            # member 0 of every slot is the winner: the grouped call's row, id and score bits
            assert np.array_equal(got[1][:, :, 0], gr1) and np.array_equal(got[2], gg1) and np.array_equal(got[0][:, :, 0].view(np.uint32), gs1.view(np.uint32))
            if s == 1:
                assert np.array_equal(got[3], (gr1 >= 0).astype(np.int32))
            if pattern == "none":
                ps, pr = wide.idx.search(q, 10, metric)
                assert np.array_equal(got[1][:, :, 0], pr) and np.array_equal(got[0][:, :, 0].view(np.uint32), ps.view(np.uint32))
                assert (got[3] == 1).all() and (got[2] == NONE).all() and (got[1][:, :, 1:] == -1).all()
            if pattern == "one" and s == 8:
                assert (got[3][:, 0] == 8).all() and (got[2][:, 0] == 5).all()
    assert int(wide.idx.get_option("group_fill_repaired")) == repaired, "nothing exceeds the default cap: nothing is repaired"
    wide.idx.set_groups(np.full(N_BASE, NONE))


@pytest.mark.parametrize("B", [1, 16, 70])
@pytest.mark.parametrize("shape", ["wide", "narrow", "dim33"])
def test_group_sizes_around_s_the_lane_rounds_and_the_sort_sizes(request, shape, B):
    sh = request.getfixturevalue(shape)
    groups = patterns(sh.n)["sized"]
    sh.idx.set_groups(groups)
    repaired = int(sh.idx.get_option("group_fill_repaired"))
    for k, s, metric in ((10, 3, COS), (7, 8, IP)) if B != 16 else ((10, 2, COS), (10, 3, IP), (33, 8, COS)):
        got = sh.idx.search_group_members(sh.q[:B], k, s, metric)
        want = sh.want(groups, k, s, metric, B)
        agrees(sh, got, want, metric, f"{shape} B={B} k={k} s={s} metric {metric}")
        size = gmo.table_sizes(groups)
        seen = {size[int(g)] for g in want[2].ravel() if g >= 0}
        print(f"{shape} B={B} k={k} s={s}: winning groups of sizes {sorted(seen)}")
    assert int(sh.idx.get_option("group_fill_repaired")) == repaired
    sh.idx.set_groups(np.full(sh.n, NONE))


def test_k_times_s_of_1024_exactly_and_1025_is_refused(wide):
    groups = patterns(N_BASE)["runs8"]
    wide.idx.set_groups(groups)
    got = wide.idx.search_group_members(wide.q[:2], 128, 8)
    agrees(wide, got, wide.want(groups, 128, 8, B=2), COS, "k=128 s=8")
    assert (got[3] == 8).sum() > 200                                     # runs of 8: most slots are full
    got = wide.idx.search_group_members(wide.q[:1], 1, 1024)
    agrees(wide, got, wide.want(groups, 1, 1024, B=1), COS, "k=1 s=1024")
    assert got[3][0, 0] == 8 and (got[1][0, 0, 8:] == -1).all()
    lib, P = nat.load_library(), nat._ptr
    q = np.ascontiguousarray(wide.q[:1])
    for k, s in ((205, 5), (1025, 1), (1, 1025), (129, 8)):
        hs, hr, hg, hc = np.zeros((1, k, s), np.float32), np.zeros((1, k, s), np.int64), np.zeros((1, k), np.int32), np.zeros((1, k), np.int32)
        assert lib.rq_search_group_members(wide.idx._h, None, P(q), 1, k, s, COS, P(hs), P(hr), P(hg), P(hc)) == -1 and "outside 1..1024" in nat.last_error()
        with pytest.raises(ValueError):
            wide.idx.search_group_members(q, k, s)
    wide.idx.set_groups(np.full(N_BASE, NONE))


# ---- 2. filters -----------------------------------------------------------------------------------------------------------------
def test_every_filter_route_gives_the_oracle_and_a_stale_filter_is_refused():
    sh = Shape(seed=13, nq=16)
    groups = patterns(N_BASE)["sized"]
    sh.idx.set_groups(groups)
    masks = fo.standard_masks(N_BASE)
    plain = sh.want(groups, 10, 3)
    gone = np.isin(groups, plain[2][:, :3].ravel())                       # a filter that removes the three best groups of every query, whole
    masks = {"random50": masks["random50"], "rotation": masks["rotation"], "five_rows": masks["five_rows"], "none": masks["none"], "whole_groups": ~gone}
    for name, mask in masks.items():
        flt = sh.idx.make_filter(mask)
        want = sh.want(groups, 10, 3, mask=mask)
        if name == "random50":                                            # it removes some members of winning groups: their counts shrink
            full = np.array([[min(3, gmo.table_sizes(groups).get(int(g), 1)) for g in row] for row in want[2]])
            assert (want[3] < full).any()
        if name == "whole_groups":
            assert not np.isin(want[2], plain[2][:, :3]).any()
        results = []
        for route in (-1, 1, 2, 3):
            sh.idx.set_option("filter_route", route)
            got = sh.idx.search_group_members(sh.q[:16], 10, 3, row_filter=flt)
            agrees(sh, got, want, COS, f"{name} route {route}")
            results.append(got)
        for got in results[1:]:
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, results[0])), f"{name}: the routes differ"
        flt.close()
    sh.idx.set_option("filter_route", -1)
    flt = sh.idx.make_filter(masks["random50"])
    sh.idx.add_f16(sh.x16[:10])
    with pytest.raises(nat.RqError, match="stale filter"):
        sh.idx.search_group_members(sh.q[:16], 10, 3, row_filter=flt)
    flt.close()
    sh.close()


# ---- 3. value rules ---------------------------------------------------------------------------------------------------------------
def test_a_zero_norm_query_returns_the_lowest_rows_of_the_first_groups(wide):
    groups = patterns(N_BASE)["random"].copy()
    groups[:40] = np.repeat(np.arange(10), 4) + 50                     # the first 40 rows: ten groups of four
    wide.idx.set_groups(groups)
    q = np.stack([np.zeros(768, np.float32), wide.q[0]])
    for metric in (COS, IP):
        s_all = np.stack([np.zeros(N_BASE, np.float32), wide.scores(metric)[0]])
        got = wide.idx.search_group_members(q, 5, 3, metric)
        agrees(wide, got, gmo.members_from_scores(s_all, groups, 5, 3), metric, f"zero-norm query, metric {metric}", q=q, scores_all=s_all)
        assert not got[0][0].any() and got[1][0, :, 0].tolist() == [0, 4, 8, 12, 16]
        for j in range(5):
            assert got[1][0, j].tolist() == sorted(np.flatnonzero(groups == got[2][0, j]).tolist())[:3]      # the lowest three rows of the group
    wide.idx.set_groups(np.full(N_BASE, NONE))


def test_duplicate_stored_rows_inside_one_group_tie_by_row():
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=5)
    base = orc.synthetic_queries(4, 768, seed=6)
    x16[100] = x16[7]                                      # duplicates inside ONE group: the tie goes by row
    x16[300] = x16[7]
    groups = np.arange(N_BASE, dtype=np.int64) // 8 + 1000
    groups[[100, 300]] = groups[7]                         # the group of row 7: rows 0..7, 100 and 300
    q = np.stack([x16[7].astype(np.float32) + base[0] / np.linalg.norm(base[0]), x16[2].astype(np.float32) + base[1] / np.linalg.norm(base[1]), base[2], base[3]])
    sh = Shape(x16=x16, q=q, seed=5)
    sh.idx.set_groups(groups)
    for metric in (COS, IP):
        got = sh.idx.search_group_members(q, 6, 16, metric)
        agrees(sh, got, sh.want(groups, 6, 16, metric, B=4), metric, f"duplicates, metric {metric}")
        assert got[2][0, 0] == groups[7] and got[3][0, 0] == 10
        rows0 = got[1][0, 0, :10].tolist()
        assert rows0[:3] == [7, 100, 300] and got[0][0, 0, 0] == got[0][0, 0, 1] == got[0][0, 0, 2]
        assert set(rows0) == {0, 1, 2, 3, 4, 5, 6, 7, 100, 300}
    sh.close()


def test_nonfinite_rows_inside_the_winning_group_under_both_metrics():
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=15)
    base = orc.synthetic_queries(2, 768, seed=16)
    x16[41, 5] = np.nan
    x16[42, 9] = np.inf
    x16[43, 2] = -np.inf
    groups = np.arange(N_BASE, dtype=np.int64) // 8                       # rows 40..47 are group 5
    q = np.stack([x16[44].astype(np.float32) + base[0] / np.linalg.norm(base[0]), base[1]])
    sh = Shape(x16=x16, q=q, seed=15)
    sh.idx.set_groups(groups)
    for metric in (COS, IP):
        got = sh.idx.search_group_members(q, 4, 8, metric)
        agrees(sh, got, sh.want(groups, 4, 8, metric, B=2), metric, f"non-finite rows, metric {metric}")
        assert got[2][0, 0] == 5 and got[3][0, 0] == 8 and (got[1][0, 0, 0] == 44 or metric == IP)      # (an infinite row may win the inner product)
        members = got[1][0, 0].tolist()
        assert set(members) == set(range(40, 48))                          # NaN and infinite rows still count as members
        if metric == COS:                                                  # an infinite row's cosine is NaN too: all three count as -inf and come last, by row
            assert members[-3:] == [41, 42, 43] and np.isneginf(got[0][0, 0, -3:]).all()
        else:
            assert np.isneginf(got[0][0, 0][members.index(41)])            # the NaN row: -inf
        s = got[0][0, 0]
        assert not np.isnan(s).any() and (s[:-1] >= s[1:]).all()
    sh.close()


def test_row_offset_global_rows_come_out():
    sh = Shape(n=1000, seed=9, nq=8, row_offset=10 ** 6)
    groups = patterns(1000)["sized"]
    sh.idx.set_groups(groups)
    got = sh.idx.search_group_members(sh.q, 10, 3)
    assert got[1][got[1] >= 0].min() >= 10 ** 6
    agrees(sh, got, sh.want(groups, 10, 3, B=8), COS, "row_offset")
    sh.close()


# ---- 4. the device forms, overflow and repair ---------------------------------------------------------------------------------------
def members_dev(idx, q, k, s, metric=COS, stream=0, row_filter=None):
    import torch
    B = q.shape[0]
    bufs = {"q": torch.from_numpy(np.ascontiguousarray(q)).cuda(), "s": torch.full((B, k, s), 7.0, dtype=torch.float32, device="cuda"),
            "r": torch.full((B, k, s), 7, dtype=torch.int64, device="cuda"), "g": torch.full((B, k), 7, dtype=torch.int32, device="cuda"),
            "c": torch.full((B, k), 7, dtype=torch.int32, device="cuda"), "st": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    idx.search_group_members_device(bufs["q"], B, k, s, metric, bufs["s"], bufs["r"], bufs["g"], bufs["c"], bufs["st"], stream, row_filter=row_filter)
    return bufs


def members_fixup(idx, bufs, k, s, metric=COS, stream=0, row_filter=None):
    return idx.search_group_members_fixup_device(bufs["q"], bufs["q"].shape[0], k, s, metric, bufs["s"], bufs["r"], bufs["g"], bufs["c"], bufs["st"], stream,
                                                 row_filter=row_filter)


def host(bufs):
    import torch
    torch.cuda.synchronize()
    return bufs["s"].cpu().numpy(), bufs["r"].cpu().numpy(), bufs["g"].cpu().numpy(), bufs["c"].cpu().numpy(), bufs["st"].cpu().numpy()


@pytest.fixture(scope="module")
def capped():
    """Runs of 8, and three planted groups around a cap of 16: 9000 (17 rows = cap + 1, holds the best row of query 3), 9001 (16 rows =
    the cap, holds the best row of query 5), 9002 (100 rows, holds the second-best row of query 7)."""
    sh = Shape(seed=29, nq=16)
    top = orc.topk_from_scores(sh.scores()[:16], 2)[1]
    groups = np.arange(N_BASE, dtype=np.int64) // 8
    spare = np.setdiff1d(np.arange(1000, 1400), top.ravel())
    groups[np.concatenate([[top[3, 0]], spare[:16]])] = 9000
    groups[np.concatenate([[top[5, 0]], spare[16:31]])] = 9001
    groups[np.concatenate([[top[7, 1]], spare[31:130]])] = 9002
    sh.groups = groups
    sh.idx.set_groups(groups)
    yield sh
    sh.close()


def test_overflow_flags_exactly_the_oversized_queries_and_the_fixup_repairs_them(capped):
    sh, groups = capped, capped.groups
    B, k, s, cap = 16, 10, 3, 16
    size = gmo.table_sizes(groups)
    assert size[9000] == cap + 1 and size[9001] == cap and size[9002] == 100
    want = sh.want(groups, k, s, B=B)
    over = gmo.oversized_queries(want[2], groups, cap)
    assert over[3] and over[7] and not over[5] and 0 < over.sum() < B, "the precondition, on the oracle alone"
    over_slot = np.array([[g >= 0 and size.get(int(g), 0) > cap for g in row] for row in want[2]])
    sh.idx.set_option("group_fill_cap", cap)
    try:
        before = int(sh.idx.get_option("group_fill_repaired"))
        bufs = members_dev(sh.idx, sh.q[:B], k, s)
        first = host(bufs)
        assert first[4].tolist() == over.astype(int).tolist(), "status 1 for exactly the queries that hold an oversized group"
        assert np.array_equal(first[3] == -1, over_slot), "count -1 on exactly the oversized slots"
        assert (first[1][over_slot] == -1).all() and not first[0][over_slot].any()
        keep = ~over_slot
        assert np.array_equal(first[3][keep], want[3][keep]) and np.array_equal(first[1][keep], want[1][keep]) and np.array_equal(first[2], want[2])
        assert want[3][5, 0] == 3 and first[2][5, 0] == 9001, "a group of exactly the cap is filled by the kernel"
        n = members_fixup(sh.idx, bufs, k, s)
        after = host(bufs)
        assert n == int(over.sum()) and int(sh.idx.get_option("group_fill_repaired")) == before + n
        assert not after[4].any()
        agrees(sh, after, want, COS, "after the repair")
        for a, b in zip(first, after):
            assert np.array_equal(a[~over].view(np.uint8), b[~over].view(np.uint8)), "the unflagged queries are untouched"
        assert members_fixup(sh.idx, bufs, k, s) == 0
        # the blocking form equals the device form plus fixup, bit for bit
        blocking = sh.idx.search_group_members(sh.q[:B], k, s)
        for a, b in zip(blocking, after[:4]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert int(sh.idx.get_option("group_fill_repaired")) == before + 2 * n
        # within a filter the exact route takes the group's rows IN PLAY
        mask = np.arange(N_BASE) % 2 == 0
        mask[orc.topk_from_scores(sh.scores()[:16], 1)[1][:, 0]] = True
        flt = sh.idx.make_filter(mask)
        agrees(sh, sh.idx.search_group_members(sh.q[:B], k, s, row_filter=flt), sh.want(groups, k, s, B=B, mask=mask), COS, "repair within a filter")
        flt.close()
    finally:
        sh.idx.set_option("group_fill_cap", 0)
    repaired = int(sh.idx.get_option("group_fill_repaired"))
    agrees(sh, sh.idx.search_group_members(sh.q[:B], k, s), want, COS, "the cap at its default")
    assert int(sh.idx.get_option("group_fill_repaired")) == repaired


def test_a_group_beyond_the_structural_maximum_takes_the_exact_route():
    sh = Shape(seed=31, nq=4)
    groups = np.full(N_BASE, 5, np.int64)                                  # 4101 rows in one group: one more bin than RQ_GROUP_FILL_MAX
    sh.idx.set_groups(groups)
    got = sh.idx.search_group_members(sh.q[:4], 3, 8)
    agrees(sh, got, sh.want(groups, 3, 8, B=4), COS, "one group of 4101 rows")
    assert (got[3][:, 0] == 8).all() and (got[3][:, 1:] == 0).all() and int(sh.idx.get_option("group_fill_repaired")) == 4
    sh.close()


def test_one_query_needs_the_grouped_repair_and_the_member_repair():
    sh = Shape(seed=29, nq=16)
    B, k, s, bad, cap = 16, 5, 3, 3, 16
    sh.idx.set_option("group_fetch_cap", 64)
    sh.idx.set_option("group_fill_cap", cap)
    groups = np.full(N_BASE, NONE, np.int64)
    groups[orc.topk_from_scores(sh.scores()[bad:bad + 1], 200)[1][0]] = 7          # one group owns the 200 best rows of query 3
    sh.idx.set_groups(groups)
    m1 = min(int(sh.idx.get_option("group_fetch")) * k, 64)
    top_s, top_r = orc.topk_from_scores(sh.scores()[:B], m1)
    short = gro.collapse_batch(top_s, top_r, gro.lookup_groups(top_r, groups), k, N_BASE)[3].astype(bool)      # the grouped stage cannot prove these
    want = sh.want(groups, k, s, B=B)
    over = gmo.oversized_queries(want[2], groups, cap)
    assert short.tolist() == [b == bad for b in range(B)] and over[bad], "the precondition, on the oracle alone: query 3 needs both repairs"
    bufs = members_dev(sh.idx, sh.q[:B], k, s)
    first = host(bufs)
    flagged = short | over
    assert first[4].tolist() == flagged.astype(int).tolist()
    n = members_fixup(sh.idx, bufs, k, s)
    after = host(bufs)
    assert n == int(flagged.sum()) and not after[4].any()
    assert int(sh.idx.get_option("group_rounds_last")) >= 1, "rung 3 ran"
    agrees(sh, after, want, COS, "after both repairs")
    assert after[2][bad, 0] == 7 and after[3][bad, 0] == 3
    sh.close()


# ---- 5. the member table's lifetime ------------------------------------------------------------------------------------------------
def test_the_table_is_built_once_rebuilt_after_set_groups_and_kept_across_appends():
    x16 = orc.synthetic_corpus(N_BASE + 5000, 768, seed=41)
    q = np.concatenate([orc.synthetic_queries(4, 768, seed=42), x16[N_BASE + 10:N_BASE + 14].astype(np.float32)])      # four of them: rows appended later
    idx = nat.NativeIndex(768, 0)
    idx.set_option("scan8", 0)
    idx.add_f16(x16[:N_BASE])
    sh = type("S", (), {"idx": idx, "q": q, "row_offset": 0})()
    first = np.arange(N_BASE, dtype=np.int64) // 8
    idx.set_groups(first)
    assert int(idx.get_option("group_table_builds")) == 0 and int(idx.get_option("group_fill_rows_last")) == -1      # built by the first call that needs it
    idx.search_grouped(q, 10)
    assert int(idx.get_option("group_table_builds")) == 0                                                          # ... and a one-row-per-group user pays nothing
    s_all = nfo.scores(q, x16[:N_BASE])
    for _ in range(2):
        got = idx.search_group_members(q, 10, 3)
        agrees(sh, got, gmo.members_from_scores(s_all, first, 10, 3), COS, "first ids", q=q, scores_all=s_all)
    assert int(idx.get_option("group_table_builds")) == 1
    assert int(idx.get_option("group_fill_rows_last")) == int(sum(gmo.table_sizes(first)[int(g)] for g in got[2].ravel()))      # every member of every winning group was scored
    second = patterns(N_BASE)["sized"]
    idx.set_groups(second)
    got = idx.search_group_members(q, 10, 3)
    agrees(sh, got, gmo.members_from_scores(s_all, second, 10, 3), COS, "second ids", q=q, scores_all=s_all)
    assert int(idx.get_option("group_table_builds")) == 2
    idx.add_f16(x16[N_BASE:])                                              # beyond the capacity: the rows move, the table stays
    grown = np.concatenate([second, np.full(5000, NONE, np.int64)])
    s_all = nfo.scores(q, x16)
    got = idx.search_group_members(q, 10, 3)
    agrees(sh, got, gmo.members_from_scores(s_all, grown, 10, 3), COS, "after the append", q=q, scores_all=s_all)
    assert got[1][4:, 0, 0].tolist() == list(range(N_BASE + 10, N_BASE + 14)) and (got[3][4:, 0] == 1).all() and (got[2][4:, 0] == NONE).all()
    assert int(idx.get_option("group_table_builds")) == 2, "rows appended after the build are groups of their own and cause no rebuild"
    grown[N_BASE + 10:N_BASE + 13] = int(second[0])                        # a sub-range joins an existing group: the table follows
    idx.set_groups(grown[N_BASE + 10:N_BASE + 13], N_BASE + 10)
    got = idx.search_group_members(q, 10, 3)
    agrees(sh, got, gmo.members_from_scores(s_all, grown, 10, 3), COS, "after the sub-range", q=q, scores_all=s_all)
    assert int(idx.get_option("group_table_builds")) == 3
    idx.close()


# ---- 6. the pure fill -----------------------------------------------------------------------------------------------------------------
def test_the_pure_fill_over_hand_made_winner_lists(wide):
    import torch
    groups = patterns(N_BASE)["sized"]
    wide.idx.set_groups(groups)
    B, k, s = 2, 6, 4
    size = gmo.table_sizes(groups)
    big = next(g for g, n in size.items() if n == 9)
    small = next(g for g, n in size.items() if n == 2)
    lone = int(np.flatnonzero(groups == small)[0])
    row_of_big = int(np.flatnonzero(groups == big)[3])
    #        a group         absent slot   an id no row carries   the same group again      a row on its own        outside the shard
    rows = [[row_of_big,     -1,           lone,                  row_of_big,               lone,                   N_BASE + 5]] * B
    ids = [[big,             big,          777_777,               big,                      NONE,                   small]] * B
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    d_wr, d_wg = torch.tensor(rows, dtype=torch.int64, device="cuda"), torch.tensor(ids, dtype=torch.int32, device="cuda")
    mask = np.ones(N_BASE, bool)
    mask[np.flatnonzero(groups == big)[::2]] = False                       # with a filter: five of the nine rows go
    flt = wide.idx.make_filter(mask)
    for metric in (COS, IP):
        for f, in_play in ((None, np.ones(N_BASE, bool)), (flt, mask)):
            o_s = torch.full((B, k, s), 7.0, dtype=torch.float32, device="cuda")
            o_r = torch.full((B, k, s), 7, dtype=torch.int64, device="cuda")
            o_c = torch.full((B, k), 7, dtype=torch.int32, device="cuda")
            o_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            calls = int(wide.idx.get_option("group_fill_calls"))
            wide.idx.group_fill_device(d_q, B, k, s, metric, d_wr, d_wg, o_s, o_r, o_c, o_st, row_filter=f)
            torch.cuda.synchronize()
            gs, gr, gc, gst = o_s.cpu().numpy(), o_r.cpu().numpy(), o_c.cpu().numpy(), o_st.cpu().numpy()
            assert int(wide.idx.get_option("group_fill_calls")) == calls + 1 and not gst.any()
            s_all = wide.scores(metric)
            for b in range(B):
                members = np.flatnonzero((groups == big) & in_play)
                order = members[np.lexsort((members, -s_all[b, members].astype(np.float64)))][:s]
                for j in (0, 3):
                    assert gc[b, j] == len(order) and gr[b, j, :len(order)].tolist() == order.tolist() and (gr[b, j, len(order):] == -1).all()
                assert gc[b, [1, 2, 5]].tolist() == [0, 0, 0] and (gr[b, [1, 2, 5]] == -1).all() and not gs[b, [1, 2, 5]].any()
                assert gc[b, 4] == 1 and gr[b, 4].tolist() == [lone, -1, -1, -1]
            sr = wide.idx.score_rows(wide.q[:B], gr.reshape(B, k * s), metric)
            assert np.array_equal(gs.reshape(B, k * s).view(np.uint32), sr.view(np.uint32))
            assert int(wide.idx.get_option("group_fill_rows_last")) == B * (2 * int(((groups == big) & in_play).sum()) + 1)
    flt.close()
    wide.idx.set_groups(np.full(N_BASE, NONE))


# ---- 7. stream order, timing ---------------------------------------------------------------------------------------------------------
def test_the_fill_runs_in_stream_order_behind_the_search_on_a_stream(wide):
    import torch
    B, k, s = 64, 10, 3
    groups = patterns(N_BASE)["runs8"]
    wide.idx.set_groups(groups)
    st = torch.cuda.Stream()
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    w_s = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    w_r = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    w_g = torch.full((B, k), 7, dtype=torch.int32, device="cuda")
    w_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    o_s = torch.full((B, k, s), 7.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((B, k, s), 7, dtype=torch.int64, device="cuda")
    o_c = torch.full((B, k), 7, dtype=torch.int32, device="cuda")
    o_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    want = wide.want(groups, k, s, B=B)
    try:
        wide.idx.search_grouped_device(d_q, B, k, COS, w_s, w_r, w_g, None, w_st, st.cuda_stream)
        wide.idx.group_fill_device(d_q, B, k, s, COS, w_r, w_g, o_s, o_r, o_c, o_st, st.cuda_stream)      # no host synchronisation in between
        st.synchronize()
        assert not w_st.cpu().numpy().any() and not o_st.cpu().numpy().any()
        agrees(wide, (o_s.cpu().numpy(), o_r.cpu().numpy(), w_g.cpu().numpy(), o_c.cpu().numpy()), want, COS, "fill behind the grouped search")
        t0 = wide.idx.timing()
        bufs = members_dev(wide.idx, wide.q[:B], k, s, stream=st.cuda_stream)                                 # the one-call form, same stream
        st.synchronize()
        got = host(bufs)
        assert not got[4].any()
        agrees(wide, got, want, COS, "device form on a stream")
        t1 = wide.idx.timing()
        assert t1["searches"] == t0["searches"] + 1 and t1["queries"] == t0["queries"] + B                   # counted as a search, as a grouped call is
        assert members_fixup(wide.idx, bufs, k, s, stream=st.cuda_stream) == 0
    finally:
        wide.idx.stream_release(st.cuda_stream)
        wide.idx.set_groups(np.full(N_BASE, NONE))


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(wide):
    import torch
    lib = nat.load_library()
    B, k, s = 2, 4, 3
    P = nat._ptr
    h = wide.idx._h
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    o_s = torch.zeros((B, k, s), dtype=torch.float32, device="cuda")
    o_r = torch.zeros((B, k, s), dtype=torch.int64, device="cuda")
    o_g = torch.zeros((B, k), dtype=torch.int32, device="cuda")
    o_c = torch.zeros((B, k), dtype=torch.int32, device="cuda")
    o_st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    w_r = torch.zeros((B, k), dtype=torch.int64, device="cuda")
    EINVAL, EUNSUP = -1, -6

    def dev(fn, idx_h=h, f=None, q_=d_q, B=B, k=k, s=s, metric=COS, os_=o_s, or_=o_r, og=o_g, oc=o_c, st=o_st):
        return fn(idx_h, f, P(q_), B, k, s, metric, P(os_), P(or_), P(og), P(oc), P(st), None)
    bad_args = (dict(idx_h=None), dict(q_=None), dict(os_=None), dict(or_=None), dict(og=None), dict(oc=None), dict(st=None), dict(B=0), dict(B=65536), dict(k=0),
                dict(s=0), dict(k=-1), dict(s=-2), dict(k=nat.MAX_K + 1), dict(k=342, s=3), dict(k=2 ** 16, s=2 ** 16), dict(metric=2), dict(metric=-1))
    for fn in (lib.rq_search_group_members_device, lib.rq_search_group_members_fixup_device):
        assert dev(fn) >= 0                                                          # (the fixup returns how many it repaired)
        for bad in bad_args:
            assert dev(fn, **bad) == EINVAL, (fn.__name__, bad)

    def fill(idx_h=h, f=None, q_=d_q, B=B, k=k, s=s, metric=COS, wr=w_r, wg=o_g, os_=o_s, or_=o_r, oc=o_c, st=o_st):
        return lib.rq_group_fill_device(idx_h, f, P(q_), B, k, s, metric, P(wr), P(wg), P(os_), P(or_), P(oc), P(st), None)
    assert fill() == 0
    for bad in (dict(idx_h=None), dict(q_=None), dict(wr=None), dict(wg=None), dict(os_=None), dict(or_=None), dict(oc=None), dict(st=None), dict(B=0), dict(k=0), dict(s=0),
                dict(k=342, s=3), dict(metric=7)):
        assert fill(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    q = np.ascontiguousarray(wide.q[:B])
    hs, hr, hg, hc = np.zeros((B, k, s), np.float32), np.zeros((B, k, s), np.int64), np.zeros((B, k), np.int32), np.zeros((B, k), np.int32)

    def srch(idx_h=h, f=None, q_=q, B=B, k=k, s=s, metric=COS, hs_=hs, hr_=hr, hg_=hg, hc_=hc):
        return lib.rq_search_group_members(idx_h, f, P(q_), B, k, s, metric, P(hs_), P(hr_), P(hg_), P(hc_))
    assert srch() == 0
    for bad in (dict(idx_h=None), dict(q_=None), dict(hs_=None), dict(hr_=None), dict(hg_=None), dict(hc_=None), dict(B=0), dict(k=0), dict(s=0), dict(k=1025, s=1),
                dict(k=1, s=1025), dict(metric=7)):
        assert srch(**bad) == EINVAL, bad
    other = nat.NativeIndex(768, 0)
    other.add_f16(wide.x16[:300])
    flt = other.make_filter(np.arange(0, 300, 3))
    assert srch(f=flt._h) == EINVAL and "another index" in nat.last_error()
    assert fill(f=flt._h) == EINVAL and dev(lib.rq_search_group_members_device, f=flt._h) == EINVAL
    flt.close(); other.close()
    for name in ("group_table_builds", "group_fill_calls", "group_fill_repaired", "group_fill_rows_last"):
        with pytest.raises(nat.RqError):
            wide.idx.set_option(name, 1)                                             # read-only
    with pytest.raises(nat.RqError):
        wide.idx.set_option("group_fill_cap", FILL_MAX + 1)                          # the hook can only lower the maximum
    multi = nat.NativeIndex(768, devices=[0, 0])                                     # the same GPU named twice
    multi.add_f16(wide.x16[:300])
    for rc in (dev(lib.rq_search_group_members_device, idx_h=multi._h), dev(lib.rq_search_group_members_fixup_device, idx_h=multi._h), fill(idx_h=multi._h),
               srch(idx_h=multi._h)):
        assert rc == EUNSUP and "RQ_EUNSUPPORTED" in nat.last_error()
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_group_members(q, 2, 2)
    multi.close()
    empty = nat.NativeIndex(768, 0)
    es, er, eg, ec = empty.search_group_members(q, 3, 2)                             # no rows: padding
    assert (er == -1).all() and not es.any() and (eg == NONE).all() and not ec.any()
    empty.close()


# ---- 9. the Python surface --------------------------------------------------------------------------------------------------------------
def test_dense_index_and_hybrid_retriever_return_two_passages_per_title(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    topics = ["solar panels", "wind turbines", "river dams", "coal plants", "gas pipelines", "nuclear reactors", "tidal barrages"]
    texts = [f"report {i} on {topics[i % 7]} in region {i % 13} covering output {i * 31 % 101} and cost {i * 17 % 53}" for i in range(210)]
    titles = [topics[i % 7] for i in range(210)]                                       # seven articles of thirty passages
    titles[5] = ""                                                                     # a passage without a title: its own group
    docs = [si.Document(id=f"p{i}", text=t, title=ti) for i, (t, ti) in enumerate(zip(texts, titles))]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs)
    emb = HashEmbedder()
    x16 = orc.prepare_rows_f32(emb.embed(texts), True)
    ids = [d.id for d in docs]
    table = {}
    groups = np.array([NONE if not t else table.setdefault(t, len(table)) for t in titles], np.int64)
    for qtext in ("report on solar panels in region 3 covering output 93", "cost of wind turbines in region 8"):
        qv = emb.embed([qtext])
        s_all = orc.exact_scores(qv, x16)
        ws, wr, wg, wc = gmo.members_from_scores(s_all, groups, 5, 2)
        got = r.dense_index.search(qtext, 5, distinct_by="title", per_group=2)
        assert [d for d, _, _ in got] == [ids[i] for j in range(5) for i in wr[0, j, :wc[0, j]]]
        np.testing.assert_allclose([sc for _, sc, _ in got], [v for j in range(5) for v in ws[0, j, :wc[0, j]]], atol=SCORE_TOL)
        got_titles = [titles[int(d[1:])] or d for d, _, _ in got]
        assert len(set(got_titles)) == 5 and all(got_titles.count(t) <= 2 for t in got_titles) and 5 < len(got) <= 10
        assert r.dense_index.search_batch([qtext, "coal"], 5, distinct_by="title", per_group=2)[0] == got
        assert r.dense_search(qtext, 5, distinct_by="title", per_group=2) == [(d, sc) for d, sc, _ in got]
        one = r.dense_index.search(qtext, 5, distinct_by="title")
        assert [g for i, g in enumerate(got) if i == 0 or got_titles[i - 1] != got_titles[i]] == one == r.dense_index.search(qtext, 5, distinct_by="title", per_group=1)
        assert len(r.dense_index.search(qtext, 50, distinct_by="title", per_group=2)) == 7 * 2 + 1      # every article twice and the untitled passage: no padding
        allowed = ids[::2]
        mask = np.zeros(210, dtype=bool)
        mask[::2] = True
        fs, fr, fg, fc = gmo.members_from_scores(s_all, groups, 5, 2, mask)
        got = r.dense_index.search(qtext, 5, allowed_ids=allowed, distinct_by="title", per_group=2)
        assert [d for d, _, _ in got] == [ids[i] for j in range(5) for i in fr[0, j, :fc[0, j]]]
        with pytest.raises(ValueError):
            r.hybrid_search(qtext, 4, 30, distinct_by="title", per_group=2)
        with pytest.raises(ValueError):
            r.dense_index.search(qtext, 5, per_group=2)
    assert int(r.dense_index._index.get_option("group_fill_calls")) > 0 and int(r.dense_index._index.get_option("group_table_builds")) == 1
