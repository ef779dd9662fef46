"""Grouped searches on the MI355X (include/rq.h "grouped searches", csrc/rq_group.hip): rows and group ids equal the
oracle's (tests/group_oracle.py: the collapse of the FULL exact ranking of oracle/dense_oracle.py), scores agree to SCORE_TOL
(the bar of tests/test_gpu_parity.py: 1e-6, times the largest |score| for the inner product); a pure collapse passes its candidates'
scores through bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import group_oracle as gro  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
NONE = nat.GROUP_NONE
N_BASE = 4101                      # 65 bins, a ragged last bin
NQ = 70
BIG_ID = 2 ** 31 - 1


class Shape:
    """One index with its rows, NQ queries and their canonical score matrix per metric (computed once, shared, never changed)."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, nq=NQ, options=(("scan8", 0),), row_offset=0, x16=None):
        self.n, self.dim, self.row_offset = n, dim, row_offset
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed) if x16 is None else x16
        self.q = orc.synthetic_queries(nq, dim, seed=seed + 1)
        self.idx = nat.NativeIndex(dim, 0)
        for name, v in options:
            self.idx.set_option(name, v)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self._scores = {}

    def scores(self, metric=COS):
        if metric not in self._scores:
            s = orc.exact_scores(self.q, self.x16, metric)
            s.setflags(write=False)
            self._scores[metric] = s
        return self._scores[metric]

    def want(self, groups, k, metric=COS, B=16, mask=None):
        return gro.grouped_from_scores(self.scores(metric)[:B], groups, k, mask, self.row_offset)

    def close(self):
        self.idx.close()


def agrees(got, want, scores_all, what=""):
    """(scores, rows, groups) of a grouped call against the oracle's: rows and ids identical, scores within the parity bar."""
    gs, gr, gg = got[:3]
    ws, wr, wg = want
    assert np.array_equal(gr, wr), f"{what}: rows differ\n{gr[:2]}\n{wr[:2]}"
    assert np.array_equal(gg, wg), f"{what}: group ids differ"
    tol = SCORE_TOL * max(1.0, float(np.abs(scores_all).max()))
    err = float(np.abs(gs.astype(np.float64) - ws.astype(np.float64)).max(initial=0.0))
    print(f"{what}: largest score difference {err} (bar {tol})")
    assert err <= tol, f"{what}: scores differ by {err}"


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
def big():
    sh = Shape(n=20_000, seed=77, nq=16)
    yield sh
    sh.close()


def patterns(n, seed=3):
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, max(n // 6, 2), size=n).astype(np.int64)
    rand[rng.random(n) < 0.1] = NONE
    rand[0], rand[1], rand[n - 1] = 0, BIG_ID, BIG_ID
    return {"none": np.full(n, NONE, np.int64), "one": np.full(n, 5, np.int64), "runs8": np.arange(n, dtype=np.int64) // 8, "random": rand}


# ---- 1. the pure collapse ---------------------------------------------------------------------------------------------------
def collapse_dev(idx, cs, cr, cg, k, stream=0, want_keys=True):
    """One rq_group_collapse_device call over host candidates [B][m] -> (scores, rows, groups, status, keys) on the host."""
    import torch
    B, m = cr.shape
    d_r = torch.from_numpy(np.ascontiguousarray(cr, np.int64)).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(cs, np.float32)).cuda()
    d_g = torch.from_numpy(np.ascontiguousarray(cg, np.int32)).cuda() if cg is not None else None
    o_s = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    o_g = torch.full((B, k), 7, dtype=torch.int32, device="cuda")
    o_k = torch.full((B, k), 7, dtype=torch.int64, device="cuda") if want_keys else None
    o_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.group_collapse_device(d_r, d_s, d_g, B, m, k, o_s, o_r, o_g, o_k, o_st, stream)
    torch.cuda.synchronize()
    return o_s.cpu().numpy(), o_r.cpu().numpy(), o_g.cpu().numpy(), o_st.cpu().numpy(), (o_k.cpu().numpy().view(np.uint64) if want_keys else None)


def host_keys(scores, rows):
    from rag_uq_amd import distributed as d
    return np.where(rows >= 0, d.pack_keys(scores.reshape(-1), rows.reshape(-1)).reshape(rows.shape), np.uint64(0))


@pytest.fixture(scope="module")
def looked_up():
    """N_BASE rows whose index carries the "random" pattern."""
    sh = Shape(seed=91)
    sh.groups = patterns(N_BASE)["random"]
    sh.idx.set_groups(sh.groups)
    yield sh
    sh.close()


@pytest.mark.parametrize("B", [1, 16, 70])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1024])
def test_pure_collapse_equals_the_oracle(looked_up, m, B):
    sh = looked_up
    rng = np.random.default_rng(1000 * m + B)
    for metric in (COS, IP):
        s_all = sh.scores(metric)[:B]
        half = max(m // 2, 1)
        top = orc.topk_from_scores(s_all, half)[1]                            # half of the candidates: the query's best rows; the rest: any others
        cr = np.stack([rng.permutation(np.concatenate([top[b], rng.choice(np.setdiff1d(np.arange(N_BASE), top[b]), size=m - half, replace=False)]))
                       for b in range(B)]).astype(np.int64)                   # unsorted, distinct
        cs = np.where(cr >= 0, np.take_along_axis(s_all, np.maximum(cr, 0), axis=1), 0.0).astype(np.float32)
        if m >= 63:                                                           # absent entries of every kind, between present ones
            cr[:, 3] = -1; cr[:, 17] = N_BASE; cr[:, 29] = 2 ** 40; cs[:, 41] = np.nan
            cs[:, 50] = -0.0                                                  # and a -0.0, which ranks with and leaves as +0.0
        explicit = rng.integers(0, max(m // 4, 2), size=(B, m)).astype(np.int64)
        explicit[rng.random((B, m)) < 0.15] = NONE
        explicit[:, 0] = 0
        explicit[:, m - 1] = BIG_ID
        if m > 2:
            explicit[:, m // 2] = BIG_ID
        for k in sorted({1, min(10, m), m}):
            for cg, what in ((explicit, "explicit"), (None, "looked up")):
                g_in = explicit if cg is not None else gro.lookup_groups(cr, sh.groups)
                ws, wr, wg, wst = gro.collapse_batch(cs, cr, g_in, k, N_BASE)
                gs, gr, gg, gst, gk = collapse_dev(sh.idx, cs, cr, cg, k)
                tag = f"m={m} B={B} k={k} metric={metric} {what}"
                assert np.array_equal(gr, wr), tag
                assert np.array_equal(gg, wg), tag
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{tag}: scores are passed through bit for bit"
                assert np.array_equal(gst, wst), f"{tag}: status"
                assert np.array_equal(gk, host_keys(ws, wr)), f"{tag}: keys"
    assert collapse_dev(sh.idx, cs, cr, None, 1, want_keys=False)[4] is None                                  # d_keys may be NULL


# ---- 2. group patterns ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["none", "one", "runs8", "random"])
def test_group_patterns_equal_the_oracle(wide, pattern):
    groups = patterns(N_BASE)[pattern]
    wide.idx.set_groups(groups)
    q = wide.q[:16]
    for metric in (COS, IP):
        got = wide.idx.search_grouped(q, 10, metric)
        agrees(got, wide.want(groups, 10, metric), wide.scores(metric), f"{pattern} metric {metric}")
        if pattern == "none":
            ps, pr = wide.idx.search(q, 10, metric)
            assert np.array_equal(got[1], pr) and np.array_equal(got[0].view(np.uint32), ps.view(np.uint32)) and (got[2] == NONE).all()
        if pattern == "one":
            assert (got[1][:, 1:] == -1).all() and (got[2][:, 0] == 5).all() and (got[2][:, 1:] == NONE).all() and not got[0][:, 1:].any()
    wide.idx.set_groups(np.full(N_BASE, NONE))


@pytest.mark.parametrize("shape", ["narrow", "dim33", "big"])
@pytest.mark.parametrize("pattern", ["runs8", "random"])
def test_group_patterns_on_the_narrow_layout_and_a_larger_index(request, shape, pattern):
    sh = request.getfixturevalue(shape)
    groups = patterns(sh.n)[pattern]
    sh.idx.set_groups(groups)
    for k in (1, 10, 100):
        agrees(sh.idx.search_grouped(sh.q[:16], k), sh.want(groups, k), sh.scores(), f"{shape} {pattern} k={k}")


def test_duplicate_stored_rows_inside_one_group_and_across_groups():
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=5)
    x16[100] = x16[7]                                      # a pair inside ONE group: the tie goes by row
    x16[200] = x16[3000] = x16[9]                          # a triple in DIFFERENT groups: all three are winners, in row order
    sh = Shape(x16=x16, seed=5)
    groups = np.arange(N_BASE, dtype=np.int64) // 8 + 1000
    groups[100] = groups[7]
    assert len({int(groups[9]), int(groups[200]), int(groups[3000])}) == 3
    sh.idx.set_groups(groups)
    q = np.stack([x16[7].astype(np.float32) + sh.q[0] / np.linalg.norm(sh.q[0]), x16[9].astype(np.float32) + sh.q[1] / np.linalg.norm(sh.q[1])])
    s_all = orc.exact_scores(q, x16)
    got = sh.idx.search_grouped(q, 10)
    agrees(got, gro.grouped_from_scores(s_all, groups, 10), s_all, "duplicates")
    assert got[1][0, 0] == 7 and 100 not in got[1][0]
    assert got[1][1, :3].tolist() == [9, 200, 3000] and got[0][1, 0] == got[0][1, 1] == got[0][1, 2]
    sh.close()


# ---- 3. further cases ---------------------------------------------------------------------------------------------------------------
def test_small_index_equals_the_host_collapse_of_the_full_search_bit_for_bit():
    sh = Shape(n=1000, seed=9, nq=16)
    groups = patterns(1000)["random"]
    sh.idx.set_groups(groups)
    for metric in (COS, IP):
        fs, fr = sh.idx.search(sh.q, 1000, metric)
        for k in (1, 10, 400):
            ws, wr, wg, _ = gro.collapse_batch(fs, fr, gro.lookup_groups(fr, groups), k, 1000)
            gs, gr, gg = sh.idx.search_grouped(sh.q, k, metric)
            assert np.array_equal(gr, wr) and np.array_equal(gg, wg) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (metric, k)
    sh.close()


def test_scores_have_the_bits_of_score_rows(wide):
    groups = patterns(N_BASE)["runs8"]
    wide.idx.set_groups(groups)
    for metric in (COS, IP):
        gs, gr, gg = wide.idx.search_grouped(wide.q[:16], 33, metric)
        assert (gr >= 0).all()
        assert np.array_equal(gs.view(np.uint32), wide.idx.score_rows(wide.q[:16], gr, metric).view(np.uint32))
    wide.idx.set_groups(np.full(N_BASE, NONE))


def test_a_zero_norm_query_returns_the_lowest_row_of_the_first_groups(wide):
    groups = patterns(N_BASE)["random"]
    groups[:40] = np.repeat(np.arange(10), 4) + 50                     # the first 40 rows: ten groups of four
    wide.idx.set_groups(groups)
    q = np.stack([np.zeros(768, np.float32), wide.q[0]])
    for metric in (COS, IP):
        gs, gr, gg = wide.idx.search_grouped(q, 12, metric)
        ws, wr, wg = gro.grouped_from_scores(np.stack([np.zeros(N_BASE, np.float32), wide.scores(metric)[0]]), groups, 12)
        assert np.array_equal(gr, wr) and np.array_equal(gg, wg) and not gs[0].any()
        assert gr[0, :10].tolist() == list(range(0, 40, 4))
    wide.idx.set_groups(np.full(N_BASE, NONE))


def test_row_offset_global_rows_come_out():
    sh = Shape(n=1000, seed=9, nq=8, row_offset=10 ** 6)
    groups = patterns(1000)["runs8"]
    sh.idx.set_groups(groups)
    got = sh.idx.search_grouped(sh.q, 10)
    assert got[1].min() >= 10 ** 6
    agrees(got, sh.want(groups, 10, B=8), sh.scores(), "row_offset")
    assert np.array_equal(sh.idx.get_groups(), groups.astype(np.int32))      # (set and read back by LOCAL row)
    sh.close()


# ---- 4. with a filter ---------------------------------------------------------------------------------------------------------------
def test_every_filter_route_gives_the_oracle_and_a_stale_filter_is_refused():
    sh = Shape(seed=13, nq=16)
    groups = patterns(N_BASE)["runs8"]
    sh.idx.set_groups(groups)
    masks = fo.standard_masks(N_BASE)
    for name in ("random50", "rotation", "five_rows", "none"):
        flt = sh.idx.make_filter(masks[name])
        want = sh.want(groups, 10, mask=masks[name])
        results = []
        for route in (-1, 1, 2, 3):
            sh.idx.set_option("filter_route", route)
            got = sh.idx.search_grouped(sh.q, 10, row_filter=flt)
            agrees(got, want, sh.scores(), f"{name} route {route}")
            results.append(got)
        for got in results[1:]:
            assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                       for a, b in zip(got, results[0])), f"{name}: the routes differ"
        flt.close()
    sh.idx.set_option("filter_route", -1)
    flt = sh.idx.make_filter(masks["random50"])
    sh.idx.add_f16(sh.x16[:10])
    with pytest.raises(nat.RqError, match="stale filter"):
        sh.idx.search_grouped(sh.q, 10, row_filter=flt)
    flt.close()
    sh.close()


# ---- 5. repair -----------------------------------------------------------------------------------------------------------------------
def grouped_dev(idx, q, k, metric=COS, stream=0, row_filter=None):
    import torch
    B = q.shape[0]
    bufs = {"q": torch.from_numpy(np.ascontiguousarray(q)).cuda(), "s": torch.full((B, k), 7.0, dtype=torch.float32, device="cuda"),
            "r": torch.full((B, k), 7, dtype=torch.int64, device="cuda"), "g": torch.full((B, k), 7, dtype=torch.int32, device="cuda"),
            "k": torch.full((B, k), 7, dtype=torch.int64, device="cuda"), "st": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    idx.search_grouped_device(bufs["q"], B, k, metric, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"], stream, row_filter=row_filter)
    return bufs


def host(bufs):
    import torch
    torch.cuda.synchronize()
    return bufs["s"].cpu().numpy(), bufs["r"].cpu().numpy(), bufs["g"].cpu().numpy(), bufs["st"].cpu().numpy(), bufs["k"].cpu().numpy().view(np.uint64)


def test_repair_one_group_owns_the_best_rows_of_one_query():
    sh = Shape(seed=29, nq=16)
    B, k, bad = 16, 5, 3
    sh.idx.set_option("group_fetch_cap", 64)
    groups = np.full(N_BASE, NONE, np.int64)
    groups[orc.topk_from_scores(sh.scores()[bad:bad + 1], 200)[1][0]] = 7          # one group owns the 200 best rows of query 3
    sh.idx.set_groups(groups)
    m1 = min(int(sh.idx.get_option("group_fetch")) * k, 64)
    top_s, top_r = orc.topk_from_scores(sh.scores()[:B], m1)
    flagged = gro.collapse_batch(top_s, top_r, gro.lookup_groups(top_r, groups), k, N_BASE)[3]
    assert flagged.tolist() == [1 if b == bad else 0 for b in range(B)]                  # the precondition, on the oracle alone
    want = sh.want(groups, k, B=B)
    before = {o: int(sh.idx.get_option(o)) for o in ("group_repaired", "group_rounds_last", "repaired_queries")}
    bufs = grouped_dev(sh.idx, sh.q[:B], k)
    first = host(bufs)
    assert first[3].tolist() == flagged.tolist(), "the device form flags exactly that query"
    ok = np.arange(B) != bad
    agrees([a[ok] for a in first[:3]], [w[ok] for w in want], sh.scores(), "unflagged queries before the repair")
    assert first[1][bad, 0] == want[1][bad, 0] and (first[1][bad, 1:] == -1).all()      # what the list proves: the best group
    n = sh.idx.search_grouped_fixup_device(bufs["q"], B, k, COS, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"])
    assert n == 1
    after = host(bufs)
    assert not after[3].any()
    agrees(after, want, sh.scores(), "after the repair")
    for a, b in zip(first, after):
        assert np.array_equal(a[ok].view(np.uint8), b[ok].view(np.uint8)), "the unflagged queries are untouched"
    assert np.array_equal(after[4], host_keys(after[0], after[1]))
    assert int(sh.idx.get_option("group_repaired")) == before["group_repaired"] + 1
    assert int(sh.idx.get_option("group_rounds_last")) == 1
    assert sh.idx.search_grouped_fixup_device(bufs["q"], B, k, COS, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"]) == 0
    # the same through the blocking form, and with the cap lifted (rung 2 alone then holds five groups)
    agrees(sh.idx.search_grouped(sh.q[:B], k), want, sh.scores(), "blocking form")
    assert int(sh.idx.get_option("group_repaired")) == before["group_repaired"] + 2
    sh.idx.set_option("group_fetch_cap", 0)
    agrees(sh.idx.search_grouped(sh.q[:B], k), want, sh.scores(), "blocking form, no cap")
    assert int(sh.idx.get_option("group_repaired")) == before["group_repaired"] + 3 and int(sh.idx.get_option("group_rounds_last")) == 0
    sh.close()


def test_repair_takes_as_many_exclusion_rounds_as_the_groups_need():
    sh = Shape(seed=31, nq=4)
    sh.idx.set_option("group_fetch_cap", 64)
    groups = np.full(N_BASE, NONE, np.int64)
    ranked = orc.topk_from_scores(sh.scores()[:1], 600)[1][0]
    groups[ranked] = np.arange(600) // 50 + 40                            # query 0: its best 600 rows in twelve groups of 50, by rank
    sh.idx.set_groups(groups)
    want = sh.want(groups, 10, B=1)
    assert want[2][0].tolist() == list(range(40, 50))
    agrees(sh.idx.search_grouped(sh.q[:1], 10), want, sh.scores(), "rounds")
    # rung 2 sees 64 rows = groups 40, 41; every round then sees the next 64 rows in play = two more groups: four rounds to ten
    assert int(sh.idx.get_option("group_rounds_last")) == 4
    flt = sh.idx.make_filter(np.arange(N_BASE) % 2 == 0)                  # ... and within a filter
    got = sh.idx.search_grouped(sh.q[:1], 10, row_filter=flt)
    agrees(got, sh.want(groups, 10, B=1, mask=np.arange(N_BASE) % 2 == 0), sh.scores(), "rounds, filtered")
    flt.close()
    sh.close()


@pytest.fixture(scope="module")
def small():
    sh = Shape(n=2000, seed=57)                                           # 32 bins, the last one ragged
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
    """rq_search_grouped_device without a fixup, then on the device: status 1 for a chosen subset and garbage over those queries'
    outputs, then the fixup form.  Groups of four consecutive rows, k = 3: rung 2 alone answers (no exclusion round).  It returns the
    size of the subset, the flagged queries equal the oracle, every other query keeps the first call's bits, every status is 0 and
    "group_repaired" rose by the size of the subset."""
    import torch
    sh = request.getfixturevalue(shape)
    k = 3
    groups = np.arange(sh.n, dtype=np.int64) // 4
    sh.idx.set_groups(groups)
    want = sh.want(groups, k, metric, B=B)
    what = f"by hand: {shape}, metric {metric}, B {B}"
    bufs = grouped_dev(sh.idx, sh.q[:B], k, metric)
    first = host(bufs)
    assert not first[3].any(), f"{what}: the first call flagged {np.nonzero(first[3])[0].tolist()} itself"
    sel = torch.tensor(flagged, device="cuda")
    bufs["st"][sel] = 1
    bufs["s"][sel] = float("nan")
    bufs["r"][sel] = -7
    bufs["g"][sel] = -7
    bufs["k"][sel] = -1                                                   # all ones
    before = int(sh.idx.get_option("group_repaired"))
    n = sh.idx.search_grouped_fixup_device(bufs["q"], B, k, metric, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"])
    after = host(bufs)
    assert n == len(flagged), f"{what}: the fixup returned {n}"
    assert not after[3].any(), f"{what}: status after the fixup {after[3].tolist()}"
    agrees([a[flagged] for a in after[:3]], [w[flagged] for w in want], sh.scores(metric), f"{what}, flagged queries")
    assert np.array_equal(after[4][flagged], host_keys(after[0][flagged], after[1][flagged])), f"{what}: keys of the flagged queries"
    other = np.setdiff1d(np.arange(B), flagged)
    for a, b in zip(first, after):
        assert np.array_equal(a[other].view(np.uint8), b[other].view(np.uint8)), f"{what}: an unflagged query changed"
    assert int(sh.idx.get_option("group_repaired")) == before + len(flagged) and int(sh.idx.get_option("group_rounds_last")) == 0, what


# ---- 6. storage --------------------------------------------------------------------------------------------------------------------
def test_rows_appended_after_set_groups_are_their_own_groups_and_sub_ranges_read_back():
    x16 = orc.synthetic_corpus(9101, 768, seed=41)
    q = orc.synthetic_queries(8, 768, seed=42)
    idx = nat.NativeIndex(768, 0)
    idx.set_option("scan8", 0)
    idx.add_f16(x16[:N_BASE])
    assert (idx.get_groups() == NONE).all()                                # nothing set yet
    groups = np.full(9101, NONE, np.int64)
    groups[:N_BASE] = np.arange(N_BASE) // 8
    idx.set_groups(groups[:N_BASE])
    idx.add_f16(x16[N_BASE:])                                              # beyond the capacity of 8192 rows: the ids follow the rows
    assert np.array_equal(idx.get_groups(), groups.astype(np.int32))
    s_all = orc.exact_scores(q, x16)
    agrees(idx.search_grouped(q, 20), gro.grouped_from_scores(s_all, groups, 20), s_all, "after the append")
    groups[5000:5100] = 3                                                  # a sub-range, joining an existing group
    idx.set_groups(groups[5000:5100], 5000)
    assert np.array_equal(idx.get_groups(4990, 120), groups[4990:5110].astype(np.int32))
    agrees(idx.search_grouped(q, 20), gro.grouped_from_scores(s_all, groups, 20), s_all, "after the sub-range")
    idx.reserve(20_000)
    assert np.array_equal(idx.get_groups(), groups.astype(np.int32))
    with pytest.raises(nat.RqError):
        idx.set_groups(np.zeros(10, np.int32), 9100)                       # reaches beyond the stored rows
    with pytest.raises(nat.RqError):
        idx.get_groups(9000, 200)
    idx.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(wide):
    import torch
    lib = nat.load_library()
    B, m, k = 2, 16, 4
    P = nat._ptr
    h = wide.idx._h
    top_s, top_r = orc.topk_from_scores(wide.scores()[:B], m)
    d_r, d_s = torch.from_numpy(top_r).cuda(), torch.from_numpy(top_s).cuda()
    o_s = torch.zeros((B, m), dtype=torch.float32, device="cuda")
    o_r = torch.zeros((B, m), dtype=torch.int64, device="cuda")
    o_g = torch.zeros((B, m), dtype=torch.int32, device="cuda")
    o_st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    EINVAL, EUNSUP = -1, -6

    def col(idx_h=h, cr=d_r, cs=d_s, B=B, m=m, k=k, os_=o_s, or_=o_r, og=o_g, st=o_st):
        return lib.rq_group_collapse_device(idx_h, P(cr), P(cs), None, B, m, k, P(os_), P(or_), P(og), None, P(st), None)
    before = int(wide.idx.get_option("group_calls"))
    assert col() == 0
    assert int(wide.idx.get_option("group_calls")) == before + 1
    for bad in (dict(idx_h=None), dict(cr=None), dict(cs=None), dict(os_=None), dict(or_=None), dict(og=None), dict(st=None), dict(B=0), dict(B=65536),
                dict(m=0), dict(m=nat.MAX_K + 1), dict(k=0), dict(k=m + 1)):
        assert col(**bad) == EINVAL, bad
    assert int(wide.idx.get_option("group_calls")) == before + 1

    def dev(fn, idx_h=h, f=None, q_=d_q, B=B, k=k, metric=COS, os_=o_s, or_=o_r, og=o_g, st=o_st):
        return fn(idx_h, f, P(q_), B, k, metric, P(os_), P(or_), P(og), None, P(st), None)
    for fn in (lib.rq_search_grouped_device, lib.rq_search_grouped_fixup_device):
        assert dev(fn) >= 0                                                          # (the fixup returns how many it repaired)
        for bad in (dict(idx_h=None), dict(q_=None), dict(os_=None), dict(or_=None), dict(og=None), dict(st=None), dict(B=0), dict(B=65536), dict(k=0),
                    dict(k=nat.MAX_K + 1), dict(metric=2), dict(metric=-1)):
            assert dev(fn, **bad) == EINVAL, (fn.__name__, bad)
    torch.cuda.synchronize()
    q = np.ascontiguousarray(wide.q[:B])
    hs, hr, hg = np.zeros((B, k), np.float32), np.zeros((B, k), np.int64), np.zeros((B, k), np.int32)

    def srch(idx_h=h, f=None, q_=q, B=B, k=k, metric=COS, hs_=hs, hr_=hr, hg_=hg):
        return lib.rq_search_grouped(idx_h, f, P(q_), B, k, metric, P(hs_), P(hr_), P(hg_))
    assert srch() == 0
    for bad in (dict(idx_h=None), dict(q_=None), dict(hs_=None), dict(hr_=None), dict(hg_=None), dict(B=0), dict(k=0), dict(k=nat.MAX_K + 1), dict(metric=7)):
        assert srch(**bad) == EINVAL, bad
    ids = np.zeros(4, np.int32)
    assert lib.rq_index_set_groups(h, 0, 4, None) == EINVAL and lib.rq_index_set_groups(h, -1, 4, P(ids)) == EINVAL
    assert lib.rq_index_set_groups(h, N_BASE - 3, 4, P(ids)) == EINVAL and lib.rq_index_get_groups(h, 0, N_BASE + 1, P(ids)) == EINVAL
    below = np.array([0, -2, 1, 1], np.int32)
    assert lib.rq_index_set_groups(h, 0, 4, P(below)) == EINVAL and "RQ_GROUP_NONE" in nat.last_error()
    assert (wide.idx.get_groups(0, 4) == NONE).all()                                 # a refused call writes nothing
    other = nat.NativeIndex(768, 0)
    other.add_f16(wide.x16[:300])
    flt = other.make_filter(np.arange(0, 300, 3))
    assert srch(f=flt._h) == EINVAL and "another index" in nat.last_error()
    flt.close(); other.close()
    multi = nat.NativeIndex(768, devices=[0, 0])                                     # the same GPU named twice
    multi.add_f16(wide.x16[:300])
    for rc in (col(idx_h=multi._h), dev(lib.rq_search_grouped_device, idx_h=multi._h), dev(lib.rq_search_grouped_fixup_device, idx_h=multi._h),
               srch(idx_h=multi._h), lib.rq_index_set_groups(multi._h, 0, 4, P(ids)), lib.rq_index_get_groups(multi._h, 0, 4, P(ids))):
        assert rc == EUNSUP and "RQ_EUNSUPPORTED" in nat.last_error()
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_grouped(q, 2)
    multi.close()
    empty = nat.NativeIndex(768, 0)
    s, r, g = empty.search_grouped(q, 3)                                             # no rows: padding
    assert (r == -1).all() and not s.any() and (g == NONE).all()
    empty.close()


# ---- 8. stream order, timing ---------------------------------------------------------------------------------------------------------
def test_the_collapse_runs_in_stream_order_behind_the_search(wide):
    import torch
    B, m, k = 64, 40, 10
    groups = patterns(N_BASE)["runs8"]
    wide.idx.set_groups(groups)
    st = torch.cuda.Stream()
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    c_s = torch.full((B, m), 7.0, dtype=torch.float32, device="cuda")
    c_r = torch.full((B, m), 7, dtype=torch.int64, device="cuda")
    c_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    o_s = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    o_g = torch.full((B, k), 7, dtype=torch.int32, device="cuda")
    o_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    want = gro.grouped_from_scores(wide.scores()[:B], groups, k)
    try:
        wide.idx.search_device(d_q, B, m, COS, c_s, c_r, None, c_st, st.cuda_stream)
        wide.idx.search_flush_device(st.cuda_stream)
        wide.idx.group_collapse_device(c_r, c_s, None, B, m, k, o_s, o_r, o_g, None, o_st, st.cuda_stream)      # no host synchronisation in between
        st.synchronize()
        assert not c_st.cpu().numpy().any() and not o_st.cpu().numpy().any()
        agrees((o_s.cpu().numpy(), o_r.cpu().numpy(), o_g.cpu().numpy()), want, wide.scores(), "collapse behind the search")
        t0 = wide.idx.timing()
        bufs = grouped_dev(wide.idx, wide.q[:B], k, stream=st.cuda_stream)                                        # the one-call form, same stream
        st.synchronize()
        got = host(bufs)
        assert not got[3].any()
        agrees(got, want, wide.scores(), "grouped device form on a stream")
        t1 = wide.idx.timing()
        assert t1["searches"] == t0["searches"] + 1 and t1["queries"] == t0["queries"] + B                         # a grouped call counts as a search
    finally:
        wide.idx.stream_release(st.cuda_stream)
        wide.idx.set_groups(np.full(N_BASE, NONE))


# ---- 9. the int8 image as the operand --------------------------------------------------------------------------------------------------
def test_a_shard_of_200000_rows_scans_its_int8_image():
    sh = Shape(n=200_000, seed=5, nq=8, options=())
    groups = np.arange(200_000, dtype=np.int64) // 8
    sh.idx.set_groups(groups)
    want = sh.want(groups, 10, B=8)
    # "scan8" = 1, the default: the shard is large enough for the image, and the build's own measurement says which rung each class
    # of k starts on (include/rq.h) -- possibly the fp16 rows
    agrees(sh.idx.search_grouped(sh.q, 10), want, sh.scores(), "200 000 rows, automatic rule")
    used = int(sh.idx.get_option("scan8_used"))
    print(f"automatic rule: scan8_used {used}, scan8_level {sh.idx.get_option('scan8_level')}")
    sh.idx.set_option("scan8", 2)                                          # always: the image is the operand of the m1 = 80 search
    agrees(sh.idx.search_grouped(sh.q, 10), want, sh.scores(), "200 000 rows, int8 image")
    used8 = int(sh.idx.get_option("scan8_used"))
    assert used8 > used
    agrees(sh.idx.search_grouped(sh.q, 4), sh.want(groups, 4, B=8), sh.scores(), "200 000 rows, int8 image, one-image class")      # (m1 = 32)
    assert int(sh.idx.get_option("scan8_used")) > used8
    sh.close()


# ---- 10. the Python surface --------------------------------------------------------------------------------------------------------------
def test_dense_index_and_hybrid_retriever_return_one_passage_per_title(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    topics = ["solar panels", "wind turbines", "river dams", "coal plants", "gas pipelines", "nuclear reactors", "tidal barrages"]
    texts = [f"report {i} on {topics[i % 7]} in region {i % 13} covering output {i * 31 % 101} and cost {i * 17 % 53}" for i in range(210)]
    titles = [topics[i % 7] for i in range(210)]                                       # seven articles of thirty passages
    titles[5] = ""                                                                     # a passage without a title: its own group
    docs = [si.Document(id=f"p{i}", text=t, title=ti) for i, (t, ti) in enumerate(zip(texts, titles))]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs[:150])
    emb = HashEmbedder()
    x16 = orc.prepare_rows_f32(emb.embed(texts), True)
    ids = [d.id for d in docs]
    table = {}
    groups = np.array([NONE if not t else table.setdefault(t, len(table)) for t in titles], np.int64)
    queries = ["report on solar panels in region 3 covering output 93", "cost of wind turbines in region 8"]
    for n in (150, 210):
        if n == 210:
            r.add_documents(docs[150:])                                                # only the new rows' ids are pushed
        for qtext in queries:
            qv = emb.embed([qtext])
            s_all = orc.exact_scores(qv, x16[:n])
            ws, wr, _ = gro.grouped_from_scores(s_all, groups[:n], 5)
            plain = [titles[i] for i in orc.topk_from_scores(s_all, 10)[1][0]]
            assert len(set(plain)) < 10                                                # the plain top 10 repeats a title: there are eight values
            got = r.dense_index.search(qtext, 5, distinct_by="title")
            assert [d for d, _, _ in got] == [ids[i] for i in wr[0]]
            np.testing.assert_allclose([s for _, s, _ in got], ws[0], atol=SCORE_TOL)
            got_titles = [titles[int(d[1:])] for d, _, _ in got]
            assert len(set(got_titles)) == 5
            assert r.dense_index.search_batch([qtext, queries[0]], 5, distinct_by="title")[0] == got
            assert r.dense_search(qtext, 5, distinct_by="title") == [(d, s) for d, s, _ in got]
            assert len(r.dense_index.search(qtext, 50, distinct_by="title")) == 8      # every article and the untitled passage: no padding tuples
            rows = r.dense_index.search_rows_batch([qtext], 5, distinct_by="title")[1]
            assert rows[0].tolist() == wr[0].tolist()
            allowed = ids[:n:2]
            mask = np.zeros(n, dtype=bool)
            mask[::2] = True
            fs, fr, _ = gro.grouped_from_scores(s_all, groups[:n], 5, mask)
            got = r.dense_index.search(qtext, 5, allowed_ids=allowed, distinct_by="title")
            assert [d for d, _, _ in got] == [ids[i] for i in fr[0]]
            fused = r.hybrid_search(qtext, 4, 30, distinct_by="title")
            ft = [x.title for x in fused]
            assert len(fused) == 4 and len(set(ft)) == 4
            assert [x.hybrid_score for x in fused] == sorted((x.hybrid_score for x in fused), reverse=True)
            assert r.dense_index.search(qtext, 8) == r.dense_index.search(qtext, 8, distinct_by=None)       # without the keyword: the plain search
    assert int(r.dense_index._index.get_option("group_calls")) > 0
    assert r.dense_index._index.get_groups().tolist() == groups.astype(np.int32).tolist()
    r.close()
