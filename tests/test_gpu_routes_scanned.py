"""The calls built on top of the plain search -- rq_search_mmr, rq_search_grouped*, rq_search_group_members, rq_search_filtered_each*
 -- at shapes where their fetch stage is the APPROXIMATE scan in wide passes, which the 4 101-row
shape of their own suites never reaches (65 bins: every fetch of 25 rows and more is the exact fp64 scan, 70 queries are one
128-query pass).  Oracles, score bars and helpers are those of the routes' own suites, imported, not copied.  What is new here:

  * the shapes of tests/route_shapes.py (12 805 rows / 201 bins, 49 157 rows / 769 bins, the narrow layout, the int8 image), with
    batches of 130 (one 256-query pass), 300 (256 + 64: two scan grids) and, on the narrow layout, 200 (128 + 128);
  * every test confirms the route that ran with "profile" = 1 and timing(): at least (device form before its fixup: exactly) the
    scan launches tests/route_shapes.py predicts, `exact_scans` == 0 and `widened` == 0 -- the prediction itself is pinned to
    plan_call on the host by tests/test_route_shapes.py;
  * repairs that are themselves wide calls ("eps" = 10: no certificate holds, all 130 queries come back flagged).

One fp64 score matrix per shape is shared by every test of that shape.

Seeds.  `exact_scans` == 0 and `widened` == 0 hold only while no query of a batch fails its certificate; that is a property of the
inputs, established with the plain search (idx.search(q, m), same options) for every (shape, B, m) of route_shapes.FETCHES.
Observed on an MI355X, seeds 301 / 311 / 321 (S1, S1i), 302 / 312 / 322 (S2), 303 / 313 / 323 (S1n), the first of each kept:
  S1, S1n   every (B, m): 0 queries repaired, 0 exact scans, the predicted launches, with all three seeds.
  S2        m = 330: 0 repaired.  m = 257 and 320 at B = 130: 130 of 130 repaired with all three seeds -- not the inputs but a defect
            (the fast tail behind a wide pass has 256 partition maxima to choose its threshold from), fixed in rq_plan.h
            fast_tail_fits; since then 0.
  S1i       m = 10 at B = 300: 0 repaired.  m = 64 and 80 at B = 130: 129 - 130 of 130 repaired with all three seeds, by the ladder's
            fp16 rung (no query widened, none scanned exactly): on 201 bins ONE int8 image per query does not certify a class k > 32
            call, and after a window of 256 checked queries the ladder takes the class's wide calls off the image (B = 300 then scans
            the fp16 rows).  No seed meets "at most B / 16 repaired" here; the tests start the ladder over before each call
            (Scanned.fresh_ladder), so the image is the operand of every fetch they check, and assert that `scan8_used` grows,
            `exact_scans` == 0 and `widened` == 0."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import mmr_oracle as mo  # noqa: E402
import route_shapes as rs  # noqa: E402
import test_gpu_filter_each as tfe  # noqa: E402
import test_gpu_group_members as tgm  # noqa: E402
import test_gpu_grouped as tg  # noqa: E402
import test_gpu_mmr as tm  # noqa: E402

pytestmark = pytest.mark.gpu
COS = nat.METRIC_COSINE
SCORE_TOL = 1e-6                   # the bar of every route's own suite (tests/test_gpu_parity.py)
GATHER, SCAN, EXACT, NULL_BIT = tfe.GATHER, tfe.SCAN, tfe.EXACT, tfe.NULL_BIT
# corpus seed per data set (queries: seed + 1); what the plain search showed for each: the module's docstring
SEEDS = {"S1": 301, "S2": 302, "S1n": 303}
NQ = {"S1": 300, "S2": 130, "S1n": 200}


class Scanned:
    """One shape of tests/route_shapes.py: its rows, queries, index ("profile" = 1) and the canonical score matrix, computed once,
    shared and never changed.  S1i is S1's data behind an index with "scan8" = 2."""

    def __init__(self, name, data=None):
        sh = rs.SHAPES[name]
        self.name, self.n, self.dim, self.row_offset = name, sh.rows, sh.dim, 0
        self.image = sh.scan8 == 2
        self.narrow = sh.row_pad == 384
        if data is None:
            self.x16 = orc.synthetic_corpus(sh.rows, sh.dim, seed=SEEDS[name])
            self.q = orc.synthetic_queries(NQ[name], sh.dim, seed=SEEDS[name] + 1)
            self._scores = orc.exact_scores(self.q, self.x16, COS)
            self._scores.setflags(write=False)
        else:
            self.x16, self.q, self._scores = data.x16, data.q, data._scores
        self.idx = self.new_index()
        assert self.idx.row_pad == sh.row_pad and len(self.idx) == sh.rows
        self.masks = fo.standard_masks(self.n)

    def new_index(self):
        sh = rs.SHAPES[self.name]
        idx = nat.NativeIndex(sh.dim, 0)
        idx.set_option("scan8", sh.scan8)
        idx.set_option("profile", 1)
        idx.add_f16(self.x16)
        return idx

    def fresh_ladder(self, idx=None):
        """S1i: "scan8" = 2 set again starts the int8 ladder over, so that the NEXT call scans the image whatever the calls before
        it had repaired (a window of 256 checked queries with more than 1 in 16 repaired moves a class of k off the image)."""
        if self.image:
            (self.idx if idx is None else idx).set_option("scan8", 2)

    def scores(self, metric=COS):
        assert metric == COS
        return self._scores

    def plan(self, B, m, filtered=False):
        p = rs.shape_plan(self.name, B, m, filtered)
        assert not p.exact, f"{self.name}: a fetch of {m} rows is planned exact"
        return p

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def s1():
    sh = Scanned("S1")
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def s2():
    sh = Scanned("S2")
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def s1n():
    sh = Scanned("S1n")
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def s1i(s1):
    sh = Scanned("S1i", data=s1)
    yield sh
    sh.close()


def opt(idx, name):
    return int(idx.get_option(name))


def counters(idx):
    t = idx.timing()
    return {"scan_launches": t["scan_launches"], "exact_scans": t["exact_scans"], "widened": t["widened"], "repaired_queries": opt(idx, "repaired_queries"),
            "scan8_used": opt(idx, "scan8_used")}


def ran_on_the_scan(sh, before, npass, what, exactly=False, idx=None, widened=0):
    """The counters of the index since `before`: the predicted scan launches (exactly: a device form read before its fixup), no query
    widened (but `widened`, where the inputs themselves put queries beyond a certificate) or scanned exactly; on the int8 shape the
    image was the operand."""
    idx = sh.idx if idx is None else idx
    now = counters(idx)
    d = {name: now[name] - before[name] for name in now}
    print(f"{what}: predicted passes {npass}, counters {d}")
    assert d["exact_scans"] == 0 and d["widened"] == widened, f"{what}: {d}"
    assert d["scan_launches"] == npass if exactly else d["scan_launches"] >= npass, f"{what}: {d['scan_launches']} scan launches, predicted {npass}"
    if sh.image:
        assert d["scan8_used"] > 0 and idx.get_option("scan8_row_err") >= 0, f"{what}: the int8 image was not scanned ({d})"
    else:
        assert d["scan8_used"] == 0
    return d


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b, what):
    assert len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), f"{what}: not bit for bit"


# ---- 1. MMR on the scan ----------------------------------------------------------------------------------------------------------
def mmr_end_to_end(sh, B, k, fetch_k, lam, mask=None, flt=None, what=""):
    """tests/test_gpu_mmr.py _end_to_end over the shape's shared score matrix: the returned relevances are the oracle's candidates'
    within SCORE_TOL, every step's pick is the oracle's from the same state (follows_oracle), the rows equal mmr_oracle's."""
    q = sh.q[:B]
    m = max(k, min(fetch_k, sh.n if mask is None else int(mask.sum())))
    if mask is None:
        rel, rows = orc.topk_from_scores(sh.scores()[:B], m)
    else:
        rel, rows = fo.filtered_topk_from_scores(sh.scores()[:B], mask, m)
    sh.fresh_ladder()
    before = counters(sh.idx)
    got = sh.idx.search_mmr(q, k, fetch_k, lam, row_filter=flt, return_mmr=True)
    ran_on_the_scan(sh, before, sh.plan(B, m, mask is not None).npass, what)
    gs = got[0].copy()
    worst = 0.0
    for b in range(B):
        sel = {int(r): float(s) for r, s in zip(rows[b], rel[b]) if r >= 0}
        assert all(int(r) in sel for r in got[1][b]), f"{what}: query {b} returned a row outside the exact top {m}"
        worst = max(worst, max(abs(sel[int(r)] - float(s)) for r, s in zip(got[1][b], gs[b])))
        pos = {int(r): i for i, r in enumerate(rows[b])}
        gs[b] = [rel[b, pos[int(r)]] for r in got[1][b]]
    print(f"{what}: largest score difference {worst} (bar {SCORE_TOL})")
    assert worst <= SCORE_TOL, f"{what}: relevances differ by {worst}"
    tm.follows_oracle(sh.x16, rel, rows, (gs, got[1], got[2]), k, lam, what=what)
    want = mo.mmr_select_batch(rel, rows, sh.x16, k, lam)
    assert np.array_equal(got[1], want[1]), what
    return got


@pytest.mark.parametrize("lam", [0.3, 0.5])
@pytest.mark.parametrize("B", [16, 130, 300])
def test_mmr_on_the_scan(s1, B, lam):
    assert s1.plan(B, 64).fast                                   # 64 of the 201 partition maxima: the fast tail, in every pass
    mmr_end_to_end(s1, B, 10, 64, lam, what=f"S1 B={B} fetch 64 lambda {lam}")


@pytest.mark.parametrize("lam", [0.3, 0.5])
@pytest.mark.parametrize("k,fetch_k", [(33, 257), (10, 320), (10, 330)])
def test_mmr_beyond_the_fast_tail_of_a_wide_pass(s2, k, fetch_k, lam):
    """One 256-query pass leaves 256 partition maxima, one per workgroup, and the fast tail's threshold is the m-th largest of them:
    a fetch of 257 rows and more has none.  Such a call takes the generic tail with its radix select at once -- 257 just beyond the
    workgroups, 320 = RQ_FAST_MAX_K (which 64 queries still take on the fast tail), 330 beyond that.  Before plan_call knew
    (rq_plan.h fast_tail_fits) the fetches of 257 and 320 rows ran the fast tail without a threshold: all 130 queries failed their
    certificate and were searched again by the ladder, whatever the seed -- which `widened` == 0 catches."""
    p = s2.plan(130, fetch_k)
    assert not p.fast and not p.exact and p.pass_q == (256,) and s2.plan(64, 320).fast
    mmr_end_to_end(s2, 130, k, fetch_k, lam, what=f"S2 B=130 k={k} fetch {fetch_k} lambda {lam}")


@pytest.mark.parametrize("lam", [0.3, 0.5])
def test_mmr_on_the_scan_with_a_filter(s1, lam):
    mask = s1.masks["random50"]
    flt = s1.idx.make_filter(mask)
    try:
        mmr_end_to_end(s1, 130, 10, 64, lam, mask, flt, what=f"S1 B=130 random50 lambda {lam}")
        assert opt(s1.idx, "filter_route_last") == SCAN
    finally:
        flt.close()


@pytest.mark.parametrize("shape", ["s1", "s1i"])
def test_mmr_lambda_one_is_the_search_bit_for_bit_at_300_queries(request, shape):
    sh = request.getfixturevalue(shape)
    q = sh.q[:300]
    sh.fresh_ladder()
    before = counters(sh.idx)
    ps, pr = sh.idx.search(q, 10)
    s, r, v = sh.idx.search_mmr(q, 10, 64, 1.0, return_mmr=True)
    ran_on_the_scan(sh, before, sh.plan(300, 10).npass + sh.plan(300, 64).npass, f"{sh.name} lambda 1")
    assert sh.plan(300, 64).pass_q == (256, 64)
    assert np.array_equal(r, pr) and np.array_equal(s.view(np.uint32), ps.view(np.uint32)) and np.array_equal(v.view(np.uint32), ps.view(np.uint32))
    ws, wr = orc.topk_from_scores(sh.scores()[:300], 10)
    assert np.array_equal(r, wr) and float(np.abs(s - ws).max()) <= SCORE_TOL


@pytest.mark.parametrize("lam", [0.3, 0.5])
@pytest.mark.parametrize("B", [130, 300])
def test_mmr_over_the_int8_image(s1i, B, lam):
    mmr_end_to_end(s1i, B, 10, 64, lam, what=f"S1i B={B} fetch 64 lambda {lam}")


# ---- 2. grouped on the scan --------------------------------------------------------------------------------------------------------
def grouped_both_forms(sh, B, groups, k=10, mask=None, flt=None, what="", idx=None):
    """search_grouped and search_grouped_device + its fixup over the first B queries: both equal the oracle, the device form ran
    exactly the predicted passes before its fixup.  Returns (blocking answer, device answer after the fixup)."""
    idx = sh.idx if idx is None else idx
    want = tg.gro.grouped_from_scores(sh.scores()[:B], groups, k, mask)
    m1 = min(opt(idx, "group_fetch") * k, sh.n if mask is None else int(mask.sum()))
    npass = sh.plan(B, m1, mask is not None).npass
    sh.fresh_ladder(idx)
    before = counters(idx)
    blocking = idx.search_grouped(sh.q[:B], k, row_filter=flt)
    ran_on_the_scan(sh, before, npass, f"{what}, blocking", idx=idx)
    tg.agrees(blocking, want, sh.scores(), f"{what}, blocking")
    sh.fresh_ladder(idx)
    before = counters(idx)
    bufs = tg.grouped_dev(idx, sh.q[:B], k, row_filter=flt)
    first = tg.host(bufs)
    ran_on_the_scan(sh, before, npass, f"{what}, device form", exactly=True, idx=idx)
    flagged = int((first[3] != 0).sum())
    n = idx.search_grouped_fixup_device(bufs["q"], B, k, COS, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"], row_filter=flt)
    after = tg.host(bufs)
    print(f"{what}: {flagged} of {B} queries flagged by the device form")
    assert n == flagged and not after[3].any(), f"{what}: the fixup returned {n}, {flagged} were flagged"
    ran_on_the_scan(sh, before, npass, f"{what}, device form and fixup", idx=idx)
    tg.agrees(after, want, sh.scores(), f"{what}, device form")
    assert np.array_equal(after[4], tg.host_keys(after[0], after[1])), f"{what}: keys"
    return blocking, after


@pytest.mark.parametrize("pattern", ["random", "runs8"])
@pytest.mark.parametrize("B", [130, 300])
def test_grouped_on_the_scan(s1, pattern, B):
    groups = tg.patterns(s1.n)[pattern]
    s1.idx.set_groups(groups)
    blocking, dev = grouped_both_forms(s1, B, groups, what=f"S1 {pattern} B={B}")
    if B == 300:
        assert s1.plan(300, 80).pass_q == (256, 64)
        same_bits(blocking, dev[:3], f"S1 {pattern} B=300: blocking and device forms")


def test_grouped_on_the_scan_with_a_filter(s1):
    groups = tg.patterns(s1.n)["random"]
    s1.idx.set_groups(groups)
    mask = s1.masks["random50"]
    flt = s1.idx.make_filter(mask)
    try:
        grouped_both_forms(s1, 130, groups, mask=mask, flt=flt, what="S1 random random50 B=130")
        assert opt(s1.idx, "filter_route_last") == SCAN
    finally:
        flt.close()


def test_grouped_batches_of_300_then_3_then_130_on_one_handle(s1):
    """The candidate buffers of a stream grow once (B = 300) and never shrink: the calls of 3 and of 130 queries run in buffers that
    hold the larger call's rows, scores and status words, and answer as if they were fresh."""
    groups = tg.patterns(s1.n)["random"]
    idx = s1.new_index()
    try:
        idx.set_groups(groups)
        for B in (300, 3, 130):
            grouped_both_forms(s1, B, groups, what=f"S1 one handle, B={B}", idx=idx)
    finally:
        idx.close()


@pytest.mark.parametrize("shape,B", [("s1i", 130), ("s1i", 300), ("s1n", 200)])
def test_grouped_over_the_int8_image_and_the_narrow_layout(request, shape, B):
    sh = request.getfixturevalue(shape)
    groups = tg.patterns(sh.n)["random"]
    sh.idx.set_groups(groups)
    if sh.narrow:
        assert sh.plan(200, 80).pass_q == (128, 128)
    grouped_both_forms(sh, B, groups, what=f"{sh.name} random B={B}")


# ---- 3. group members on the scan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(10, 3), (4, 8)])
@pytest.mark.parametrize("shape,B", [("s1", 130), ("s1", 300), ("s1n", 200)])
def test_group_members_on_the_scan(request, shape, B, k, s):
    sh = request.getfixturevalue(shape)
    groups = tgm.patterns(sh.n)["random"]
    sh.idx.set_groups(groups)
    want = tgm.gmo.members_from_scores(sh.scores()[:B], groups, k, s)
    what = f"{sh.name} random B={B} k={k} s={s}"
    before = counters(sh.idx)
    got = sh.idx.search_group_members(sh.q[:B], k, s)
    ran_on_the_scan(sh, before, sh.plan(B, opt(sh.idx, "group_fetch") * k).npass, what)
    tgm.agrees(sh, got, want, COS, what)


# ---- 4. per-query filters beyond one pass ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def each_world(s1):
    """S1's rows and 300 queries as a World of tests/test_gpu_filter_each.py (its masks, one filter per mask), "profile" = 1."""
    w = tfe.World(s1.n, x16=s1.x16, q=s1.q, options=(("profile", 1),))
    w._scores[COS] = s1.scores()
    yield w
    w.close()


def singles(idx, q, k, filters, route):
    """The loop of single-filter device calls and their fixups over the same groups (host_loop of tests/test_gpu_filter_each.py), which
    also notes the route every group's own call took: (scores, rows, keys, {group: (queries, route)})."""
    B = len(filters)
    s = np.zeros((B, k), np.float32); r = np.zeros((B, k), np.int64); keys = np.zeros((B, k), np.int64)
    groups = {}
    for i, f in enumerate(filters):
        groups.setdefault(id(f), (f, []))[1].append(i)
    took = {}
    idx.set_option("filter_route", route)
    try:
        for key, (f, pos) in groups.items():
            d = tfe.Dev(q[pos], k).single(idx, f)
            took[key] = (len(pos), NULL_BIT if f is None else opt(idx, "filter_route_last"))
            d.single_fixup(idx, f)
            s[pos], r[pos], keys[pos] = d.all()
    finally:
        idx.set_option("filter_route", -1)
    return s, r, keys, took


@pytest.mark.parametrize("route", tfe.ROUTES)
@pytest.mark.parametrize("B", [130, 300])
def test_per_query_filters_beyond_one_pass(s1, each_world, B, route):
    w, idx = each_world, each_world.idx
    names = tfe.deal(tfe.MIXED, B)
    filters = w.filters(names)
    q = w.q[:B]
    what = f"S1 each B={B} route {route}"
    ls, lr, lkeys, took = singles(idx, q, 10, filters, route)
    scanned = sum(s1.plan(nq, 10, filtered=r != NULL_BIT).npass for nq, r in took.values() if r in (SCAN, NULL_BIT))
    # The forced scan route alone sends five_rows to the scan, which plan_filter never would: its five rows lie in four bins, so
    # fewer partitions than the min(k, 5) = 5 rows wanted hold an allowed row, the fast tail has no threshold, and every query of that
    # group fails its certificate by construction and is widened.  No other query of any route may be.
    beyond = [i for i, nm in enumerate(names) if nm == "five_rows"] if route == SCAN else []
    assert len({int(r) // 64 for r in np.flatnonzero(w.masks["five_rows"])}) == 4
    idx.set_option("filter_route", route)
    try:
        before = counters(idx)
        d = tfe.Dev(q, 10).each(idx, filters)
        st = d.status()
        ran_on_the_scan(s1, before, scanned, f"{what}, device form", exactly=True, idx=idx)
        assert np.flatnonzero(st).tolist() == beyond, f"{what}: flagged {np.flatnonzero(st).tolist()}"
        assert opt(idx, "filter_each_groups_last") == len(took) == len(tfe.MIXED)
        routes_implied = 0
        for _, r in took.values():
            routes_implied |= 1 << r
        assert opt(idx, "filter_each_routes_last") == routes_implied, f"{what}: routes {opt(idx, 'filter_each_routes_last'):#x}, the single calls took {routes_implied:#x}"
        repaired = d.each_fixup(idx, filters)
        assert repaired == int((st != 0).sum()) and not d.status().any()
        ran_on_the_scan(s1, before, scanned, f"{what}, device form and fixup", idx=idx, widened=len(beyond))
        s, r, keys = d.all()
        before = counters(idx)
        blocking = idx.search_filtered_each(q, 10, filters)
        ran_on_the_scan(s1, before, scanned, f"{what}, blocking", idx=idx, widened=len(beyond))
    finally:
        idx.set_option("filter_route", -1)
    want = w.want(names, 10, s1.scores()[:B])
    print(f"{what}: largest score difference {float(np.abs(s - want[0]).max())} (bar {SCORE_TOL}); {int((st != 0).sum())} flagged; scan passes {scanned}")
    tfe._same((s, r), want, what)
    tfe._same(blocking, want, f"{what}, blocking")
    assert np.array_equal(blocking[1], r)
    assert np.array_equal(r, lr) and np.array_equal(keys, lkeys), f"{what}: rows or keys differ from the single calls"
    gathered = [i for i, nm in enumerate(names) if nm is not None and (nm.startswith("t") or nm == "five_rows")]
    sel = slice(None) if route in (GATHER, EXACT) else gathered
    assert np.array_equal(s[sel].view(np.uint32), ls[sel].view(np.uint32)), f"{what}: score bits differ from the single calls"
    if route == -1:                  # the rule: sixteen tenants and five_rows are gathered, "all" and random50 scan, NULL searches
        assert routes_implied == 1 | (1 << GATHER) | (1 << SCAN) | (1 << NULL_BIT) and scanned == 3


# ---- 5. repairs that are themselves wide ------------------------------------------------------------------------------------------------
def test_a_repair_of_130_flagged_queries(s1, each_world):
    """ "eps" = 10: no certificate of the scan holds, every query of a call that scans comes back flagged, and the repair packs all
    130 of them into one wide call of its own."""
    B, k = 130, 10
    q = s1.q[:B]
    groups = tg.patterns(s1.n)["random"]
    s1.idx.set_groups(groups)
    names = tfe.deal(tfe.MIXED, B)
    filters = each_world.filters(names)
    plain_mmr = s1.idx.search_mmr(q, k, 64, 0.5, return_mmr=True)
    plain_each = each_world.idx.search_filtered_each(q, k, filters)
    want = tg.gro.grouped_from_scores(s1.scores()[:B], groups, k)
    s1.idx.set_option("eps", 10)
    each_world.idx.set_option("eps", 10)
    try:
        before = {name: opt(s1.idx, name) for name in ("group_repaired", "repaired_queries")}
        bufs = tg.grouped_dev(s1.idx, q, k)
        first = tg.host(bufs)
        assert (first[3] != 0).all(), f"grouped: {int((first[3] != 0).sum())} of {B} queries flagged"
        n = s1.idx.search_grouped_fixup_device(bufs["q"], B, k, COS, bufs["s"], bufs["r"], bufs["g"], bufs["k"], bufs["st"])
        after = tg.host(bufs)
        assert n == B and not after[3].any()
        assert opt(s1.idx, "group_repaired") == before["group_repaired"] + B
        tg.agrees(after, want, s1.scores(), "grouped, all 130 repaired")
        assert np.array_equal(after[4], tg.host_keys(after[0], after[1]))
        t0 = counters(s1.idx)
        same_bits(s1.idx.search_mmr(q, k, 64, 0.5, return_mmr=True), plain_mmr, "search_mmr under eps = 10")
        t1 = counters(s1.idx)
        assert t1["repaired_queries"] - t0["repaired_queries"] == B, "every query of the MMR fetch climbs the ladder"
        f0 = opt(each_world.idx, "filter_repaired")
        same_bits(each_world.idx.search_filtered_each(q, k, filters), plain_each, "search_filtered_each under eps = 10")
        scanning = sum(1 for nm in names if nm in (None, "all", "random50"))           # the groups the rule sends to the scan
        assert opt(each_world.idx, "filter_repaired") - f0 >= scanning
    finally:
        s1.idx.set_option("eps", -1)
        each_world.idx.set_option("eps", -1)
    tfe._same(plain_each, each_world.want(names, k, s1.scores()[:B]), "search_filtered_each")


# ---- 6. the Python seam -------------------------------------------------------------------------------------------------------------------
def test_dense_index_reaches_the_scanned_routes(s1):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    B = 130
    groups = tg.patterns(s1.n)["random"]
    ids = [f"p{i}" for i in range(s1.n)]
    metas = [{} if g == tg.NONE else {"article": int(g)} for g in groups]
    di = si.DenseIndex(persist_directory="", embedder=HashEmbedder(), load_persisted=False, auto_persist=False, backend_options={"scan8": 0, "profile": 1})
    try:
        di.add_vectors(ids, s1.x16.astype(np.float32), metadatas=metas)
        native = di._index
        stored = native.get_rows_f16(0, s1.n)
        q = s1.q[:B]
        scores = orc.exact_scores(q, stored, COS)
        before = counters(native)
        got = di.search_vectors(q, 10, distinct_by="article")
        ran_on_the_scan(s1, before, s1.plan(B, 80).npass, "DenseIndex distinct_by", idx=native)
        ns, nr, ng = native.search_grouped(q, 10)
        assert [[(d, s) for d, s, _ in row] for row in got] == [[(ids[r], float(s)) for s, r in zip(ns[b], nr[b]) if r >= 0] for b in range(B)]
        tg.agrees((ns, nr, ng), tg.gro.grouped_from_scores(scores, native.get_groups().astype(np.int64), 10), scores, "DenseIndex distinct_by")
        ws, wr, _ = tg.gro.grouped_from_scores(scores, groups, 10)          # the caller's partition, whatever ids the seam assigned
        assert np.array_equal(nr, wr)
        before = counters(native)
        got = di.search_mmr_vectors(q, 10, 64, 0.5)
        ran_on_the_scan(s1, before, s1.plan(B, 64).npass, "DenseIndex MMR", idx=native)
        ms, mr = native.search_mmr(q, 10, 64, 0.5)
        assert [[(d, s) for d, s, _ in row] for row in got] == [[(ids[r], float(s)) for s, r in zip(ms[b], mr[b])] for b in range(B)]
        rel, rows = orc.topk_from_scores(scores, 64)
        assert np.array_equal(mr, mo.mmr_select_batch(rel, rows, stored, 10, 0.5)[1])
    finally:
        di._index.close()
