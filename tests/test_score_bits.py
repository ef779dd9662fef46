"""tests/score_bits.py has teeth, and the inputs of tests/test_gpu_score_bits.py fit its caps (CPU only).

  * the reference agrees with the oracle (orc.exact_scores) on every decided pair;
  * host models of the natural wrong "optimisations" of a re-score kernel are REJECTED by assert_score_bits although two of
    them stay within SCORE_TOL = 1e-6 of the oracle on every pair -- the bar of the other GPU tests is blind to them;
  * fp64 sums in another order (sequential, reversed, the 16-lane order of csrc/rq_rowdot.h) PASS: the bound is not fitted to one order;
  * every input of the GPU tests keeps its undecided share within the cap with the reference alone, the ranking around every
    position the GPU tests cut at holds no undecided pair, and the twins are the pairs make_case promises.
The inputs are the GPU tests' own (score_bits.make_case: Gaussian rows, the cancelling rows and the twins), computed once per
(dim, metric) for the whole module."""
import numpy as np
import pytest

from oracle import dense_oracle as orc

import group_members_oracle as gmo
import score_bits as sb
from score_bits import COS, IP

DIMS = [768, 384, 300]
CASES = [(d, m) for d in DIMS for m in (COS, IP)]
SCORE_TOL = 1e-6


def _all_rows(case):
    return np.broadcast_to(np.arange(len(case.x16)), (len(case.q), len(case.x16)))


@pytest.mark.parametrize("dim,metric", CASES)
def test_the_oracle_agrees_with_the_reference_on_every_decided_pair(dim, metric):
    for case in (sb.make_case(dim, metric), sb.make_small(dim, metric)):
        ex = orc.exact_scores(case.q, case.x16, metric)
        ex[ex == 0] = 0.0
        d = case.ref.decided
        assert np.array_equal(sb.bits(ex)[d], sb.bits(case.ref.lo)[d])
        sb.assert_score_bits(ex, _all_rows(case), case.ref, "oracle", sb.CAP)


@pytest.mark.parametrize("dim,metric,model", [(d, COS, m) for d in DIMS for m in ("fp32_dot", "recip_norm", "fp32_norms", "round_before_div")]
                         + [(d, IP, "fp32_dot") for d in DIMS])
def test_wrong_models_are_rejected(dim, metric, model):
    case = sb.make_case(dim, metric)
    got = sb.model_scores(case.x16, case.q, metric, model)
    wrong = float((sb.bits(got) != sb.bits(case.ref.lo))[case.ref.decided].mean())
    err = float(np.abs(got.astype(np.float64) - orc.exact_scores(case.q, case.x16, metric)).max())
    print(f"{model} dim {dim} metric {metric}: {wrong:.1%} of the decided scores have other bits, largest error {err:.2e}")
    with pytest.raises(AssertionError, match="do not have the bits of the definition"):
        sb.assert_score_bits(got, _all_rows(case), case.ref, model, sb.CAP)
    assert wrong > 0.05                                       # not a rare boundary effect: a plain share of all scores
    if metric == COS and model in ("fp32_dot", "recip_norm"):
        assert err <= SCORE_TOL                               # ... which the 1e-6 bar of the other tests lets through
    # the cancelling rows alone convict an fp32 accumulation: their dot products lose tens of ulps
    if model == "fp32_dot":
        ulps = np.abs(sb.mono(sb.bits(got[0, sb.CANCEL_ROWS])) - sb.mono(sb.bits(case.ref.lo[0, sb.CANCEL_ROWS])))
        print(f"   cancelling rows: median distance {np.median(ulps):.0f} ulp")
        assert np.median(ulps) >= 4


def test_omitted_special_rules_are_rejected_on_a_planted_negative_zero_and_a_nan():
    x16 = np.zeros((3, 8), np.float16)
    x16[0, 0] = np.float16(2.0 ** -24)                        # x q = -2^-154: underflows to -0.0 in fp32
    x16[1, 1] = np.nan
    x16[2, 2] = 1.0
    q = np.zeros((1, 8), np.float32)
    q[0, 0], q[0, 2] = -2.0 ** -130, 2.0 ** -130
    ref = sb.reference(x16, q, IP)
    assert ref.decided.all() and sb.bits(ref.lo)[0].tolist() == [0, 0xFF800000, sb.bits(np.float32(2.0 ** -130))[()]]
    rows = np.arange(3)[None, :]
    got = sb.model_scores(x16, q, IP, "no_rules")
    assert np.signbit(got[0, 0]) and np.isnan(got[0, 1])
    for bad in ([0], [1]):
        with pytest.raises(AssertionError, match="do not have the bits of the definition"):
            sb.assert_score_bits(got[:, bad], rows[:, bad], ref, "no rules", 0.0)
    sb.assert_score_bits(sb.model_scores(x16, q, IP, "sequential"), rows, ref, "rules", 0.0)
    with pytest.raises(AssertionError, match="padding"):
        sb.assert_score_bits(np.float32([[-0.0]]), np.array([[-1]]), ref, "padding", 0.0)
    zero = sb.reference(x16, np.zeros((1, 8), np.float32), COS)                       # a zero-norm query scores 0.0, also the NaN row
    assert zero.decided.all() and not sb.bits(zero.lo).any()


@pytest.mark.parametrize("dim,metric", CASES)
def test_fp64_sums_in_another_order_pass(dim, metric):
    case = sb.make_case(dim, metric)
    for model in ("sequential", "reversed", "lanes16"):
        sb.assert_score_bits(sb.model_scores(case.x16, case.q, metric, model), _all_rows(case), case.ref, model, sb.CAP)


def test_an_undecided_pair_accepts_lo_to_hi_and_nothing_else_and_counts_against_the_cap():
    case = sb.make_case(768, COS)
    und = np.argwhere(~case.ref.decided)
    assert len(und)
    b, r = und[0]
    sel = np.zeros((sb.B, 1), np.int64)
    sel[:] = r                                                                       # row r for every query; undecided for b
    lo, hi = case.ref.lo[:, [r]].copy(), case.ref.hi[:, [r]].copy()
    n_und = int((~case.ref.decided[:, r]).sum())
    for got in (lo, hi):
        assert sb.assert_score_bits(got, sel, case.ref, "either", 1.0) == (sb.B, n_und)
    beyond = hi.copy()
    beyond[b] = np.nextafter(hi[b], np.float32(np.inf))
    with pytest.raises(AssertionError, match="do not have the bits"):
        sb.assert_score_bits(beyond, sel, case.ref, "beyond", 1.0)
    with pytest.raises(AssertionError, match="above the cap"):
        sb.assert_score_bits(lo, sel, case.ref, "cap", sb.CAP)
    assert sb.canonical_topk(case.ref, len(case.x16) - 1)[2][b]                      # ... and flags its query once k reaches it


@pytest.mark.parametrize("dim,metric", CASES)
def test_every_input_of_the_gpu_tests_stays_within_its_cap(dim, metric):
    case, small = sb.make_case(dim, metric), sb.make_small(dim, metric)
    ref = case.ref
    und, pairs = int((~ref.decided).sum()), ref.decided.size
    und_c = int((~ref.decided[sb.CANCEL_QUERY, sb.CANCEL_ROWS]).sum())
    planted = sb.planted_rows(case)
    und_p = int((~ref.decided[:, planted]).sum())
    print(f"dim {dim} metric {metric}: {und} of {pairs} pairs undecided; cancelling rows {und_c} of {len(sb.CANCEL_ROWS)}; "
          f"planted list {und_p} of {sb.B * len(planted)}; 130-row index {int((~small.ref.decided).sum())} of {small.ref.decided.size}")
    assert und <= sb.CAP * pairs
    assert und_c <= sb.CAP_CANCEL * len(sb.CANCEL_ROWS)
    assert und_p <= sb.CAP * sb.B * len(planted)
    # the cancelling rows cancel: sum|q x| is more than 100 times |dot|
    p = case.q[sb.CANCEL_QUERY].astype(np.float64) * case.x16[sb.CANCEL_ROWS].astype(np.float64)
    assert (np.abs(p).sum(axis=1) > 100 * np.abs(p.sum(axis=1))).all()
    # no ranking the GPU tests compare rows against is cut near an undecided pair
    third = np.arange(len(case.x16)) % 3 == 0
    only_cancel = np.isin(np.arange(len(case.x16)), sb.CANCEL_ROWS)
    for k, allowed in ((sb.K, None), (20, None), (64, None), (sb.K, third), (sb.K, ~third), (64, only_cancel)):
        assert not sb.canonical_topk(ref, k, allowed)[2].any(), (k, "filtered" if allowed is not None else "all rows")
    for allowed in (None, third):
        assert not sb.range_thresholds(ref, 40, allowed)[1].any()
    for shared in (True, False):                                                     # grouped answers: the same from either end of every interval
        groups = sb.twin_groups(case, shared)
        for s in (1, 3):
            a, b = (gmo.members_from_scores(v, groups, sb.K, s) for v in (ref.lo, ref.hi))
            assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and np.array_equal(sb.bits(a[0]), sb.bits(b[0]))
    assert small.ref.decided.all()                                                   # k = 130 returns the whole order
    assert not sb.bits(small.ref.lo[:, 9]).any() and (small.ref.lo < 0).any()        # the zero row scores +0.0; negative scores exist


@pytest.mark.parametrize("dim,metric", CASES)
def test_the_twins_are_the_pairs_they_promise(dim, metric):
    case = sb.make_case(dim, metric)
    ref = case.ref
    _, rows, flagged = sb.canonical_topk(ref, sb.K + 2)
    assert not flagged.any()
    assert sorted((t.query, t.kind, t.straddles) for t in case.twins) == sorted(
        (b, kind, (kind == sb.TIE) == (b % 2 == 0)) for b in range(sb.B) for kind in (sb.TIE, sb.ONE_ULP))
    for t in case.twins:
        pair = [t.base, t.twin]
        assert ref.decided[t.query, pair].all()
        assert (case.x16[t.base] != case.x16[t.twin]).sum() == 1                     # one element moved ...
        a, c = case.x16[t.base].view(np.uint16).astype(np.int64), case.x16[t.twin].view(np.uint16).astype(np.int64)
        assert np.abs(a - c).max() == 1                                              # ... by one fp16 ulp
        lo_id, hi_id = min(pair), max(pair)
        assert ref.val[t.query, hi_id] > ref.val[t.query, lo_id]                     # the higher fp64 score has the larger row id
        step = int((sb.mono(sb.bits(ref.lo[t.query, hi_id])) - sb.mono(sb.bits(ref.lo[t.query, lo_id])))[0])
        first = 4 if not t.straddles else sb.K - 1                                   # ranks the pair holds: 4, 5 or K - 1, K
        if t.kind == sb.TIE:
            assert step == 0
            assert rows[t.query, first:first + 2].tolist() == [lo_id, hi_id]         # canonical: equal bits order by row ...
        else:
            assert step == 1
            assert rows[t.query, first:first + 2].tolist() == [hi_id, lo_id]         # ... adjacent values by score
