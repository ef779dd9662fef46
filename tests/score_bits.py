"""The score definition of include/rq.h held to the BIT -- TEST INFRASTRUCTURE (numpy + math.fsum, no GPU).

    cosine: s = fp32( dot64(q, x) / (|q|_64 * |x|_64 + 1e-30) )        inner product: s = fp32( dot64(q, x) )

Every re-scoring kernel claims that definition: exact fp16 x fp32 products, summed in fp64 in SOME order, the definition's own
fp64 operations, ONE rounding to fp32.  SCORE_TOL = 1e-6 of the other GPU tests cannot tell that from an fp32 accumulation or
from a second rounding (tests/test_score_bits.py shows it); this module can.

reference() evaluates the definition with exactly rounded sums (math.fsum over the exact fp64 products) and bounds how far a
CORRECT kernel's fp64 value may lie from it:

    u = 2^-53, g = (dim + 16) u
    a sum of dim exact products in any order is off by at most (dim - 1) u sum|q[e] x[e]|; each norm by a relative (dim - 1) u / 2
    plus one sqrt rounding; the product of the norms, + 1e-30 and the division add one rounding each (the 16 of g covers them all,
    the 8 below the two norms, their product and the second-order terms with room to spare)
    cosine:        delta = g sum|q[e] x[e]| / (|q| |x| + 1e-30) + 8 g |val|
    inner product: delta = g sum|q[e] x[e]|

The bound is the worst case of any order of correctly rounded fp64 operations, not a fit to today's kernels.  A pair is DECIDED
when fp32(val - delta) and fp32(val + delta) are the same bits: a correct kernel must return exactly those.  For an undecided
pair the fp32 values from the one to the other are accepted and nothing else: nearly always two neighbours, but where a dot product
cancels to a millionth of sum|q x| delta itself exceeds an fp32 ulp of the result and a correct kernel may land between them.
Callers cap the share of undecided pairs (CAP), so a check can never pass by deciding nothing.  On top come the rules of
tests/nonfinite_oracle.py: a zero-norm query or row scores 0.0, -0.0 leaves as +0.0, NaN counts as -inf.

The second half builds the fixed inputs of tests/test_gpu_score_bits.py (make_case, make_small): Gaussian rows, 64 CANCELLING
rows (nearly orthogonal to query 0: sum|q x| > 100 |dot|, where an fp32 accumulation is off by tens of ulps of the result) and
TWINS, pairs of rows whose scores for one query lie within one fp32 ulp of each other, planted around position k.
tests/test_score_bits.py (CPU) proves the teeth of the checker and that every input stays within its cap.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from oracle import dense_oracle as orc

COS, IP = orc.METRIC_COSINE, orc.METRIC_IP
U = 2.0 ** -53
CAP = 0.002                  # undecided share allowed among checked pairs: Gaussian and twin inputs
CAP_CANCEL = 0.02            # ... among the cancelling rows against their query

N, B, K = 4_101, 8, 10       # 65 bins with a ragged last one; the module's queries; the k the twins are planted around
N_SMALL = 130
CANCEL_QUERY, CANCEL_COS = 0, 1e-3
CANCEL_ROWS = 37 + 64 * np.arange(64)          # one per whole bin
TIE, ONE_ULP = "tie", "one-ulp"


class Ref(NamedTuple):
    val: np.ndarray          # [B][n] fp64: the definition with exactly rounded sums
    lo: np.ndarray           # [B][n] fp32(val - delta), special rules applied
    hi: np.ndarray           # [B][n] fp32(val + delta), special rules applied
    decided: np.ndarray      # [B][n] lo and hi are the same bits


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mono(b) -> np.ndarray:
    """Order-preserving integer image of fp32 bits (as rq_mono32): differences are distances in ulps."""
    b = np.asarray(b, dtype=np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)


def _fsum_rows(m: np.ndarray) -> np.ndarray:
    """Exactly rounded sum of every row of m [n][d] fp64 (rows with a non-finite entry: numpy's sum)."""
    with np.errstate(all="ignore"):
        out = m.sum(axis=1)
        finite = np.isfinite(m).all(axis=1)
    for i, row in zip(np.nonzero(finite)[0].tolist(), m[finite].tolist()):
        out[i] = math.fsum(row)
    return out


def apply_rules(s32: np.ndarray, qn: np.ndarray) -> np.ndarray:
    """NaN -> -inf, a zero-norm query scores 0.0, -0.0 -> +0.0 (in place, [B][n] fp32)."""
    s32[np.isnan(s32)] = -np.inf
    s32[np.asarray(qn) == 0.0] = 0.0
    s32[s32 == 0] = 0.0
    return s32


def reference(x16: np.ndarray, q: np.ndarray, metric: int) -> Ref:
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    x16 = np.asarray(x16)
    assert x16.dtype == np.float16 and x16.ndim == 2 and q.shape[1] == x16.shape[1]
    nq, n, dim = q.shape[0], x16.shape[0], x16.shape[1]
    q64, x64 = q.astype(np.float64), x16.astype(np.float64)
    g = (dim + 16) * U
    with np.errstate(all="ignore"):
        qn, xn = np.sqrt(_fsum_rows(q64 * q64)), np.sqrt(_fsum_rows(x64 * x64))     # squares: exact in fp64 (48 / 22 bits)
        dot, mag = np.empty((nq, n)), np.empty((nq, n))
        for b in range(nq):
            p = q64[b] * x64                                                        # exact: 24 + 11 significand bits
            dot[b] = _fsum_rows(p)
            mag[b] = np.abs(p).sum(axis=1) * (1.0 + 2.0 ** -40)                     # (numpy's sum of non-negative terms, rounded up)
        if metric == COS:
            den = qn[:, None] * xn[None, :] + 1e-30
            val = dot / den
            delta = g * mag / den + 8.0 * g * np.abs(val)
        else:
            val = dot
            delta = g * mag
        lo = apply_rules((val - delta).astype(np.float32), qn)
        hi = apply_rules((val + delta).astype(np.float32), qn)
    return Ref(val, lo, hi, bits(lo) == bits(hi))


def assert_score_bits(got_scores, got_rows, ref: Ref, what: str, cap: float, row_offset: int = 0) -> Tuple[int, int]:
    """Every returned (query, row, score) [B][...] has the bits the definition decides (a value from lo to hi where it does not); padding
    (row -1) is +0.0; at most `cap` of the checked pairs are undecided.  Prints and returns (pairs checked, undecided)."""
    nq, n = ref.lo.shape
    gs = np.ascontiguousarray(got_scores, dtype=np.float32)
    gr = np.asarray(got_rows, dtype=np.int64)
    assert gs.shape == gr.shape and gs.shape[0] == nq, f"{what}: shapes {gs.shape} / {gr.shape} for {nq} queries"
    gb, gr = bits(gs).reshape(nq, -1), gr.reshape(nq, -1)
    pad = gr == -1
    assert not gb[pad].any(), f"{what}: a padding entry does not score +0.0"
    loc = np.where(pad, 0, gr - row_offset)
    assert ((loc >= 0) & (loc < n)).all(), f"{what}: rows outside the index"
    qi = np.broadcast_to(np.arange(nq)[:, None], gr.shape)
    lo, hi, dec = bits(ref.lo)[qi, loc], bits(ref.hi)[qi, loc], ref.decided[qi, loc]
    bad = ~pad & ((mono(gb) < mono(lo)) | (mono(gb) > mono(hi)))       # (a NaN's image lies beyond either infinity's)
    if bad.any():
        near = np.where(np.abs(mono(gb) - mono(lo)) <= np.abs(mono(gb) - mono(hi)), lo, hi)
        lines = [f"(query {qi[i, j]}, row {gr[i, j]}): got {int(gb[i, j]):#010x}, want {int(near[i, j]):#010x}"
                 f"{'' if dec[i, j] else ' (undecided: the nearest value allowed)'}, {int(mono(gb[i, j]) - mono(near[i, j])):+d} ulp"
                 for i, j in np.argwhere(bad)[:6].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {int((~pad).sum())} scores do not have the bits of the definition: " + "; ".join(lines))
    checked, und = int((~pad).sum()), int((~pad & ~dec).sum())
    print(f"score bits [{what}]: {checked} pairs checked, {und} undecided")
    assert und <= cap * max(checked, 1), f"{what}: {und} of {checked} checked pairs undecided, above the cap of {cap:.2%}"
    return checked, und


def canonical_topk(ref: Ref, k: int, allowed: Optional[np.ndarray] = None, row_offset: int = 0):
    """The oracle ranking from the decided fp32 bits, (score desc, row asc) over the allowed rows: (scores [B][k], rows [B][k],
    flagged [B]), (0.0, -1) padded.  flagged: an undecided pair could lie at or above position k + 1 -- its upper value reaches
    the (k + 1)-th lower value -- so the ranking is not the definition's to state; callers leave such queries out of row comparisons."""
    nq, n = ref.lo.shape
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    cand = np.nonzero(ok)[0]
    out_s, out_r = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64)
    flagged = np.zeros(nq, dtype=bool)
    for b in range(nq):
        lo, hi = ref.lo[b, cand], ref.hi[b, cand]
        order = np.lexsort((cand, -lo.astype(np.float64)))
        ke = min(k, len(cand))
        out_s[b, :ke], out_r[b, :ke] = lo[order[:ke]], cand[order[:ke]] + row_offset
        reach = lo[order[k]] if len(cand) > k else -np.inf
        flagged[b] = bool((~ref.decided[b, cand] & (hi >= reach)).any())
    return out_s, out_r, flagged


# ---- CPU models of a score kernel: correct ones (any fp64 order) and the wrong ones the checker must reject ----------------------
def _finish(dot64, qn, xn, metric, qnorm_for_rules=None):
    with np.errstate(all="ignore"):
        s = dot64 / (qn[:, None] * xn[None, :] + 1e-30) if metric == COS else dot64
        return apply_rules(np.asarray(s).astype(np.float32), qn if qnorm_for_rules is None else qnorm_for_rules)


def _dot_in_order(q64, x64, order) -> np.ndarray:
    """sum over e in `order` of q[e] x[e], one fp64 addition after the other: [B][n]"""
    acc = np.zeros((q64.shape[0], x64.shape[0]))
    for e in order:
        acc += q64[:, e, None] * x64[None, :, e]
    return acc


def _dot_lanes16(q64, x64) -> np.ndarray:
    """The order of csrc/rq_rowdot.h: lane sub of 16 owns elements pp * 128 + 8 sub + e in element order, then an xor butterfly."""
    dim = q64.shape[1]
    lanes = []
    for sub in range(16):
        own = [pp * 128 + 8 * sub + e for pp in range((dim + 127) // 128) for e in range(8) if pp * 128 + 8 * sub + e < dim]
        lanes.append(_dot_in_order(q64, x64, own))
    for off in (8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i ^ off] for i in range(16)]
    return lanes[0]


def model_scores(x16, q, metric, model: str) -> np.ndarray:
    """fp32 scores [B][n] of a host model.  Correct: "sequential", "reversed", "lanes16" (fp64 sums in that order, norms alike).
    Wrong: "fp32_dot" (dot accumulated in fp32), "recip_norm" (fp64 dot * fp32(1 / |x|), rounded, / fp32(|q|)), "fp32_norms"
    (fp64 dot over fp32-rounded norms), "round_before_div" (numerator and denominator rounded to fp32, divided in fp32),
    "no_rules" (NaN and -0.0 leave as they are)."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    q64, x64 = q.astype(np.float64), np.asarray(x16).astype(np.float64)
    dim = q64.shape[1]
    with np.errstate(all="ignore"):
        if model in ("sequential", "reversed", "lanes16"):
            order = list(range(dim)) if model != "reversed" else list(range(dim - 1, -1, -1))
            if model == "lanes16":
                dot = _dot_lanes16(q64, x64)
            else:
                dot = _dot_in_order(q64, x64, order)
            qn = np.sqrt(np.array([sum_in_order(r, order) for r in (q64 * q64)]))
            xn = np.sqrt(_cols_in_order(x64 * x64, order))
            return _finish(dot, qn, xn, metric)
        qn, xn = np.sqrt((q64 * q64).sum(axis=1)), np.sqrt((x64 * x64).sum(axis=1))
        dot = q64 @ x64.T
        if model == "fp32_dot":
            return _finish((q @ np.asarray(x16).astype(np.float32).T).astype(np.float64), qn, xn, metric)
        if model == "no_rules":
            return (dot / (qn[:, None] * xn[None, :] + 1e-30) if metric == COS else dot).astype(np.float32)
        assert metric == COS, f"{model} is a model of the cosine"
        if model == "recip_norm":
            s = (dot * (1.0 / xn).astype(np.float32)[None, :].astype(np.float64)).astype(np.float32) / qn.astype(np.float32)[:, None]
            return apply_rules(s.astype(np.float32), qn)
        if model == "fp32_norms":
            den = qn.astype(np.float32).astype(np.float64)[:, None] * xn.astype(np.float32).astype(np.float64)[None, :] + 1e-30
            return apply_rules((dot / den).astype(np.float32), qn)
        if model == "round_before_div":
            s = dot.astype(np.float32) / (qn[:, None] * xn[None, :] + 1e-30).astype(np.float32)
            return apply_rules(s.astype(np.float32), qn)
    raise ValueError(model)


def sum_in_order(v, order) -> float:
    acc = 0.0
    for e in order:
        acc += float(v[e])
    return acc


def _cols_in_order(m, order) -> np.ndarray:
    acc = np.zeros(m.shape[0])
    for e in order:
        acc += m[:, e]
    return acc


# ---- the fixed inputs of the GPU tests ------------------------------------------------------------------------------------------
class Twin(NamedTuple):
    query: int
    kind: str                # TIE: the same fp32 bits; ONE_ULP: adjacent fp32 values.  Either way the fp64 scores differ and the
    base: int                # higher one has the larger row id; `base` is the original row, `twin` its copy with one element
    twin: int                # moved by one fp16 ulp
    straddles: bool          # the pair holds positions K and K + 1 of its query (else: both inside the top K)


class Case(NamedTuple):
    dim: int
    metric: int
    x16: np.ndarray          # [N][dim] fp16
    q: np.ndarray            # [B][dim] fp32
    twins: Tuple[Twin, ...]
    ref: Ref


def gaussian_rows(n: int, dim: int, metric: int, seed: int) -> np.ndarray:
    """Cosine: orc.synthetic_corpus (unit rows).  Inner product: the same directions at norms 0.5 .. 2, scaled before the fp16
    rounding (geometry 6 of tests/tail_cases.py), so that scores span several binades."""
    if metric == COS:
        return orc.synthetic_corpus(n, dim, seed=seed)
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32).astype(np.float64)
    x *= (np.random.default_rng(seed + 1000).uniform(0.5, 2.0, n) / np.sqrt((x * x).sum(axis=1)))[:, None]
    return x.astype(np.float32).astype(np.float16)


def queries(nq: int, dim: int, metric: int, seed: int = 6) -> np.ndarray:
    q = orc.synthetic_queries(nq, dim, seed=seed)
    if metric == IP:                                                                # norm 3
        q64 = q.astype(np.float64)
        q = (3.0 * q64 / np.sqrt((q64 * q64).sum(axis=1, keepdims=True))).astype(np.float32)
    return q


def cancelling_rows(q0: np.ndarray, count: int, metric: int, seed: int) -> np.ndarray:
    """Rows orthogonal to q0 in fp64, given back a cosine of CANCEL_COS, rounded to fp16: sum|q x| is several hundred times |dot|."""
    rng = np.random.default_rng(seed)
    u = q0.astype(np.float64)
    u /= np.sqrt((u * u).sum())
    g = rng.standard_normal((count, len(u)))
    g -= (g @ u)[:, None] * u[None, :]
    g /= np.sqrt((g * g).sum(axis=1, keepdims=True))
    x = g + CANCEL_COS * u[None, :]
    if metric == IP:
        x *= rng.uniform(0.5, 2.0, count)[:, None]
    return x.astype(np.float32).astype(np.float16)


def _one_ulp_copies(row16: np.ndarray) -> np.ndarray:
    """Every copy of the row with ONE element's magnitude moved by one fp16 ulp, up then down, element by element: [<= 2 dim][dim]"""
    b = row16.view(np.uint16)
    out = []
    for e in range(len(b)):
        for step in (1, -1):
            mag = int(b[e] & 0x7FFF) + step
            if 0 <= mag < 0x7C00:                                                   # stays finite; a zero element moves up only
                c = b.copy()
                c[e] = (b[e] & 0x8000) | mag
                out.append(c)
    return np.array(out, dtype=np.uint16).view(np.float16)


def find_twin(row16: np.ndarray, qv: np.ndarray, metric: int, kind: str, want_higher: bool) -> Optional[np.ndarray]:
    """The first one-ulp copy of the row that is decided for qv, whose fp64 score is higher (lower) than the row's and whose fp32
    score is the same bits (TIE) or the adjacent value (ONE_ULP)."""
    base = reference(row16[None, :], qv, metric)
    assert base.decided[0, 0], "the base row of a twin must be decided"
    copies = _one_ulp_copies(row16)
    r = reference(copies, qv, metric)
    step = mono(bits(r.lo[0])) - mono(bits(base.lo[0, 0]))
    fits = r.decided[0] & ((r.val[0] > base.val[0, 0]) if want_higher else (r.val[0] < base.val[0, 0]))
    fits &= (step == 0) if kind == TIE else (step == (1 if want_higher else -1))
    hit = np.nonzero(fits)[0]
    return copies[hit[0]] if len(hit) else None


@lru_cache(maxsize=None)
def make_case(dim: int, metric: int) -> Case:
    x16 = gaussian_rows(N, dim, metric, seed=5).copy()
    q = queries(B, dim, metric)
    for seed in range(dim + metric, dim + metric + 100, 2):                          # the first seed that leaves them decided for EVERY query:
        x16[CANCEL_ROWS] = cancelling_rows(q[CANCEL_QUERY], len(CANCEL_ROWS), metric, seed)   # a filter that allows only them returns them all
        if reference(x16[CANCEL_ROWS], q, metric).decided.all():
            break
    # a twin ranks wherever its base row does: rows that rank near the top for two queries (the long rows of the inner product do)
    # are drawn again, so that a pair planted for one query moves no other query's positions
    for attempt in range(1, 100):
        rank = np.argsort(-orc.exact_scores(q, x16, metric), axis=1, kind="stable")
        rows, seen = np.unique(rank[:, :K + 4], return_counts=True)
        again = rows[seen > 1]
        if not len(again):
            break
        plain = ~np.isin(again, CANCEL_ROWS)
        x16[again[plain]] = gaussian_rows(int(plain.sum()), dim, metric, seed=1000 * attempt + dim)
        x16[again[~plain]] = cancelling_rows(q[CANCEL_QUERY], int((~plain).sum()), metric, seed=1000 * attempt + dim)
    taken = set(rank[:, :200].reshape(-1).tolist()) | set(CANCEL_ROWS.tolist())     # rows a twin must not overwrite
    twins: List[Twin] = []
    for b in range(B):
        # the pair planted at rank 4 holds ranks 4 and 5; then the row at rank 9 = position K and its twin hold positions K and
        # K + 1 (ranks as the corpus stands when the pair is planted: an earlier query's twin may rank high for this one too).
        # Even queries: the tie twins straddle; odd queries: the one-ulp twins.
        for r0, straddles in ((4, False), (K - 1, True)):
            kind = TIE if (b % 2 == 0) == straddles else ONE_ULP
            base = int(np.argsort(-orc.exact_scores(q[b:b + 1], x16, metric)[0], kind="stable")[r0])
            for want_higher in (True, False):                                       # the higher fp64 score gets the larger row id
                spots = [r for r in (range(base + 1, N) if want_higher else range(base - 1, -1, -1)) if r not in taken]
                copy = find_twin(x16[base], q[b:b + 1], metric, kind, want_higher) if spots else None
                if copy is not None:
                    break
            assert copy is not None, f"no {kind} twin for query {b}, row {base} (dim {dim}, metric {metric})"
            x16[spots[0]] = copy
            taken.add(spots[0])
            twins.append(Twin(b, kind, base, spots[0], straddles))
    x16.setflags(write=False)
    q.setflags(write=False)
    return Case(dim, metric, x16, q, tuple(twins), reference(x16, q, metric))


@lru_cache(maxsize=None)
def make_small(dim: int, metric: int) -> Case:
    """130 rows (the exact route, three bins with a ragged last one) under the module's queries: negative scores, a zero row (+0.0)
    and a duplicated row, so that k = 130 returns the whole order."""
    x16 = gaussian_rows(N_SMALL, dim, metric, seed=8).copy()      # (a seed that leaves no pair undecided)
    x16[9] = 0
    x16[77] = x16[3]
    q = queries(B, dim, metric)
    x16.setflags(write=False)
    q.setflags(write=False)
    return Case(dim, metric, x16, q, (), reference(x16, q, metric))


def planted_rows(case: Case) -> np.ndarray:
    """The cancelling rows and every twin pair, ascending."""
    return np.unique(np.concatenate([CANCEL_ROWS, [r for t in case.twins for r in (t.base, t.twin)]])).astype(np.int64)


def twin_groups(case: Case, shared: bool) -> np.ndarray:
    """Groups of 8 consecutive rows; every twin joins its base row's group (shared) or gets a group of its own (not shared)."""
    g = (np.arange(len(case.x16)) // 8).astype(np.int32)
    for i, t in enumerate(case.twins):
        g[t.twin] = g[t.base] if shared else 100_000 + i
    if not shared:
        for t in case.twins:                                                        # (a base row in a twin's old octet stays there)
            assert g[t.base] != g[t.twin]
    return g


def range_thresholds(ref: Ref, below: int = 40, allowed: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Per query the fp32 midpoint between the `below`-th and the next score of the canonical ranking (strictly between them), and
    the queries canonical_topk flags there."""
    s, _, flagged = canonical_topk(ref, below + 1, allowed)
    thr = ((s[:, below - 1].astype(np.float64) + s[:, below].astype(np.float64)) / 2).astype(np.float32)
    assert ((thr < s[:, below - 1]) & (thr > s[:, below])).all(), "no fp32 value strictly between two neighbours of the ranking"
    return thr, flagged


def range_want(ref: Ref, thr: np.ndarray, cap: int, allowed: Optional[np.ndarray] = None):
    """(scores [B][cap], rows [B][cap], counts [B]) of a range search from the decided bits."""
    nq, n = ref.lo.shape
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    s, r, _ = canonical_topk(ref, cap, ok)
    counts = np.array([int((ok & (ref.lo[b] >= thr[b])).sum()) for b in range(nq)], dtype=np.int64)
    for b in range(nq):
        s[b, min(counts[b], cap):], r[b, min(counts[b], cap):] = 0.0, -1
    return s, r, counts
