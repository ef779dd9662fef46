"""The planted corpora of tests/test_select_oracle.py (CPU: every geometry is structured as named and decided by the model) and
tests/test_gpu_select.py (the generic tail and the repair ladder against tests/select_oracle.py on the same corpora).  numpy only.

One Gaussian unit-row background of 200 bins and a ragged last bin hosts one geometry per query (a row planted for query j is
background for every other query).  At k = 10 and the default slack nb = 18 and the widened nb1 = 72 < 201 / 2: the widened pass is
still an approximate pass.  Each case names its query, k, the status of the first generic pass and of the widened pass per metric
(None: whatever the model derives from the records), and whether it is a tie geometry.  Nothing here looks at kernel output.
"""
from __future__ import annotations

import functools

import numpy as np

import select_oracle as so
import tail_cases as tc
import tail_oracle as to

N_MAIN = 200 * 64 + 37      # 12 837 rows: 201 bins, the last one of 37 rows
K = 10
NB = so.nb_default(K)       # 18
NB1 = so.nb_widened(K)      # 72
COS, IP = so.METRIC_COSINE, so.METRIC_IP
NAN_ROWS = [150 * 64 + 5, 151 * 64 + 40, 152 * 64 + 63]      # rows with one NaN element: their score is NaN = -inf for every query, both metrics
TINY = 1e-17                # a query norm below RQ_TINY_QUERY_NORM

assert NB == 18 and NB1 == 72 and 2 * NB1 < (N_MAIN + 63) // 64


def _positions(count, last):
    """Positions 0, 63 and in between, one per bin; `last`: the position inside the ragged last bin (the final entry)."""
    pos = [0, 63] + [(7 + 11 * i) % 64 for i in range(count - 3)]
    return pos + [last]


@functools.lru_cache(maxsize=None)
def main_corpus(dim: int = 768):
    """(x16, queries [6][dim] fp32, cases).  Queries: 0 separated, 1 tied shelf, 2 wide tied shelf, 3 ladder steps, 4 k-th gap, 5 tiny."""
    x = tc._gaussian_unit_rows(N_MAIN, 20401 + dim, dim)
    nbins = (N_MAIN + 63) // 64
    p = tc.Planner(x, 20402, nbins)                      # (G = bins: free_bins hands out any free bin)
    dirs = to.unit(np.random.default_rng(20403).standard_normal((8, dim)))
    eps = to.EPS_DEFAULT
    last = nbins - 1
    cases = []
    # rows that are never candidates: one NaN element each.  `short of rows` allows them.
    p.take(150, 151, 152)
    for r in NAN_ROWS:
        x[r, 3] = np.nan

    # separated: ten winners 0.59 .. 0.50, everything else is background (|cosine| below 0.2)
    bins = p.free_bins(10, lo=3, step=7)
    rows = p.plant(dirs[0], bins, [0, 63, 17, 5, 40, 62, 1, 33, 20, 9], [0.59 - 0.01 * i for i in range(10)])
    cases.append(dict(name="separated", q=0, k=K, status={COS: 0, IP: 0}, widened={COS: None, IP: None}, tie=False, winners=rows))

    # tied shelf: ONE stored row in nb + 5 = 23 bins, the ragged last bin among them; the query is that row
    p.take(last)
    bins = p.free_bins(NB + 4, lo=5, step=5) + [last]
    v1 = to.unit(dirs[1]).astype(np.float32).astype(np.float16)
    rows1 = np.asarray(bins) * 64 + np.asarray(_positions(NB + 5, 36))
    x[rows1] = v1
    cases.append(dict(name="tied shelf", q=1, k=K, status={COS: 1, IP: 1}, widened={COS: 0, IP: 0}, tie=True, ties=np.sort(rows1), nties=NB + 5))

    # wide tied shelf: ONE stored row in 4 nb_default + 5 = 77 bins: the widened pass cannot certify either
    bins = p.free_bins(NB1 + 5, lo=0)
    v2 = to.unit(dirs[2]).astype(np.float32).astype(np.float16)
    rows2 = np.asarray(bins) * 64 + np.asarray(_positions(NB1 + 5, 50))
    x[rows2] = v2
    cases.append(dict(name="wide tied shelf", q=2, k=K, status={COS: 1, IP: 1}, widened={COS: 1, IP: 1}, tie=True, ties=np.sort(rows2), nties=NB1 + 5))

    # ladder steps: 23 bins, five rows well above, then cosines descending in steps of eps / 50 around the k-th (rank 9): the
    # (nb+1)-th bin sits 9 steps = 0.18 eps below s_k, so b + eps exceeds s_k by about 0.8 eps
    bins = p.free_bins(NB + 5, lo=1)
    cosl = [0.59 - 0.01 * i for i in range(5)] + [0.5 - (i - 9) * eps / 50 for i in range(5, NB + 5)]
    rows = p.plant(dirs[3], bins, [(13 * i) % 64 for i in range(NB + 5)], cosl)
    cases.append(dict(name="ladder steps", q=3, k=K, status={COS: None, IP: None}, widened={COS: 0, IP: 0}, tie=False, planted=rows))

    # k-th gap: nine winners 0.59 .. 0.51, then 14 rows from 0.5 down in steps of eps / 50: b + eps lies between s_k and s_(k-1)
    bins = p.free_bins(NB + 5, lo=2)
    cosg = [0.59 - 0.01 * i for i in range(9)] + [0.5 - (i - 9) * eps / 50 for i in range(9, NB + 5)]
    rows = p.plant(dirs[4], bins, [(29 * i) % 64 for i in range(NB + 5)], cosg)
    cases.append(dict(name="k-th gap", q=4, k=K, status={COS: 1, IP: 1}, widened={COS: 0, IP: 0}, tie=False, planted=rows))

    # tiny query: the separated geometry's direction at norm 1e-17: never certified under cosine by an approximate pass
    cases.append(dict(name="tiny query", q=5, k=K, status={COS: 1, IP: 0}, widened={COS: 1, IP: None}, tie=False))

    q = (2.5 * dirs[:6]).astype(np.float32)
    q[1] = v1.astype(np.float32)
    q[2] = v2.astype(np.float32)
    q[5] = (TINY * dirs[0]).astype(np.float32)
    return x, q, cases


def short_filter(cases) -> np.ndarray:
    """short of rows: the filter allows nine of `separated`'s winners and the three rows of NAN_ROWS: 12 > k rows overall.  A scan with
    the filter's row scale scores an excluded row NaN, which the records clamp to the smallest value -- the same as the maximum of a
    bin whose only allowed row scores NaN.  So every bin but the nine winners' ties at the bottom, the order among them is bin
    ascending, and neither nb = 18 nor nb1 = 72 bins reach bins 150 .. 152: nine non-empty keys, have < kk = 10, status 1 twice.
    (With finite rows alone `have < kk` cannot happen: each re-scored bin holds the allowed row that made its maximum, and
    nb >= k.)"""
    allowed = np.zeros(N_MAIN, dtype=bool)
    allowed[np.asarray(cases["separated"]["winners"])[:9]] = True
    allowed[NAN_ROWS] = True
    return allowed


@functools.lru_cache(maxsize=None)
def negative_shelf_corpus(dim: int = 768):
    """All-negative, tied-shelf form: N_MAIN rows norm * (-c u + noise), c in 0.42 .. 0.60, norm 0.5 .. 2; ONE row of norm 0.5 and cosine
    -0.1 in nb + 5 bins (the ragged last bin among them).  The query is 3 u: every score is negative, the tied rows are the best."""
    rng = np.random.default_rng(20411 + dim)
    u = to.unit(rng.standard_normal(dim))
    x = np.empty((N_MAIN, dim), dtype=np.float16)
    to.plant(x, np.arange(N_MAIN), -rng.uniform(0.42, 0.60, N_MAIN), u, rng, norms=rng.uniform(0.5, 2.0, N_MAIN))
    nbins = (N_MAIN + 63) // 64
    one = np.empty((1, dim), dtype=np.float16)
    to.plant(one, [0], [-0.1], u, rng, norms=[0.5])
    bins = [4 + 8 * i for i in range(NB + 4)] + [nbins - 1]
    rows = np.asarray(bins) * 64 + np.asarray(_positions(NB + 5, 36))
    x[rows] = one[0]
    cases = [dict(name="negative tied shelf", q=0, k=K, status={COS: 1, IP: 1}, widened={COS: 0, IP: 0}, tie=True, ties=np.sort(rows), nties=NB + 5)]
    return x, (3.0 * u[None, :]).astype(np.float32), cases


def negative_separated(dim: int = 768):
    """All-negative, separated form: tests/tail_cases.py negative_corpus (8 229 rows = 129 bins, so its widened pass would be the exact
    route; it is never needed: status 0 at the first generic pass)."""
    x, q, cases = tc.negative_corpus(dim)
    return x, q, [dict(name="negative separated", q=0, k=K, status={COS: 0, IP: 0}, widened={COS: None, IP: None}, tie=False, winners=cases[0]["winners"])]


@functools.lru_cache(maxsize=None)
def small_corpus(nbins: int, dim: int = 768):
    """nbins - 1 whole bins and a ragged one of 37 rows, Gaussian; four Gaussian queries."""
    n = (nbins - 1) * 64 + 37
    return tc._gaussian_unit_rows(n, 20420 + nbins, dim), np.random.default_rng(20430 + nbins).standard_normal((4, dim)).astype(np.float32)


# (k, slack_bins 0 -> nb = k, bins): 3 bins is the smallest shard that is not the exact route at nb = 1, 7 at nb = 3
SMALL = [dict(k=1, nbins=3, exact=False), dict(k=1, nbins=2, exact=True), dict(k=3, nbins=7, exact=False), dict(k=3, nbins=6, exact=True),
         dict(k=3, nbins=3, exact=True)]

K321_BINS = 723             # nb_default(321) = 361: 722 bins would be the exact route
K1024_BINS = 6143           # nb1 = min(3071, 4 * 1152) = 3071: 6142 bins would make the widened pass the exact route


@functools.lru_cache(maxsize=None)
def k321_corpus():
    n = (K321_BINS - 1) * 64 + 37
    return tc._gaussian_unit_rows(n, 20441, 768), np.random.default_rng(20442).standard_normal((3, 768)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def k1024_corpus():
    n = (K1024_BINS - 1) * 64 + 5
    return tc._gaussian_unit_rows(n, 20451, 32), np.random.default_rng(20452).standard_normal((2, 32)).astype(np.float32)


def filler_queries(count: int, dim: int, seed: int = 20461) -> np.ndarray:
    return np.random.default_rng(seed + dim).standard_normal((count, dim)).astype(np.float32)
