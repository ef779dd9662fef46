"""The score definition of include/rq.h for non-finite and extreme inputs -- TEST INFRASTRUCTURE.

oracle/dense_oracle.py states the arithmetic for finite inputs; a NaN breaks its topk_from_scores.  include/rq.h adds three
rules, for both metrics and every route, and this module restates them on top of orc.exact_scores:
  * a NaN score counts as -inf;
  * a zero-norm query scores every row 0.0, whatever the row holds: its answer is rows 0 .. k_eff-1 at 0.0;
  * +-inf scores are legitimate and order like any other (score descending, then row ascending); a -inf row is still a row,
    k_eff = min(k, N) does not shrink.
-0.0 is returned as +0.0 (rq_make_key).  Used by tests/test_nonfinite.py (CPU) and tests/test_gpu_nonfinite.py.
"""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc

import filter_oracle as fo

N_A = 4_101          # 64 whole bins and a ragged one of 5 rows: the smallest shape that still takes the approximate route at k = 10


def scores(q, x16, metric=orc.METRIC_COSINE) -> np.ndarray:
    """Canonical fp32 scores [B][N] under the rules above."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    with np.errstate(all="ignore"):
        s = orc.exact_scores(q, x16, metric)
        q64 = q.astype(np.float64)
        zero = np.sqrt((q64 * q64).sum(axis=1)) == 0.0
    s[np.isnan(s)] = -np.inf
    s[zero] = 0.0
    s[s == 0] = 0.0
    return s


def topk(q, x16, k, metric=orc.METRIC_COSINE, row_offset=0, mask=None):
    """(scores [B][k], rows [B][k]) in the canonical order, padded with (0.0, -1); mask: the allowed rows of a filtered search."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    if x16.shape[0] == 0:
        return np.zeros((q.shape[0], k), np.float32), np.full((q.shape[0], k), -1, np.int64)
    s = scores(q, x16, metric)
    if mask is None:
        return orc.topk_from_scores(s, k, row_offset)
    return fo.filtered_topk_from_scores(s, mask, k, row_offset)


def assert_matches(got_scores, got_rows, want_scores, want_rows, tol, what=""):
    """Rows exactly; scores bit for bit where the oracle's are non-finite, within tol elsewhere."""
    got_scores, want_scores = np.asarray(got_scores, np.float32), np.asarray(want_scores, np.float32)
    assert np.array_equal(got_rows, want_rows), \
        f"{what}: rows differ at (query, rank) {np.argwhere(np.asarray(got_rows) != np.asarray(want_rows))[:4].tolist()}"
    fin = np.isfinite(want_scores)
    assert np.array_equal(got_scores[~fin], want_scores[~fin]), f"{what}: non-finite scores differ"
    assert np.isfinite(got_scores[fin]).all(), f"{what}: a finite score came back non-finite"
    err = float(np.abs(got_scores[fin].astype(np.float64) - want_scores[fin].astype(np.float64)).max(initial=0.0))
    assert err <= tol, f"{what}: scores differ by {err}"
    assert not np.signbit(got_scores[got_scores == 0]).any(), f"{what}: -0.0 returned"


# ---- the shards and queries of the non-finite tests ------------------------------------------------------------------------------
NAN_BIN = (64, 128)          # rows of shard A that are all NaN: one whole bin, a failed embedding batch
PLANTED_A = [5, 200, 300, 2049, 2050, 4099, 4100] + list(range(*NAN_BIN)) + list(range(1000, 1010))


def queries(dim: int, B: int = 64, seed: int = 97) -> np.ndarray:
    """q0, q6 planted matches (Gaussian); q1 all NaN; q2 one +inf element; q3 fp32-subnormal; q4 x 1e36; q5 zero; q7 one -inf
    element; the rest Gaussian."""
    q = orc.synthetic_queries(B, dim, seed=seed)
    q[1] = np.nan
    q[2, 3] = np.inf
    q[3] = (q[3].astype(np.float64) * 1e-40).astype(np.float32)
    q[4] *= np.float32(1e36)
    q[5] = 0.0
    q[7, dim // 2] = -np.inf
    return q


def _direction(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float16)


def shard_a(dim: int, q: np.ndarray, n: int = N_A, seed: int = 4101) -> np.ndarray:
    """synthetic_corpus with the planted rows of the non-finite tests (module docstring of tests/test_gpu_nonfinite.py)."""
    x = orc.synthetic_corpus(n, dim, seed=seed)
    x[5, 7] = np.inf
    x[NAN_BIN[0]:NAN_BIN[1]] = np.nan
    x[200, 1], x[200, 2] = np.inf, -np.inf
    x[300] = np.float16(65504.0)
    x[1000:1010] = 0
    x[2049] = np.nan
    x[2050] = _direction(q[0])
    x[4099] = _direction(q[6])
    x[4100, dim - 1] = -np.inf
    return x


def twin_a(x16: np.ndarray) -> np.ndarray:
    """Shard A with every row that holds a non-finite element zeroed."""
    t = x16.copy()
    t[~np.isfinite(x16.astype(np.float32)).all(axis=1)] = 0
    return t


FINITE_B = [3, 70, 1500, 2048, 2051, 4000, 4100]


def shard_b(dim: int, n: int = N_A, seed: int = 4102) -> np.ndarray:
    """Only the 7 rows FINITE_B are finite, every other row is NaN."""
    x = orc.synthetic_corpus(n, dim, seed=seed)
    keep = x[FINITE_B].copy()
    x[:] = np.nan
    x[FINITE_B] = keep
    return x


def shard_c(dim: int, q: np.ndarray, n: int = 130, seed: int = 130) -> np.ndarray:
    """130 rows (the exact route) with a NaN row, an inf row, a zero row and a planted match in the ragged last bin."""
    x = orc.synthetic_corpus(n, dim, seed=seed)
    x[2] = np.nan
    x[5, 7] = np.inf
    x[9] = 0
    x[70, 0] = -np.inf
    x[129] = _direction(q[0])
    return x
