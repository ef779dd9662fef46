"""The oracle of a filtered search (include/rq.h rq_search_filtered) and the masks the tests share.

The top-k is taken over the allowed rows only, in the canonical order (score descending, then row ascending): the canonical
scores of oracle/dense_oracle.py restricted to the allowed columns, ranked by its own topk_from_scores, and mapped back
through the ASCENDING array of allowed rows, so ties stay in row order.  k_eff = min(k, allowed rows); the rest is (0.0, -1)."""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc


def filtered_topk_from_scores(scores: np.ndarray, mask: np.ndarray, k: int, row_offset: int = 0):
    """scores [B][N] canonical fp32 scores (orc.exact_scores), mask [N] bool -> (scores [B][k], rows [B][k], -1 padded)."""
    allowed = np.flatnonzero(np.asarray(mask, dtype=bool))
    B = scores.shape[0]
    if allowed.size == 0:
        return np.zeros((B, k), np.float32), np.full((B, k), -1, np.int64)
    s, r = orc.topk_from_scores(np.ascontiguousarray(scores[:, allowed]), k)
    ok = r >= 0
    return s, np.where(ok, allowed[np.where(ok, r, 0)] + row_offset, -1)


def filtered_topk(q, x16, mask, k, metric=orc.METRIC_COSINE, row_offset=0):
    """dense_topk(q, x16[allowed], k) with the rows mapped back through the ascending `allowed` array."""
    allowed = np.flatnonzero(np.asarray(mask, dtype=bool))
    q = np.atleast_2d(np.asarray(q, np.float32))
    if allowed.size == 0:
        return np.zeros((q.shape[0], k), np.float32), np.full((q.shape[0], k), -1, np.int64)
    s, r = orc.dense_topk(q, x16[allowed], k, metric)
    ok = r >= 0
    return s, np.where(ok, allowed[np.where(ok, r, 0)] + row_offset, -1)


def pack_bits_reference(mask: np.ndarray) -> np.ndarray:
    """The C bit order spelled out: bit r % 32 of uint32 word r / 32 (independent of numpy's packbits)."""
    mask = np.asarray(mask, dtype=bool)
    words = np.zeros((mask.size + 31) // 32, dtype=np.uint32)
    for r in np.flatnonzero(mask).tolist():
        words[r // 32] |= np.uint32(1) << np.uint32(r % 32)
    return words


def rotation_mask(n: int, seed: int = 3) -> np.ndarray:
    """Bins (64 rows) with exactly 0, 1, 2, 3 and 64 allowed rows in rotation (a ragged last bin: as many as it has)."""
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, dtype=bool)
    for b in range((n + 63) // 64):
        rows = np.arange(64 * b, min(64 * b + 64, n))
        want = min((0, 1, 2, 3, 64)[b % 5], rows.size)
        mask[rng.choice(rows, size=want, replace=False)] = True
    return mask


def standard_masks(n: int, top3_rows=None) -> dict:
    """The masks of tests/test_gpu_filter.py over n rows; top3_rows: rows to exclude (each query's unfiltered top 3)."""
    rng = np.random.default_rng(11)
    m = {"random50": rng.random(n) < 0.5,
         "one_per_bin": np.arange(n) % 64 == 7,
         "rotation": rotation_mask(n),
         "contiguous10": (np.arange(n) >= n // 4) & (np.arange(n) < n // 4 + n // 10),
         "five_rows": np.isin(np.arange(n), [3, n // 6, n // 6 + 1, n // 2, n - 1]),
         "none": np.zeros(n, dtype=bool),
         "all": np.ones(n, dtype=bool)}
    if top3_rows is not None:
        t = np.ones(n, dtype=bool)
        t[np.asarray(top3_rows).reshape(-1)] = False
        m["top3_excluded"] = t
    return m
