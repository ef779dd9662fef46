"""The oracle of a grouped search (include/rq.h "grouped searches"): a host model of the collapse of a candidate list, and the
grouped answer from a full exact ranking (oracle/dense_oracle.py).

A group's winner is its best row in the canonical order (score descending, then row ascending; NaN counts as -inf, -0.0 is +0.0);
groups rank by their winners; a row whose id is negative (GROUP_NONE) is a group of its own.  k_eff = min(k, distinct groups among
the rows in play); the rest is (0.0, -1, GROUP_NONE)."""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc

GROUP_NONE = -1


def present_mask(scores, rows, n_rows: int, row_offset: int = 0) -> np.ndarray:
    """Candidates that take part: a row inside [row_offset, row_offset + n_rows) and a score that is not NaN."""
    rows = np.asarray(rows, np.int64)
    scores = np.asarray(scores, np.float32)
    return (rows >= 0) & (rows >= row_offset) & (rows < row_offset + n_rows) & ~np.isnan(scores)


def collapse(scores, rows, groups, k: int, n_rows: int, row_offset: int = 0):
    """One query's candidates (any order) -> (scores [k], rows [k], groups [k], status): the winners of the k best groups, best
    first; status 0 when the present candidates hold at least k distinct groups, else 1."""
    scores = np.asarray(scores, np.float32)
    rows = np.asarray(rows, np.int64)
    groups = np.asarray(groups, np.int64)
    ok = np.flatnonzero(present_mask(scores, rows, n_rows, row_offset))
    s = scores[ok] + np.float32(0.0)                                    # -0.0 ranks with, and is returned as, +0.0
    order = np.lexsort((rows[ok], -s.astype(np.float64)))               # score descending, then row ascending
    out_s, out_r, out_g = np.zeros(k, np.float32), np.full(k, -1, np.int64), np.full(k, GROUP_NONE, np.int32)
    seen, found = set(), 0
    for i in order.tolist():
        g = int(groups[ok[i]])
        if g >= 0:
            if g in seen:
                continue
            seen.add(g)
        if found < k:
            out_s[found], out_r[found], out_g[found] = s[i], rows[ok[i]], g if g >= 0 else GROUP_NONE
        found += 1
    return out_s, out_r, out_g, 0 if found >= k else 1


def collapse_batch(scores, rows, groups, k: int, n_rows: int, row_offset: int = 0):
    """[B][m] candidates -> (scores [B][k], rows [B][k], groups [B][k], status [B])."""
    res = [collapse(scores[b], rows[b], groups[b], k, n_rows, row_offset) for b in range(len(rows))]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), np.array([r[3] for r in res], np.int32))


def lookup_groups(rows, index_groups, row_offset: int = 0) -> np.ndarray:
    """The ids a collapse without explicit groups sees: the index's id of every candidate row inside the index, GROUP_NONE else."""
    rows = np.asarray(rows, np.int64)
    index_groups = np.asarray(index_groups, np.int64)
    loc = rows - row_offset
    ok = (rows >= 0) & (loc >= 0) & (loc < index_groups.size)
    return np.where(ok, index_groups[np.where(ok, loc, 0)], GROUP_NONE)


def grouped_from_scores(scores: np.ndarray, index_groups, k: int, mask=None, row_offset: int = 0):
    """scores [B][N] canonical fp32 scores (orc.exact_scores) -> the grouped answer (scores, rows, groups, each [B][k]) over the
    rows in play (mask [N] bool, None = every row), from the FULL exact ranking."""
    B, N = scores.shape
    play = np.arange(N) if mask is None else np.flatnonzero(np.asarray(mask, bool))
    index_groups = np.asarray(index_groups, np.int64)
    out = []
    for b in range(B):
        out.append(collapse(scores[b, play], play + row_offset, index_groups[play], k, N, row_offset)[:3])
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def grouped_topk(q, x16, index_groups, k: int, metric: int = orc.METRIC_COSINE, mask=None, row_offset: int = 0):
    q = np.atleast_2d(np.asarray(q, np.float32))
    return grouped_from_scores(orc.exact_scores(q, x16, metric), index_groups, k, mask, row_offset)


def naive_dict_collapse(scores, rows, groups, k: int):
    """The textbook form the oracle is checked against: best (score, -row) per group in a dict, ungrouped rows under their own key,
    then the groups sorted by their best.  Every candidate is taken as present."""
    best = {}
    for s, r, g in zip(np.asarray(scores, np.float32).tolist(), np.asarray(rows).tolist(), np.asarray(groups).tolist()):
        key = ("g", g) if g >= 0 else ("row", r)
        cand = (s + 0.0, -r)
        if key not in best or cand > best[key][0]:
            best[key] = (cand, g if g >= 0 else GROUP_NONE)
    ranked = sorted(best.values(), key=lambda v: v[0], reverse=True)[:k]
    return [(-c[1], c[0], g) for c, g in ranked]                      # (row, score, group), best first
