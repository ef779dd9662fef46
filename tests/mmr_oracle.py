"""The oracle of an MMR selection (include/rq.h rq_mmr_select_device / rq_search_mmr), step by step as the header defines it.

Per query: candidate positions 0..m-1, each a global row (absent: -1, outside the shard, or a NaN relevance) and a relevance.
sim(i, j) is the canonical score of oracle/dense_oracle.py with the STORED row j as the query: exact_scores(x16[row_j] as
float32, x16[candidate rows], metric) -- a NaN counts as -inf.  pen (float32) is 0 before the first pick, afterwards the maximum
of sim over the picked rows.  v = lam * float64(rel) - (1 - lam) * float64(pen): two products and a subtraction in float64 (numpy
never fuses), a term whose weight is exactly 0 being 0 whatever its other factor; a NaN v counts as -inf.  A step takes the greatest v among the present, unselected candidates, the lowest position
on equal v.  k_eff = min(k, present); the rest is (0.0, -1, 0.0)."""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc

import filter_oracle as fo


def _sims(x16, picked_local, cand_local, metric):
    """float32 [len(picked)][len(cand)]: sim of every candidate row to every picked row, NaN -> -inf."""
    s = orc.exact_scores(x16[np.asarray(picked_local, np.int64)].astype(np.float32), x16[np.asarray(cand_local, np.int64)], metric)
    return np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)


def _values(rel, pen, lam):
    lam, oml = np.float64(lam), np.float64(1.0) - np.float64(lam)
    with np.errstate(invalid="ignore"):
        gain = lam * rel.astype(np.float64) if lam != 0 else np.zeros(rel.shape)      # a term whose weight is exactly 0 is 0
        loss = oml * pen.astype(np.float64) if oml != 0 else np.zeros(pen.shape)
        v = gain - loss
    return np.where(np.isnan(v), -np.inf, v)


def _best(v, live):
    c = np.flatnonzero(live)
    return int(c[np.argmax(v[c])])          # argmax: the first of equal maxima = the lowest position


def present_mask(rel, rows, n_rows, row_offset=0):
    rel, rows = np.asarray(rel, np.float32), np.asarray(rows, np.int64)
    return (rows >= 0) & (rows >= row_offset) & (rows < row_offset + n_rows) & ~np.isnan(rel)


def mmr_select(rel, rows, x16, k, lam, metric=orc.METRIC_COSINE, row_offset=0, follow=None):
    """One query.  rel [m] float32, rows [m] global rows -> (scores [k], rows [k], mmr [k]) in selection order.

    follow (optional): positions some implementation picked, in its order.  The state of step t is then built from follow[:t]
    and the returned arrays hold what THIS oracle picks at every step from that state (the relevance, row and v of its own
    choice), so a divergence shows at the step where it happens and does not cascade; a fourth result lists the positions."""
    rel, rows = np.asarray(rel, np.float32), np.asarray(rows, np.int64)
    m = rel.size
    live = present_mask(rel, rows, x16.shape[0], row_offset)
    local = np.where(live, rows - row_offset, 0)
    k_eff = min(int(k), int(live.sum())) if follow is None else len(follow)
    out_s, out_r, out_v = np.zeros(k, np.float32), np.full(k, -1, np.int64), np.zeros(k, np.float32)
    pos = []
    pen = np.zeros(m, np.float32)
    sims = None
    if follow is not None and len(follow) > 1:
        sims = _sims(x16, local[np.asarray(follow[:-1], np.int64)], local, metric)      # one product for the whole path
    for t in range(k_eff):
        p = _best(_values(rel, pen, lam), live)
        out_s[t], out_r[t], out_v[t] = rel[p], rows[p], np.float32(_values(rel, pen, lam)[p])
        pos.append(p)
        if follow is not None:
            p = int(follow[t])
        live[p] = False
        if t + 1 < k_eff:
            s = sims[t] if sims is not None else _sims(x16, [local[p]], local, metric)[0]
            pen = s.copy() if t == 0 else np.maximum(pen, s)
    return (out_s, out_r, out_v, pos) if follow is not None else (out_s, out_r, out_v)


def mmr_select_batch(rel, rows, x16, k, lam, metric=orc.METRIC_COSINE, row_offset=0):
    out = [mmr_select(rel[b], rows[b], x16, k, lam, metric, row_offset) for b in range(len(rel))]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def mmr_topk(q, x16, k, fetch_k, lam, metric=orc.METRIC_COSINE, mask=None, row_offset=0):
    """rq_search_mmr: the exact top min(fetch_k, rows in play) (filtered by `mask` when given), then the selection."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    n_play = x16.shape[0] if mask is None else int(np.asarray(mask, bool).sum())
    m = max(int(k), min(int(fetch_k), n_play))
    if mask is None:
        s, r = orc.dense_topk(q, x16, m, metric, row_offset)
    else:
        s, r = fo.filtered_topk(q, x16, mask, m, metric, row_offset)
    return mmr_select_batch(s, r, x16, k, lam, metric, row_offset)


def naive_gram_mmr(rel, x16_rows, k, lam, metric=orc.METRIC_COSINE):
    """The textbook form over the whole Gram matrix of the candidates (all present): an independent restatement for small inputs."""
    rel = np.asarray(rel, np.float32)
    m = rel.size
    gram = orc.exact_scores(x16_rows.astype(np.float32), x16_rows, metric)       # gram[j][i] = sim(i, j), row j as the query
    chosen, vals = [], []
    for _ in range(min(k, m)):
        best, best_v = -1, None
        for i in range(m):
            if i in chosen:
                continue
            pen = np.float32(max(gram[j][i] for j in chosen)) if chosen else np.float32(0.0)
            v = np.float64(lam) * np.float64(rel[i]) - (np.float64(1.0) - np.float64(lam)) * np.float64(pen)
            if best < 0 or v > best_v:
                best, best_v = i, v
        chosen.append(best)
        vals.append(np.float32(best_v))
    return chosen, vals
