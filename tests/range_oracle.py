"""Oracle for range searches (include/rq.h rq_search_range*) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The definition restated on top of oracle.dense_oracle.exact_scores (fp64 arithmetic, one rounding to fp32) and the rules of
tests/nonfinite_oracle.py (a NaN score counts as -inf, -0.0 is +0.0, a zero-norm query scores every row 0.0): a row qualifies iff its
fp32 score s satisfies s >= thr[q] (with a mask: allowed rows only); count[q] is the number of qualifying rows, exact also beyond
cap; the outputs are the min(count, cap) best qualifying rows, score descending then row ascending, global rows = row_offset +
local row, padded with (0.0, -1).  A non-finite threshold (the device forms only) returns nothing with count 0."""
import numpy as np

from oracle import dense_oracle as orc

import nonfinite_oracle as nfo


def from_scores(s, thr, cap, row_offset=0, mask=None):
    """s [B][N] canonical fp32 scores (nonfinite_oracle.scores), thr a scalar or [B] -> (scores [B][cap], rows [B][cap], counts [B])."""
    s = np.asarray(s, dtype=np.float32)
    B, n = s.shape
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (B,))
    out_s, out_r, counts = np.zeros((B, cap), np.float32), np.full((B, cap), -1, np.int64), np.zeros(B, np.int64)
    allowed = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    for b in range(B):
        if not np.isfinite(thr[b]):
            continue
        ok = (s[b] >= thr[b]) & allowed
        rows = np.flatnonzero(ok)
        counts[b] = rows.size
        order = np.lexsort((rows, -s[b, rows].astype(np.float64)))[:cap]          # score descending, then row ascending
        m = order.size
        out_s[b, :m] = s[b, rows[order]]
        out_r[b, :m] = rows[order] + row_offset
    out_s[out_s == 0] = 0.0
    return out_s, out_r, counts


def search_range(q, x16, thr, cap, metric=orc.METRIC_COSINE, row_offset=0, mask=None, scores=None):
    """`scores`: nonfinite_oracle.scores(q, x16, metric) when the caller has computed it already (a reference shared between tests)."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    if x16.shape[0] == 0:
        return np.zeros((q.shape[0], cap), np.float32), np.full((q.shape[0], cap), -1, np.int64), np.zeros(q.shape[0], np.int64)
    s = nfo.scores(q, x16, metric) if scores is None else scores
    return from_scores(s, thr, cap, row_offset, mask)


def threshold_for(sorted_desc, target, min_gap, window=8):
    """A threshold that `about target` rows clear: the midpoint of a gap of at least min_gap between neighbouring scores of one query
    (sorted_desc: its finite scores, best first), the nearest such gap within `window` ranks of `target`.  Returns (thr, rows that clear
    it) or None when there is no such gap -- the caller asserts that there is.  target = 0: above the best score."""
    s = np.asarray(sorted_desc, dtype=np.float64)
    if target <= 0:
        return np.float32(s[0] + max(min_gap, abs(s[0]) * 1e-3)), 0
    for d in sorted(range(-window, window + 1), key=abs):
        r = target + d                                   # r rows clear the threshold: it sits between s[r - 1] and s[r]
        if r < 1 or r >= s.size:
            continue
        if s[r - 1] - s[r] >= min_gap:
            t = np.float32((s[r - 1] + s[r]) / 2)
            if s[r - 1] - float(t) >= min_gap / 4 and float(t) - s[r] >= min_gap / 4:
                return t, r
    return None
