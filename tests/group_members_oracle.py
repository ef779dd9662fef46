"""The oracle of a group-members search (include/rq.h "group members"): the best s rows of each of the k best groups, from a full
exact ranking (oracle/dense_oracle.py).

Groups and their rank are tests/group_oracle.py's: a group's winner is its best row in the canonical order (score descending, then
row ascending; NaN counts as -inf, -0.0 is +0.0), groups rank by their winners, a row whose id is negative (GROUP_NONE) is a group
of one.  A group's members are its rows in play in that order; slot j < k_eff holds count = min(s, rows in play of the group)
of them, best first, (0.0, -1) beyond; slots beyond k_eff are (0.0, -1, GROUP_NONE, count 0)."""
from __future__ import annotations

import numpy as np

from oracle import dense_oracle as orc

GROUP_NONE = -1


def canonical(scores) -> np.ndarray:
    """Scores as they rank and leave: NaN -> -inf, -0.0 -> +0.0."""
    s = np.asarray(scores, np.float32)
    return np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32) + np.float32(0.0)


def members(scores, rows, groups, k: int, s: int):
    """One query's rows in play (any order; every one present) -> (scores [k][s], rows [k][s], groups [k], counts [k]): ONE walk down
    the canonical ranking -- a row opens a slot when its group is new and a slot is free, and joins its group's slot while that
    slot holds fewer than s rows."""
    sc = canonical(scores)
    rows = np.asarray(rows, np.int64)
    groups = np.asarray(groups, np.int64)
    order = np.lexsort((rows, -sc.astype(np.float64)))
    out_s, out_r = np.zeros((k, s), np.float32), np.full((k, s), -1, np.int64)
    out_g, out_c = np.full(k, GROUP_NONE, np.int32), np.zeros(k, np.int32)
    slot_of, found = {}, 0
    for i in order.tolist():
        g = int(groups[i])
        key = ("g", g) if g >= 0 else ("row", int(rows[i]))
        j = slot_of.get(key)
        if j is None:
            if found >= k:
                continue
            j = slot_of[key] = found
            out_g[j] = g if g >= 0 else GROUP_NONE
            found += 1
        if j >= 0 and out_c[j] < s:
            out_s[j, out_c[j]], out_r[j, out_c[j]] = sc[i], rows[i]
            out_c[j] += 1
    return out_s, out_r, out_g, out_c


def members_from_scores(scores: np.ndarray, index_groups, k: int, s: int, mask=None, row_offset: int = 0):
    """scores [B][N] canonical fp32 scores (orc.exact_scores) -> (scores [B][k][s], rows [B][k][s], groups [B][k], counts [B][k]) over
    the rows in play (mask [N] bool, None = every row), from the FULL exact ranking; rows are global (row_offset + local row)."""
    B, N = scores.shape
    play = np.arange(N) if mask is None else np.flatnonzero(np.asarray(mask, bool))
    index_groups = np.asarray(index_groups, np.int64)
    res = [members(scores[b, play], play + row_offset, index_groups[play], k, s) for b in range(B)]
    return tuple(np.stack([r[i] for r in res]) for i in range(4))


def members_topk(q, x16, index_groups, k: int, s: int, metric: int = orc.METRIC_COSINE, mask=None, row_offset: int = 0):
    q = np.atleast_2d(np.asarray(q, np.float32))
    return members_from_scores(orc.exact_scores(q, x16, metric), index_groups, k, s, mask, row_offset)


def naive_dict_of_lists(scores, rows, groups, k: int, s: int):
    """The textbook form the oracle is checked against: every group's (score, -row) pairs in a dict of lists, each list sorted, the
    groups sorted by their best pair.  -> [(group, [(row, score), ...]), ...], best group first, at most s members each."""
    lists = {}
    for sc, r, g in zip(canonical(scores).tolist(), np.asarray(rows).tolist(), np.asarray(groups).tolist()):
        lists.setdefault(("g", g) if g >= 0 else ("row", r), []).append((sc, -r))
    for v in lists.values():
        v.sort(reverse=True)
    ranked = sorted(lists.items(), key=lambda kv: kv[1][0], reverse=True)[:k]
    return [(key[1] if key[0] == "g" else GROUP_NONE, [(-nr, sc) for sc, nr in v[:s]]) for key, v in ranked]


def table_sizes(index_groups) -> dict:
    """Rows per id >= 0 as the member table holds them: every stored row, whatever a filter allows."""
    g = np.asarray(index_groups, np.int64)
    ids, counts = np.unique(g[g >= 0], return_counts=True)
    return dict(zip(ids.tolist(), counts.tolist()))


def oversized_queries(out_groups, index_groups, cap: int) -> np.ndarray:
    """[B] bool: the query's top groups include one whose table size exceeds cap (what the fill leaves to the fixup)."""
    size = table_sizes(index_groups)
    return np.array([any(int(g) >= 0 and size.get(int(g), 0) > cap for g in row) for row in np.asarray(out_groups)], dtype=bool)
