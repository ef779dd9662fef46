"""The yardstick of the GROUPED sparse top-k (include/rq.h rq_sparse_set_groups, rq_sparse_topk_grouped*), in pure numpy over CSR arrays and
a group table, with no import of the code under test: BM25Index._search_distinct restated.

    scores   added exactly as tests/sparse_oracle.py adds them: float64, in query order, from 0.0
    mask     a document outside the query's allowed set scores 0.0 (tests/sparse_masked_oracle.py: masks, mask_of; None = no masks)
    order    the documents with score > 0 by score descending, exact ties by DESCENDING row
    walk     the first document of every group is kept; group -1 is a group of its own and is never collapsed
    output   the first k kept documents: rows int32 [B][k] (-1 padded), scores float64 [B][k] (0.0 padded), count int32 [B]
"""
import numpy as np

import sparse_masked_oracle as mo
import sparse_oracle as so


def topk(ix, q_indptr, q_tokens, k, groups, masks=None, mask_of=None):
    indptr, rows, contrib, n_docs = ix["indptr"], ix["rows"], ix["contrib"], ix["n_docs"]
    groups = np.asarray(groups, np.int64)
    assert groups.shape == (n_docs,) and (groups >= -1).all()
    B = len(q_indptr) - 1
    out_rows, out_scores, count = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            scores = np.zeros(n_docs, np.float64)
            for j in q_tokens[q_indptr[b]: q_indptr[b + 1]]:
                if 0 <= j < ix["n_tokens"]:
                    lo, hi = indptr[j], indptr[j + 1]
                    scores[rows[lo:hi]] += contrib[lo:hi]
            keep = None if mask_of is None else mo.keep_of(masks, mask_of, b, n_docs)
            if keep is not None:
                scores = np.where(keep, scores, 0.0)
            pos = np.flatnonzero(scores > 0)
            seen, sel = set(), []
            for i in pos[np.lexsort((-pos, -scores[pos]))].tolist():
                if len(sel) >= k:
                    break
                g = int(groups[i])
                if g != -1:
                    if g in seen:
                        continue
                    seen.add(g)
                sel.append(i)
            count[b] = len(sel)
            out_rows[b, :len(sel)] = sel
            out_scores[b, :len(sel)] = scores[sel]
    return out_rows, out_scores, count


def same(got, want):
    """Rows identical, every score identical in its bits, counts identical."""
    return (len(got) == 3 and so.same(got[:2], want[:2]) and np.asarray(got[2]).dtype == np.int32 and np.array_equal(got[2], want[2]))


def group_ids_of(values):
    """Values (None = a group of its own) as int32 ids in first-seen order."""
    table = {}
    return np.array([-1 if v is None else table.setdefault(v, len(table)) for v in values], np.int32)
