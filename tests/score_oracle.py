"""Oracle for scoring given rows (include/rq.h rq_score_rows_device / rq_score_rows) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`pairs` is oracle.dense_oracle.exact_scores taken along the lists: the canonical fp32 score of every (query, row) pair on the STORED
fp16 rows, a NaN score mapped to -inf ("as for every score"), an absent entry -- outside [row_offset, row_offset + N), -1 included --
0.0, the reference's own value for "not scored" (rag_uq/streaming_index.py:498-499)."""
import numpy as np

from oracle import dense_oracle as orc


def pairs(q, x16, rows, metric=orc.METRIC_COSINE, row_offset=0, scores=None):
    """q [B][dim] fp32, x16 [N][dim] fp16, rows [B][m] global rows -> float32 [B][m].  `scores`: exact_scores(q, x16, metric) when
    the caller has computed it already (a reference shared between tests)."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    rows = np.atleast_2d(np.asarray(rows, dtype=np.int64))
    assert rows.shape[0] == q.shape[0]
    n = x16.shape[0]
    local = rows - row_offset
    present = (rows >= row_offset) & (local < n)
    out = np.zeros(rows.shape, dtype=np.float32)
    if n == 0:
        return out
    for b in range(q.shape[0]):
        if not present[b].any():
            continue
        if scores is not None:
            s = np.asarray(scores[b], dtype=np.float32)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                s = orc.exact_scores(q[b:b + 1], x16, metric)[0]      # one query against every row: the values a search of that query ranks
        s = np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)
        out[b, present[b]] = s[local[b][present[b]]]
    return out
