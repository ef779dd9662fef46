"""The yardstick of GROUPED hybrid fusion (include/rq.h rq_hybrid_set_groups, rq_hybrid_fuse_grouped*), in pure numpy, with no import of
the code under test: the ranking of tests/hybrid_oracle.py over ALL K1 + K2 candidates -- validity, the merge of a key held by both
pools, the maxima and h taken before any collapse -- followed by the collapse of HybridRetriever._fuse(..., distinct_by=):

    walk     the ranked candidates in order (h descending, equal h by ascending position, a NaN h as -inf)
    keep     the first candidate of every group; key_group[key] == -1 is a group of its own and is always kept
    output   the first top_k kept candidates in hybrid_oracle.fuse's layout; count = min(kept, top_k)
"""
import numpy as np

import hybrid_oracle as ho


def fuse(ks, key_group, sp_rows, sp_scores, de_rows, de_scores, top_k):
    """(keys int32, b, d, h float64, positions int32 -- all [B][top_k] -- and count int32 [B])"""
    key_group = np.asarray(key_group, np.int64)
    assert key_group.shape == (ks["n_keys"],) and (key_group >= -1).all()
    B, n_cand = np.asarray(sp_rows).shape[0], np.asarray(sp_rows).shape[1] + np.asarray(de_rows).shape[1]
    keys, b, d, h, pos, count = ho.fuse(ks, sp_rows, sp_scores, de_rows, de_scores, n_cand)      # the full ranking
    out_keys, out_pos = np.full((B, top_k), -1, np.int32), np.full((B, top_k), -1, np.int32)
    out_b, out_d, out_h = np.zeros((B, top_k)), np.zeros((B, top_k)), np.zeros((B, top_k))
    out_count = np.zeros(B, np.int32)
    for q in range(B):
        seen, kept = set(), []
        for i in range(int(count[q])):
            g = int(key_group[keys[q, i]])
            if g != -1:
                if g in seen:
                    continue
                seen.add(g)
            kept.append(i)
        kept = kept[:top_k]
        n = len(kept)
        out_count[q] = n
        out_keys[q, :n], out_pos[q, :n] = keys[q, kept], pos[q, kept]
        out_b[q, :n], out_d[q, :n], out_h[q, :n] = b[q, kept], d[q, kept], h[q, kept]
    return out_keys, out_b, out_d, out_h, out_pos, out_count


same = ho.same
