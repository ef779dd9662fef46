"""A host model of the generic sorted tail, the repair ladder and the key merge (csrc/rq_select.hip, rq_search.hip fixup_ladder,
rq_plan.h): numpy, fp64 and exact fp32, no library import.

Unlike the fast tail's model (tests/tail_oracle.py), which reasons from exact scores through error bands, the generic tail is a
FUNCTION of the bin records the scan wrote: rq_select_bins_kernel sorts the records' maxima, rq_rescore_kernel re-scores the first
nb bins exactly, rq_final_kernel ranks those rows and compares the (nb+1)-th maximum with the k-th exact score.  So the model takes
the records as the device wrote them (rq_debug_bin_records) -- or, on the CPU, records made from exact scores with
tests/bin_records.py records_from_scores -- and repeats that arithmetic line for line.  The one thing numpy does not reproduce bit
for bit is the fp64 sum order of a re-scored row (about 1e-16 relative before the one rounding to fp32, rq_exact.hip header): a
query whose fp32 bound lies within UNDECIDED_ULPS = 4 ulps of s_k is reported as undecided, never guessed.

Keys (csrc/rq_device.h): key = mono32(score) << 32 | (0xffffffff - index); larger key = better rank (score descending, index
ascending); 0 is the empty slot; a NaN score counts as -inf (rq_sanitize) and -0.0 ranks with +0.0 (rq_make_key).
"""
from __future__ import annotations

import numpy as np

BIN = 64                   # RQ_BIN_ROWS
NB_MAX = 3071              # RQ_NB_MAX (rq_index.h)
MAX_K = 1024               # RQ_MAX_K
TINY_QUERY_NORM = 2e-17    # RQ_TINY_QUERY_NORM (rq_final_body.h)
UNDECIDED_ULPS = 4.0
METRIC_COSINE, METRIC_IP = 0, 1


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def _bits(f) -> np.ndarray:
    return np.array(f, dtype=np.float32, copy=True).reshape(np.shape(f)).view(np.uint32)


def mono32(f) -> np.ndarray:
    u = _bits(f)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unmono32(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return np.array(np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k), dtype=np.uint32).view(np.float32)


def sanitize(f) -> np.ndarray:
    f = np.array(f, dtype=np.float32, copy=True)
    return np.where(np.isnan(f), np.float32(-np.inf), f).astype(np.float32)


def make_key(score, index) -> np.ndarray:
    """rq_make_key (the score must not be NaN: rq_sanitize first, as every caller on the device does)."""
    s = np.array(score, dtype=np.float32, copy=True)
    s = np.where(s == 0, np.float32(0.0), s).astype(np.float32)
    idx = np.asarray(index, dtype=np.uint64)
    return (mono32(s).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)


def key_score(key) -> np.ndarray:
    return unmono32((np.asarray(key, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32))


def key_index(key) -> np.ndarray:
    return (np.uint64(0xFFFFFFFF) - (np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


def topm(keys, m: int) -> np.ndarray:
    """rq_wg_topm: the best min(m, non-empty keys) keys of one list, descending.  A sort."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    srt = np.sort(keys[keys != 0])[::-1]
    return srt[:m]


def merge(keys, k: int) -> tuple:
    """rq_merge_keys_kernel: keys [B][n] -> (scores [B][k], rows [B][k], keys [B][k]); an empty slot is (0.0, -1, 0)."""
    keys = np.asarray(keys, dtype=np.uint64)
    B = keys.shape[0]
    out_k = np.zeros((B, k), dtype=np.uint64)
    for b in range(B):
        t = topm(keys[b], k)
        out_k[b, :t.size] = t
    empty = out_k == 0
    sc = np.where(empty, np.float32(0.0), key_score(out_k)).astype(np.float32)
    rows = np.where(empty, np.int64(-1), key_index(out_k)).astype(np.int64)
    return sc, rows, out_k


# ---- the ladder (rq_plan.h nb_default / plan_call, rq_search.hip fixup_ladder) -----------------------------------------------------
def nb_default(k: int, slack_bins: int = -1) -> int:
    return k + (slack_bins if slack_bins >= 0 else max(8, k // 8))


def nb_widened(k: int, slack_bins: int = -1) -> int:
    return min(NB_MAX, 4 * nb_default(k, slack_bins))


def exact_route(nb: int, nbins: int) -> bool:
    """Fewer than two bins per wanted bin: the pass re-scores every bin and certifies whatever it finds."""
    return 2 * nb >= nbins


def ladder_counts(status_first, status_widened) -> dict:
    """Counter movements of rq_search_fixup_device over one call.  status_first [B]: the unrepaired status of every query;
    status_widened: {query: status of its widened pass} for the queries that were not certified."""
    bad = [int(q) for q in np.nonzero(np.asarray(status_first) != 0)[0]]
    exact = [q for q in bad if status_widened[q] != 0]
    return {"repaired": len(bad), "widened": len(bad), "exact_scans": len(exact), "bad": bad, "exact": exact}


# ---- the generic tail of one query -----------------------------------------------------------------------------------------------
def exact_row_scores(q, x16_rows, metric: int) -> np.ndarray:
    """The score definition on a few stored rows (oracle/dense_oracle.py exact_scores): fp64, one rounding to fp32."""
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    x64 = np.asarray(x16_rows).astype(np.float64)
    dot = x64 @ q64
    if metric == METRIC_COSINE:
        qn = np.sqrt((q64 * q64).sum())
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            dot = dot / (qn * np.sqrt((x64 * x64).sum(1)) + 1e-30)
    with np.errstate(over="ignore", invalid="ignore"):
        return dot.astype(np.float32)


def certified(b: float, eps: float, max_row_norm: float, qn: float, metric: int, sk) -> tuple:
    """rq_certified (csrc/rq_device.h) in the same fp64 / fp32 steps; returns (certified, the fp32 bound)."""
    b = np.float64(b); eps = np.float64(np.float32(eps)); mrn = np.float64(np.float32(max_row_norm)); qn = np.float64(qn)
    with np.errstate(over="ignore", invalid="ignore"):
        bound = b + eps
        if metric != METRIC_COSINE:
            v = (b + eps * mrn) * qn
            bound = v * (1.0 + 1e-6) if v >= 0 else v * (1.0 - 1e-6)
        fb = np.float32(bound)
    return bool(fb < np.float32(sk)), fb


def select_bins(rec: np.ndarray, m: int, tie_bin_descending: bool = False) -> np.ndarray:
    """rq_select_bins_kernel: keys of the m best bins by the record's maximum with its 6 low bits cleared (rq_rec_m1; NaN counts as
    -inf), then bin ascending.  (tie_bin_descending: a wrong selection, for tests/test_select_oracle.py.)"""
    rec = np.asarray(rec, dtype=np.uint32)
    m1 = sanitize(np.array(rec[:, 0] & np.uint32(0xFFFFFFC0), dtype=np.uint32).view(np.float32))
    bins = np.arange(rec.shape[0], dtype=np.uint64)
    if tie_bin_descending:
        order = np.lexsort((-bins.astype(np.int64), -mono32(m1).astype(np.int64)))
        return make_key(m1, bins)[order][:m]
    return topm(make_key(m1, bins), m)


def generic_tail(rec: np.ndarray, x16: np.ndarray, q: np.ndarray, k: int, nb: int, metric: int, eps: float, max_row_norm: float,
                 allowed=None, mutant: str = None, next_rec: np.ndarray = None) -> dict:
    """One query through rq_select_bins_kernel, rq_rescore_kernel and rq_final_kernel.
    rec [nbins][2]: the query's bin records; x16 [n][dim]: the shard; q [dim] fp32; eps: eps_cosine / eps_ip and max_row_norm as the
    index reports them (the kernel is handed max_row_norm * (1 + 1e-6) as fp32, rq_search.hip generic_tail); allowed: bool [n] or None.
    mutant: one of the wrong certificates of tests/test_select_oracle.py ("eps_dropped", "le", "kth_minus_2", "bin_ties_descending",
    "next_query_key": the (nb+1)-th key of next_rec).
    Returns bins (the m = nb + 1 best, best first), rows / scores (top k of the re-scored rows, padded with -1 / 0.0), have, kk,
    status (None = undecided), margin (ulps of s_k between the fp32 bound and s_k; None where no bound is compared), why."""
    rec = np.asarray(rec, dtype=np.uint32)
    n, nbins = x16.shape[0], rec.shape[0]
    assert nbins == (n + BIN - 1) // BIN
    q = np.asarray(q, dtype=np.float32)
    qn = float(np.sqrt((q.astype(np.float64) ** 2).sum()))
    n_rows = n if allowed is None else int(np.asarray(allowed, dtype=bool).sum())      # the rows that can be returned
    kk = min(k, n_rows)
    out = {"k": k, "nb": nb, "kk": kk, "margin": None, "bound": None, "sk": None}
    rows_out = np.full(k, -1, dtype=np.int64); sc_out = np.zeros(k, dtype=np.float32)
    if exact_route(nb, nbins):                 # plan_call: every bin re-scored, rq_final_kernel `nbins <= nb`
        binkeys = None
        bins = np.arange(nbins, dtype=np.int64)
        resc = bins
    else:
        assert nb <= NB_MAX
        binkeys = select_bins(rec, nb + 1, tie_bin_descending=(mutant == "bin_ties_descending"))
        bins = key_index(binkeys)
        resc = bins[:nb]
    out["bins"] = bins
    if qn == 0.0:                              # rq_final_kernel: a zero-norm query scores every row 0, the first rows that can be returned
        first = np.arange(n) if allowed is None else np.nonzero(np.asarray(allowed, dtype=bool))[0]
        rows_out[:kk] = first[:kk]
        out.update(rows=rows_out, scores=sc_out, have=kk, status=0, why="zero query")
        return out
    cand = (resc[:, None] * BIN + np.arange(BIN)[None, :]).reshape(-1)
    cand = cand[cand < n]
    if allowed is not None:                    # rq_mask_keys: the keys of excluded rows become 0
        cand = cand[np.asarray(allowed, dtype=bool)[cand]]
    s = sanitize(exact_row_scores(q, x16[cand], metric))
    keys = topm(make_key(s, cand), k)
    have = int(keys.size)
    rows_out[:have] = key_index(keys); sc_out[:have] = key_score(keys)
    out.update(rows=rows_out, scores=sc_out, have=have)
    if binkeys is None:
        out.update(status=0, why="whole shard re-scored")
    elif have < kk or (metric == METRIC_COSINE and qn < TINY_QUERY_NORM):
        out.update(status=1, why="have < kk" if have < kk else "tiny query")
    elif kk == 0:
        out.update(status=0, why="kk == 0")
    else:
        src = binkeys
        if mutant == "next_query_key":
            src = select_bins(next_rec, nb + 1)
        bkey = src[nb] if src.size > nb else np.uint64(0)
        if bkey == 0:
            out.update(status=0, why="no (nb+1)-th bin")
        else:
            b = float(key_score(bkey))
            sk = np.float32(key_score(keys[kk - 1 - (1 if mutant == "kth_minus_2" else 0)]))
            mrn32 = np.float32(max_row_norm * (1.0 + 1e-6))
            ok, fb = certified(b, 0.0 if mutant == "eps_dropped" else eps, mrn32, qn, metric, sk)
            if mutant == "le":
                ok = bool(fb <= sk)
            with np.errstate(invalid="ignore", over="ignore"):
                ulp = float(np.spacing(np.abs(sk))) if np.isfinite(sk) else np.inf
                margin = (float(fb) - float(sk)) / ulp if np.isfinite(fb) and np.isfinite(sk) else (np.inf if not ok else -np.inf)
            out.update(margin=margin, bound=float(fb), sk=float(sk), b=b, why="certificate")
            out["status"] = (0 if ok else 1) if (abs(margin) > UNDECIDED_ULPS or mutant) else None
    return out


# ---- rq_wg_topm step by step (for the statements about its paths; the expected values of every test come from topm, a sort) -----------
SEL_THREADS, SEL_L = 1024, 4096


def wg_topm_steps(keys, m: int, thr_at: int = -1, compact_at: int = SEL_L - SEL_THREADS + 1) -> dict:
    """The chunk loop of rq_wg_topm: chunks of 1 024 keys, a key joins the LDS list when it beats the threshold of the last compaction,
    the list is sorted and cut to m when it holds more than 3 072 keys (or at the last chunk).  thr_at / compact_at: the right values are
    m - 1 + 0 (list[m - 1]) and 3 073; others are the wrong selections of tests/test_select_oracle.py.  Returns the result, the number of
    compactions, the keys the threshold kept out and the largest list length (beyond 4 096 the kernel would write past its LDS list)."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    lst = np.zeros(0, dtype=np.uint64)
    thr = np.uint64(0)
    out = {"compactions": 0, "pruned": 0, "longest": 0}
    n = keys.size
    for base in range(0, n, SEL_THREADS):
        chunk = keys[base:base + SEL_THREADS]
        take = chunk[chunk > thr]
        out["pruned"] += int((chunk != 0).sum() - take.size)
        lst = np.concatenate([lst, take])
        out["longest"] = max(out["longest"], int(lst.size))
        last = base + SEL_THREADS >= n
        if lst.size >= compact_at or last:
            srt = np.sort(lst)[::-1]
            pos = m + thr_at
            thr = srt[pos] if srt.size >= m and pos < srt.size else np.uint64(0)
            lst = srt[:m]
            out["compactions"] += 1
    out["result"] = lst if n else np.zeros(0, dtype=np.uint64)
    return out
