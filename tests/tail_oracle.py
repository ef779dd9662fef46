"""A host model of the fast tail (csrc/rq_tail.hip, rq_tail_body.h, rq_final_body.h): numpy / fp64, no library import.

From the EXACT scores of one query over the shard the model derives what the tail must do with ANY bin records the scan may have
written within its error bound: an interval that contains the kernel's threshold T, per bin whether it is a hit and whether it
becomes 1, 2 or 64 row jobs, hits / jobs per chunk, the three overflow conditions, the candidate total as the kernel counts it
(option "tail_stop" = 5) and the unrepaired status of the fp16 scan.  A decision the exact scores do not settle -- a score inside
one of the bands below around T -- is reported as AMBIGUOUS; a geometry is usable only when nothing is.

Units: everything is in the scan's unit-query units (cosine: the score; inner product: dot / |q|), e = the bound the tail was
handed: eps_cosine, or eps_ip * max_row_norm * (1 + 1e-6) (rq_tail_body.h:106, rq_search.hip tail_args).

Bands, each from the code (none is tuned):
  EPS      |scan score - exact| <= e: the tail's own premise (rq_tail_body.h:44, 106), pinned for every scan form by
           tests/test_gpu_bin_records.py I2 / I3 / I6 / I7.  It holds for the per-workgroup maxima too (the same scores).
  POS6     the 6 position bits that replace / are OR-ed into the low mantissa bits (rq_device.h rq_pos_score, rq_record_from_triple:
           `b | 63`): 64 ulp = 2^-17 relative.  (rq_device.h:86 counts the perturbation inside EPS; it is kept separate here,
           which can only make more decisions ambiguous, never fewer.)
  ROUND26  m1 is rounded UP to 26 bits (rq_up26): at most 64 ulp = 2^-17 relative (tests/bin_records.py ROUNDUP26).
  TRUNC20  P is truncated to its 20 leading key bits (rq_tail_body.h:90 `bit >= 12`): 12 mantissa bits dropped, the value moves
           DOWN by at most 2^-11 relative.  The model applies the truncation itself (trunc20) to both ends of P's interval.
  CODE16   c2 / c3 are 16-bit codes rounded up (rq_code16: 7 mantissa bits kept): decode(code(v)) lies in [v, v + 2^-7 |v|]
           (a negative value is truncated toward zero).  The model applies code16 / code16_value itself to both ends.
  FP32     T is computed in fp32 from P (rq_tail_body.h:110): four operations, each within 2^-24 relative of operands below
           |P| + 4 e: 2^-21 (|P| + 4 e) covers them and a contracted multiply-add.
"""
from __future__ import annotations

import numpy as np

HITCAP = 768            # RQ_TAIL_HITCAP
JOBCAP = 2048           # RQ_TAIL_JOBCAP
CAND_CAP = 4096         # RQ_CAND_CAP
BIN = 64                # RQ_BIN_ROWS
WGMAX_STRIDE = 1024     # RQ_WGMAX_STRIDE
TINY_QUERY_NORM = 2e-17 # RQ_TINY_QUERY_NORM
EPS_DEFAULT = 7.0e-4    # RQ_EPS_DEFAULT (rq_index.h)
POS6 = 2.0 ** -17
ROUND26 = 2.0 ** -17
FP32 = 2.0 ** -21
METRIC_COSINE, METRIC_IP = 0, 1


# ---- bit helpers (rq_device.h) -------------------------------------------------------------------------------------------------
def _bits(f) -> np.ndarray:
    return np.array(f, dtype=np.float32, copy=True).reshape(np.shape(f)).view(np.uint32)


def _f32(b) -> np.ndarray:
    return np.array(b, dtype=np.uint32, copy=True).view(np.float32)


def mono32(f) -> np.ndarray:
    u = _bits(f)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unmono32(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return _f32(np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32))


def trunc20(f) -> np.ndarray:
    """The value the 20-bit radix select returns for a key f (rq_tail_body.h:90-96): the low 12 key bits cleared.  A positive
    value loses mantissa bits (toward zero), a negative one has them SET in its own bits (away from zero): lower either way."""
    return unmono32(mono32(f) & np.uint32(0xFFFFF000))


def up16(f) -> np.ndarray:
    f = np.asarray(f, dtype=np.float32)
    u = _bits(np.where(f == 0, np.float32(0), f))
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0xFFFF0000), (u + np.uint32(0xFFFF)) & np.uint32(0xFFFF0000)).astype(np.uint32)


def up26(f) -> np.ndarray:
    f = np.asarray(f, dtype=np.float32)
    u = _bits(np.where(f == 0, np.float32(0), f))
    return _f32(np.where(u & np.uint32(0x80000000), u & np.uint32(0xFFFFFFC0), (u + np.uint32(63)) & np.uint32(0xFFFFFFC0)).astype(np.uint32))


def code16(f) -> np.ndarray:
    u = up16(f)
    return (np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32) >> np.uint32(16)).astype(np.uint32)


def code16_value(c) -> np.ndarray:
    c = np.asarray(c, dtype=np.uint32) & np.uint32(0xFFFF)
    return unmono32((c << np.uint32(16)) | np.where(c & np.uint32(0x8000), np.uint32(0), np.uint32(0xFFFF)).astype(np.uint32))


def _f32_down(v) -> np.ndarray:
    """Largest float32 <= the float64 v."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _f32_up(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


# ---- layout (rq_plan.h scan_grid, rq_scan_body.h:88, rq_tail_body.h:76-100) -------------------------------------------------------
def scan_grid(nquads: int, cu_count: int, wg_per_cu: int) -> int:
    return int(min(nquads, WGMAX_STRIDE, cu_count * wg_per_cu))


def wg_of_quad(nquads: int, G: int) -> np.ndarray:
    """Workgroup b owns quads [b * nquads // G, (b + 1) * nquads // G)."""
    out = np.empty(nquads, dtype=np.int64)
    for b in range(G):
        out[b * nquads // G:(b + 1) * nquads // G] = b
    return out


def npl_of(m: int) -> int:
    return 1 if m <= 8 else (4 if m <= 64 else 8)


def partition_of_quad(nquads: int, G: int, m: int) -> np.ndarray:
    """Partition of workgroup j = j mod (64 * NPL): lane l, slot i reads j = i * 64 + l, then every 64 * NPL-th."""
    return wg_of_quad(nquads, G) % (64 * npl_of(m))


def shard_eps(x16: np.ndarray, metric: int, base: float = EPS_DEFAULT) -> tuple:
    """(eps, max_row_norm) of a shard as rq_plan.h scan_eps derives them: the base bound plus the share of the worst row that
    sits in fp16-subnormal elements (rq_select.hip rq_rownorm_kernel); eps as fp32."""
    x = np.asarray(x16)
    sub = (x.view(np.uint16) & np.uint16(0x7C00)) == 0
    x64 = x.astype(np.float64)
    acc = (x64 * x64).sum(1)
    s = np.where(sub, x64 * x64, 0.0).sum(1)
    ok = np.isfinite(acc)
    mrn = float(np.sqrt(acc[ok].max(initial=0.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = float(np.sqrt(np.where(ok & (s > 0), s / acc, 0.0)).max(initial=0.0))
    ab = float(np.sqrt(np.where(ok, s, 0.0).max(initial=0.0)))
    if metric == METRIC_COSINE:
        return float(np.float32(base + rel * (1.0 + 1e-6))), mrn
    return float(np.float32(base + (ab / mrn * (1.0 + 1e-6) if mrn > 0 else 0.0))), mrn


def tail_bound(eps: float, max_row_norm: float, metric: int) -> float:
    """e of the module docstring, as the kernel forms it in fp32 (rq_search.hip:414, rq_tail_body.h:106)."""
    if metric == METRIC_COSINE:
        return float(np.float32(eps))
    return float(np.float32(eps) * np.float32(max_row_norm * (1.0 + 1e-6)))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _lo(v, e):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), v - e - POS6 * np.abs(v), v)                # EPS, POS6 (-inf: no such row)


def _hi(v, e):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), v + e + (POS6 + ROUND26) * np.abs(v), v)    # EPS, POS6, ROUND26


def _threshold_fp32(P, e, thr_mult, slack):
    """rq_tail_body.h:106-110 in fp32."""
    P = np.float32(P); e = np.float32(e)
    es = np.maximum(e, np.float32(slack))
    return np.float32(np.float32(np.float32(P - e) - np.float32(np.float32(np.float32(thr_mult) - np.float32(1)) * es)) - np.float32(np.float32(4e-6) * np.abs(P)))


def threshold_interval(binmax: np.ndarray, part: np.ndarray, m: int, e: float, thr_mult: float = 2.25, slack: float = 0.0) -> tuple:
    """[T_lo, T_hi] that contains the kernel's T, and the exact m-th largest partition maximum P.  binmax: exact maximum of every
    bin (-inf: no row in play), part: the bin's partition.  Fewer than m partitions that hold anything: T = -inf, every bin."""
    nparts = 64 * npl_of(m)
    pm = np.full(nparts, -np.inf)
    np.maximum.at(pm, part, binmax)
    if m > nparts:
        return -np.inf, -np.inf, -np.inf
    P = float(np.sort(pm)[::-1][m - 1])
    if not np.isfinite(P):                                                  # rq_tail_body.h:101-104
        return -np.inf, -np.inf, P
    p_lo = trunc20(_f32_down(_lo(P, e)))                                    # TRUNC20 of the lowest P the scan may have seen
    p_hi = trunc20(_f32_up(_hi(P, e) - ROUND26 * abs(P)))                   # (the workgroup maxima are not rounded to 26 bits)
    t_lo = float(_threshold_fp32(p_lo, e, thr_mult, slack)); t_hi = float(_threshold_fp32(p_hi, e, thr_mult, slack))
    g = FP32 * (max(abs(float(p_lo)), abs(float(p_hi))) + 4 * e)            # FP32
    return t_lo - g, t_hi + g, P


def _top3(scores: np.ndarray, n: int, allowed=None):
    nbins = (n + BIN - 1) // BIN
    E = np.full(nbins * BIN, -np.inf)
    E[:n] = np.asarray(scores, dtype=np.float64)[:n]
    E[:n] = np.where(np.isnan(E[:n]), -np.inf, E[:n])
    if allowed is not None:
        E[:n] = np.where(np.asarray(allowed, dtype=bool)[:n], E[:n], -np.inf)
    E = E.reshape(nbins, BIN)
    live = np.zeros(nbins * BIN, dtype=bool)
    live[:n] = True if allowed is None else np.asarray(allowed, dtype=bool)[:n]
    top = -np.sort(-E, axis=1)[:, :3]
    return top[:, 0], top[:, 1], top[:, 2], live.reshape(nbins, BIN).sum(1)


def model_query(scores, n: int, k: int, e: float, G: int, nv: int = 1, tail_local: bool = True, metric: int = METRIC_COSINE,
                qnorm: float = 1.0, allowed=None, thr_mult: float = 2.25, slack: float = 0.0) -> dict:
    """The tail of one query.  scores: exact scores [n] in unit-query units (fp64 kept); e: tail_bound(); G: the scan grid of the
    pass that held the query; nv: the tail's chunk is 512 * nv bins; allowed: the filter's rows (bool [n]) or None.
    Returns T_lo / T_hi / P, per bin `hit` and `jobs` (-1 = ambiguous), `ambiguous` (bins), per chunk nh / njob, the overflow
    flags, `total` (None where the kernel's own count is not determined: more than HITCAP hits of unequal job counts), `have`
    and `status`."""
    nbins = (n + BIN - 1) // BIN
    s1, s2, s3, nlive = _top3(scores, n, allowed)
    rows_in_play = int(nlive.sum())
    m = int(min(k, rows_in_play))
    out = {"n": n, "k": k, "m": m, "G": G, "nv": nv}
    if qnorm == 0.0:                                                        # rq_final_body.h:115: rows 0 .. kk-1, status 0
        out.update(status=0, zero_query=True, ambiguous=np.zeros(0, dtype=np.int64), total=None)
        return out
    part = partition_of_quad(nbins, G, max(m, 1))
    t_lo, t_hi, P = threshold_interval(s1, part, max(m, 1), e, thr_mult, slack)
    with np.errstate(invalid="ignore", over="ignore"):
        # hit: rq_rec_m1(x) >= T, m1 in [lo(S1), hi(S1)] (rq_tail_body.h:134)
        hit_yes = _lo(s1, e) >= t_hi
        hit_no = ~(_hi(s1, e) >= t_lo)
        # two: decode(c2) >= T (rq_tail_body.h:139); CODE16 applied to both ends of the second-largest approximate score
        c2lo, c2hi = code16(_f32_down(_lo(s2, e))), code16(_f32_up(_hi(s2, e)))
        two_yes = code16_value(c2lo).astype(np.float64) >= t_hi
        two_no = ~(code16_value(c2hi).astype(np.float64) >= t_lo)
        # whole: decode(c2 - d) >= T, d = min(c2 - c3, 1023): decode(max(c3, c2 - 1023)), monotone in both codes
        c3lo, c3hi = code16(_f32_down(_lo(s3, e))), code16(_f32_up(_hi(s3, e)))
        sat = lambda c2, c3: np.where(c2 - np.minimum(c3, c2) > 1023, c2 - np.uint32(1023), np.minimum(c3, c2)).astype(np.uint32)
        whole_yes = two_yes & (code16_value(sat(c2lo, c3lo)).astype(np.float64) >= t_hi)
        whole_no = two_no | ~(code16_value(sat(c2hi, c3hi)).astype(np.float64) >= t_lo)
    if t_hi == -np.inf:                                                     # T = -inf: every bin, every row (x >= -inf holds for -inf too)
        hit_yes = np.ones(nbins, dtype=bool); hit_no = ~hit_yes
        two_yes = hit_yes.copy(); two_no = hit_no.copy(); whole_yes = hit_yes.copy(); whole_no = hit_no.copy()
    hit = np.where(hit_yes, 1, np.where(hit_no, 0, -1))
    jobs = np.where(whole_yes, BIN, np.where(two_yes & whole_no, 2, np.where(two_no, 1, -1)))
    jobs = np.where(hit == 1, jobs, np.where(hit == 0, 0, -1))
    amb = np.nonzero((hit < 0) | (jobs < 0))[0]
    out.update(T_lo=t_lo, T_hi=t_hi, P=P, hit=hit, jobs=jobs, ambiguous=amb, part=part)
    if amb.size:
        out.update(status=None, total=None)
        return out
    chunk = 512 * nv
    nchunks = (nbins + chunk - 1) // chunk
    nh = np.array([int((hit[c * chunk:(c + 1) * chunk] == 1).sum()) for c in range(nchunks)])
    total_lo = total_hi = 0
    njob = np.zeros(nchunks, dtype=np.int64)
    ovf = False
    for c in range(nchunks):
        j = np.sort(jobs[c * chunk:(c + 1) * chunk][hit[c * chunk:(c + 1) * chunk] == 1])
        # beyond HITCAP hits a bin gets no jobs (rq_tail_body.h:136): which ones is a race, the count is only known when they agree
        jl, jh = int(j[:HITCAP].sum()), int(j[::-1][:HITCAP].sum())
        njob[c] = jh
        for which, nj in ((0, jl), (1, jh)):
            local = tail_local and k < nj <= JOBCAP                         # rq_tail_body.h:158
            cnt = k if local else nj                                        # rq_tail_body.h:160 (uncapped)
            if which == 0: total_lo += cnt
            else: total_hi += cnt
        ovf |= nh[c] > HITCAP or jh > JOBCAP or jl > JOBCAP                 # rq_tail_body.h:161
    out.update(nh=nh, njob=njob, ovf_hit=bool((nh > HITCAP).any()), ovf_job=bool((njob > JOBCAP).any()),
               total=total_lo if total_lo == total_hi else None, total_range=(total_lo, total_hi))
    out["ovf_cand"] = total_hi > CAND_CAP                                   # rq_final_body.h:174
    # rows that get a non-empty key: the job rows that exist (and pass the filter)
    rescored = int(np.where(jobs == BIN, nlive, np.minimum(jobs, nlive)).sum())
    out["rescored"] = rescored
    overflow = ovf or out["ovf_cand"]
    out["overflow"] = bool(overflow)
    kk = min(k, rows_in_play)
    have = min(k, rescored)
    out["have"] = have
    tiny = metric == METRIC_COSINE and qnorm < TINY_QUERY_NORM              # rq_final_body.h:175
    # thr_mult 2.25: T + e < P - e <= s_k by construction (rq_tail_body.h:70-75), so the certificate holds whenever it is evaluated
    out["status"] = 0 if (not overflow and not tiny and have >= kk) else 1
    return out


def count_at(scores, n: int, T: float, allowed=None) -> int:
    """Rows a tail re-scores at least when its threshold is T and its scan were exact: one per bin whose maximum reaches T."""
    s1, _, _, _ = _top3(scores, n, allowed)
    return int((s1 >= T).sum())


# ---- planting ------------------------------------------------------------------------------------------------------------------
def unit(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def plant(x16: np.ndarray, rows, cosines, u: np.ndarray, rng, norms=None) -> None:
    """x16[rows[i]] = fp16(fp32(norm_i * (c_i u + sqrt(1 - c_i^2) w_i))), w_i a random unit vector orthogonal to the unit vector u.
    What the stored rows really score is the oracle's business: nothing downstream assumes the targets were met."""
    rows = np.atleast_1d(np.asarray(rows, dtype=np.int64)); c = np.atleast_1d(np.asarray(cosines, dtype=np.float64))
    assert rows.shape == c.shape and len(set(rows.tolist())) == rows.size
    u = unit(u)
    w = rng.standard_normal((rows.size, u.size))
    w = unit(w - (w @ u)[:, None] * u[None, :])
    v = c[:, None] * u[None, :] + np.sqrt(1.0 - c * c)[:, None] * w
    if norms is not None:
        v = v * np.atleast_1d(np.asarray(norms, dtype=np.float64))[:, None]
    x16[rows] = v.astype(np.float32).astype(np.float16)


def unit_scores(q: np.ndarray, x16: np.ndarray, metric: int) -> np.ndarray:
    """fp64 scores [B][n] in the scan's unit-query units (cosine with the definition's 1e-30; inner product: dot / |q|)."""
    q64 = np.atleast_2d(np.asarray(q, dtype=np.float32)).astype(np.float64)
    qn = np.sqrt((q64 * q64).sum(1))
    out = np.empty((q64.shape[0], x16.shape[0]))
    for lo in range(0, x16.shape[0], 16384):
        x64 = x16[lo:lo + 16384].astype(np.float64)
        dot = q64 @ x64.T
        if metric == METRIC_COSINE:
            dot = dot / (qn[:, None] * np.sqrt((x64 * x64).sum(1))[None, :] + 1e-30)
        else:
            dot = dot / np.where(qn > 0, qn, 1.0)[:, None]
        out[:, lo:lo + 16384] = dot
    return out
