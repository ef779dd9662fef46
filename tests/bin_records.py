"""The scan's bin records (csrc/rq_device.h) in numpy: a decoder, a faithful encoder and the invariants the tail relies on.

Every exact answer rests on the 8-byte record the scan writes per (query, bin of 64 rows):
  x = [31:6] m1, the bin's largest approximate score rounded UP to 26 bits | [5:0] p1, its row in the bin
  y = [31:16] c2, 16-bit code of the second largest rounded up | [15:6] d, decode(c2 - d) >= the third largest | [5:0] p2
The tail (csrc/rq_tail_body.h) re-scores only row p1 when decode(c2) < T, rows p1 and p2 when only decode(c2 - d) < T, all 64
rows otherwise, and the certificate (rq_final_body.h) assumes every row left out has an approximate score below T.
check_records() tests exactly that premise against the exact scores.  Used by tests/test_gpu_bin_records.py (records of the
GPU) and tests/test_bin_records.py (this module against hand-made bit patterns and planted faults).

The bound `beta` is the one the tail itself uses for |approximate - exact| (unit-query units):
  * fp16, cosine: beta = eps_cosine (option), = scan_eps(COSINE) (rq_plan.h scan_eps) -- the derived 7e-4 (or option "eps") plus the
    fp16-subnormal share of the worst row.  The tail tests bins against T with it (rq_tail_body.h:36, 98) and the certificate
    bounds a row left out by T + eps (rq_final_body.h:172).
  * fp16, inner product: the scan scores the UNIT query, so its records compare with E_ip / ||q||_64; the tail scales the bound by
    the largest row norm (rq_tail_body.h:98, rq_search.hip tail_args: max_row_norm * (1 + 1e-6)), so beta = eps_ip * max_row_norm * (1 + 1e-6).
  * int8 image (rq_plan.h scan8_eps, rq_search.hip tail_args): |approx - exact| <= e_q + (1 + e_q) e_rows, e_rows the worst relative error of
    the bin's rows.  With option "bin_bound" the tail tests bin b with its own rows' error (rq_tail_body.h:117-125), so per bin
    beta_b = e_q + (1 + e_q)(binerr_b * 1.000001 + 2e-5), binerr_b from rq_debug_bin_err and e_q the query's one-image (or split)
    error recomputed in numpy (int8_query_error); times max_row_norm for the inner product.
The 26-bit round-up of m1 (at most 2^-17 relative) only matters where m1 is bounded from above (I3).
"""
from __future__ import annotations

import numpy as np

POISON = 0xFFFFFFFF
ROUNDUP26 = 2.0 ** -17
FLT_MAX = np.float32(3.4028234664e38)


# ---- decoder: rq_rec_m1, rq_code16_value and the field split of rq_device.h -------------------------------------------------
def _f32(bits: np.ndarray) -> np.ndarray:
    return np.array(bits, dtype=np.uint32, copy=True).view(np.float32)


def rec_m1(x) -> np.ndarray:
    return _f32(np.asarray(x, dtype=np.uint32) & np.uint32(0xFFFFFFC0))


def unmono32(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return _f32(u)


def code16_value(c) -> np.ndarray:
    c = np.asarray(c, dtype=np.uint32) & np.uint32(0xFFFF)        # (C: uint32 c << 16 keeps the low 16 bits of c)
    k = (c << np.uint32(16)) | np.where(c & np.uint32(0x8000), np.uint32(0), np.uint32(0xFFFF)).astype(np.uint32)
    return unmono32(k)


def decode(rec: np.ndarray) -> dict:
    """rec [..., 2] uint32 -> m1, p1, c2val = decode(c2), c3val = decode(c2 - d), p2 (and the raw c2, d)."""
    rec = np.asarray(rec, dtype=np.uint32)
    x, y = rec[..., 0], rec[..., 1]
    c2 = y >> np.uint32(16)
    d = (y >> np.uint32(6)) & np.uint32(1023)
    return {"m1": rec_m1(x), "p1": (x & np.uint32(63)).astype(np.int64), "c2": c2, "d": d,
            "c2val": code16_value(c2), "c3val": code16_value(c2 - d), "p2": (y & np.uint32(63)).astype(np.int64)}


# ---- encoder: rq_up16 / rq_code16 / rq_pos_score / rq_record_from_triple -----------------------------------------------------
def _bits(f) -> np.ndarray:
    return np.array(f, dtype=np.float32, copy=True).view(np.uint32)


def up16(f) -> np.ndarray:
    f = np.asarray(f, dtype=np.float32)
    u = _bits(np.where(f == 0, np.float32(0), f))
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, u & np.uint32(0xFFFF0000), (u + np.uint32(0xFFFF)) & np.uint32(0xFFFF0000)).astype(np.uint32)


def code16(f) -> np.ndarray:
    u = up16(f)
    return (np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32) >> np.uint32(16)).astype(np.uint32)


def pos_score(score, pos) -> np.ndarray:
    """rq_pos_score: clamp to the finite range (NaN becomes the smallest value: v_med3_f32 with a NaN operand returns the minimum
    of the other two), replace the 6 low mantissa bits by the row's position."""
    s = np.asarray(score, dtype=np.float32)
    s = np.clip(np.where(np.isnan(s), -FLT_MAX, s), -FLT_MAX, FLT_MAX).astype(np.float32)
    return _f32((_bits(s) & np.uint32(0xFFFFFFC0)) | np.asarray(pos, dtype=np.uint32))


def record_from_triple(x1, x2, x3) -> np.ndarray:
    """rq_record_from_triple: the record of a merged triple x1 >= x2 >= x3 whose values carry their positions."""
    b1, b2, b3 = _bits(x1), _bits(x2), _bits(x3)
    pos1 = (b1.view(np.int32) >= 0)
    f1 = ((b1 & np.uint32(0xFFFFFFC0)) + np.where(pos1, np.uint32(64), np.uint32(0))).astype(np.uint32)
    u2 = np.where(b2.view(np.int32) >= 0, b2 | np.uint32(63), b2 & np.uint32(0xFFFFFFC0)).astype(np.uint32)
    u3 = np.where(b3.view(np.int32) >= 0, b3 | np.uint32(63), b3 & np.uint32(0xFFFFFFC0)).astype(np.uint32)
    c2, c3 = code16(_f32(u2)), code16(_f32(u3))
    d = np.minimum(c2 - c3, np.uint32(1023)).astype(np.uint32)
    x = f1 | (b1 & np.uint32(63))
    y = (c2 << np.uint32(16)) | (d << np.uint32(6)) | (b2 & np.uint32(63))
    return np.stack([x, y], axis=-1).astype(np.uint32)


def records_from_scores(approx: np.ndarray, n: int) -> np.ndarray:
    """Records [B][nbins][2] of approximate scores [B][n] as the scan forms them: positions in the low bits, the three largest
    of each bin (pad rows beyond n never win), rq_record_from_triple."""
    approx = np.asarray(approx, dtype=np.float32)
    B, nbins = approx.shape[0], (n + 63) // 64
    a = np.zeros((B, nbins * 64), dtype=np.float32)
    a[:, :n] = approx[:, :n]
    pos = np.broadcast_to(np.arange(64, dtype=np.uint32), (B, nbins, 64))
    ps = pos_score(a.reshape(B, nbins, 64), pos)
    pad = (np.arange(nbins * 64) >= n).reshape(1, nbins, 64)
    ps = np.where(pad, np.float32(-np.inf), ps)   # (a pad row stays below every row, a clamped NaN or -inf row included)
    top = -np.sort(-ps, axis=2)[:, :, :3]
    return record_from_triple(top[..., 0], top[..., 1], top[..., 2])


# ---- the int8 scan's per-query error (rq_device.h rq_prep_body, in numpy) --------------------------------------------------
def int8_query_error(q: np.ndarray, split: bool = False) -> np.ndarray:
    """Relative quantisation error of each query's int8 image (split: left after the value and the residual image), rounded up
    as the device does (x 1.000001).  0 for a zero query."""
    q = np.asarray(q, dtype=np.float32)
    qd = q.astype(np.float64)
    nrm = np.sqrt((qd * qd).sum(1))
    am = np.abs(q).max(1)
    live = am > 0
    sq = np.where(live, am / np.float32(127.0), np.float32(0)).astype(np.float32)
    inv = np.where(live, np.float32(127.0) / np.where(live, am, 1), np.float32(0)).astype(np.float32)
    r = np.clip(np.rint(q * inv[:, None]), -127, 127).astype(np.float32)
    d = qd - sq.astype(np.float64)[:, None] * r.astype(np.float64)
    if split:
        slo = (sq / np.float32(254.0)).astype(np.float32)
        invlo = np.where(live, np.float32(254.0) / np.where(live, sq, 1), np.float32(0)).astype(np.float32)
        rl = np.clip(np.rint(d.astype(np.float32) * invlo[:, None]), -127, 127).astype(np.float32)
        d = d - slo.astype(np.float64)[:, None] * rl.astype(np.float64)
    e = np.sqrt((d * d).sum(1)) / np.where(live, nrm, 1.0)
    return np.where(live, e * 1.000001, 0.0)


# ---- the invariants --------------------------------------------------------------------------------------------------------
INVARIANTS = {
    "I1": "m1 finite for every bin with a valid row (-inf allowed where every row of the bin scores -inf)",
    "I2": "max E(R_b) <= m1 + beta",
    "I3": "m1 <= max E(R_b) + beta + 2^-17 |m1| (bins with a finite maximum)",
    "I4": "64 b + p1 valid and E(64 b + p1) >= max E(R_b) - 2 beta",
    "I5": "|R_b| >= 2: p2 != p1 and 64 b + p2 valid (unless the second-best exact score and decode(c2) are both -inf: p2 is then never used on its own)",
    "I6": "E(r) <= decode(c2) + beta for every valid r != p1",
    "I7": "E(r) <= decode(c2 - d) + beta for every valid r not p1 / p2",
    "I8": "query slots [B, slots) still hold the poison pattern",
}


def check_records(rec: np.ndarray, exact: np.ndarray, n: int, beta, B: int = None) -> dict:
    """rec [slots][nbins][2] uint32 (rq_debug_bin_records), exact [B][n] canonical scores in the scan's units (cosine: the score;
    inner product: E_ip / ||q||_64), beta scalar / [B] / [B][nbins] (module docstring).  Slots [B, slots) must hold the poison
    pattern (option "poison_bins").  Returns {invariant: {"ok", "margin" (worst; < 0 = violated), "first" (query, bin, row)}}."""
    rec = np.asarray(rec, dtype=np.uint32)
    exact = np.asarray(exact)
    B = exact.shape[0] if B is None else B
    nbins = (n + 63) // 64
    assert rec.ndim == 3 and rec.shape[1] == nbins and rec.shape[0] >= B, (rec.shape, B, nbins)
    assert exact.shape == (B, n), (exact.shape, B, n)
    beta = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(
        (B, 1) if np.ndim(beta) == 1 else ((B, nbins) if np.ndim(beta) == 2 else (1, 1))), (B, nbins))
    f = decode(rec[:B])
    m1 = f["m1"].astype(np.float64)
    p1, p2 = f["p1"], f["p2"]
    c2v, c3v = f["c2val"].astype(np.float64), f["c3val"].astype(np.float64)
    E = np.full((B, nbins * 64), -np.inf)
    E[:, :n] = exact
    E = E.reshape(B, nbins, 64)
    valid = (np.arange(nbins * 64) < n).reshape(nbins, 64)
    nvalid = valid.sum(1)
    M = E.max(axis=2)                                              # max over the valid rows (pad rows -inf)
    slot = np.arange(64)
    is1 = slot[None, None, :] == p1[..., None]
    is2 = slot[None, None, :] == p2[..., None]
    out = {}

    def report(name, margin, rows=None):
        """margin [B][nbins] (or [B][nbins][64] with rows): >= 0 everywhere = holds."""
        margin = np.where(np.isnan(margin), -np.inf, margin)
        worst = float(margin.min()) if margin.size else 0.0
        first = None
        if worst < 0:
            idx = np.argwhere(margin < 0)[0]
            qb = (int(idx[0]), int(idx[1]))
            row = int(idx[2]) if margin.ndim == 3 else int(p1[qb])
            first = (qb[0], qb[1], 64 * qb[1] + row)
        out[name] = {"ok": worst >= 0, "margin": worst, "first": first}

    with np.errstate(invalid="ignore", over="ignore"):
        # Exact scores may hold -inf (a NaN score counts as -inf, include/rq.h).  Every field is an upper bound, and -inf is
        # below everything: a row at -inf constrains no field, and a bin of nothing else (`dead`) has no maximum to be tight
        # against -- its m1 is the clamp value (positions inside the scores) or -inf (compare / select drops a NaN), then with
        # decode(c2) = -inf, which makes the tail take the whole bin whenever it takes a second row.
        dead = np.isneginf(M)
        low = np.isneginf(E)
        report("I1", np.where(np.isfinite(m1) | (dead & np.isneginf(m1)), 0.0, -np.inf))
        report("I2", np.where(dead, np.inf, m1 + beta - M))
        report("I3", np.where(dead, np.inf, M + beta + ROUNDUP26 * np.abs(m1) - m1))
        p1_ok = valid[np.arange(nbins)[None, :], p1]
        e_p1 = np.take_along_axis(E, p1[..., None], axis=2)[..., 0]
        report("I4", np.where(p1_ok, np.where(dead, np.inf, e_p1 - (M - 2 * beta)), -np.inf))
        p2_ok = valid[np.arange(nbins)[None, :], p2] & (p2 != p1)
        # (waived only where the bin's second-best exact score is -inf and the field says so: decode(c2) = -inf is then honest, and
        # the tail never uses p2 on its own, decode(c2 - d) being -inf too)
        second = np.sort(E, axis=2)[:, :, -2]
        report("I5", np.where((nvalid[None, :] < 2) | p2_ok | (np.isneginf(second) & np.isneginf(c2v)), 0.0, -np.inf))
        vr = valid[None, :, :]
        m6 = np.where(vr & ~is1 & ~low, c2v[..., None] + beta[..., None] - E, np.inf)
        report("I6", m6, rows=True)
        m7 = np.where(vr & ~is1 & ~is2 & ~low, c3v[..., None] + beta[..., None] - E, np.inf)
        report("I7", m7, rows=True)
    tail = rec[B:]
    if tail.size:
        bad = np.argwhere(tail != np.uint32(POISON))
        out["I8"] = {"ok": bad.size == 0, "margin": 0.0 if bad.size == 0 else -1.0,
                     "first": None if bad.size == 0 else (B + int(bad[0][0]), int(bad[0][1]), None)}
    else:
        out["I8"] = {"ok": True, "margin": 0.0, "first": None}
    return out


def failures(report: dict) -> list:
    return [f"{k} ({INVARIANTS[k]}): margin {v['margin']:.3g}, first (query, bin, row) {v['first']}" for k, v in report.items() if not v["ok"]]


def tightness(rec: np.ndarray, exact: np.ndarray, n: int) -> float:
    """max |m1 - max E(R_b)| over the B queries of `exact` (the scan's actual error on the bin maxima)."""
    B, nbins = exact.shape[0], (n + 63) // 64
    E = np.full((B, nbins * 64), -np.inf)
    E[:, :n] = exact
    M = E.reshape(B, nbins, 64).max(axis=2)
    return float(np.abs(decode(rec[:B])["m1"].astype(np.float64) - M).max())
