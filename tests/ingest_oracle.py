"""The state an index derives from its rows when they are appended -- TEST INFRASTRUCTURE (numpy fp64, no GPU).

Everything here is a function of the STORED fp16 rows [n][dim] alone, stated from the definitions in csrc/rq_select.hip
(rq_rownorm_kernel, rq_rowscale_kernel, rq_quant_rows_kernel) and csrc/rq_plan.h (scan_eps), with plain np.float64 sums per
row: no lane order, no launch boundaries, no capacity.  An index is a function of its rows, not of its history; this module is
that function.

  row_norms     sqrt(sum x^2) in fp64
  shard_stats   (max_row_norm, max_sub_rel, max_sub_abs): the largest norm, and the largest mass a row keeps in elements whose fp16
                exponent field is 0 (zeros and subnormals: the matrix cores flush them), relative to the row norm and absolute.
                Rows whose norm is NaN or infinite are left out of all three.
  eps           the bound the tails are handed ("eps_cosine" / "eps_ip"): scan_eps, factor (1 + 1e-6) and fp32 cast included
  row_scales    the fp32 scale of the cosine scan, float(1 / norm) * 2^-12, 0 for a norm that is not > 0
  int8_image    the int8 image of the rows, its per-row scales, every row's relative quantisation error, the per-bin maxima
                rounded up to fp32 ("debug_bin_err") and the shard's maximum ("scan8_row_err")

Used by tests/test_ingest_oracle.py (CPU), tests/test_gpu_ingest.py and tests/test_gpu_parity.py.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

COS, IP = 0, 1
BIN_ROWS = 64
EPS_BASE = float(np.float32(7.0e-4))         # RQ_EPS_DEFAULT is an fp32 constant: scan_eps widens THAT value (option "eps" < 0)


def _f16(x16) -> np.ndarray:
    x16 = np.asarray(x16)
    if x16.dtype == np.uint16:
        x16 = x16.view(np.float16)
    assert x16.dtype == np.float16 and x16.ndim == 2, (x16.dtype, x16.shape)
    return x16


def row_norms(x16) -> np.ndarray:
    """[n] fp64: sqrt(sum x^2); NaN / inf for a row that holds one."""
    x = _f16(x16).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt((x * x).sum(axis=1))


def shard_stats(x16) -> Tuple[float, float, float]:
    """(max_row_norm, max_sub_rel, max_sub_abs) over the rows whose norm is finite; 0.0 where no row contributes."""
    x16 = _f16(x16)
    x = x16.astype(np.float64)
    flushed = (x16.view(np.uint16) & 0x7C00) == 0                      # exponent field 0: +-0 or subnormal
    with np.errstate(all="ignore"):
        sq = x * x
        acc = sq.sum(axis=1)
        sub = np.where(flushed, sq, 0.0).sum(axis=1)
        nrm = np.sqrt(acc)
    counted = np.isfinite(nrm)                                         # a NaN or infinite norm: the row is in no statistic
    has = counted & (sub > 0.0)
    mx_norm = float(nrm[counted].max(initial=0.0))
    mx_rel = float(np.sqrt(sub[has] / acc[has]).max(initial=0.0))
    mx_abs = float(np.sqrt(sub[has]).max(initial=0.0))
    return mx_norm, mx_rel, mx_abs


def eps(metric: int, stats, base: float = EPS_BASE) -> np.float32:
    """scan_eps (csrc/rq_plan.h): base + the shard's flush term, times (1 + 1e-6), cast to fp32.  base: option "eps" when set."""
    mx_norm, mx_rel, mx_abs = (float(v) for v in stats)
    if metric == COS:
        return np.float32(base + mx_rel * (1.0 + 1e-6))
    return np.float32(base + (mx_abs / mx_norm * (1.0 + 1e-6) if mx_norm > 0.0 else 0.0))


def row_scales(x16) -> np.ndarray:
    """[n] fp32: float(1 / norm) * 2^-12 (the queries carry 2^12), 0 for a norm that is not > 0 (zero rows, NaN rows)."""
    nrm = row_norms(x16)
    ok = nrm > 0.0
    with np.errstate(all="ignore"):
        inv = np.where(ok, 1.0 / np.where(ok, nrm, 1.0), 0.0).astype(np.float32)
    return (inv * np.float32(2.0 ** -12)).astype(np.float32)


def round_up_f32(v) -> np.ndarray:
    """fp64 -> the smallest fp32 that is not below it (non-negative values and +inf)."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


class Int8Image(NamedTuple):
    q8: np.ndarray           # [n][dim] int8 (a row that is not live: zeros; the image of a row with a non-finite element is not modelled, its scales are 0)
    scale_ip: np.ndarray     # [n] fp32: am / 127, 0 for a row that is not live
    scale_cos: np.ndarray    # [n] fp32: float(scale_ip / norm)
    row_err: np.ndarray      # [n] fp64: |row - scale_ip * q8| / norm; +inf for a row with a non-finite element, 0 for a zero row
    bin_err: np.ndarray      # [ceil(n / 64)] fp32: the largest row_err of every bin of 64 rows, rounded UP
    shard_err: float         # the largest row_err


def int8_image(x16) -> Int8Image:
    """rq_quant_rows_kernel: symmetric per-row scale from the row's largest magnitude am, fp32 am / 127 and 127 / am, rint, clip to
    +-127.  The error is summed in fp64 from the values the scan will use (the fp32 scale times the int8 element).  A row is live
    only if every element is finite, am > 0 and norm > 0."""
    x16 = _f16(x16)
    n = x16.shape[0]
    f = x16.astype(np.float32)
    xf = x16.astype(np.float64)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(f).all(axis=1)
        am = np.where(bad, np.float32(0), np.abs(np.where(np.isfinite(f), f, np.float32(0))).max(axis=1, initial=0.0)).astype(np.float32)
        nrm = row_norms(x16)
        live = ~bad & (am > 0) & (nrm > 0.0)
        am1 = np.where(live, am, np.float32(1)).astype(np.float32)
        sr = np.where(live, am1 / np.float32(127.0), np.float32(0)).astype(np.float32)
        inv = np.where(live, np.float32(127.0) / am1, np.float32(0)).astype(np.float32)
        q = np.clip(np.rint(np.where(live[:, None], f, np.float32(0)) * inv[:, None]), -127, 127)
        d = np.where(live[:, None], xf - sr.astype(np.float64)[:, None] * q.astype(np.float64), 0.0)
        err = np.sqrt((d * d).sum(axis=1)) / np.where(live, nrm, 1.0)
        row_err = np.where(bad, np.inf, np.where(live, err, 0.0))
        scale_cos = np.where(live, sr.astype(np.float64) / np.where(live, nrm, 1.0), 0.0).astype(np.float32)
    nbins = (n + BIN_ROWS - 1) // BIN_ROWS
    padded = np.zeros(nbins * BIN_ROWS)
    padded[:n] = row_err
    bin_err = round_up_f32(padded.reshape(nbins, BIN_ROWS).max(axis=1)) if nbins else np.zeros(0, np.float32)
    return Int8Image(q.astype(np.int8), sr, scale_cos, row_err, bin_err, float(row_err.max(initial=0.0)))
