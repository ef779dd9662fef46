"""tests/ingest_oracle.py against cases worked out by hand, and against oracle/dense_oracle.py where the two overlap (CPU)."""
import math
import os
import sys

import numpy as np

from oracle import dense_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_oracle as ino  # noqa: E402

DIM = 768
SUB_MIN = 2.0 ** -24          # fp16 bits 0x0001
SUB_MAX = 1023 * 2.0 ** -24   # fp16 bits 0x03ff
NORMAL_MIN = 2.0 ** -14       # fp16 bits 0x0400


def _bits_row(pairs, dim=DIM):
    r = np.zeros(dim, np.uint16)
    for i, b in pairs:
        r[i] = b
    return r.view(np.float16)[None, :]


def test_a_zero_row_counts_nowhere_and_scales_to_zero():
    x = np.zeros((1, DIM), np.float16)
    assert ino.row_norms(x).tolist() == [0.0]
    assert ino.shard_stats(x) == (0.0, 0.0, 0.0)
    assert ino.row_scales(x).tolist() == [0.0]
    assert ino.eps(ino.COS, ino.shard_stats(x)) == np.float32(7e-4) and ino.eps(ino.IP, ino.shard_stats(x)) == np.float32(7e-4)
    im = ino.int8_image(x)
    assert not im.q8.any() and im.scale_ip.tolist() == [0.0] and im.scale_cos.tolist() == [0.0]
    assert im.row_err.tolist() == [0.0] and im.bin_err.tolist() == [0.0] and im.shard_err == 0.0


def test_a_row_of_one_subnormal_is_all_flushed_mass():
    x = _bits_row([(5, 0x0001)])
    assert ino.row_norms(x).tolist() == [SUB_MIN]
    assert ino.shard_stats(x) == (SUB_MIN, 1.0, SUB_MIN)
    assert ino.row_scales(x).tolist() == [4096.0]                                   # float(2^24) * 2^-12
    st = ino.shard_stats(x)
    assert ino.eps(ino.COS, st) == np.float32(float(np.float32(7e-4)) + 1.0 * (1 + 1e-6))
    assert ino.eps(ino.IP, st) == np.float32(float(np.float32(7e-4)) + 1.0 * (1 + 1e-6))   # abs / max norm = 1
    assert ino.eps(ino.COS, st, base=0.25) == np.float32(1.250001)                  # option "eps" set: the base is that double
    im = ino.int8_image(x)
    assert im.q8[0, 5] == 127 and int(np.abs(im.q8).sum()) == 127
    assert abs(float(im.scale_ip[0]) * 127 / SUB_MIN - 1.0) <= 2.0 ** -23           # fp32 am / 127
    assert abs(float(im.scale_cos[0]) * 127 - 1.0) <= 2.0 ** -22                    # ... / norm = 1 / 127
    assert 0.0 <= im.row_err[0] <= 127 * 2.0 ** -24                                 # only the fp32 rounding of the scale is left
    assert im.shard_err == im.row_err[0] and float(im.bin_err[0]) >= im.row_err[0]


def test_the_exponent_test_separates_0x03ff_from_0x0400_and_ignores_signed_zeros():
    x = _bits_row([(0, 0x03FF), (1, 0x0400), (2, 0x8000), (3, 0x0000)])
    nrm, rel, ab = ino.shard_stats(x)
    assert nrm == math.sqrt(SUB_MAX ** 2 + NORMAL_MIN ** 2)
    assert ab == SUB_MAX                                                            # 0x0400 is a normal number: not flushed
    assert math.isclose(rel, 1023 / math.sqrt(1023 ** 2 + 1024 ** 2), rel_tol=1e-15)
    neg = _bits_row([(0, 0x83FF), (1, 0x8400)])                                     # the sign bit is not part of the test
    assert ino.shard_stats(neg) == (nrm, rel, ab)
    assert ino.shard_stats(_bits_row([(1, 0x0400), (2, 0x8000)])) == (NORMAL_MIN, 0.0, 0.0)


def test_a_row_of_65504s():
    x = np.full((1, DIM), 65504.0, np.float16)
    x[0, 1::2] = -65504.0
    want = 65504.0 * math.sqrt(768.0)
    assert math.isclose(ino.row_norms(x)[0], want, rel_tol=1e-15)
    nrm, rel, ab = ino.shard_stats(x)
    assert math.isclose(nrm, want, rel_tol=1e-15) and rel == 0.0 and ab == 0.0
    assert ino.row_scales(x)[0] == np.float32(np.float32(1.0 / ino.row_norms(x)[0]) * np.float32(2.0 ** -12))
    assert math.isclose(float(ino.row_scales(x)[0]), 2.0 ** -12 / want, rel_tol=2.0 ** -23)
    im = ino.int8_image(x)
    assert np.array_equal(im.q8[0], np.where(np.arange(DIM) % 2 == 0, 127, -127))
    sr = float(im.scale_ip[0])
    assert abs(sr - 65504.0 / 127.0) <= 2.0 ** -15                                   # half an fp32 ulp in [512, 1024)
    # every element is off by |65504 - 127 sr|: relative to the norm that is the same figure over 65504
    assert math.isclose(im.row_err[0], abs(65504.0 - 127.0 * sr) / 65504.0, rel_tol=1e-12)
    assert im.row_err[0] <= 127 * 2.0 ** -15 / 65504.0
    assert math.isclose(float(im.scale_cos[0]), sr / want, rel_tol=2.0 ** -23)


def test_rows_with_an_inf_or_a_nan_stay_out_of_the_statistics_and_switch_the_image_off():
    x = orc.synthetic_corpus(130, DIM, seed=3)
    base = ino.shard_stats(x)
    y = x.copy()
    y[7, 100] = np.inf
    y[70, 3] = -np.inf
    y[129] = np.nan
    assert np.isinf(ino.row_norms(y)[[7, 70]]).all() and np.isnan(ino.row_norms(y)[129])
    keep = np.ones(130, bool)
    keep[[7, 70, 129]] = False
    assert ino.shard_stats(y) == ino.shard_stats(x[keep])                            # as if the rows were not there
    assert ino.shard_stats(y)[0] <= base[0] and np.isfinite(ino.shard_stats(y)).all()
    assert ino.row_scales(y)[[7, 70, 129]].tolist() == [0.0, 0.0, 0.0]
    im, clean = ino.int8_image(y), ino.int8_image(x)
    assert np.isinf(im.row_err[[7, 70, 129]]).all() and (im.row_err[[7, 70, 129]] > 0).all()
    assert im.scale_ip[[7, 70, 129]].tolist() == [0.0] * 3 and im.scale_cos[[7, 70, 129]].tolist() == [0.0] * 3
    assert np.array_equal(im.row_err[keep], clean.row_err[keep]) and np.array_equal(im.q8[keep], clean.q8[keep])
    assert np.isinf(im.bin_err).tolist() == [True, True, True] and im.shard_err == np.inf
    assert np.isfinite(clean.bin_err).all() and clean.shard_err == clean.row_err.max()


def test_bin_errors_are_the_bin_maxima_rounded_up():
    x = orc.synthetic_corpus(200, DIM, seed=4)
    x[70:75] = (x[70:75].astype(np.float32) * np.linspace(0.2, 3.0, DIM, dtype=np.float32)).astype(np.float16)
    im = ino.int8_image(x)
    assert im.bin_err.shape == (4,) and im.bin_err.dtype == np.float32
    for b in range(4):
        m = im.row_err[64 * b:64 * (b + 1)].max()
        assert float(im.bin_err[b]) >= m and float(np.nextafter(im.bin_err[b], np.float32(0))) < m
    assert im.row_err[70:75].min() > np.median(im.row_err) and im.shard_err == im.row_err[70:75].max() == im.row_err[64:128].max()
    # the image reproduces the row to half a step of its scale in every element (+ the fp32 roundings of 127 / am, of the product
    # and of am / 127 at |q| <= 127: 3 x 127 x 2^-24 = 2.3e-5 of a step)
    assert (np.abs(x.astype(np.float64) - im.scale_ip.astype(np.float64)[:, None] * im.q8) <= 0.5001 * im.scale_ip[:, None]).all()
    assert ino.round_up_f32([0.0, 1.0, 1.0 + 2.0 ** -30, np.inf]).tolist() == [0.0, 1.0, float(np.float32(1.0 + 2.0 ** -23)), np.inf]


def test_the_model_agrees_with_the_dense_oracle_where_they_overlap():
    rng = np.random.default_rng(11)
    x32 = rng.standard_normal((300, 300)).astype(np.float32) * rng.uniform(0.1, 30.0, (300, 1)).astype(np.float32)
    x32[17] = 0
    unit = orc.prepare_rows_f32(x32, True)
    nrm = ino.row_norms(unit)
    assert nrm[17] == 0.0 and ino.row_scales(unit)[17] == 0.0
    rest = np.delete(nrm, 17)
    # fp16 rounding of a unit row: 2^-11 relative per normal element, 2^-25 absolute per subnormal one
    assert np.abs(rest - 1.0).max() <= 2.0 ** -11 + math.sqrt(300) * 2.0 ** -25
    assert np.abs(np.delete(ino.row_scales(unit), 17) * 4096.0 - 1.0).max() <= 2.0 ** -10
    raw = orc.prepare_rows_f32(x32 * 0.01, False)
    n2 = ino.row_norms(raw)
    # the oracle's cosine divides by the same norms: a row against itself scores 1, against its negative -1
    s = orc.exact_scores(raw[:8].astype(np.float32), raw, orc.METRIC_COSINE)
    assert np.array_equal(np.diag(s[:, :8]), np.ones(8, np.float32))
    ip = orc.exact_scores(raw[:8].astype(np.float32), raw, orc.METRIC_IP)
    assert np.allclose(np.diag(ip[:, :8]).astype(np.float64), n2[:8] ** 2, rtol=2.0 ** -23, atol=0)
    assert ino.shard_stats(raw)[0] == n2.max()
