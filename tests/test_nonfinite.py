"""Non-finite and extreme scores on the host: the test oracle of include/rq.h's three rules (tests/nonfinite_oracle.py), the host
key codec of distributed.py against oracle merge_topk, and the numpy restatement of the scan's records (tests/bin_records.py)
with NaN and infinite approximate scores.  The device side is tests/test_gpu_nonfinite.py; the C key codec's infinities are in
tests/native/codec_check.cpp (tests/test_abi.py)."""
import os
import sys

import numpy as np

from oracle import dense_oracle as orc
from rag_uq_amd import distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bin_records as br  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402

COS, IP = orc.METRIC_COSINE, orc.METRIC_IP
INF = np.float32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the helper itself: 130 rows, k = 130 -------------------------------------------------------------------------------------------
def _case130():
    q = nfo.queries(768, 8)
    return q, nfo.shard_c(768, q)


def test_helper_scores_follow_the_three_rules():
    q, x = _case130()
    for metric in (COS, IP):
        s = nfo.scores(q, x, metric)
        assert s.dtype == np.float32 and s.shape == (8, 130) and not np.isnan(s).any()
        assert np.array_equal(_bits(s[5]), np.zeros(130, np.uint32))              # the zero query: +0.0 on the NaN and inf rows too
        assert np.isneginf(s[1]).all()                                            # the NaN query
        assert np.isneginf(s[[0, 3, 4, 6], 2]).all()                              # the NaN row, every finite non-zero query
        assert not np.signbit(s[s == 0]).any()
    c = nfo.scores(q, x, COS)
    assert np.isneginf(c[0, [5, 70]]).all() and np.isneginf(c[[2, 7]]).all()      # cosine: an infinite norm on either side
    assert c[0, 9] == 0 and abs(float(c[0, 129]) - 1.0) < 1e-3 and np.isfinite(c[[3, 4]][:, [0, 1, 129]]).all()
    p = nfo.scores(q, x, IP)
    x32 = x.astype(np.float32)
    assert p[0, 5] == np.sign(q[0, 7]) * INF and p[0, 70] == -np.sign(q[0, 0]) * INF
    fin = np.isfinite(x32).all(axis=1)
    assert np.array_equal(p[2, fin & (x32[:, 3] > 0)], np.full(int((fin & (x32[:, 3] > 0)).sum()), INF))
    assert np.isneginf(p[2, 9])                                                   # inf x 0 on the zero row: NaN, hence -inf
    assert np.isfinite(p[4, fin]).all() and np.abs(p[4, fin]).max() > 1e35        # 1e36 x unit rows stays inside fp32


def test_helper_topk_orders_infinities_and_keeps_every_row():
    q, x = _case130()
    for metric in (COS, IP):
        s = nfo.scores(q, x, metric)
        gs, gr = nfo.topk(q, x, 130, metric)
        for b in range(8):
            want = sorted(range(130), key=lambda r: (-float(s[b, r]), r))         # independent: python's sort on (score desc, row asc)
            assert gr[b].tolist() == want, (metric, b)
            assert np.array_equal(_bits(gs[b]), _bits(s[b, want]))
        assert gr[5].tolist() == list(range(130)) and not gs[5].any()             # zero query: rows in order at 0.0
        assert gr[1].tolist() == list(range(130)) and np.isneginf(gs[1]).all()    # NaN query: every row is still a row, at -inf
        g200s, g200r = nfo.topk(q, x, 200, metric)                                # k beyond the shard: k_eff = 130, padding (0.0, -1)
        assert np.array_equal(g200r[:, :130], gr) and (g200r[:, 130:] == -1).all() and not g200s[:, 130:].any()
        off = nfo.topk(q, x, 7, metric, row_offset=1000)[1]
        assert np.array_equal(off, gr[:, :7] + 1000)
    mask = np.zeros(130, bool)
    mask[[2, 5, 9, 70, 100, 129]] = True
    fs, fr = nfo.topk(q, x, 10, COS, mask=mask)
    assert fr[5].tolist() == [2, 5, 9, 70, 100, 129, -1, -1, -1, -1] and not fs[5].any()
    assert fr[0, :3].tolist() == [129, 100, 9] or fr[0, :3].tolist() == [129, 9, 100]
    assert sorted(fr[0, 3:6].tolist()) == [2, 5, 70] and np.isneginf(fs[0, 3:6]).all() and fr[0, 3:6].tolist() == [2, 5, 70]


def test_planted_shards_have_the_shapes_the_gpu_tests_rely_on():
    q = nfo.queries(768)
    a = nfo.shard_a(768, q)
    assert a.shape == (nfo.N_A, 768) and nfo.N_A == 64 * 64 + 5
    bad = ~np.isfinite(a.astype(np.float32)).all(axis=1)
    assert sorted(np.flatnonzero(bad).tolist()) == sorted([5, 200, 2049, 4100] + list(range(64, 128)))
    s = nfo.scores(q[[0, 6]], a, COS)
    assert int(s[0].argmax()) == 2050 and int(s[1].argmax()) == 4099 and s[0, 2050] > 0.99 and s[1, 4099] > 0.99
    t = nfo.twin_a(a)
    assert np.isfinite(t.astype(np.float32)).all() and np.array_equal(t[~bad], a[~bad]) and not t[bad].any()
    b = nfo.shard_b(768)
    assert np.flatnonzero(np.isfinite(b.astype(np.float32)).all(axis=1)).tolist() == nfo.FINITE_B
    gs, gr = nfo.topk(q[[0, 6, 8]], b, 10, COS)
    assert all(sorted(r[:7].tolist()) == nfo.FINITE_B and r[7:].tolist() == [0, 1, 2] for r in gr)
    assert np.isfinite(gs[:, :7]).all() and np.isneginf(gs[:, 7:]).all()


# ---- host keys: distributed.pack_keys / merge_keys_host against merge_topk ---------------------------------------------------------------
def test_host_keys_apply_the_device_rules_for_nan_and_negative_zero():
    s = np.array([[INF, -INF, np.nan, -0.0, 0.0, 1.0, -1.0, np.float32(3.4e38), np.float32(-3.4e38)]], np.float32)
    r = np.array([[9, 8, 7, 6, 5, 4, 3, 2, 1]], np.int64)
    keys = dist.pack_keys(s, r)
    assert (keys != 0).all()                                                   # -inf and NaN are rows, not empty slots
    hi = (keys >> np.uint64(32)).astype(np.uint32)[0]
    assert hi[2] == hi[1]                                                      # NaN counts as -inf (rq_sanitize)
    assert hi[3] == hi[4]                                                      # -0.0 ranks with +0.0 (rq_make_key)
    assert hi[0] > hi[7] > hi[5] > hi[4] > hi[6] > hi[8] > hi[1]
    us, ur = dist.unpack_keys(keys)
    assert np.array_equal(ur, r)
    assert np.array_equal(_bits(us), _bits(np.array([[INF, -INF, -INF, 0.0, 0.0, 1.0, -1.0, 3.4e38, -3.4e38]], np.float32)))
    assert s[0, 3] == 0 and np.signbit(s[0, 3]) and np.isnan(s[0, 2])          # the caller's array is left alone
    assert dist.pack_keys(np.array([np.nan], np.float32), np.array([-1]))[0] == 0


def test_host_merge_with_infinite_nan_and_negative_zero_scores_matches_merge_topk():
    rng = np.random.default_rng(5)
    B, k, world = 6, 12, 3
    parts = []
    for w in range(world):
        s = rng.standard_normal((B, k)).astype(np.float32)
        s[0, :4] = INF; s[1, -5:] = -INF; s[2, 3:6] = np.nan; s[3, :] = -0.0 if w == 1 else 0.0; s[4, ::2] = -INF; s[4, 1] = INF
        s[5] = np.where(rng.random(k) < 0.5, -0.0, 0.0)
        r = (w * 1000 + np.argsort(rng.random((B, k)), axis=1)).astype(np.int64)
        if w == 2:
            r[:, -2:] = -1                                                     # a short shard: padding
        parts.append((s, r))
    # merge_topk under the same two rules: NaN -> -inf, -0.0 -> +0.0
    canon = []
    for s, r in parts:
        c = np.where(np.isnan(s), -INF, s)
        canon.append((np.where(c == 0, np.float32(0), c).astype(np.float32), r))
    for kk in (1, 5, 12, 34, 40):
        ws, wr = orc.merge_topk(canon, kk)
        keys = np.concatenate([dist.pack_keys(s, r) for s, r in parts], axis=1)
        gs, gr = dist.merge_keys_host(keys[:, rng.permutation(keys.shape[1])], kk)
        assert np.array_equal(gr, wr), kk
        assert np.array_equal(_bits(gs), _bits(ws)), kk
    assert wr[3, :10].tolist() == sorted(np.concatenate([p[1][3] for p in parts])[np.concatenate([p[1][3] for p in parts]) >= 0].tolist())[:10]


# ---- the numpy restatement of the scan's records ----------------------------------------------------------------------------------------
def test_pos_score_clamps_like_v_med3():
    got = br.pos_score(np.array([np.nan, INF, -INF, 1.0, -1.0, 0.0], np.float32), np.array([3, 4, 5, 6, 7, 8], np.uint32))
    fmax = np.float32(3.4028234664e38)
    want = (_bits(np.array([-fmax, fmax, -fmax, 1.0, -1.0, 0.0], np.float32)) & np.uint32(0xFFFFFFC0)) | np.array([3, 4, 5, 6, 7, 8], np.uint32)
    assert np.array_equal(_bits(got), want)
    assert np.isfinite(got).all()
    # a quiet NaN of either sign and with any payload
    odd = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert np.array_equal(_bits(br.pos_score(odd, np.zeros(4, np.uint32))), np.full(4, _bits(np.array([-fmax]))[0] & np.uint32(0xFFFFFFC0)))


def test_records_from_nonfinite_approximate_scores_pass_against_an_exact_matrix_with_minus_inf():
    n, B = 64 * 5 + 5, 3
    rng = np.random.default_rng(8)
    exact = (0.1 * rng.standard_normal((B, n))).astype(np.float32)
    exact[:, 64:128] = -INF                    # a whole bin of NaN rows
    exact[:, 130] = -INF                       # a NaN row beside finite ones
    exact[:, n - 1] = -INF                     # ... and in the ragged last bin
    exact[0, 200] = 0.9
    exact[2] = -INF                            # a NaN query: every score
    approx = exact + np.float32(1e-5) * rng.standard_normal((B, n)).astype(np.float32)
    approx[:, 64:128] = np.nan                 # what the scan sees there: NaN (x a zero row scale) ...
    approx[:, 130] = np.nan
    approx[:, n - 1] = -INF                    # ... or an infinity, clamped like it
    approx[2, ::2] = np.nan; approx[2, 1::2] = -INF
    rec = br.records_from_scores(approx, n)
    f = br.decode(rec)
    assert np.isfinite(f["m1"]).all() and not np.isnan(f["c2val"]).any() and not np.isnan(f["c3val"]).any()
    assert (f["m1"][:, 1] < -1.0 - 1e-3).all() and (f["m1"][2] < -1e38).all()
    assert f["p1"][0, 3] == 200 - 192
    rep = br.check_records(rec, exact, n, 1e-4)
    assert not br.failures(rep), br.failures(rep)
    # compare / select forms drop a NaN: a bin of nothing else keeps -inf in every field, which is as good an upper bound
    drop = rec.copy()
    drop[:, 1] = br.record_from_triple(*(np.full(B, -INF, np.float32),) * 3)
    assert np.isneginf(br.decode(drop)["m1"][:, 1]).all() and np.isneginf(br.decode(drop)["c2val"][:, 1]).all()
    assert not br.failures(br.check_records(drop, exact, n, 1e-4))
    # ... and the check still bites: a NaN or +inf m1, -inf on a live bin, an arg-max on a -inf row of a live bin
    for word in (0x7FC00000, 0x7F800000):
        bad = rec.copy(); bad[0, 1, 0] = np.uint32(word)
        assert not br.check_records(bad, exact, n, 1e-4)["I1"]["ok"]
    bad = rec.copy(); bad[0, 3, 0] = np.uint32(0xFF800000)
    rep = br.check_records(bad, exact, n, 1e-4)
    assert not rep["I1"]["ok"] and not rep["I2"]["ok"]
    bad = rec.copy(); bad[0, 2, 0] = (bad[0, 2, 0] & np.uint32(0xFFFFFFC0)) | np.uint32(2)     # row 130: -inf in a live bin
    assert not br.check_records(bad, exact, n, 1e-4)["I4"]["ok"]
