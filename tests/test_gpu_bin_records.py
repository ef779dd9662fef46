"""Every scan form's bin records against the exact scores (MI355X).

The tail re-scores only the rows the 8-byte record of each (query, bin) points at (csrc/rq_device.h, rq_tail_body.h), and the
certificate cannot notice a wrong record: it is its input.  Top-k parity tests touch at most k bins per query, so a rare record
fault -- or a wrong second / third code, which matters only when two top rows share a bin -- slips through them.  Here every
record of every query of a call is read back (rq_debug_bin_records, option poison_bins) and checked with
tests/bin_records.check_records (invariants I1..I8, the bound the tail itself uses).

Each case asserts that its route really ran (scan8_used / hints_used / profiled scan launches) and that no repair pass
replaced the records.  Shards: 40 033 rows (33 valid rows in the last bin), 4 101 (5) and 65 537 (1); 300k and 1M rows built on
the device.  Planted: for query j a near-copy at position j mod 64 of bin 10 + j (every position 0..63), two strong rows of
query 1 in one bin (c2 / p2), three of query 2 in another (d), a zero row, a duplicate block across a bin edge, a near-copy of
query 3 in the ragged last bin.
"""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bin_records as br  # noqa: E402

pytestmark = pytest.mark.gpu
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
IP_SCALE = 3.0
N40, N4, N64 = 40_033, 4_101, 65_537
BMAX = 576

# ---- the forms (tests/test_bin_records.py checks that every built variant appears here) -------------------------------------
# 64-query rq_scan_kernel: the option sets of test_gpu_parity.test_every_kernel_variant_is_exact; (kstage, ring, prefetch) of every
# RQ_CASE, epi 0 / 1, nt 0 / 1, the generic and piped tails
SCAN64_FORMS = [dict(), dict(epi=0), dict(fast_tail=0), dict(fast_tail=0, slack_bins=0), dict(pipeline=1), dict(pipeline=2),
                dict(wide_batch=0), dict(epi=0, pipeline=2), dict(epi=0, pipeline=1), dict(wg_per_cu=1), dict(wg_per_cu=3),
                dict(slack_bins=0), dict(nt=1),
                dict(kstage=1, ring=2, prefetch=1), dict(kstage=1, ring=2, prefetch=4), dict(kstage=1, ring=3, prefetch=4),
                dict(kstage=1, ring=3, prefetch=12), dict(kstage=1, ring=4, prefetch=4),
                dict(kstage=2, ring=3, prefetch=1), dict(kstage=2, ring=4, prefetch=1), dict(kstage=2, ring=4, prefetch=4),
                dict(kstage=2, ring=6, prefetch=4), dict(kstage=2, ring=5, prefetch=6, nt=0), dict(kstage=2, ring=6, prefetch=12)]
GRIDS = [(2, 256), (1, 7), (2, 3)]                                    # (wg_per_cu, cu_count) of the default form
WIDE128_FORMS = [dict(wide_batch=3, wide128=v) for v in (0, 1, 4, 5, 6, 7)] + [dict(wide_batch=2)]
WIDE256_FORMS = [dict(wide_batch=1, wide256=2)]
I8_SCAN_FORMS = {1: dict(scan8=2, scan8_split=0), 2: dict(scan8=2, scan8_split=1),   # rq_scan.hip a.i8: 64 queries, one / two images
                 3: dict(scan8=2, wide256_8=0)}                                       # 128 queries (calls of 65..128 queries)
I8_256_VARIANTS = (22, 25, 30, 31, 32, 33)
FUSED_FORMS = [dict(epi=e, fused_nv=nv) for e in (1, 0) for nv in (1, 4, 8)]


# ---- data ---------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _plan(n, q):
    """Planted rows {row: fp16 vector} and the records they pin {(query, bin): (p1, p2 or None)}."""
    rng = np.random.default_rng(n)
    nbins = (n + 63) // 64
    noise = _unit(rng.standard_normal((BMAX + 8, 768)))
    qh = _unit(q[:, :768])
    rows, pins = {}, {}
    near = lambda j, c, t: (c * qh[j] + np.sqrt(1 - c * c) * noise[t]).astype(np.float32)
    for j in range(min(BMAX, nbins - 16)):                           # query j: position j mod 64 of bin 10 + j
        rows[64 * (10 + j) + j % 64] = near(j, 0.995, j)
        pins[(j, 10 + j)] = (j % 64, None)
    s2, s3 = nbins - 6, nbins - 4
    rows[64 * s2 + 5], rows[64 * s2 + 40] = near(1, 0.9, BMAX), near(1, 0.8, BMAX + 1)
    pins[(1, s2)] = (5, 40)
    rows[64 * s3 + 3], rows[64 * s3 + 30], rows[64 * s3 + 61] = near(2, 0.9, BMAX + 2), near(2, 0.8, BMAX + 3), near(2, 0.7, BMAX + 4)
    pins[(2, s3)] = (3, 30)
    rows[n - 1] = near(3, 0.995, BMAX + 5)                            # the ragged last bin
    pins[(3, nbins - 1)] = ((n - 1) % 64, None)
    return {r: v.astype(np.float16) for r, v in rows.items()}, pins


def _edit_rows(x, lo, rows):
    """Planted rows, a zero row (5) and a duplicate block across a bin edge (200..259 = row 7), on rows [lo, lo + len(x))."""
    for r, v in rows.items():
        if lo <= r < lo + len(x):
            x[r - lo] = v
    if lo == 0:
        x[5] = 0
        x[200:260] = x[7]


class Shard:
    """An index of n rows with non-unit rows (norms 0.5..2, planted rows unit), its fixed query set and exact scores in the
    scan's units (cosine: the score; inner product of IP_SCALE x the queries: E_ip / ||q||_64), computed once per query range."""

    def __init__(self, n, seed, device=False):
        self.n, self.nbins = n, (n + 63) // 64
        self.q = orc.synthetic_queries(BMAX, 768, seed=seed + 1)
        self.rows, self.pins = _plan(n, self.q)
        self.idx = nat.NativeIndex(768, 0)
        self.cu = int(self.idx.get_option("cu_count"))
        if device:
            self._build_device(seed)
            self.x16 = self.idx.get_rows_f16(0, n)
        else:
            x = orc.synthetic_corpus(n, 768, seed=seed).astype(np.float32)
            x *= np.random.default_rng(seed).uniform(0.5, 2.0, (n, 1)).astype(np.float32)
            x16 = x.astype(np.float16)
            _edit_rows(x16, 0, self.rows)
            self.x16 = x16
            self.idx.add_f16(x16)
        self._exact = {}

    def _build_device(self, seed, chunk=125_000):
        import torch
        dev = torch.device("cuda:0")
        self.idx.reserve(self.n)
        for c in range((self.n + chunk - 1) // chunk):
            lo, m = c * chunk, min(chunk, self.n - c * chunk)
            g = torch.Generator(device=dev); g.manual_seed(seed + c)
            s = 0.5 + 1.5 * torch.rand((m, 1), device=dev, generator=g)
            x = (torch.nn.functional.normalize(torch.randn((m, 768), device=dev, generator=g), dim=1) * s).half()
            mine = {r - lo: v for r, v in self.rows.items() if lo <= r < lo + m}
            if mine:
                x[list(mine)] = torch.from_numpy(np.stack(list(mine.values()))).to(dev)
            if lo == 0:
                x[5] = 0
                x[200:260] = x[7]
            x = x.contiguous()
            self.idx.add_f16_device(x, m)
            del x

    def queries(self, metric, q0, B):
        return self.q[q0:q0 + B] * (IP_SCALE if metric == IP else 1.0)

    def exact(self, metric, q0, B):
        """Small shards: all BMAX queries once per metric; 300k / 1M rows: the range asked for (discarded with _exact.clear())."""
        lo, hi = (0, BMAX) if self.n < 100_000 else (q0, q0 + B)
        if (metric, lo, hi) not in self._exact:
            q = self.queries(metric, lo, hi - lo)
            e = orc.exact_scores(q, self.x16, metric).astype(np.float64)
            if metric == IP:
                e /= np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None]
            self._exact[(metric, lo, hi)] = e
        return self._exact[(metric, lo, hi)][q0 - lo:q0 - lo + B]

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(n, device=False):
        if n not in made:
            made[n] = Shard(n, 700 + n % 997, device)
        return made[n]
    yield get
    for s in made.values():
        s.close()


# ---- one call and its records -------------------------------------------------------------------------------------------------
class Call:
    """Buffers of one rq_search_device call, kept alive until the records have been read."""

    def __init__(self, q):
        import torch
        self.B = q.shape[0]
        self.dq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()

    def run(self, idx, k, metric, stream=0, hint=None):
        import torch
        self.sc = torch.empty((self.B, k), device="cuda"); self.rw = torch.empty((self.B, k), device="cuda", dtype=torch.int64)
        self.st = torch.full((self.B,), 9, device="cuda", dtype=torch.int32)
        if hint is not None:
            idx.search_hint_next_device(hint.dq, hint.B, stream)
        idx.search_device(self.dq, self.B, k, metric, self.sc, self.rw, None, self.st, stream)
        return self


def _counters(idx):
    t = idx.timing()
    return dict(launches=t["scan_launches"], exact=t["exact_scans"], repaired=int(idx.get_option("repaired_queries")),
                scan8=int(idx.get_option("scan8_used")), hints=int(idx.get_option("hints_used")))


def _fp16_beta(idx, metric):
    if metric == COS:
        return idx.get_option("eps_cosine")
    return idx.get_option("eps_ip") * idx.get_option("max_row_norm") * (1 + 1e-6)


def _int8_beta(idx, q, metric, split):
    eq = br.int8_query_error(q, split)[:, None]
    be = idx.debug_bin_err((len(idx) + 63) // 64).astype(np.float64)[None, :]
    beta = eq + (1 + eq) * (be * 1.000001 + 2e-5)
    return beta * (idx.get_option("max_row_norm") if metric == IP else 1.0)


def _check(sh, rec, metric, q0, B, beta, int8=False, what=""):
    """I1..I8 on records rec[:B] of queries q0 .. q0 + B (pad slots rec[B:]), tightness, and the planted positions."""
    exact = sh.exact(metric, q0, B)
    rep = br.check_records(rec, exact, sh.n, beta, B)
    bad = br.failures(rep)
    assert not bad, f"{what}: " + "; ".join(bad)
    tight = br.tightness(rec, exact, sh.n)
    lim = 0.3 * float(np.max(beta)) if int8 else 1e-4
    assert tight <= lim, f"{what}: bin maxima off by {tight} (limit {lim})"
    f = br.decode(rec[:B])
    pinned = 0
    for (j, b), (p1, p2) in sh.pins.items():
        if q0 <= j < q0 + B:
            assert f["p1"][j - q0, b] == p1, (what, j, b, int(f["p1"][j - q0, b]), p1)
            if p2 is not None:
                assert f["p2"][j - q0, b] == p2, (what, j, b, int(f["p2"][j - q0, b]), p2)
            pinned += 1
    return pinned


def _records(idx, slots, stream=0):
    rec = idx.debug_bin_records(0, slots, stream)
    with pytest.raises(nat.RqError):                                  # the hook knows how many slots the call's passes covered
        idx.debug_bin_records(0, slots + 1, stream)
    return rec


def _plain(sh, opts, B, metric=COS, k=10, slots=None, passes=1, int8=False, split=False, q0=0):
    """One rq_search_device call on the null stream under `opts`; every record of its slots checked."""
    import torch
    idx = sh.idx
    for name in ("poison_bins", "profile"):
        idx.set_option(name, 1)
    for name, v in opts.items():
        idx.set_option(name, v)
    try:
        before = _counters(idx)
        q = sh.queries(metric, q0, B)
        c = Call(q).run(idx, k, metric)
        idx.search_flush_device(0)
        torch.cuda.synchronize()
        after = _counters(idx)
        if int8:
            assert after["scan8"] == before["scan8"] + 1, opts
        else:
            assert after["scan8"] == before["scan8"] and after["launches"] == before["launches"] + passes, (opts, before, after)
        assert after["exact"] == before["exact"] and after["repaired"] == before["repaired"]
        rec = _records(idx, slots or 64)
        beta = _int8_beta(idx, q, metric, split) if int8 else _fp16_beta(idx, metric)
        _check(sh, rec, metric, q0, B, beta, int8, what=f"{opts} B={B}")
        del c
    finally:
        idx.search_flush_device(0)
        _restore(sh, opts)


_DEFAULTS = dict(kstage=2, ring=3, prefetch=1, epi=1, nt=-1, fast_tail=1, slack_bins=-1, pipeline=0, wide_batch=1, wg_per_cu=0,
                 wide128=0, wide256=2, scan8=1, scan8_split=-1, wide256_8=31, fused_nv=0, scan_ahead=1)


def _restore(sh, opts):
    """Back to the defaults for the next case (the shard's index is shared by the module)."""
    for name in opts:
        sh.idx.set_option(name, sh.cu if name == "cu_count" else _DEFAULTS[name])
    sh.idx.set_option("profile", 0)


# ---- 64-query rq_scan_kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", SCAN64_FORMS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_scan64_records(shards, opts):
    _plain(shards(N40), dict(opts, scan8=0), 64)


@pytest.mark.parametrize("n", [N40, N4, N64])
@pytest.mark.parametrize("wg,cus", GRIDS)
def test_scan64_default_records_across_grids_and_inner_product(shards, n, wg, cus):
    sh = shards(n)
    _plain(sh, dict(scan8=0, wg_per_cu=wg, cu_count=cus), 64)
    if (wg, cus) == GRIDS[0]:
        _plain(sh, dict(scan8=0), 64, metric=IP)
        _plain(sh, dict(scan8=0), 37, metric=IP)


def test_zero_query_records(shards):
    """A zero query may end uncertified (every score ties) and take the repair route, so it has a case of its own: the records
    of its call are read before any repair."""
    import torch
    sh = shards(N4)
    idx = sh.idx
    idx.set_option("poison_bins", 1)
    for scan8 in (0, 2):
        idx.set_option("scan8", scan8)
        q = np.stack([np.zeros(768, np.float32), sh.q[1]])
        before = _counters(idx)
        c = Call(q).run(idx, 10, COS)
        torch.cuda.synchronize()
        assert _counters(idx)["scan8"] == before["scan8"] + (1 if scan8 else 0)
        rec = _records(idx, 64)
        exact = np.stack([np.zeros(sh.n), sh.exact(COS, 1, 1)[0]])
        beta = _int8_beta(idx, q, COS, False) if scan8 else _fp16_beta(idx, COS)
        rep = br.check_records(rec, exact, sh.n, beta, 2)
        assert not br.failures(rep), br.failures(rep)
        del c
    idx.set_option("scan8", 1)


def test_records_hook_follows_the_last_call_and_refuses_without_a_scan(shards):
    """rq_debug_bin_records / rq_debug_pooled read where the stream's LAST call put its records: after a scanned call every slot its
    passes covered (and no more), nothing after a call that scanned nothing (exact route of a tiny shard, empty shard), nothing on a
    multi-device index.  rq_debug_pooled returns the decoded maxima of the same records."""
    import torch
    sh = shards(N4)
    q = sh.queries(COS, 0, 70)
    c = Call(q).run(sh.idx, 10, COS)                                   # 70 queries: one 128-query pass
    torch.cuda.synchronize()
    rec = _records(sh.idx, 128)
    assert np.array_equal(sh.idx.debug_pooled(69, sh.nbins), br.decode(rec[69])["m1"])
    with pytest.raises(nat.RqError):
        sh.idx.debug_pooled(128, sh.nbins)
    assert sh.idx.debug_bin_records(5, 3)[0].tobytes() == rec[5].tobytes()
    tiny = nat.NativeIndex(768, 0)
    tiny.add_f16(sh.x16[:100])                                         # two bins: every call takes the exact route
    for idx in (tiny, nat.NativeIndex(768, 0)):                        # ... and an empty index
        c2 = Call(q[:4]).run(idx, 10, COS)
        torch.cuda.synchronize()
        with pytest.raises(nat.RqError):
            idx.debug_bin_records(0, 1)
        with pytest.raises(nat.RqError):
            idx.debug_pooled(0, 2)
        idx.close()
    multi = nat.NativeIndex(768, devices=[0, 0])
    multi.add_f16(sh.x16[:8192])
    multi.search(q[:4], 10)
    with pytest.raises(nat.RqError):
        multi.debug_bin_records(0, 1)
    multi.close()
    del c, c2


# ---- passes of 128 and 256 queries (rq_scan_wide.hip, rq_scan.hip wide_batch = 2) ------------------------------------------
@pytest.mark.parametrize("opts", WIDE128_FORMS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("B", [65, 128])
def test_wide128_records(shards, opts, B):
    for n in (N40, N4):
        _plain(shards(n), dict(opts, scan8=0), B, slots=128)


@pytest.mark.parametrize("opts", WIDE256_FORMS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_wide256_records(shards, opts):
    sh = shards(N40)
    _plain(sh, dict(opts, scan8=0), 200, slots=256)
    _plain(sh, dict(opts, scan8=0), 333, slots=384, passes=2)                     # 256 + 128: the second grid (nwg_split)
    _plain(sh, dict(opts, scan8=0), 333, metric=IP, slots=384, passes=2)
    _plain(shards(N4), dict(opts, scan8=0), 200, slots=256)


# ---- the int8 image -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i8", [1, 2])
def test_int8_scan64_records(shards, i8):
    for n in (N40, N4):
        sh = shards(n)
        _plain(sh, I8_SCAN_FORMS[i8], 64, int8=True, split=i8 == 2)
        _plain(sh, I8_SCAN_FORMS[i8], 64, metric=IP, int8=True, split=i8 == 2)


def test_int8_top_row_in_a_ragged_last_bin_is_found(shards):
    """The int8 forms once left the triple of a lane with no valid row of the quad at -inf, and the lane's position bits made it a
    signalling NaN that the selection returned instead of dropping: the ragged last bin (5 or 1 valid rows) recorded m1 = NaN and
    was never re-scored.  Query 3's near-copy sits there; every int8 form must return it at rank 1, like the oracle."""
    for n in (N4, N64):
        sh = shards(n)
        for opts, B in ((I8_SCAN_FORMS[1], 64), (I8_SCAN_FORMS[2], 64), (I8_SCAN_FORMS[3], 128), (dict(scan8=2, wide256_8=22), 256),
                        (dict(scan8=2), 256)):
            for name, v in opts.items():
                sh.idx.set_option(name, v)
            before = _counters(sh.idx)
            s, r = sh.idx.search(sh.q[:B], 10, COS)
            assert _counters(sh.idx)["scan8"] == before["scan8"] + 1, opts
            es, er = orc.dense_topk(sh.q[:B], sh.x16, 10)
            assert r[3, 0] == n - 1 and np.array_equal(r, er), (n, opts, np.argwhere(r != er)[:4].tolist())
            assert float(np.abs(s - es).max()) <= 1e-6
            _restore(sh, opts)


def test_int8_wide128_records(shards):
    for n in (N40, N4):
        _plain(shards(n), I8_SCAN_FORMS[3], 128, slots=128, int8=True)                # rq_scan.hip I8 = 3
        _plain(shards(n), I8_SCAN_FORMS[3], 65, slots=128, int8=True)


@pytest.mark.parametrize("variant", I8_256_VARIANTS)
def test_int8_wide256_records(shards, variant):
    sh = shards(N40)
    for B, slots in ((256, 256), (333, 384), (576, 576)):                              # 256 + 128, 2 x 256 + 64
        _plain(sh, dict(scan8=2, wide256_8=variant), B, slots=slots, int8=True)
    _plain(shards(N4), dict(scan8=2, wide256_8=variant), 256, slots=256, int8=True)      # 5 valid rows in the last bin


def test_int8_wide256_records_odd_quads_per_workgroup(shards):
    """773 quads over 256 workgroups (3 or 4 each: both ring parities), then over 3 workgroups (many record flushes)."""
    sh = shards(256 * 3 * 64 + 64 * 5 + 9)
    for cus in (256, 3):
        _plain(sh, dict(scan8=2, cu_count=cus), 260, slots=320, int8=True)            # 256 + 64


# ---- fused scan + tail (pipeline = 2), the scanned-ahead pair ------------------------------------------------------------------
def _stream_calls(sh, opts, plan, check_after, int8=False):
    """Consecutive calls on one stream under `opts`: plan = [(q0, B, k, metric, announce the next call's queries)]; after call i
    of check_after the records of that call are checked: check_after[i] = (slots, route)."""
    import torch
    idx = sh.idx
    idx.set_option("poison_bins", 1)
    idx.set_option("profile", 1)
    for name, v in opts.items():
        idx.set_option(name, v)
    st = torch.cuda.Stream()
    calls = [Call(sh.queries(m, q0, B)) for q0, B, k, m, _ in plan]      # (an announced batch is claimed by its pointer)
    try:
        with torch.cuda.stream(st):
            for i, (q0, B, k, metric, hint) in enumerate(plan):
                before = _counters(idx)
                calls[i].run(idx, k, metric, st.cuda_stream, hint=calls[i + 1] if hint else None)
                if i not in check_after:
                    continue
                slots, route = check_after[i]
                st.synchronize()
                after = _counters(idx)
                assert after["exact"] == before["exact"] and after["repaired"] == before["repaired"]
                assert after["scan8"] == before["scan8"] + (1 if int8 else 0)
                if route == "pair2":                                     # no scan: the previous pass holds this batch's records
                    assert after["launches"] == before["launches"] and after["hints"] == before["hints"] + 1, (before, after)
                else:                                                    # one launch: the fused scan + tail, or the 128-query pair pass
                    assert after["launches"] == before["launches"] + 1, (before, after)
                rec = _records(idx, slots, st.cuda_stream)
                q = sh.queries(metric, q0, B)
                beta = _int8_beta(idx, q, metric, False) if int8 else _fp16_beta(idx, metric)
                what = f"{opts} call {i} ({route})"
                if route == "pair1":                                     # lower half: this call; upper half: the announced batch
                    _check(sh, rec[:B], metric, q0, B, beta, what=what + " lower half")
                    q1, B1, _, m1, _ = plan[i + 1]
                    _check(sh, rec[64:], m1, q1, B1, beta, what=what + " upper half")
                else:
                    _check(sh, rec, metric, q0, B, beta, int8, what=what)
        idx.search_flush_device(st.cuda_stream)
        st.synchronize()
    finally:
        idx.stream_release(st.cuda_stream)
        _restore(sh, opts)


@pytest.mark.parametrize("opts", FUSED_FORMS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_fused_scan_tail_records(shards, opts):
    """rq_scan_tail_kernel: the second and third calls of a loop carry the previous call's tail (scan_ahead = 0: no pairs)."""
    plan = [(0, 64, 10, COS, False), (64, 64, 10, COS, False), (128, 64, 50, COS, False)]
    _stream_calls(shards(N40), dict(opts, scan8=0, pipeline=2, scan_ahead=0), plan, {1: (64, "fused"), 2: (64, "fused")})


def test_int8_fused_records(shards):
    plan = [(0, 64, 10, COS, False), (64, 64, 10, COS, False), (128, 64, 10, IP, False)]
    _stream_calls(shards(N40), dict(scan8=2, pipeline=2), plan, {1: (64, "fused"), 2: (64, "fused")}, int8=True)


def test_pair_pass_records_300k(shards):
    """scan_ahead (shards beyond 208 MiB): one 128-query pass scans a call and the batch it announced; the second call runs no
    scan and its records are the pass's upper half.  Full and ragged second halves, a matched pair with another k."""
    sh = shards(300_000, device=True)
    assert sh.n * 1536 > (208 << 20)
    plan = [(0, 64, 10, IP, True), (64, 64, 10, IP, False), (128, 64, 10, IP, True), (192, 37, 50, IP, False)]
    _stream_calls(sh, dict(scan8=0, pipeline=2), plan, {0: (128, "pair1"), 1: (64, "pair2"), 2: (128, "pair1"), 3: (64, "pair2")})


def test_headline_loop_records_1m(shards):
    """The loop bench.py times at 1M rows: fp16 pairs of hinted 64-query batches, then the int8 fused pair of calls."""
    sh = shards(1_000_000, device=True)
    plan = [(0, 64, 10, COS, True), (64, 64, 10, COS, False)]
    _stream_calls(sh, dict(scan8=0, pipeline=2), plan, {0: (128, "pair1"), 1: (64, "pair2")})
    sh._exact.clear()
    plan = [(128, 64, 10, COS, False), (192, 64, 10, COS, False)]
    _stream_calls(sh, dict(scan8=2, pipeline=2), plan, {1: (64, "fused")}, int8=True)
    sh._exact.clear()
