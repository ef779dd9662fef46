"""Non-finite and extreme values through every search route (MI355X), against tests/nonfinite_oracle.py -- include/rq.h's rules:
a NaN score counts as -inf, a zero-norm query scores every row 0.0, +-inf scores order like any other, a -inf row is still a row.

Every case compares rows exactly and scores bit for bit where they are non-finite, to SCORE_TOL elsewhere.  The shapes are the
smallest that still take the approximate route (2 nb < bins: at k = 10, nb = 18, more than 2 304 rows).

Shard A, 4 101 rows (64 whole bins and a ragged one of 5), at dim 768 and at dim 384 (the narrow layout in every test of shard A;
the 768-element layout of dim 384, which runs the kernels of dim 768, in the blocking, score_rows and exact-route tests), synthetic_corpus with
  row 5 one +inf element | rows 64..127 all NaN (a whole bin: a failed embedding batch) | row 200 one +inf and one -inf element |
  row 300 every element 65 504 | rows 1000..1009 zero | row 2049 NaN | row 2050 the direction of query 0 (the NaN row is its
  neighbour in the bin) | row 4099 the direction of query 6, in the ragged last bin | row 4100 one -inf element, same bin.
Queries: 0 and 6 the planted matches, 1 all NaN, 2 one +inf element, 3 Gaussian x 1e-40 (fp32 subnormal), 4 Gaussian x 1e36, 5 zero,
  7 one -inf element, the rest Gaussian.
Shard B: the same size, 7 finite rows, every other row NaN.  Shard C: 130 rows, the exact route.
"""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bin_records as br  # noqa: E402
import mmr_oracle as mmo  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402

pytestmark = pytest.mark.gpu
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
METRICS = [COS, IP]
SCORE_TOL = 1e-6
N = nfo.N_A
LAYOUTS = {"768": (768, 768), "384narrow": (384, 384), "384wide": (384, 768)}      # name: (dim, row_pad)
BQ = 257                                                                             # queries made per dim
NONFINITE_Q = (1, 2, 7)


def _index(dim, row_pad, **kw):
    idx = nat.NativeIndex(dim, **kw)
    if idx.row_pad != row_pad:
        idx.set_option("row_pad", row_pad)
    assert idx.row_pad == row_pad
    return idx


class World:
    """Queries and shard A per dim, one index per layout, and the helper's score matrices, each made once and left unchanged."""

    def __init__(self):
        self._q, self._x, self._idx, self._s = {}, {}, {}, {}

    def q(self, dim):
        if dim not in self._q:
            q = nfo.queries(dim, BQ)
            q[122:130] = q[:8]                      # the special queries again at the end of a 130- and of a 257-query call:
            q[249:257] = q[:8]                      # in the ragged last pass, and in slots other than 0..7
            q.setflags(write=False)
            self._q[dim] = q
        return self._q[dim]

    def x(self, dim):
        if dim not in self._x:
            x = nfo.shard_a(dim, self.q(dim))
            x.setflags(write=False)
            self._x[dim] = x
        return self._x[dim]

    def idx(self, layout):
        if layout not in self._idx:
            dim, pad = LAYOUTS[layout]
            idx = _index(dim, pad)
            idx.add_f16(self.x(dim)[:2000]); idx.add_f16(self.x(dim)[2000:])
            self._idx[layout] = idx
        return self._idx[layout]

    def scores(self, dim, metric):
        if (dim, metric) not in self._s:
            s = nfo.scores(self.q(dim), self.x(dim), metric)
            s.setflags(write=False)
            self._s[(dim, metric)] = s
        return self._s[(dim, metric)]

    def gold(self, dim, metric, B, k, row_offset=0):
        return orc.topk_from_scores(self.scores(dim, metric)[:B], k, row_offset)

    def close(self):
        for i in self._idx.values():
            i.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def _ok(res, gold, what):
    nfo.assert_matches(res[0], res[1], gold[0], gold[1], SCORE_TOL, what)


_DEFAULTS = dict(epi=1, fast_tail=1, eps=-1, wide_batch=1, pipeline=0, filter_route=-1, poison_bins=0, scan8=1)


class _Options:
    def __init__(self, idx, **opts):
        self.idx, self.opts = idx, opts

    def __enter__(self):
        for name, v in self.opts.items():
            self.idx.set_option(name, v)
        return self.idx

    def __exit__(self, *exc):
        for name in self.opts:
            self.idx.set_option(name, _DEFAULTS[name])


class _Dev:
    """Device buffers of one search_device call."""

    def __init__(self, q, k):
        import torch
        self.k, self.B = k, q.shape[0]
        self.dq = torch.from_numpy(np.array(q, dtype=np.float32, order="C")).cuda()      # (a copy: the module's queries are read-only)
        self.sc = torch.full((self.B, k), -7.0, device="cuda")
        self.rw = torch.full((self.B, k), -7, device="cuda", dtype=torch.int64)
        self.ky = torch.zeros((self.B, k), device="cuda", dtype=torch.int64)
        self.st = torch.full((self.B,), 9, device="cuda", dtype=torch.int32)

    def run(self, idx, metric, stream=0, hint=None):
        if hint is not None:
            idx.search_hint_next_device(hint.dq, hint.B, stream)
        idx.search_device(self.dq, self.B, self.k, metric, self.sc, self.rw, self.ky, self.st, stream)
        return self

    def fixup(self, idx, metric, stream=0):
        idx.search_fixup_device(self.dq, self.B, self.k, metric, self.sc, self.rw, self.ky, self.st, stream)
        return self

    def result(self):
        import torch
        torch.cuda.synchronize()
        assert int(self.st.abs().sum()) == 0
        return self.sc.cpu().numpy(), self.rw.cpu().numpy()


# ---- blocking rq_search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_blocking_search(world, layout, metric):
    """k = 10 (the fast tail), 100 and 321 (beyond RQ_FAST_MAX_M: the generic tail / the exact route at this size)."""
    dim = LAYOUTS[layout][0]
    idx, q = world.idx(layout), world.q(dim)
    for k in (10, 100, 321):
        _ok(idx.search(q[:64], k, metric), world.gold(dim, metric, 64, k), f"{layout} metric {metric} k {k}")


@pytest.mark.parametrize("metric", METRICS)
def test_zero_norm_query_answers_the_first_rows_at_zero_on_every_route(world, metric):
    """include/rq.h: rows 0 .. k-1 at 0.0 whatever they hold -- row 5 carries an infinite element, rows 64..127 are NaN.  The
    routes: fast tail, generic tail (fast_tail = 0, and k = 321), widened and exact rungs (eps = 10), the exact route of a small
    shard, filtered searches by gather, scan and exact scan, score_rows."""
    idx, q = world.idx("768"), world.q(768)[5:6]
    assert not q.any()
    want = lambda k, n=N: (np.zeros((1, k), np.float32), np.where(np.arange(k) < n, np.arange(k), -1)[None, :].astype(np.int64))
    for opts, k in [(dict(), 10), (dict(), 100), (dict(), 321), (dict(fast_tail=0), 10), (dict(fast_tail=0), 100), (dict(eps=10), 10),
                    (dict(epi=0), 10)]:
        with _Options(idx, **opts):
            _ok(idx.search(q, k, metric), want(k), f"zero query {opts} k {k}")
    small = _index(768, 768)
    small.add_f16(world.x(768)[:130])
    for k in (10, 130, 200):
        _ok(small.search(q, k, metric), want(k, 130), f"zero query, 130 rows, k {k}")
    small.close()
    mask = np.zeros(N, bool)
    mask[[5, 64, 65, 200, 2049, 2050, 4100]] = True
    mask[1::2] = True
    allowed = np.flatnonzero(mask)
    flt = idx.make_filter(mask)
    for route in (1, 2, 3):
        with _Options(idx, filter_route=route):
            s, r = idx.search(q, 10, metric, row_filter=flt)
            assert int(idx.get_option("filter_route_last")) == route
        _ok((s, r), (np.zeros((1, 10), np.float32), allowed[None, :10]), f"zero query filter route {route}")
    flt.close()
    rows = np.array([[5, 64, 200, 300, 1000, 2049, 4100, -1]], np.int64)
    assert np.array_equal(idx.score_rows(q, rows, metric).view(np.uint32), np.zeros((1, 8), np.uint32))


# ---- the options that choose a kernel or a rung -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("opts", [dict(epi=0), dict(epi=1), dict(fast_tail=0), dict(eps=10)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_scan_and_tail_forms(world, opts, metric):
    """epi 0 / 1 (compare-select / positions inside the scores), the generic tail, and eps = 10: no query certifies, every one is
    widened -- at this size the widened pass already re-scores every bin, which is the exact route."""
    for layout in ("768", "384narrow"):
        dim = LAYOUTS[layout][0]
        idx = world.idx(layout)
        with _Options(idx, **opts):
            t0 = idx.timing()
            _ok(idx.search(world.q(dim)[:64], 10, metric), world.gold(dim, metric, 64, 10), f"{layout} {opts} metric {metric}")
            t1 = idx.timing()
        if "eps" in opts:
            assert t1["widened"] - t0["widened"] >= 63, (t0, t1)   # (all but the zero query)


@pytest.mark.parametrize("metric", METRICS)
def test_eps_forces_widening_and_then_the_exact_scan(world, metric):
    """9 301 rows = 146 bins: the widened pass re-scores 4 x 18 = 72 bins, fewer than half, so it is still an approximate pass
    with a certificate; under eps = 10 it refuses too and the queries reach the ladder's last rung.  All but the zero query are
    widened.  Under cosine all 63 go on to the exact scan (bound = b + 10 is never below a cosine).  Under the inner product the two
    queries with an infinite element certify in the widened pass, rightly: their norm is infinite, every approximate score is the
    clamp value, so the bound (b + eps |x|max) |q| is -inf and the lowest bins, which equal maxima select, hold the first k rows at
    +inf -- the answer under the tie rule."""
    n = 9_301
    q = world.q(768)[:64]
    x = nfo.shard_a(768, q, n=n)
    idx = _index(768, 768)
    idx.add_f16(x)
    gold = nfo.topk(q, x, 10, metric)
    _ok(idx.search(q, 10, metric), gold, f"{n} rows metric {metric}")
    with _Options(idx, eps=10):
        t0 = idx.timing()
        _ok(idx.search(q, 10, metric), gold, f"{n} rows eps 10 metric {metric}")
        t1 = idx.timing()
    idx.close()
    assert t1["widened"] - t0["widened"] == 63 and t1["exact_scans"] - t0["exact_scans"] == (63 if metric == COS else 61), (t0, t1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B,opts", [(130, dict()), (257, dict()), (130, dict(wide_batch=0)), (257, dict(wide_batch=0))],
                         ids=["128-query pass", "256-query pass", "130 in passes of 64", "257 in passes of 64"])
def test_wide_passes(world, B, opts, metric):
    for layout in ("768", "384narrow"):
        dim = LAYOUTS[layout][0]
        idx = world.idx(layout)
        with _Options(idx, **opts):
            _ok(idx.search(world.q(dim)[:B], 10, metric), world.gold(dim, metric, B, 10), f"{layout} B {B} {opts} metric {metric}")


# ---- device calls: fused tails with hints, trains, merged shards, several devices ---------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", ["768", "384narrow"])
def test_fused_pipeline_with_hints_and_train(world, layout, metric):
    """pipeline = 2 on one stream: two batches, the second announced to the first, flushed at the end, then repaired; and the same
    two batches as one rq_search_train_device call."""
    import torch
    dim = LAYOUTS[layout][0]
    idx, q = world.idx(layout), world.q(dim)
    batches = [q[:64], q[64:128]]
    gold = [orc.topk_from_scores(world.scores(dim, metric)[lo:lo + 64], 10) for lo in (0, 64)]
    st = torch.cuda.Stream()
    with _Options(idx, pipeline=2):
        try:
            calls = [_Dev(b, 10) for b in batches]
            torch.cuda.synchronize()
            h0 = int(idx.get_option("hints_used"))
            with torch.cuda.stream(st):
                calls[0].run(idx, metric, st.cuda_stream, hint=calls[1])
                calls[1].run(idx, metric, st.cuda_stream)
                idx.search_flush_device(st.cuda_stream)
                assert int(idx.get_option("hints_used")) - h0 >= 1
                for c, g, name in zip(calls, gold, ("first", "second")):
                    _ok(c.fixup(idx, metric, st.cuda_stream).result(), g, f"{layout} fused {name} batch metric {metric}")
            calls = [_Dev(b, 10) for b in batches]
            torch.cuda.synchronize()
            train = idx.make_train([c.dq for c in calls], [c.sc for c in calls], [c.rw for c in calls], [c.ky for c in calls],
                                   [c.st for c in calls], [st.cuda_stream])
            idx.search_train_device(train, 64, 10, metric)
            idx.search_flush_device(st.cuda_stream)
            with torch.cuda.stream(st):
                for c, g, name in zip(calls, gold, ("first", "second")):
                    _ok(c.fixup(idx, metric, st.cuda_stream).result(), g, f"{layout} train {name} batch metric {metric}")
        finally:
            idx.search_flush_device(st.cuda_stream)
            idx.stream_release(st.cuda_stream)


@pytest.mark.parametrize("metric", METRICS)
def test_multi_device_index_and_merged_row_offset_shards(world, metric):
    import torch
    q, x = world.q(768)[:64], world.x(768)
    gold = world.gold(768, metric, 64, 10)
    multi = nat.NativeIndex(768, devices=[0, 0, 0])
    multi.set_option("stripe_rows", 1024)
    multi.add_f16(x[:3000]); multi.add_f16(x[3000:])
    _ok(multi.search(q, 10, metric), gold, f"multi-device metric {metric}")
    multi.close()
    # two shards with row offsets: their keys (+-inf scores among them) merged on the device
    k, cut, off = 10, 2051, 1_000_000
    keys = torch.zeros((64, 2 * k), device="cuda", dtype=torch.int64)
    for j, (lo, hi) in enumerate(((0, cut), (cut, N))):
        s = _index(768, 768)
        s.add_f16(x[lo:hi])
        s.set_row_offset(off + lo)
        c = _Dev(q, k).run(s, metric).fixup(s, metric)
        _ok(c.result(), nfo.topk(q, x[lo:hi], k, metric, row_offset=off + lo), f"shard {j} metric {metric}")
        keys[:, j * k:(j + 1) * k] = c.ky
        s.close()
    sc = torch.empty((64, k), device="cuda"); rw = torch.empty((64, k), device="cuda", dtype=torch.int64)
    ko = torch.zeros((64, k), device="cuda", dtype=torch.int64)
    nat.merge_keys_device(keys, 2 * k, 64, k, sc, rw, ko)
    torch.cuda.synchronize()
    want = world.gold(768, metric, 64, k, row_offset=off)
    _ok((sc.cpu().numpy(), rw.cpu().numpy()), want, f"merged shards metric {metric}")
    from rag_uq_amd import distributed as dist
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), dist.pack_keys(*want))       # the host codec builds the device's keys


# ---- filtered, diversified, scored -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("route", [1, 2, 3], ids=["gather", "scan", "exact"])
def test_filtered_search(world, route, metric):
    """A mask that allows every planted row and half of the others."""
    for layout in ("768", "384narrow"):
        dim = LAYOUTS[layout][0]
        idx, q = world.idx(layout), world.q(dim)[:64]
        mask = np.random.default_rng(12).random(N) < 0.5
        mask[nfo.PLANTED_A] = True
        flt = idx.make_filter(mask)
        with _Options(idx, filter_route=route):
            res = idx.search(q, 10, metric, row_filter=flt)
            assert int(idx.get_option("filter_route_last")) == route
        flt.close()
        _ok(res, nfo.topk(q, world.x(dim), 10, metric, mask=mask), f"{layout} filter route {route} metric {metric}")


@pytest.mark.parametrize("metric", METRICS)
def test_mmr_over_nonfinite_candidates(world, metric):
    idx, q, x = world.idx("768"), world.q(768)[:64], world.x(768)
    s, r = idx.search_mmr(q, 10, 10, 1.0, metric)                       # lambda = 1: the search itself
    _ok((s, r), world.gold(768, metric, 64, 10), f"mmr lambda 1 metric {metric}")
    ss, sr = idx.search(q, 10, metric)
    assert np.array_equal(sr, r) and ss.tobytes() == s.tobytes()
    gs, gr = world.gold(768, metric, 64, 20)                            # lambda = 0.5 over the helper's candidates
    with np.errstate(all="ignore"):
        ws, wr, wv = mmo.mmr_select_batch(gs, gr, x, 5, 0.5, metric)
    s, r, v = idx.search_mmr(q, 5, 20, 0.5, metric, return_mmr=True)
    _ok((s, r), (ws, wr), f"mmr lambda 0.5 metric {metric}")
    fin = np.isfinite(wv)
    assert np.array_equal(v[~fin], wv[~fin])
    assert float(np.abs(v[fin].astype(np.float64) - wv[fin]).max(initial=0.0)) <= SCORE_TOL * max(1.0, float(np.abs(wv[fin]).max(initial=0.0)))


@pytest.mark.parametrize("metric", METRICS)
def test_mmr_similarity_of_a_picked_zero_row_has_no_zero_norm_rule(world, metric):
    """sim(i, j) has no query: a picked zero row against a row with an infinite element is 0 x inf = NaN = -inf (include/rq.h).  The
    zero query's candidates under a filter are the first allowed rows at 0.0 -- zero rows, infinite rows and the 65 504 row among them."""
    idx, q, x = world.idx("768"), world.q(768)[5:6], world.x(768)
    mask = np.zeros(N, bool)
    mask[[1000, 1001, 5, 200, 300, 1002, 2049, 2050, 4100, 7, 8]] = True
    flt = idx.make_filter(mask)
    gs, gr = nfo.topk(q, x, 11, metric, mask=mask)
    assert gr[0].tolist() == sorted(np.flatnonzero(mask).tolist()) and not gs.any()
    for lam in (0.5, 0.0, 1.0):
        with np.errstate(all="ignore"):
            ws, wr, wv = mmo.mmr_select_batch(gs, gr, x, 8, lam, metric)
        s, r, v = idx.search_mmr(q, 8, 11, lam, metric, row_filter=flt, return_mmr=True)
        _ok((s, r), (ws, wr), f"zero rows among the candidates, lambda {lam} metric {metric}")
        fin = np.isfinite(wv)
        assert np.array_equal(v[~fin], wv[~fin]) and float(np.abs(v[fin] - wv[fin]).max(initial=0.0)) <= SCORE_TOL * max(1.0, float(np.abs(wv[fin]).max(initial=0.0)))
    flt.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_score_rows_reproduces_the_search_bit_for_bit(world, layout, metric):
    dim = LAYOUTS[layout][0]
    idx, q = world.idx(layout), world.q(dim)[:64]
    s, r = idx.search(q, 10, metric)
    _ok((s, r), world.gold(dim, metric, 64, 10), f"{layout} metric {metric}")
    again = idx.score_rows(q, r, metric)
    assert np.array_equal(again.view(np.uint32), s.view(np.uint32)), np.argwhere(again.view(np.uint32) != s.view(np.uint32))[:4].tolist()
    assert r[5].tolist() == list(range(10)) and not again[5].any()      # the zero query: row 5 (an infinite element) at 0.0
    full = idx.score_rows(q[:8], np.tile(np.arange(N, dtype=np.int64), (8, 1)), metric)      # ... and every pair of the special queries
    want = world.scores(dim, metric)[:8]
    fin = np.isfinite(want)
    assert np.array_equal(full[~fin], want[~fin]) and np.isfinite(full[fin]).all()
    assert float(np.abs(full[fin].astype(np.float64) - want[fin]).max()) <= SCORE_TOL * max(1.0, float(np.abs(want[fin]).max()))


# ---- shards B and C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_shard_of_seven_finite_rows(world, metric):
    """k = 10 over 7 finite rows among 4 094 NaN rows: the 7, then the three lowest NaN rows at -inf."""
    q = world.q(768)[:64]
    x = nfo.shard_b(768)
    idx = _index(768, 768)
    idx.add_f16(x)
    s, r = idx.search(q, 10, metric)
    _ok((s, r), nfo.topk(q, x, 10, metric), f"shard B metric {metric}")
    for b in (0, 4, 6, 8):
        assert sorted(r[b, :7].tolist()) == nfo.FINITE_B and r[b, 7:].tolist() == [0, 1, 2] and np.isneginf(s[b, 7:]).all()
    with _Options(idx, fast_tail=0):
        _ok(idx.search(q, 10, metric), nfo.topk(q, x, 10, metric), f"shard B generic tail metric {metric}")
    idx.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_exact_route_of_a_small_shard(world, layout, metric):
    dim, pad = LAYOUTS[layout]
    q = world.q(dim)[:64]
    x = nfo.shard_c(dim, q)
    idx = _index(dim, pad)
    idx.add_f16(x)
    for k in (130, 200):
        _ok(idx.search(q, k, metric), nfo.topk(q, x, k, metric), f"shard C {layout} k {k} metric {metric}")
    idx.close()


# ---- the int8 image ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_int8_image_declines_a_shard_with_an_infinite_row(world, metric):
    q = world.q(768)[:64]
    x = orc.synthetic_corpus(N, 768, seed=77)
    idx = _index(768, 768)
    idx.add_f16(x)
    idx.set_option("scan8", 2)
    _ok(idx.search(q, 10, metric), nfo.topk(q, x, 10, metric), f"int8 scan, clean shard, metric {metric}")
    used = int(idx.get_option("scan8_used"))
    assert used > 0 and 0 <= idx.get_option("scan8_row_err") < 0.03
    bad = x[:1].copy()
    bad[0, 3] = np.float16(np.inf)
    idx.add_f16(bad)
    x = np.concatenate([x, bad], 0)
    for k in (10, 100):
        _ok(idx.search(q, k, metric), nfo.topk(q, x, k, metric), f"int8 scan declined, metric {metric} k {k}")
    assert idx.get_option("scan8_row_err") == np.inf
    assert int(idx.get_option("scan8_used")) == used
    idx.close()


# ---- the scan's records -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,epi", [("768", 1), ("768", 0), ("384narrow", 1)], ids=["epi=1", "epi=0", "narrow"])
def test_scan_records_over_nonfinite_rows_and_queries(world, layout, epi):
    """Every record of a 64-query cosine search over shard A, read before any repair (poison_bins), against the helper's matrix with
    the bound the tail uses (tests/test_gpu_bin_records._fp16_beta: option eps_cosine), all 64 queries.  Two rows of that matrix
    are not what a scan can bound, and say so here.  The zero query: its prepared vector is zero, every finite row scans as 0 and
    every non-finite row as the clamp value, while the rule gives those rows 0.0 too -- the tail never looks at a record of such a
    query (rq_final_body answers it first), so its records are checked against 0.0 on the finite rows and -inf on the others.  The
    fp32-subnormal query, below RQ_TINY_QUERY_NORM: the scan scores the cosine, the definition's 1e-30 makes the score ~1e-9 of it,
    and the certificate refuses such a query by rule; what must survive are the upper bounds (I1, I2, I6, I7), not the tightness."""
    import torch
    dim = LAYOUTS[layout][0]
    idx, q = world.idx(layout), world.q(dim)[:64]
    with _Options(idx, poison_bins=1, epi=epi):
        c = _Dev(q, 10).run(idx, COS)
        torch.cuda.synchronize()
        rec = idx.debug_bin_records(0, 64)
        beta = idx.get_option("eps_cosine")
        c.fixup(idx, COS)
        _ok(c.result(), world.gold(dim, COS, 64, 10), f"records call {layout} epi {epi}")
    assert 0 < beta < 2e-3
    f = br.decode(rec)
    assert not np.isnan(f["m1"]).any() and not np.isnan(f["c2val"]).any()
    assert (f["m1"][:, 1] < -1.0 - beta).all(), float(f["m1"][:, 1].max())           # the all-NaN bin, every query
    assert f["p1"][0, 32] == 2050 - 64 * 32 and f["p1"][6, 64] == 4099 - 64 * 64     # the planted matches beside NaN / -inf rows
    full = world.scores(dim, COS)[:64].astype(np.float64)
    assert not full[5].any()
    full[5, ~np.isfinite(world.x(dim).astype(np.float32)).all(axis=1)] = -np.inf          # (docstring: what the scan sees of the zero query)
    sel = [j for j in range(64) if j != 3]
    exact = full[sel]
    rep = br.check_records(rec[sel], exact, N, beta)
    assert not br.failures(rep), "; ".join(br.failures(rep))
    tiny = br.check_records(rec[3:4], full[3:4], N, beta)
    assert all(tiny[name]["ok"] for name in ("I1", "I2", "I6", "I7")), br.failures(tiny)
    finite_q = [i for i, j in enumerate(sel) if j not in NONFINITE_Q and j != 5]
    m1 = f["m1"][sel][finite_q][:, :64].astype(np.float64)
    M = exact[finite_q][:, :64 * 64].reshape(len(finite_q), 64, 64).max(axis=2)          # the 64 whole bins
    live = np.isfinite(M)
    assert float(np.abs(m1[live] - M[live]).max()) <= 1e-4                            # as tight as on finite data


# ---- the append paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 100])
def test_append_paths_round_non_finite_and_overflowing_values_like_the_oracle(dim):
    import torch
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((70, dim)).astype(np.float32)
    x[1, 2] = np.nan
    x[2, 0] = np.inf
    x[3, dim - 1] = -np.inf
    x[4, 1], x[4, 5] = np.inf, -np.inf
    x[5, 3] = np.float32(65519.996)           # the last fp32 below the rounding boundary: stays 65 504
    x[6, 3] = np.float32(65520.0)             # the boundary: rounds to even = infinity
    x[7, 4] = np.float32(-65520.0)
    x[8] *= np.float32(1e38) / np.abs(x[8]).max()
    x[9] = np.float32(1e38)
    x[10] = np.nan
    x[11] = 0
    x[12] *= np.float32(1e-30)
    x[69, dim // 2] = np.nan                  # the last row of a ragged block
    assert x[5, 3] < 65520.0
    for normalize in (False, True):
        with np.errstate(all="ignore"):
            want = orc.prepare_rows_f32(x, normalize)
        for device in (False, True):
            idx = nat.NativeIndex(dim, 0)
            if device:
                d = torch.from_numpy(x).cuda()
                idx.add_f32_device(d, 70, normalize)
            else:
                idx.add_f32(x, normalize)
            got = idx.get_rows_f16(0, 70)
            idx.close()
            what = f"dim {dim} normalize {normalize} device {device}"
            assert np.array_equal(np.isnan(got), np.isnan(want)), what          # NaN by position, not by payload
            ok = ~np.isnan(want)
            assert np.array_equal(got.view(np.uint16)[ok], want.view(np.uint16)[ok]), \
                (what, np.argwhere(ok & (got.view(np.uint16) != want.view(np.uint16)))[:4].tolist())
    with np.errstate(all="ignore"):
        assert np.isposinf(orc.prepare_rows_f32(x[6:7], False)[0, 3]) and orc.prepare_rows_f32(x[5:6], False)[0, 3] == np.float16(65504.0)


# ---- no performance cliff --------------------------------------------------------------------------------------------------------------
def test_nonfinite_rows_cost_finite_queries_no_repair(world):
    """Twin A' = shard A with its non-finite rows zeroed.  For the finite queries, under cosine with eps at its default, the
    queries widened and scanned exactly on A equal those on A': rows that score -inf never hold up a certificate.  The twin is the
    measure (the fp32-subnormal query is repaired on both: below RQ_TINY_QUERY_NORM by rule)."""
    q = world.q(768)[:64]
    fq = q[[j for j in range(64) if j not in NONFINITE_Q]]
    x = world.x(768)
    counts = {}
    for name, rows in (("A", x), ("twin", nfo.twin_a(x))):
        idx = _index(768, 768)
        idx.add_f16(rows)
        for k in (10, 100):
            idx.reset_timing()
            _ok(idx.search(fq, k, COS), nfo.topk(fq, rows, k, COS), f"{name} k {k}")
            t = idx.timing()
            counts[(name, k)] = (t["widened"], t["exact_scans"])
        idx.close()
    print("widened / exact scans:", counts)
    for k in (10, 100):
        assert counts[("A", k)] == counts[("twin", k)], counts
