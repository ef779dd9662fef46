"""Option "scan_bundle" (csrc/rq_bundle_plan.h, csrc/rq_search.hip): once a hinted pipeline = 2 loop over the fp16 rows
has completed three matched pairs back to back, four consecutive 64-query calls of its stream are scanned by ONE 256-query pass
and finished by ONE tail launch.  Every query of every call of every scenario is compared with oracle.dense_oracle (rows
identical, |score difference| <= 1e-6 -- the bound of tests/test_gpu_scan_ahead.py --, status 0) with candidate lists and bin
records poisoned (poison_cand, poison_bins); the counters say what was bundled: timing()["scan_launches"] (one event pair per
corpus pass), "hints_used", "bundles4" (256-query passes of bundles).

ONE module-scoped shard of 150 017 rows (just beyond the 208 MiB rule, a ragged last quad, about 2.3 quads per workgroup) and 14
cached query batches serve every scenario; the append scenario, which grows the shard by 128 rows, runs last.  No scenario of
the list in the issue is left out or skipped.

Every output buffer, d_status included, lies between guard words (tests/guarded.py): a member's outputs are written by the tail launch
of a LATER call, "each with its own k and outputs", and that launch must write every slot of them and nothing around them."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bin_records as gbr  # noqa: E402  (the record checks and their bound are imported, not copied)
from guarded import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
N_ROWS = 150_017
NQ = 14
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP


class Shard:
    def __init__(self):
        import torch
        self.dev = torch.device("cuda:0")
        self.idx = nat.NativeIndex(768, 0)
        self.idx.reserve(N_ROWS + 4096)                   # (the append scenario does not reallocate)
        chunk = 125_000
        for c in range((N_ROWS + chunk - 1) // chunk):    # rows generated in HBM, as tests/test_gpu_scan_ahead.py does
            m = min(chunk, N_ROWS - c * chunk)
            g = torch.Generator(device=self.dev); g.manual_seed(4711 + c)
            x = torch.nn.functional.normalize(torch.randn((m, 768), device=self.dev, generator=g), dim=1).half().contiguous()
            self.idx.add_f16_device(x, m)
            del x
        self.x16 = self.idx.get_rows_f16(0, N_ROWS)
        assert N_ROWS * 1536 > (208 << 20)
        q = np.stack([orc.synthetic_queries(64, 768, seed=900 + i) for i in range(NQ)])
        self.qs = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)
        self.dqs = [torch.from_numpy(x).to(self.dev) for x in self.qs]
        self.scores = {}      # metric -> [NQ * 64][rows] exact scores, computed once
        self.topk = {}
        for name, v in dict(pipeline=2, scan8=0, poison_cand=1, poison_bins=1, profile=1).items():
            self.idx.set_option(name, v)
        assert int(self.idx.get_option("scan_ahead")) == 1

    def exact(self, qi, metric):
        if metric not in self.scores:
            self.scores[metric] = orc.exact_scores(self.qs.reshape(NQ * 64, 768), self.x16, metric)
        return self.scores[metric][64 * qi:64 * qi + 64]

    def oracle(self, qi, B, k, metric, n):
        """Top k of batch qi's first B queries over the first n rows of the shard."""
        key = (qi, B, k, metric, n)
        if key not in self.topk:
            self.topk[key] = orc.topk_from_scores(self.exact(qi, metric)[:B, :n], k)
        return self.topk[key]

    def append_rows(self, rows16):
        """Rows appended to the index and to the oracle's copy and score matrices."""
        import torch
        self.idx.add_f16_device(torch.from_numpy(rows16).to(self.dev), len(rows16))
        for metric in list(self.scores):
            extra = orc.exact_scores(self.qs.reshape(NQ * 64, 768), rows16, metric)
            self.scores[metric] = np.concatenate([self.scores[metric], extra], axis=1)
        self.x16 = np.concatenate([self.x16, rows16])

    def counters(self):
        idx = self.idx
        return (int(idx.timing()["scan_launches"]), int(idx.get_option("hints_used")), int(idx.get_option("bundles4")))

    def bufs(self, B, k):
        """(scores, rows, status) of one call, each between guard words"""
        import torch
        return guarded((B, k), torch.float32, self.dev), guarded((B, k), torch.int64, self.dev), guarded((B,), torch.int32, self.dev)

    def run(self, ops):
        """ops: ("hint", qi or None, B, stream) | ("search", qi, B, k, metric, stream) | ("flush", stream) | ("release", stream) |
        ("call", f): f() runs there (another route, an append).  Returns (scan launches, hints used, 256-query bundle passes) of the
        sequence; every search is checked against the oracle over the rows the index held when it was made."""
        import torch
        idx = self.idx
        bufs = [self.bufs(op[2], op[3]) for op in ops if op[0] == "search"]
        torch.cuda.synchronize()
        idx.reset_timing()
        _, used0, b40 = self.counters()
        outs = []
        for op in ops:
            if op[0] == "hint":
                idx.search_hint_next_device(None if op[1] is None else self.dqs[op[1]], op[2], op[3])
            elif op[0] == "search":
                _, qi, B, k, metric, s = op
                sc, rw, st = bufs[len(outs)]
                idx.search_device(self.dqs[qi], B, k, metric, sc, rw, None, st, s)
                outs.append((op, len(idx), sc, rw, st))
            elif op[0] == "flush":
                idx.search_flush_device(op[1])
            elif op[0] == "release":
                idx.stream_release(op[1])
            else:
                op[1]()
        torch.cuda.synchronize()
        self.check(outs)
        launches, used, b4 = self.counters()
        return launches, used - used0, b4 - b40

    def check(self, outs):
        for (_, qi, B, k, metric, s), n, sc, rw, st in outs:
            es, er = self.oracle(qi, B, k, metric, n)
            where = f"q{qi} B={B} k={k} metric={metric} rows={n}"
            for name, g in (("scores", sc), ("rows", rw), ("status", st)):
                g.check(f"{where}: {name}")
            assert int(st.view.abs().sum()) == 0, f"{where}: status {st.cpu().tolist()}"
            got_r, got_s = rw.numpy(), sc.numpy()
            assert np.array_equal(got_r, er), f"{where}: rows differ at {np.argwhere(got_r != er)[:4].tolist()}"
            assert float(np.abs(got_s - es).max()) <= SCORE_TOL, where


def _loop(qis, s, B=64, k=10, metric=COS, Bs=None, ks=None, flush=True):
    """A loop as bench.py runs it: before each call the stream's next batch is announced; the last call announces nothing."""
    Bs = Bs or {}
    ks = ks or {}
    ops = []
    for j, qi in enumerate(qis):
        if j + 1 < len(qis):
            ops.append(("hint", qis[j + 1], Bs.get(j + 1, B), s))
        ops.append(("search", qi, Bs.get(j, B), ks.get(j, k), metric, s))
    if flush:
        ops.append(("flush", s))
    return ops


def _formula(n):
    """(scan launches, hints used, 256-query passes) of a hinted loop of n calls that ends in a flush."""
    if n < 6:
        return (n + 1) // 2, n - 1, 0
    rest = n - 6
    return 3 + (rest + 3) // 4, n - 1, rest // 4 + (rest % 4 == 3)


@pytest.fixture(scope="module")
def shard():
    sh = Shard()
    yield sh
    sh.idx.close()


@pytest.fixture
def stream(shard):
    import torch
    st = torch.cuda.Stream(device=shard.dev)
    yield st.cuda_stream
    shard.idx.stream_release(st.cuda_stream)


WARM = list(range(6))          # six hinted calls = three matched pairs: the next call may open a bundle of four


@pytest.mark.parametrize("n", range(6, 15))
def test_hinted_loops_follow_the_launch_formula(shard, stream, n):
    assert shard.run(_loop(list(range(n)), stream)) == _formula(n)


@pytest.mark.parametrize("n", range(6, 15))
def test_scan_bundle_2_keeps_pairs(shard, stream, n):
    shard.idx.set_option("scan_bundle", 2)
    try:
        assert int(shard.idx.get_option("scan_bundle")) == 2
        assert shard.run(_loop(list(range(n)), stream)) == ((n + 1) // 2, n - 1, 0)
    finally:
        shard.idx.set_option("scan_bundle", 4)
    with pytest.raises(nat.RqError):
        shard.idx.set_option("scan_bundle", 3)
    assert int(shard.idx.get_option("scan_bundle")) == 4


@pytest.mark.parametrize("kind", ["pointer", "B", "metric"])
@pytest.mark.parametrize("pos", [1, 2, 3])
def test_mismatch_at_each_position(shard, stream, pos, kind):
    """Members 6 .. 6 + pos - 1 of a bundle are waiting (pos = 3: scanned, with batch 9 ahead) when a call brings another pointer,
    another B or the other metric than announced; it announces batch 13 itself, which then comes."""
    s = stream
    ops = _loop(WARM + [6, 7, 8, 9][:pos], s, flush=False)
    nxt = 6 + pos
    ops.insert(-1, ("hint", nxt, 64, s))                                  # the last member announces batch nxt ...
    ops.append(("hint", 13, 64, s))
    ops.append({"pointer": ("search", 12, 64, 10, COS, s), "B": ("search", nxt, 40, 10, COS, s), "metric": ("search", nxt, 64, 10, IP, s)}[kind])
    ops += [("search", 13, 64, 10, COS if kind != "metric" else IP, s), ("flush", s)]
    launches, _, b4 = shard.run(ops)
    # three pairs, ONE pass over the members that had come (64 / 128 / 256 queries), one pair pass of the mismatching call and batch 13
    assert (launches, b4) == (5, 1 if pos == 3 else 0)


def test_members_with_their_own_k(shard, stream):
    assert shard.run(_loop(list(range(10)), stream, ks={6: 1, 7: 10, 8: 50, 9: 100})) == (4, 9, 1)


def test_members_with_their_own_B_and_k(shard, stream):
    """B = (64, 1, 64, 17) with k = (1, 128, 10, 3) behind the three warm pairs: only the LAST member of a bundle may be ragged, so the
    one-query call in the second place keeps the loop with pairs -- (6, 7 [1]) and (8, 9 [17]): a 128-query pass whose second half holds
    one real query, then one with 17 --, as test_ragged_middle_member_keeps_pairs has it for B = 40.  Each tail writes [B][k] of its own
    call and nothing else: the guards of every buffer hold."""
    assert shard.run(_loop(list(range(10)), stream, Bs={7: 1, 9: 17}, ks={6: 1, 7: 128, 8: 10, 9: 3})) == (5, 9, 0)


def test_ragged_last_member(shard, stream):
    assert shard.run(_loop(list(range(10)), stream, Bs={9: 37})) == (4, 9, 1)


def test_ragged_middle_member_keeps_pairs(shard, stream):
    """Only the last member may be ragged.  B = 40 in the second place: the bundle does not open, the loop stays with pairs (7, 8
    [40]) and (9, 10)... five launches, no 256-query pass.  In the third place: the bundle closes with three members."""
    assert shard.run(_loop(list(range(10)), stream, Bs={7: 40})) == (5, 9, 0)
    assert shard.run(_loop(list(range(10)), stream, Bs={8: 40})) == (5, 9, 1)


def test_inner_product_loop(shard, stream):
    assert shard.run(_loop(list(range(10)), stream, metric=IP)) == _formula(10)


@pytest.mark.parametrize("pos", [1, 2, 3, 4])
def test_flush_at_each_position(shard, stream, pos):
    s = stream
    ops = _loop(WARM + [6, 7, 8, 9][:pos], s, flush=False)
    if pos < 4:
        ops.insert(-1, ("hint", 6 + pos, 64, s))                          # (the bundle is still open when the flush comes)
    ops += [("flush", s)] + _loop([10, 11], s)
    launches, _, b4 = shard.run(ops)
    assert (launches, b4) == (5, 1 if pos >= 3 else 0)


def test_stream_release_with_an_open_bundle(shard):
    import torch
    st = torch.cuda.Stream(device=shard.dev)
    s = st.cuda_stream
    ops = _loop(WARM + [6, 7], s, flush=False)
    ops.insert(-1, ("hint", 8, 64, s))
    assert shard.run(ops + [("release", s)]) == (4, 7, 0)


def test_other_routes_on_the_stream_with_an_open_bundle(shard, stream):
    """One filtered call and one range call arrive while two members are gathered: the members are scanned and finished first."""
    import torch
    s, idx, dev = stream, shard.idx, shard.dev
    allowed = 1000
    mask = np.zeros(len(idx), dtype=bool); mask[:allowed] = True
    flt = idx.make_filter(mask)
    f_out = (torch.empty((64, 10), device=dev), torch.empty((64, 10), device=dev, dtype=torch.int64), torch.full((64,), 9, device=dev, dtype=torch.int32))
    thr, cap = 0.12, 256
    d_thr = torch.full((64,), thr, device=dev)
    r_out = (torch.empty((64, cap), device=dev), torch.empty((64, cap), device=dev, dtype=torch.int64), torch.zeros((64,), device=dev, dtype=torch.int64),
             torch.full((64,), 9, device=dev, dtype=torch.int32))

    def filtered():
        idx.search_device(shard.dqs[12], 64, 10, COS, f_out[0], f_out[1], None, f_out[2], s, row_filter=flt)

    def ranged():
        idx.search_range_device(shard.dqs[13], 64, d_thr, cap, COS, r_out[0], r_out[1], None, r_out[2], r_out[3], s)
        idx.search_range_fixup_device(shard.dqs[13], 64, d_thr, cap, COS, r_out[0], r_out[1], None, r_out[2], r_out[3], s)

    try:
        for other in (filtered, ranged):
            ops = _loop(WARM + [6, 7], s, flush=False)
            ops.insert(-1, ("hint", 8, 64, s))
            ops += [("call", other)] + _loop([8, 9], s)
            _, _, b4 = shard.run(ops)
            assert b4 == 0
        n = len(idx)
        assert int(f_out[2].abs().sum()) == 0
        es, er = orc.topk_from_scores(shard.exact(12, COS)[:, :allowed], 10)
        assert np.array_equal(f_out[1].cpu().numpy(), er) and float(np.abs(f_out[0].cpu().numpy() - es).max()) <= SCORE_TOL
        assert int(r_out[3].abs().sum()) == 0
        e13 = shard.exact(13, COS)[:, :n].astype(np.float64)
        count = r_out[2].cpu().numpy()
        assert ((e13 >= thr + 1e-6).sum(1) <= count).all() and (count <= (e13 >= thr - 1e-6).sum(1)).all()
    finally:
        flt.close()


def test_two_streams_alternating(shard):
    import torch
    sts = [torch.cuda.Stream(device=shard.dev) for _ in range(2)]
    ss = [st.cuda_stream for st in sts]
    ops = []
    for i in range(20):
        if i + 2 < 20:
            ops.append(("hint", (i + 2) % NQ, 64, ss[i % 2]))
        ops.append(("search", i % NQ, 64, 10, COS, ss[i % 2]))
    ops += [("flush", ss[0]), ("flush", ss[1])]
    try:
        one = _formula(10)
        assert shard.run(ops) == (2 * one[0], 2 * one[1], 2 * one[2])
    finally:
        for s in ss:
            shard.idx.stream_release(s)


def test_train_of_14_batches(shard, stream):
    import torch
    idx, k = shard.idx, 10
    outs = [shard.bufs(64, k) for _ in range(NQ)]
    train = idx.make_train(shard.dqs, [o[0] for o in outs], [o[1] for o in outs], None, [o[2] for o in outs], [stream])
    torch.cuda.synchronize()
    idx.reset_timing()
    _, used0, b40 = shard.counters()
    idx.search_train_device(train, 64, k, COS)
    idx.search_flush_device(stream)
    torch.cuda.synchronize()
    launches, used, b4 = shard.counters()
    assert (launches, used - used0, b4 - b40) == (5, 13, 2)
    shard.check([(("search", qi, 64, k, COS, stream), len(idx), sc, rw, st) for qi, (sc, rw, st) in enumerate(outs)])


class _Records:
    """What test_gpu_bin_records._check asks of a shard: its rows, no planted positions, the exact scores of a query range."""

    def __init__(self, shard):
        self.sh, self.n, self.pins = shard, len(shard.idx), {}

    def exact(self, metric, q0, B):
        return self.sh.exact(q0 // 64, metric)[:B, :self.n].astype(np.float64)


def test_bin_records_of_all_256_slots_after_the_pass(shard, stream):
    import torch
    s, idx = stream, shard.idx
    ops = _loop(WARM + [6, 7, 8], s, flush=False)
    ops.insert(-1, ("hint", 9, 64, s))                    # member 2 announces batch 9: its call launches the 256-query pass
    outs = []

    def records():
        torch.cuda.synchronize()
        outs.append(gbr._records(idx, 256, s))

    launches, _, b4 = shard.run(ops + [("call", records), ("search", 9, 64, 10, COS, s), ("flush", s)])
    assert (launches, b4) == (4, 1)
    rec = outs[0]
    beta = gbr._fp16_beta(idx, COS)
    for j in range(4):
        gbr._check(_Records(shard), rec[64 * j:64 * j + 64], COS, 64 * (6 + j), 64, beta, what=f"bundle quarter {j}")


def test_rows_appended_while_two_members_are_gathered(shard, stream):
    """(Last: it grows the shard.)  The appended rows are fp16 copies of the gathered members' queries and would rank first: the
    gathered calls return the oracle over the OLD rows, a call made after the append sees the new ones."""
    s = stream
    n0 = len(shard.idx)
    new = np.concatenate([shard.qs[6], shard.qs[7]]).astype(np.float16)
    ops = _loop(WARM + [6, 7], s, flush=False)
    ops.insert(-1, ("hint", 8, 64, s))
    ops += [("call", lambda: shard.append_rows(new)), ("search", 6, 64, 10, COS, s), ("flush", s)]
    shard.exact(6, COS)
    launches, _, b4 = shard.run(ops)
    assert (launches, b4) == (5, 0) and len(shard.idx) == n0 + 128
    top = shard.oracle(6, 64, 10, COS, n0 + 128)[1][:, 0]
    assert np.array_equal(top, n0 + np.arange(64))        # (the call after the append: every query finds its own copy first)
