"""What a stream still defers when a grouped or group-member call arrives (MI355X).  include/rq.h: rq_search_grouped_device,
rq_search_group_members_device and rq_group_fill_device "first complete what `stream` defers (a fused tail, a scanned-ahead pair, a
hint)".  Four interlopers (B = 8, k = 10, groups of eight consecutive rows):
  grouped   rq_search_grouped_device                       members   rq_search_group_members_device, s = 3
  fill      rq_group_fill_device over the oracle's winners  announced rq_search_grouped_device given the very tensor announced as the next batch
are called on a "pipeline" = 2 stream in three states:
  (a) tail     search_device(q0) just enqueued, its fused tail pending, no flush;
  (b) hint     hint(q1), search(q0): the tail pending and q1 prepared ahead; then the interloper, search(q1), flush;
  (c) pair     the same on a shard beyond the cache rule of csrc/rq_plan.h (rows x 1536 B > 208 MiB), where search(q0) has scanned q1 ahead
               as the second half of a 128-query pass: the interloper must complete q0 and discard the half, and search(q1) must scan
               for itself -- scan launches = 2 + what the interloper takes alone, measured on the same index.
The output buffers hold markers before anything is enqueued, the candidate lists are poisoned before every tail ("poison_cand"),
and the host synchronises once, at the end.  Every search_device output has status 0 and equals orc.topk_from_scores (rows exactly,
scores within SCORE_TOL); in (a) a later flush changes nothing; the interloper equals tests/group_oracle.py /
tests/group_members_oracle.py, after its fixup where it flagged a query.

MMR is left out: rq_mmr_select_device and rq_group_collapse_device by design do not complete deferred work ("flush, then select"),
and rq_search_mmr stages on the index's own stream, which a blocking search leaves with nothing deferred."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_members_oracle as gmo  # noqa: E402
import group_oracle as gro  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS = nat.METRIC_COSINE
BI, K, S = 8, 10, 3                       # the interlopers' batch, k and group size
INTERLOPERS = ["grouped", "members", "fill", "announced"]
N_SMALL = 20_000                          # the Infinity Cache holds it: no scanned-ahead pairs
N_PAIRS = 143_360                         # 2 240 bins; x 1536 B = 210 MiB, just over the rule


def _device_corpus(idx, n, seed0, chunk=35_840):
    """Gaussian unit rows generated in HBM chunk by chunk (chunk c seeded seed0 + c), as tests/test_gpu_scan_ahead.py does."""
    import torch
    dev = torch.device("cuda:0")
    idx.reserve(n)
    for c in range((n + chunk - 1) // chunk):
        m = min(chunk, n - c * chunk)
        g = torch.Generator(device=dev); g.manual_seed(seed0 + c)
        x = torch.nn.functional.normalize(torch.randn((m, 768), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        del x


class Shard:
    """One index under the options of the module docstring, two 64-query batches, the interlopers' 8 queries, and the oracle's answers
    (each computed once and left unchanged)."""

    def __init__(self, n, device_corpus):
        import torch
        self.n = n
        self.idx = idx = nat.NativeIndex(768, 0)
        if device_corpus:
            _device_corpus(idx, n, 9100)
            self.x16 = idx.get_rows_f16(0, n)                       # read back once, for the oracle
        else:
            self.x16 = orc.synthetic_corpus(n, 768, seed=9100)
            idx.add_f16(self.x16)
        self.groups = np.arange(n, dtype=np.int64) // 8
        idx.set_groups(self.groups)
        for name, v in (("pipeline", 2), ("scan8", 0), ("poison_cand", 1), ("profile", 1)):
            idx.set_option(name, v)
        q = np.stack([orc.synthetic_queries(64, 768, seed=700 + i) for i in range(3)])
        self.qs = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)      # q0, q1: the searches; q2[:8]: the interlopers'
        self.dqs = [torch.from_numpy(x).cuda() for x in self.qs[:2]]
        self.dqi = torch.from_numpy(np.ascontiguousarray(self.qs[2][:BI])).cuda()
        self.top = [orc.topk_from_scores(orc.exact_scores(self.qs[i], self.x16, COS), K) for i in range(2)]
        self.want = {}
        for name, qi in (("own", self.qs[2][:BI]), ("announced", self.qs[1][:BI])):
            s_all = orc.exact_scores(qi, self.x16, COS)
            self.want[name] = (gro.grouped_from_scores(s_all, self.groups, K), gmo.members_from_scores(s_all, self.groups, K, S))

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def small():
    sh = Shard(N_SMALL, device_corpus=False)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def pairs():
    sh = Shard(N_PAIRS, device_corpus=True)
    yield sh
    sh.close()


@pytest.fixture
def stream():
    import torch
    return torch.cuda.Stream()


class Search:
    """The marked output buffers of one search_device call of 64 queries."""

    def __init__(self, sh, which):
        import torch
        self.sh, self.which = sh, which
        self.sc = torch.full((64, K), -7.0, device="cuda")
        self.rw = torch.full((64, K), -7, device="cuda", dtype=torch.int64)
        self.st = torch.full((64,), 9, device="cuda", dtype=torch.int32)

    def enqueue(self, s):
        self.sh.idx.search_device(self.sh.dqs[self.which], 64, K, COS, self.sc, self.rw, None, self.st, s)

    def bits(self):
        return self.sc.cpu().numpy().tobytes(), self.rw.cpu().numpy().tobytes(), self.st.cpu().numpy().tobytes()

    def check(self, what):
        ws, wr = self.sh.top[self.which]
        st, got_r, got_s = self.st.cpu().numpy(), self.rw.cpu().numpy(), self.sc.cpu().numpy()
        assert not st.any(), f"{what}: search(q{self.which}) status {st.tolist()}"
        assert np.array_equal(got_r, wr), f"{what}: search(q{self.which}) rows differ at {np.argwhere(got_r != wr)[:4].tolist()}"
        err = float(np.abs(got_s.astype(np.float64) - ws.astype(np.float64)).max())
        assert err <= SCORE_TOL, f"{what}: search(q{self.which}) scores differ by {err}"


class Interloper:
    """The marked output buffers of one interloper, its call and its check."""

    def __init__(self, sh, kind):
        import torch
        self.sh, self.kind = sh, kind
        self.dq = sh.dqs[1] if kind == "announced" else sh.dqi           # "announced": the pointer the hint named, B = 8 of its 64 queries
        self.grouped_want, self.members_want = sh.want["announced" if kind == "announced" else "own"]
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        self.st = full((BI,), 7, torch.int32)
        self.g = full((BI, K), 7, torch.int32)
        if kind in ("grouped", "announced"):
            self.s, self.r, self.k = full((BI, K), 7.0, torch.float32), full((BI, K), 7, torch.int64), full((BI, K), 7, torch.int64)
        else:
            self.s, self.r, self.c = full((BI, K, S), 7.0, torch.float32), full((BI, K, S), 7, torch.int64), full((BI, K), 7, torch.int32)
        if kind == "fill":
            self.wr = torch.from_numpy(self.grouped_want[1]).cuda()
            self.g = torch.from_numpy(self.grouped_want[2]).cuda()

    def enqueue(self, s):
        idx = self.sh.idx
        if self.kind in ("grouped", "announced"):
            idx.search_grouped_device(self.dq, BI, K, COS, self.s, self.r, self.g, self.k, self.st, s)
        elif self.kind == "members":
            idx.search_group_members_device(self.dq, BI, K, S, COS, self.s, self.r, self.g, self.c, self.st, s)
        else:
            idx.group_fill_device(self.dq, BI, K, S, COS, self.wr, self.g, self.s, self.r, self.c, self.st, s)

    def check(self, s, what):
        """After the synchronise: the fixup for what the call flagged, then the oracle."""
        import torch
        idx = self.sh.idx
        flagged = int(np.count_nonzero(self.st.cpu().numpy()))
        if self.kind in ("grouped", "announced"):
            assert idx.search_grouped_fixup_device(self.dq, BI, K, COS, self.s, self.r, self.g, self.k, self.st, s) == flagged, what
        elif self.kind == "members":
            assert idx.search_group_members_fixup_device(self.dq, BI, K, S, COS, self.s, self.r, self.g, self.c, self.st, s) == flagged, what
        else:
            assert flagged == 0, f"{what}: the fill flagged a query"
        torch.cuda.synchronize()
        assert not self.st.cpu().numpy().any(), what
        gs, gr, gg = self.s.cpu().numpy(), self.r.cpu().numpy(), self.g.cpu().numpy()
        ws, wr, wg = self.grouped_want if self.kind in ("grouped", "announced") else self.members_want[:3]
        assert np.array_equal(gr, wr), f"{what}: the interloper's rows differ at {np.argwhere(gr != wr)[:4].tolist()}"
        assert np.array_equal(gg, wg), f"{what}: the interloper's group ids differ"
        err = float(np.abs(gs.astype(np.float64) - ws.astype(np.float64)).max())
        assert err <= SCORE_TOL, f"{what}: the interloper's scores differ by {err}"
        if self.kind in ("members", "fill"):
            assert np.array_equal(self.c.cpu().numpy(), self.members_want[3]), f"{what}: counts"
            assert (gr >= 0).all() and (self.members_want[3] == S).all()   # (groups of eight: every slot is full)


def run(sh, s, state, kind):
    """One sequence on stream s.  state: "tail" | "hint" | "pair" (the last two differ in the shard only); kind: an interloper or None
    (the control sequence).  Returns (scan launches, hints used)."""
    import torch
    idx = sh.idx
    a = Search(sh, 0)
    b = Search(sh, 1) if state != "tail" else None
    il = Interloper(sh, kind) if kind else None
    torch.cuda.synchronize()                                               # the markers are in place before anything is enqueued
    idx.reset_timing()
    used0 = int(idx.get_option("hints_used"))
    if b:
        idx.search_hint_next_device(sh.dqs[1], 64, s)
    a.enqueue(s)
    if il:
        il.enqueue(s)
    if b:
        b.enqueue(s)
        idx.search_flush_device(s)
    torch.cuda.synchronize()                                               # the only synchronisation of the sequence
    launches, hints = int(idx.timing()["scan_launches"]), int(idx.get_option("hints_used")) - used0
    what = f"{sh.n} rows, state {state}, interloper {kind}"
    a.check(what)
    if b:
        b.check(what)
    if state == "tail":
        before = a.bits()
        idx.search_flush_device(s)
        torch.cuda.synchronize()
        assert a.bits() == before, f"{what}: a later flush changed search(q0)'s outputs"
    if il:
        il.check(s, what)
    return launches, hints


def alone(sh, s, kind):
    """Scan launches the interloper takes on the idle stream."""
    import torch
    il = Interloper(sh, kind)
    torch.cuda.synchronize()
    sh.idx.reset_timing()
    il.enqueue(s)
    torch.cuda.synchronize()
    launches = int(sh.idx.timing()["scan_launches"])
    il.check(s, f"{sh.n} rows, interloper {kind} alone")
    return launches


@pytest.mark.parametrize("kind", INTERLOPERS)
def test_an_interloper_completes_a_pending_fused_tail(small, stream, kind):
    import torch
    s = stream.cuda_stream
    try:
        # the control: without an interloper the tail stays pending -- the outputs still hold their markers once the stream is idle
        a = Search(small, 0)
        torch.cuda.synchronize()
        a.enqueue(s)
        torch.cuda.synchronize()
        assert (a.st.cpu().numpy() == 9).all() and (a.rw.cpu().numpy() == -7).all(), "the control sequence left no tail pending"
        small.idx.search_flush_device(s)
        torch.cuda.synchronize()
        a.check("the control sequence")
        run(small, s, "tail", kind)
    finally:
        small.idx.stream_release(s)


@pytest.mark.parametrize("kind", INTERLOPERS)
def test_an_interloper_between_a_hinted_search_and_the_announced_batch(small, stream, kind):
    s = stream.cuda_stream
    try:
        assert run(small, s, "hint", None) == (2, 1), "the control sequence: one launch per call, the announced batch prepared ahead"
        launches, _ = run(small, s, "hint", kind)
        assert launches == 2 + alone(small, s, kind)
    finally:
        small.idx.stream_release(s)


@pytest.mark.parametrize("kind", INTERLOPERS)
def test_an_interloper_behind_half_a_scanned_ahead_pair(pairs, stream, kind):
    s = stream.cuda_stream
    assert pairs.n * 1536 > 208 << 20 and int(pairs.idx.get_option("scan_ahead")) == 1
    try:
        assert run(pairs, s, "pair", None) == (1, 1), "the control sequence did not run as one scanned-ahead pair"
        launches, _ = run(pairs, s, "pair", kind)
        own = alone(pairs, s, kind)
        print(f"interloper {kind}: {launches} scan launches in the sequence, {own} alone")
        assert launches == 2 + own, f"interloper {kind}: {launches} scan launches, alone {own}"
    finally:
        pairs.idx.stream_release(s)
