"""Option "scan_ahead" (csrc/rq_search.hip run_pipeline): a pipeline = 2 call over the fp16 rows whose stream has announced its next
batch (rq_search_hint_next_device) scans both batches in ONE 128-query pass; the next call, if it brings exactly the announced
batch and metric, enqueues no scan and only runs the two tails.  Every query of every call is compared with the oracle (rows
identical, |score difference| <= 1e-6, status 0) with the candidate lists poisoned before every tail (poison_cand), and the
counters say which calls were paired: one scan launch per matched pair, hints_used = calls whose announcement was acted on.

Every output buffer, d_status included, lies between guard words (tests/guarded.py): a call's outputs are written by a LATER launch
here, and that launch must write every slot of them and nothing in front of or behind them."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
NQ = 10          # query batches q0..q9 of 64 unit-norm queries, shared by every scenario


def _device_corpus(idx, n, seed0, chunk=125_000):
    """Gaussian unit rows generated in HBM chunk by chunk (chunk c seeded seed0 + c), as bench.py does."""
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
    def __init__(self, n, device_corpus=True):
        import torch
        self.dev = torch.device("cuda:0")
        self.idx = nat.NativeIndex(768, 0)
        if device_corpus:
            _device_corpus(self.idx, n, 4711)
        else:
            self.idx.add_f16(orc.synthetic_corpus(n, 768, seed=4711))
        self.n = n
        self.x16 = self.idx.get_rows_f16(0, n)
        q = np.stack([orc.synthetic_queries(64, 768, seed=900 + i) for i in range(NQ)])
        self.qs = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)
        self.dqs = [torch.from_numpy(x).to(self.dev) for x in self.qs]
        self.exact = {}
        self.idx.set_option("pipeline", 2)
        self.idx.set_option("poison_cand", 1)
        self.idx.set_option("scan8", 0)
        self.idx.set_option("profile", 1)        # one event pair per scan launch: timing()["scan_launches"] counts them

    def oracle(self, qi, B, k, metric):
        if (qi, metric) not in self.exact:
            self.exact[(qi, metric)] = orc.exact_scores(self.qs[qi], self.x16, metric)
        return orc.topk_from_scores(self.exact[(qi, metric)][:B], k)

    def bufs(self, B, k):
        """(scores, rows, status) of one call, each between guard words"""
        import torch
        return guarded((B, k), torch.float32, self.dev), guarded((B, k), torch.int64, self.dev), guarded((B,), torch.int32, self.dev)

    def check(self, qi, B, k, metric, sc, rw, st):
        es, er = self.oracle(qi, B, k, metric)
        where = f"q{qi} B={B} k={k} metric={metric}"
        for name, g in (("scores", sc), ("rows", rw), ("status", st)):
            g.check(f"{where}: {name}")
        assert int(st.view.abs().sum()) == 0, f"{where}: status {st.cpu().tolist()}"
        got_r, got_s = rw.numpy(), sc.numpy()
        assert np.array_equal(got_r, er), f"{where}: rows differ at {np.argwhere(got_r != er)[:4].tolist()}"
        assert float(np.abs(got_s - es).max()) <= SCORE_TOL, where

    def run(self, ops):
        """ops: ("hint", qi or None, B, stream) | ("search", qi, B, k, metric, stream) | ("flush", stream) | ("release", stream).
        Returns (scan launches, hints used) of the sequence; every search is checked against the oracle."""
        import torch
        idx = self.idx
        # output buffers between guard words, filled with the sentinel on torch's stream BEFORE any search is enqueued on the callers' streams
        bufs = [self.bufs(op[2], op[3]) for op in ops if op[0] == "search"]
        torch.cuda.synchronize()
        idx.reset_timing()
        used0 = int(idx.get_option("hints_used"))
        outs = []
        for op in ops:
            if op[0] == "hint":
                idx.search_hint_next_device(None if op[1] is None else self.dqs[op[1]], op[2], op[3])
            elif op[0] == "search":
                _, qi, B, k, metric, s = op
                sc, rw, st = bufs[len(outs)]
                idx.search_device(self.dqs[qi], B, k, metric, sc, rw, None, st, s)
                outs.append((op, sc, rw, st))
            elif op[0] == "flush":
                idx.search_flush_device(op[1])
            else:
                idx.stream_release(op[1])
        torch.cuda.synchronize()
        for (_, qi, B, k, metric, s), sc, rw, st in outs:
            self.check(qi, B, k, metric, sc, rw, st)
        return int(idx.timing()["scan_launches"]), int(idx.get_option("hints_used")) - used0

    def close(self):
        self.idx.close()


def _train(qis, B, k, metric, s, announce_last=True):
    """A loop as bench.py runs it: before each call, the stream's next batch is announced."""
    ops = []
    for j, qi in enumerate(qis):
        if j + 1 < len(qis):
            ops.append(("hint", qis[j + 1], B, s))
        ops.append(("search", qi, B, k, metric, s))
    ops.append(("flush", s))
    return ops


@pytest.fixture(scope="module", params=[300_000, 1_000_000], ids=["300k", "1M"])
def shard(request):
    sh = Shard(request.param)
    yield sh
    sh.close()


@pytest.fixture
def stream(shard):
    import torch
    st = torch.cuda.Stream(device=shard.dev)
    yield st.cuda_stream
    shard.idx.stream_release(st.cuda_stream)


def test_matched_pairs_one_launch_per_pair(shard, stream):
    ops = _train(list(range(6)), 64, 10, 0, stream)
    assert shard.run(ops) == (3, 5)                       # pairs (0,1) (2,3) (4,5); calls 1..5 acted on their announcement
    shard.idx.set_option("scan_ahead", 0)
    try:
        assert shard.run(ops) == (6, 5)                   # A/B: one launch per call, every announced batch prepared ahead
    finally:
        shard.idx.set_option("scan_ahead", 1)


def test_second_call_that_does_not_match(shard, stream):
    s = stream
    ops = [("hint", 1, 64, s), ("search", 0, 64, 10, 0, s),          # pair (q0, q1) ...
           ("hint", 2, 64, s), ("search", 1, 64, 100, 0, s),         # ... matched with another k; q2 prepared ahead
           ("hint", 9, 64, s), ("search", 2, 64, 10, 0, s),          # pair (q2, q9) ...
           ("hint", 4, 64, s), ("search", 3, 64, 10, 0, s),          # ... not matched: another pointer; pair (q3, q4)
           ("hint", 5, 64, s), ("search", 4, 40, 10, 0, s),          # not matched: another B; pair (q4 [40], q5)
           ("hint", 6, 37, s), ("search", 5, 64, 10, 1, s),          # not matched: the other metric (q5 prepared); pair (q5, q6 [37])
           ("hint", 7, 64, s), ("search", 6, 37, 10, 1, s),          # matched, ragged
           ("search", 7, 64, 10, 0, s),                              # prepared ahead, nothing announced: one 64-query launch
           ("flush", s)]
    assert shard.run(ops) == (6, 5)


def test_flush_between_the_two_halves(shard, stream):
    s = stream
    ops = [("hint", 1, 64, s), ("search", 0, 64, 10, 0, s), ("flush", s), ("search", 1, 64, 10, 0, s), ("flush", s)]
    assert shard.run(ops) == (2, 1)                       # the scanned-ahead half is discarded; q1's prepared queries are used


def test_odd_number_of_calls(shard, stream):
    ops = _train(list(range(5)), 64, 10, 0, stream)
    ops.insert(-2, ("hint", 5, 64, stream))               # the last call announces a batch that never comes
    assert shard.run(ops) == (3, 4)


def test_two_streams_alternating(shard):
    import torch
    sts = [torch.cuda.Stream(device=shard.dev) for _ in range(2)]
    ss = [st.cuda_stream for st in sts]
    ops = []
    for i in range(8):
        if i + 2 < 8:
            ops.append(("hint", i + 2, 64, ss[i % 2]))
        ops.append(("search", i, 64, 10, 0, ss[i % 2]))
    ops += [("flush", ss[0]), ("flush", ss[1])]
    try:
        assert shard.run(ops) == (4, 6)
    finally:
        for s in ss:
            shard.idx.stream_release(s)


def test_search_train_pairs_per_stream(shard, stream):
    import torch
    idx = shard.idx
    n, k = 6, 10
    outs = [shard.bufs(64, k) for _ in range(n)]
    train = idx.make_train(shard.dqs[:n], [o[0] for o in outs], [o[1] for o in outs], None, [o[2] for o in outs], [stream])
    torch.cuda.synchronize()          # (the status markers are written on torch's stream)
    idx.reset_timing()
    used0 = int(idx.get_option("hints_used"))
    idx.search_train_device(train, 64, k, 0)
    idx.search_flush_device(stream)
    torch.cuda.synchronize()
    assert int(idx.timing()["scan_launches"]) == 3
    assert int(idx.get_option("hints_used")) - used0 == 5
    for qi, (sc, rw, st) in enumerate(outs):
        shard.check(qi, 64, k, 0, sc, rw, st)


def test_stream_release_with_a_half_pending_pair(shard):
    import torch
    st = torch.cuda.Stream(device=shard.dev)
    s = st.cuda_stream
    assert shard.run([("hint", 1, 64, s), ("search", 0, 64, 10, 0, s), ("release", s)]) == (1, 0)


def test_below_the_size_rule_nothing_changes():
    """70k rows (the Infinity Cache holds the shard): every call keeps its own 64-query launch."""
    import torch
    sh = Shard(70_000, device_corpus=False)
    st = torch.cuda.Stream(device=sh.dev)
    try:
        assert int(sh.idx.get_option("scan_ahead")) == 1
        assert sh.run(_train(list(range(6)), 64, 10, 0, st.cuda_stream)) == (6, 5)
    finally:
        sh.idx.stream_release(st.cuda_stream)
        sh.close()
