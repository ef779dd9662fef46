"""The device-resident query route of DenseIndex and HybridRetriever on an MI355X: what a request does when the embedder offers
`embed_device` and the query matrix stays in HBM (`_search_device_rows`, `_score_device_rows`, `_embed_queries` / `_search_embedded` /
`_score_embedded` on a ("device", tensor) pair, `_fuse_batch_device` with the embedder's tensor).

The embedder is tests/device_twin.py: a table (or a seeded function) from text to vector whose host route and device route return the
same numbers (tests/test_device_twin.py), so every answer is compared in its bits with the answer of an index whose embedder has a host
route only -- and, on the dense side, with the fp64 definition (tests/score_bits.py: canonical_topk for the rows, assert_score_bits for
the scores, over the inputs of make_case / make_small).  Nothing here has a tolerance except the one test over a real encoder, which
uses the suite's SCORE_TOL."""
import logging
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native as nat
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_twin as dt  # noqa: E402
import router_scenario as rs  # noqa: E402
import score_bits as sb  # noqa: E402
import score_oracle as so  # noqa: E402
from score_bits import COS, IP, K  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
SCORE_TOL = 1e-6                                                         # tests/test_gpu_parity.py, the real-encoder test only
COMBOS = [(768, COS), (768, IP), (384, COS)]                             # (dim, metric); dim 384 is stored in the narrow layout
TRAIN = [(8, 10), (130, 10), (8, 64), (1, 1), (130, 64), (3, 10)]        # (B, k) of consecutive calls over one reused block


def _texts(B, first=0):
    return [f"q{i}" for i in range(first, first + B)]


def _rows_scores(result):
    """search_batch's tuples -> (scores float32 [B][k], rows int64 [B][k]); every list has the same length here."""
    rows = np.array([[int(d[1:]) for d, _, _ in r] for r in result], dtype=np.int64).reshape(len(result), -1)
    scores = np.array([[s for _, s, _ in r] for r in result], dtype=np.float64).reshape(len(result), -1)
    assert np.array_equal(scores, scores.astype(np.float32).astype(np.float64))          # an fp32 value, carried as a Python float
    assert all(t == f"text {d[1:]}" for r in result for d, _, t in r)
    return scores.astype(np.float32), rows


def _same_arrays(got, want, what):
    (gs, gr), (ws, wr) = got, want
    assert gs.dtype == np.float32 and gr.dtype == np.int64 and gs.shape == ws.shape == gr.shape == wr.shape, what
    assert np.array_equal(gr, wr), (what, np.argwhere(gr != wr)[:4].tolist())
    assert np.array_equal(sb.bits(gs), sb.bits(ws)), (what, np.argwhere(sb.bits(gs) != sb.bits(ws))[:4].tolist())


class World:
    """One layout and metric: the 4 101-row index of make_case and the 130-row index of make_small, each wrapped twice over the SAME
    native index -- by a DenseIndex whose embedder leaves the queries on the device and by one whose embedder has a host route only."""

    def __init__(self, dim, metric):
        self.dim, self.metric = dim, metric
        self.metric_name = "cosine" if metric == COS else "ip"
        self.name = f"dim {dim} {self.metric_name}"
        self.case, self.small = sb.make_case(dim, metric), sb.make_small(dim, metric)
        self.q = np.concatenate([self.case.q, sb.queries(122, dim, metric, seed=66)])      # B = 130: the module's 8 queries first
        self.idx, self.sidx = self._native(self.case.x16), self._native(self.small.x16)
        self.dev, self.host, self.twin, self.htwin = self.pair(self.idx)
        self.sdev, self.shost, self.stwin, _ = self.pair(self.sidx)
        self._canon = {}

    def _native(self, x16):
        idx = nat.NativeIndex(self.dim, 0)
        idx.add_f16(x16)
        assert len(idx) == len(x16) and idx.row_pad == (384 if self.dim <= 384 else 768)
        return idx

    def make_twin(self, **mode):
        return dt.DeviceTwinEmbedder({"q": self.q, "p": self.case.x16}, self.dim, DEVICE, **mode)

    def wrap(self, idx, embedder):
        n = len(idx)
        di = si.DenseIndex.from_native(idx, [f"d{i}" for i in range(n)], [f"text {i}" for i in range(n)], embedder=embedder, metric=self.metric_name)
        for i in range(n):
            di._metas[i] = {"title": f"T{i % 97}"}
        return di

    def pair(self, idx, **mode):
        twin = self.make_twin(**mode)
        htwin = twin.host_twin()
        return self.wrap(idx, twin), self.wrap(idx, htwin), twin, htwin

    def canon(self, k, small=False):
        key = (k, small)
        if key not in self._canon:
            ws, wr, flagged = sb.canonical_topk((self.small if small else self.case).ref, k)
            assert not flagged.any(), f"{self.name}: an undecided pair near the cut at k = {k} (tests/test_score_bits.py keeps the inputs clear of that)"
            ws.setflags(write=False)
            wr.setflags(write=False)
            self._canon[key] = (ws, wr)
        return self._canon[key]

    def check_first8(self, scores, rows, k, what, small=False):
        """The module's queries (the first 8 of every batch) against the definition: canonical rows, score bits."""
        nq = min(8, len(rows))
        ref = (self.small if small else self.case).ref
        _, wr = self.canon(k, small)
        assert np.array_equal(rows[:nq], wr[:nq]), (self.name, what, np.argwhere(rows[:nq] != wr[:nq])[:4].tolist())
        sb.assert_score_bits(scores[:nq], rows[:nq], sb.Ref(*(a[:nq] for a in ref)), f"{self.name}: {what}", sb.CAP)

    def close(self):
        self.idx.close()
        self.sidx.close()


@pytest.fixture(scope="module", params=COMBOS, ids=lambda p: f"dim{p[0]}-{'cos' if p[1] == COS else 'ip'}")
def world(request):
    w = World(*request.param)
    yield w
    w.close()


def _calls(twin):
    return twin.device_calls, twin.host_calls


# ---- the unrestricted search through the string entry points ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64])
def test_search_batch_and_search_rows_batch_equal_the_definition_and_the_host_route(world, k):
    """k = 10: scan + tail; k = 64: the exact rung at this size (72 wanted bins of 65)."""
    w, texts = world, _texts(8)
    d0, h0 = _calls(w.twin)
    got = w.dev.search_batch(texts, k)
    assert _calls(w.twin) == (d0 + 1, h0), "search_batch must embed once, on the device"
    assert len(got) == 8 and all(len(r) == k for r in got)
    gs, gr = _rows_scores(got)
    w.check_first8(gs, gr, k, f"search_batch k = {k}")
    assert got == w.host.search_batch(texts, k)
    rs_, rr = w.dev.search_rows_batch(texts, k)
    assert _calls(w.twin) == (d0 + 2, h0)
    w.check_first8(rs_, rr, k, f"search_rows_batch k = {k}")
    _same_arrays((rs_, rr), w.host.search_rows_batch(texts, k), f"search_rows_batch k = {k}")
    _same_arrays((rs_, rr), (gs, gr), "search_batch against search_rows_batch")
    one = w.dev.search(texts[3], k)                                                      # the single-query wrapper takes the same route
    assert one == got[3] and _calls(w.twin) == (d0 + 3, h0)


def test_top_k_above_the_row_count_returns_the_whole_order_without_padding(world):
    w, texts = world, _texts(8)
    d0, h0 = _calls(w.stwin)
    got = w.sdev.search_batch(texts, top_k=1000)
    assert _calls(w.stwin) == (d0 + 1, h0)
    assert all(len(r) == sb.N_SMALL for r in got)                                        # k = the row count: no (0.0, -1) entry reaches a tuple
    gs, gr = _rows_scores(got)
    w.check_first8(gs, gr, sb.N_SMALL, "130 rows, top_k = 1000", small=True)
    assert (gs < 0).any() and not sb.bits(gs[gr == 9]).any()                             # negative scores; the zero row's +0.0
    assert got == w.shost.search_batch(texts, top_k=1000)
    rs_, rr = w.sdev.search_rows_batch(texts, top_k=1000)
    assert rr.shape == (8, sb.N_SMALL)
    _same_arrays((rs_, rr), (gs, gr), "130 rows: search_rows_batch")
    _same_arrays((rs_, rr), w.shost.search_rows_batch(texts, top_k=1000), "130 rows: the host route")


# ---- one index, one `_dev_out`, a train of calls ------------------------------------------------------------------------------------
def test_a_train_of_calls_over_the_reused_block(world):
    """The block of `_search_device_rows` packs int64 rows, fp32 scores and int32 status for the CURRENT (B, k) into a tensor sized for
    the largest B and the largest k seen: every call slices it anew.  It grows along B and along k separately and is kept by smaller calls."""
    w = world
    dev, host, twin, _ = w.pair(w.idx)                                                  # a DenseIndex of its own: no block yet
    assert "_dev_out" not in dev.__dict__
    seen = []
    for B, k in TRAIN:
        texts = _texts(B)
        d0, h0 = _calls(twin)
        got = dev.search_batch(texts, k)
        assert _calls(twin) == (d0 + 1, h0)
        assert got == host.search_batch(texts, k), (w.name, B, k)
        gs, gr = _rows_scores(got)
        assert gr.shape == (B, k)
        w.check_first8(gs, gr, k, f"train B = {B} k = {k}")
        nb, nk, block, pinned = dev.__dict__["_dev_out"]
        assert block.numel() == pinned.numel() == nb * nk * 3 + nb and nb >= B and nk >= k
        seen.append((nb, nk, block.data_ptr(), pinned.data_ptr()))
    sizes = [s[:2] for s in seen]
    assert sizes == [(8, 10), (130, 10), (130, 64), (130, 64), (130, 64), (130, 64)], sizes      # grown along B, then along k
    assert len({s[2:] for s in seen[2:]}) == 1, "a smaller call reallocated the block"
    assert seen[0][2:] != seen[1][2:] != seen[2][2:]


def test_an_answer_is_not_a_view_of_the_reused_block(world):
    """`search_rows_batch` hands back arrays: the next call over the same block must not rewrite them."""
    w = world
    dev, host, _, _ = w.pair(w.idx)
    first = dev.search_rows_batch(_texts(8), K)
    kept = (first[0].copy(), first[1].copy())
    dev.search_rows_batch(_texts(8, first=8), K)                                         # other queries, same (B, k): the same slice of the block
    _same_arrays(first, kept, "the first answer after a second call")
    _same_arrays(first, host.search_rows_batch(_texts(8), K), "the first answer against the host route")


# ---- the repair branch ----------------------------------------------------------------------------------------------------------------
def _repair_counters(idx):
    t = idx.timing()
    return np.array([t["widened"], t["exact_scans"], int(idx.get_option("repaired_queries"))])


def test_failed_certificates_are_repaired_on_the_device_route(world):
    """eps = 10: no certificate of the scan holds, every query is widened and then scanned exactly.  The device route must notice the
    status words, run rq_search_fixup_device and fetch the block AGAIN: the counters move as the host form moves them."""
    w, texts = world, _texts(8)
    w.idx.set_option("eps", 10)
    try:
        c0 = _repair_counters(w.idx)
        hs, hr = w.idx.search(w.q[:8], K, w.metric)                                      # the host form of the library
        c1 = _repair_counters(w.idx)
        got = w.dev.search_batch(texts, K)
        c2 = _repair_counters(w.idx)
        rows = w.dev.search_rows_batch(texts, K)
        c3 = _repair_counters(w.idx)
    finally:
        w.idx.set_option("eps", -1)
    assert (c1 - c0)[2] > 0 and (c1 - c0)[:2].any(), (c0, c1)                           # the lever works: queries were repaired
    assert np.array_equal(c2 - c1, c1 - c0) and np.array_equal(c3 - c2, c1 - c0), (c0, c1, c2, c3)
    gs, gr = _rows_scores(got)
    w.check_first8(gs, gr, K, "eps = 10: search_batch")
    w.check_first8(hs, hr, K, "eps = 10: the host form")
    _same_arrays((gs, gr), (hs, hr), "eps = 10: device route against the host form")
    _same_arrays(rows, (hs, hr), "eps = 10: search_rows_batch")


# ---- what the embedder hands over: fp16, not contiguous, another stream ----------------------------------------------------------------
@pytest.mark.parametrize("mode", [dict(dtype="float16"), dict(strided=True), dict(dtype="float16", strided=True)],
                         ids=["fp16", "strided", "fp16-strided"])
def test_fp16_and_strided_tensors_answer_as_their_host_twin(world, mode):
    w = world
    dev, host, twin, htwin = w.pair(w.idx, **mode)
    texts = _texts(8) + _texts(3, first=40)
    probe = twin.embed_device(texts)
    assert probe.is_contiguous() != bool(mode.get("strided")) and str(probe.dtype) == ("torch.float16" if "dtype" in mode else "torch.float32")
    d0, h0 = _calls(twin)
    got = dev.search_batch(texts, K)
    assert _calls(twin) == (d0 + 1, h0)
    assert got == host.search_batch(texts, K)
    rows = _rows_scores(got)[1]
    rows[:, 3], rows[:, 5] = -1, len(w.idx) - 1
    scored = dev.score_rows_batch(texts, rows)
    assert _calls(twin) == (d0 + 2, h0)
    assert np.array_equal(sb.bits(scored), sb.bits(host.score_rows_batch(texts, rows)))
    assert not sb.bits(scored[:, 3]).any()
    if "dtype" not in mode:                                                              # the same numbers as the module's: the definition holds
        w.check_first8(*_rows_scores(got), K, "strided twin")
        sb.assert_score_bits(scored[:8], rows[:8], w.case.ref, f"{w.name}: strided twin, score_rows_batch", sb.CAP)


def test_the_route_on_a_side_stream_after_the_default_stream_filled_the_block(world):
    import torch
    w = world
    dev, host, twin, _ = w.pair(w.idx)
    assert dev.search_batch(_texts(130), 64) == host.search_batch(_texts(130), 64)       # the default stream leaves the block full
    rows = np.ascontiguousarray(np.broadcast_to(sb.planted_rows(w.case)[:7], (8, 7)))
    side = torch.cuda.Stream()
    d0, h0 = _calls(twin)
    with torch.cuda.stream(side):
        got = dev.search_batch(_texts(8), K)
        got_rows = dev.search_rows_batch(_texts(8), K)
        scored = dev.score_rows_batch(_texts(8), rows)
    side.synchronize()
    assert _calls(twin) == (d0 + 3, h0)
    assert got == host.search_batch(_texts(8), K)
    gs, gr = _rows_scores(got)
    w.check_first8(gs, gr, K, "side stream")
    _same_arrays(got_rows, (gs, gr), "side stream: search_rows_batch")
    assert np.array_equal(sb.bits(scored), sb.bits(host.score_rows_batch(_texts(8), rows)))
    sb.assert_score_bits(scored, rows, w.case.ref, f"{w.name}: side stream, score_rows_batch", sb.CAP)


# ---- scoring given rows ------------------------------------------------------------------------------------------------------------------
def _row_lists(case, m):
    """[8][m] rows: -1, repeats, row n - 1, row 0, the query's own twin pairs, cancelling rows; m = 100 adds seeded rows."""
    n = len(case.x16)
    out = np.empty((8, m), dtype=np.int64)
    rng = np.random.default_rng(100 + m)
    for b in range(8):
        mine = [r for t in case.twins if t.query == b for r in (t.base, t.twin)]          # two pairs per query
        if m == 1:
            out[b] = [mine[1], n - 1, -1, mine[0], 0, mine[3], int(sb.CANCEL_ROWS[b]), mine[2]][b]
        elif m == 7:
            out[b] = [-1, n - 1, mine[0], mine[1], mine[0], int(sb.CANCEL_ROWS[b]), 0]
        else:
            row = rng.integers(0, n, m)
            row[:4] = mine
            row[4:8] = mine                                                              # repeats
            row[8:40] = sb.CANCEL_ROWS[:32]
            row[40], row[41], row[42], row[99] = -1, n - 1, 0, -1
            out[b] = row
    return out


@pytest.mark.parametrize("m", [1, 7, 100])
def test_score_rows_batch_scores_with_the_embedders_tensor(world, m):
    w, texts = world, _texts(8)
    rows = _row_lists(w.case, m)
    calls = int(w.idx.get_option("score_calls"))
    d0, h0 = _calls(w.twin)
    got = w.dev.score_rows_batch(texts, rows)
    assert _calls(w.twin) == (d0 + 1, h0) and int(w.idx.get_option("score_calls")) == calls + 1
    assert got.dtype == np.float32 and got.shape == (8, m)
    sb.assert_score_bits(got, rows, w.case.ref, f"{w.name}: score_rows_batch m = {m}", sb.CAP)      # (-1 must score +0.0)
    assert (rows == -1).any() and not sb.bits(got[rows == -1]).any()
    assert np.array_equal(sb.bits(got), sb.bits(w.dev.score_vectors(w.twin.embed(texts), rows)))
    assert np.array_equal(sb.bits(got), sb.bits(w.host.score_rows_batch(texts, rows)))
    if m == 7:                                                                            # a repeated row scores the same both times
        assert np.array_equal(sb.bits(got[:, 2]), sb.bits(got[:, 4]))


def test_score_ids_and_the_lists_that_never_reach_the_device(world):
    w = world
    rows = _row_lists(w.case, 7)
    d0, h0 = _calls(w.twin)
    for b in (0, 5):
        ids = [f"d{r}" if r >= 0 else "no such passage" for r in rows[b].tolist()]
        got = w.dev.score_ids(f"q{b}", ids)
        assert isinstance(got, list) and got[0] == 0.0 and got == w.host.score_ids(f"q{b}", ids)
        one = sb.Ref(*(a[b:b + 1] for a in w.case.ref))
        sb.assert_score_bits(np.array([got], dtype=np.float32), rows[b:b + 1], one, f"{w.name}: score_ids query {b}", sb.CAP)
    assert _calls(w.twin) == (d0 + 2, h0)
    calls = int(w.idx.get_option("score_calls"))
    nothing = w.dev.score_rows_batch(_texts(8), np.full((8, 5), -1))
    assert nothing.shape == (8, 5) and nothing.dtype == np.float32 and not sb.bits(nothing).any()
    assert w.dev.score_ids("q1", ["nobody", "nothing"]) == [0.0, 0.0]
    assert int(w.idx.get_option("score_calls")) == calls, "a list of -1 alone reached the device"


# ---- restricted calls keep the host path; the fall-back; the multi-device parent ---------------------------------------------------------
def test_restricted_calls_embed_on_the_host(world):
    w, texts = world, _texts(8)
    third = np.arange(len(w.idx)) % 3 == 0
    allowed = [f"d{i}" for i in np.nonzero(third)[0].tolist()]
    each = [allowed if b % 3 == 0 else (None if b % 3 == 1 else [f"d{i}" for i in range(1, len(w.idx), 2)]) for b in range(8)]
    for kw in (dict(allowed_ids=allowed), dict(allowed_ids_each=each), dict(distinct_by="title"), dict(distinct_by="title", allowed_ids=allowed)):
        d0, h0 = _calls(w.twin)
        got = w.dev.search_batch(texts, K, **kw)
        assert _calls(w.twin) == (d0, h0 + 1), list(kw)
        assert got == w.host.search_batch(texts, K, **kw) and all(len(r) == K for r in got), list(kw)
        _same_arrays(w.dev.search_rows_batch(texts, K, **kw), w.host.search_rows_batch(texts, K, **kw), str(list(kw)))
        assert _calls(w.twin) == (d0, h0 + 2), list(kw)
        if list(kw) == ["allowed_ids"]:
            _, wr, flagged = sb.canonical_topk(w.case.ref, K, third)
            gs, gr = _rows_scores(got)
            assert not flagged.any() and np.array_equal(gr, wr)
            sb.assert_score_bits(gs, gr, w.case.ref, f"{w.name}: allowed_ids", sb.CAP)
        if "distinct_by" in kw:
            assert all(len({int(d[1:]) % 97 for d, _, _ in r}) == K for r in got)         # one passage per title


def _failures(caplog):
    return [r for r in caplog.records if "Device embedding failed" in r.getMessage()]


def test_an_embedder_that_raises_falls_back_to_the_host_path(world, caplog):
    w, texts = world, _texts(8)
    twin = w.make_twin(fail_after=1)
    dev = w.wrap(w.idx, twin)
    rows = _row_lists(w.case, 7)
    with caplog.at_level(logging.ERROR):
        for n, call in enumerate((lambda d: d.search_batch(texts, K), lambda d: d.search_rows_batch(texts, K), lambda d: d.score_rows_batch(texts, rows),
                                  lambda d: d.search(texts[2], K), lambda d: d.score_ids("q4", ["d5", "d4100", "nobody"])), 1):
            got, want = call(dev), call(w.host)
            assert len(_failures(caplog)) == n, "the failure is logged once per call"
            assert (twin.device_calls, twin.device_failures, twin.host_calls) == (0, n, n)
            if isinstance(got, tuple):
                _same_arrays(got, want, "fall-back")
            elif isinstance(got, np.ndarray):
                assert np.array_equal(sb.bits(got), sb.bits(want))
            else:
                assert got == want
    later = w.make_twin(fail_after=2)                                                    # the first call on the device, the second on the host
    dev = w.wrap(w.idx, later)
    assert dev.search_batch(texts, K) == dev.search_batch(texts, K) == w.host.search_batch(texts, K)
    assert (later.device_calls, later.device_failures, later.host_calls) == (1, 1, 1)


def test_multi_device_parent_takes_the_host_form_and_refuses_to_score(world):
    """DenseIndex(devices=[0, 0]): the library's multi-device index takes host buffers only, so the embedder's tensor is brought up
    (`_search_device_rows`' first branch); scoring is refused with the documented error."""
    w, texts = world, _texts(8)
    twin = w.make_twin()
    n = len(w.idx)
    multi = si.DenseIndex(persist_directory="", embedder=twin, devices=[0, 0], metric=w.metric_name, load_persisted=False, auto_persist=False,
                          backend_options={"stripe_rows": 64})
    multi._ensure_index(w.dim)
    try:
        assert int(multi._index.get_option("stripe_rows")) == 64 and len(multi._index.devices) == 2 and not multi._can("device")
        multi._index.add_f16(w.case.x16)                                                 # the same stored rows as the single-device index
        multi._ids = [f"d{i}" for i in range(n)]
        multi._row_of = {d: i for i, d in enumerate(multi._ids)}
        multi._texts = [f"text {i}" for i in range(n)]
        multi._metas = [{} for _ in range(n)]
        for k in (K, 64):
            d0, h0 = _calls(twin)
            got = multi.search_batch(texts, k)
            assert _calls(twin) == (d0 + 1, h0)
            assert got == w.dev.search_batch(texts, k)
            w.check_first8(*_rows_scores(got), k, f"multi-device parent k = {k}")
            _same_arrays(multi.search_rows_batch(texts, k), w.dev.search_rows_batch(texts, k), "multi-device parent: search_rows_batch")
        assert "_dev_out" not in multi.__dict__
        with pytest.raises(nat.RqError, match="single-device"):
            multi.score_rows_batch(texts, _row_lists(w.case, 7))
        with pytest.raises(nat.RqError, match="single-device"):
            multi.score_ids("q0", ["d1"])
    finally:
        multi._index.close()


# =============================================================================================================================================
# hybrid side: the corpus of tests/router_scenario.py, dense vectors a seeded Gaussian per distinct text
# =============================================================================================================================================
HYBRID_DIM = 96
FIVE = (0, 1, 7, 68, 69)                                                 # questions of the per-query checks ("" and unknown words among them)


class Hybrid:
    def __init__(self, path):
        self.docs, self.questions, self.each = rs.corpus()
        self.twin = dt.DeviceTwinEmbedder(dt.seeded_gaussian(HYBRID_DIM), HYBRID_DIM, DEVICE)
        self.htwin = self.twin.host_twin()
        self.ftwin = dt.DeviceTwinEmbedder(dt.seeded_gaussian(HYBRID_DIM), HYBRID_DIM, DEVICE, fail_after=1)
        self.dev = rs.retriever(path / "dev", embedder=self.twin, sparse_backend="gpu")
        self.host = rs.retriever(path / "host", embedder=self.htwin, sparse_backend="gpu")
        self.fail = rs.retriever(path / "fail", embedder=self.ftwin, sparse_backend="gpu")
        for r in (self.dev, self.host, self.fail):
            r.add_documents(self.docs)
        self._want = {}

    def set(self, fusion="host", router="host"):
        for r in (self.dev, self.host, self.fail):
            r.fusion_backend, r.router_backend = fusion, router

    def want(self, fusion, top_k, pool, complete, filtered):
        """The host-twin retriever's answers, computed once per case and shared."""
        key = (fusion, top_k, pool, complete, filtered)
        if key not in self._want:
            self.set(fusion)
            self._want[key] = _answers(self.host, self.questions, top_k, pool, complete, **({"allowed_ids_each": self.each} if filtered else {}))
        return self._want[key]

    def close(self):
        for r in (self.dev, self.host, self.fail):
            r.close()
            r.dense_index._index.close()


def _answers(r, qs, top_k, pool, complete, **filters):
    """ids, texts, bm25, dense and hybrid scores in order; the router columns with their padding."""
    return (rs.answers(r.hybrid_search_batch(qs, top_k=top_k, retrieval_pool_size=pool, complete_scores=complete, **filters)),
            [tuple(t) for t in r.get_scores_for_router_batch(qs, num_passages=top_k, retrieval_pool_size=pool, complete_scores=complete, **filters)])


@pytest.fixture(scope="module")
def hyb(tmp_path_factory):
    h = Hybrid(tmp_path_factory.mktemp("device_queries"))
    yield h
    h.close()


@pytest.mark.parametrize("top_k,pool", [(10, 40), (100, 100), (100, 40), (10, 100)])
@pytest.mark.parametrize("fusion", ["host", "gpu"])
def test_hybrid_batches_with_a_device_embedder_equal_the_host_embedder(hyb, fusion, top_k, pool):
    """Plain, complete_scores, allowed_ids_each and both: every value of both batch calls equals the host-twin retriever's.  Each call
    embeds once -- on the device, except where the code documents the host path (host fusion with per-query filters: `host_only`)."""
    dense = 0
    for complete in (False, True):
        for filtered in (False, True):
            want = hyb.want(fusion, top_k, pool, complete, filtered)
            if fusion == "gpu":                                                           # (both run the device fusion: it must still be the host fusion's answer)
                assert want == hyb.want("host", top_k, pool, complete, filtered), (top_k, pool, complete, filtered)
            hyb.set(fusion)
            filters = {"allowed_ids_each": hyb.each} if filtered else {}
            on_host = fusion == "host" and filtered
            d0, h0 = _calls(hyb.twin)
            got_h = rs.answers(hyb.dev.hybrid_search_batch(hyb.questions, top_k=top_k, retrieval_pool_size=pool, complete_scores=complete, **filters))
            assert _calls(hyb.twin) == ((d0, h0 + 1) if on_host else (d0 + 1, h0)), (fusion, complete, filtered)
            got_r = [tuple(t) for t in hyb.dev.get_scores_for_router_batch(hyb.questions, num_passages=top_k, retrieval_pool_size=pool,
                                                                             complete_scores=complete, **filters)]
            assert _calls(hyb.twin) == ((d0, h0 + 2) if on_host else (d0 + 2, h0)), (fusion, complete, filtered)
            assert got_h == want[0] and sum(len(x) for x in got_h) > 300, (fusion, top_k, pool, complete, filtered)
            assert got_r == want[1], (fusion, top_k, pool, complete, filtered)
            assert all(len(t[0]) == len(t[1]) == len(t[2]) == len(t[3]) == top_k for t in got_r)
            dense += sum(x[3] != 0.0 for res in got_h for x in res)
            if filtered:
                assert got_h[11] == [] and got_r[11][2] == [""] * top_k                   # the empty tenant set: padding only
            if complete:                                                                  # completion changed something: the dense scores are not the pool's alone
                assert got_h != hyb.want(fusion, top_k, pool, False, filtered)[0]
    assert dense > 1000


@pytest.mark.parametrize("fusion", ["host", "gpu"])
def test_per_query_complete_scores_equal_the_batch_entry(hyb, fusion):
    """`_search_embedded` -> `_score_embedded` on ONE ("device", vector): the per-query calls embed once and answer as the batch does."""
    hyb.set(fusion)
    qs = [hyb.questions[i] for i in FIVE]
    batch = _answers(hyb.dev, hyb.questions, 10, 40, True)
    assert batch == hyb.want(fusion, 10, 40, True, False)
    dn = hyb.dev.dense_index._index
    for i, q in zip(FIVE, qs):
        d0, h0 = _calls(hyb.twin)
        scores = int(dn.get_option("score_calls"))
        one =rs.answers([hyb.dev.hybrid_search(q, 10, 40, complete_scores=True)])[0]
        assert _calls(hyb.twin) == (d0 + 1, h0)
        cols = tuple(hyb.dev.get_scores_for_router(q, 10, retrieval_pool_size=40, complete_scores=True))
        assert _calls(hyb.twin) == (d0 + 2, h0)
        assert one == batch[0][i], (fusion, i)
        assert cols == batch[1][i], (fusion, i)
        assert one == rs.answers([hyb.host.hybrid_search(q, 10, 40, complete_scores=True)])[0]
        if i < 68:                                                                        # a question with words: its BM25 pool needed dense scores
            assert int(dn.get_option("score_calls")) == scores + 2, "the missing dense scores were not computed by the index"


@pytest.mark.parametrize("normalize", ["query", "stats"])
def test_route_batch_on_the_device_with_a_device_embedder(hyb, normalize):
    """The same device gate over identical inputs: ids, b, d, the order, and w and h in their bits."""
    hyb.set("gpu", "gpu")
    gate = rs.gate(normalize)
    try:
        for P, pool in ((20, 50), (100, 100)):
            for kw in ({}, {"allowed_ids_each": hyb.each}, {"complete_scores": True}, {"allowed_ids_each": hyb.each, "complete_scores": True}):
                keywords = dict(num_passages=P, retrieval_pool_size=pool, return_weights=True, **kw)
                before = gate.native(0).get_option("rerank_calls")
                want, want_w = hyb.host.route_batch(hyb.questions, gate, 10, **keywords)
                assert gate.native(0).get_option("rerank_calls") == before + 1
                d0, h0 = _calls(hyb.twin)
                got, got_w = hyb.dev.route_batch(hyb.questions, gate, 10, **keywords)
                assert _calls(hyb.twin) == (d0 + 1, h0), (normalize, P, list(kw))
                assert gate.native(0).get_option("rerank_calls") == before + 2                                  # the device branch ran
                assert rs.answers(got) == rs.answers(want) and sum(len(x) for x in got) > 500, (normalize, P, list(kw))
                assert got_w.dtype == np.float64 and np.array_equal(got_w.view(np.uint64), want_w.view(np.uint64)), (normalize, P, list(kw))
                h = np.array([x[4] for res in rs.answers(got) for x in res])
                hw = np.array([x[4] for res in rs.answers(want) for x in res])
                assert np.array_equal(h.view(np.uint64), hw.view(np.uint64))
    finally:
        gate.close()
        hyb.set()


def test_repairs_inside_device_fusion(hyb):
    """eps = 10 on the dense index, pools of 10 (18 wanted bins of 47: the scan route): no certificate holds, `d_status.any()` is true
    and the fixup calls run -- rq_search_fixup_device for the plain batch, rq_search_filtered_each_fixup_device for the filtered one
    (its groups forced onto the scan route).  The answers are those without the lever, and the host-twin retriever's."""
    hyb.set("gpu")
    plain = hyb.want("gpu", 10, 10, True, False)
    filtered = hyb.want("gpu", 10, 10, True, True)
    moved = {}
    for r in (hyb.host, hyb.dev):
        dn = r.dense_index._index
        dn.set_option("eps", 10)
        dn.set_option("filter_route", 2)
        try:
            c0 = (int(dn.get_option("repaired_queries")), int(dn.get_option("filter_repaired")))
            got = _answers(r, hyb.questions, 10, 10, True)
            c1 = (int(dn.get_option("repaired_queries")), int(dn.get_option("filter_repaired")))
            got_f = _answers(r, hyb.questions, 10, 10, True, allowed_ids_each=hyb.each)
            c2 = (int(dn.get_option("repaired_queries")), int(dn.get_option("filter_repaired")))
        finally:
            dn.set_option("eps", -1)
            dn.set_option("filter_route", -1)
        assert got == plain and got_f == filtered
        moved[r is hyb.dev] = (c1[0] - c0[0], c2[1] - c1[1])
        assert c1[0] - c0[0] > 0, (c0, c1)                                                # rq_search_fixup_device repaired queries
        assert c2[1] - c1[1] > 0, (c1, c2)                                                # the per-query-filtered fixup repaired queries
    assert moved[True] == moved[False]


def test_hybrid_calls_fall_back_when_the_embedder_raises(hyb, caplog):
    twin = hyb.ftwin
    n = len(_failures(caplog))
    with caplog.at_level(logging.ERROR):
        for fusion in ("host", "gpu"):
            for complete, filtered in ((False, False), (True, False), (True, True)):
                want = hyb.want(fusion, 10, 40, complete, filtered)
                hyb.set(fusion)
                filters = {"allowed_ids_each": hyb.each} if filtered else {}
                tried = not (fusion == "host" and filtered)                               # (host fusion with filters never asks the device route)
                f0, h0 = twin.device_failures, twin.host_calls
                got = rs.answers(hyb.fail.hybrid_search_batch(hyb.questions, top_k=10, retrieval_pool_size=40, complete_scores=complete, **filters))
                assert got == want[0], (fusion, complete, filtered)
                n += int(tried)
                assert (twin.device_failures, twin.host_calls, twin.device_calls) == (f0 + int(tried), h0 + 1, 0) and len(_failures(caplog)) == n
    hyb.set("gpu", "gpu")
    gate = rs.gate()
    try:
        want = hyb.host.route_batch(hyb.questions, gate, 10, num_passages=20, complete_scores=True)
        assert rs.answers(hyb.fail.route_batch(hyb.questions, gate, 10, num_passages=20, complete_scores=True)) == rs.answers(want)
        assert len(_failures(caplog)) == n + 1
    finally:
        gate.close()
        hyb.set()


# ---- one real encoder -------------------------------------------------------------------------------------------------------------------
def test_nomic_embedder_scores_what_it_searched(tmp_path):
    """NomicBertEmbedder (random weights, 2 layers) leaves 70 question vectors in HBM; the device fusion searches AND completes with
    that tensor, `score_rows_batch` scores with it: every reported dense score is the oracle's score of emb.embed(question) against
    the stored row, within SCORE_TOL (the forward repeats, as tests/test_gpu_parity.py's end-to-end test relies on)."""
    import torch
    from rag_uq_amd.embedders import NomicBertEmbedder
    torch.manual_seed(0)
    emb = NomicBertEmbedder(random_init=True, num_layers=2, device=DEVICE, dtype="float16", batch_size=64)
    rng = np.random.default_rng(31)
    words = [f"w{i}" for i in range(60)]
    passages = [" ".join(rng.choice(words, rng.integers(4, 12))) for _ in range(300)]
    questions = [" ".join(rng.choice(words, rng.integers(1, 6))) for _ in range(70)]
    r = rs.retriever(tmp_path, embedder=emb, sparse_backend="gpu", fusion_backend="gpu")
    try:
        r.add_documents([si.Document(id=f"p{i}", text=t) for i, t in enumerate(passages)])
        dn = r.dense_index
        x16 = dn._index.get_rows_f16(0, 300)
        q = emb.embed(questions)
        assert q.shape == (70, 768) and np.isfinite(q).all()
        calls = int(dn._index.get_option("score_calls"))
        out = r.hybrid_search_batch(questions, top_k=20, retrieval_pool_size=30, complete_scores=True)
        assert int(dn._index.get_option("score_calls")) == calls + 1
        rows = np.full((70, 20), -1, dtype=np.int64)
        got = np.zeros((70, 20), dtype=np.float32)
        for b, res in enumerate(out):
            for j, x in enumerate(res):
                rows[b, j], got[b, j] = int(x.doc_id[1:]), x.dense_score
        assert (rows >= 0).sum() >= 70 * 15
        want = so.pairs(q, x16, rows)
        worst = float(np.abs(got - want).max())
        print(f"hybrid_search_batch over the encoder's tensor: worst |dense - oracle| = {worst:.3g}")
        assert worst <= SCORE_TOL
        scored = dn.score_rows_batch(questions, rows)
        assert int(dn._index.get_option("score_calls")) == calls + 2
        worst = float(np.abs(scored - want).max())
        print(f"score_rows_batch over the encoder's tensor: worst |score - oracle| = {worst:.3g}")
        assert worst <= SCORE_TOL and not sb.bits(scored[rows < 0]).any()
    finally:
        r.close()
        r.dense_index._index.close()
