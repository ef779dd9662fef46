"""Scoring given rows on the MI355X (include/rq.h rq_score_rows_device / rq_score_rows, csrc/rq_score.hip): every
(query, row) pair of a list comes back with its oracle score (tests/score_oracle.py) within 1e-6 -- the SCORE_TOL of the parity
tests -- position for position; absent entries come back 0.0; and the value has the BITS the other routes return for the pair: the
filter's gather route and rq_search's own top k."""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
N_BASE = 4101                      # 65 bins, a ragged last bin
NQ = 70
BATCHES = [1, 3, 64, 70]
LISTS = [1, 7, 64, 65, 100, 1500]  # one position, part of a round, one tile, a tile and one position, two tiles, 24 tiles


class Shape:
    """One index with its rows, NQ queries and their oracle scores per metric (computed once, shared, never changed)."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, row_offset=0, x16=None, q=None):
        self.n, self.dim, self.row_offset = n, dim, row_offset
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed) if x16 is None else x16
        self.q = orc.synthetic_queries(NQ, dim, seed=seed + 1) if q is None else q
        self.idx = nat.NativeIndex(dim, 0)
        self.idx.set_option("scan8", 0)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self._full = {}

    def full(self, metric=COS):
        if metric not in self._full:
            with np.errstate(invalid="ignore", over="ignore"):
                s = orc.exact_scores(self.q, self.x16, metric)
            s.setflags(write=False)
            self._full[metric] = s
        return self._full[metric]

    def want(self, B, rows, metric=COS):
        return so.pairs(self.q[:B], self.x16, rows, metric, self.row_offset, scores=self.full(metric)[:B])

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def wide():
    sh = Shape()
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def narrow():
    sh = Shape(dim=384, seed=21)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def dim33():
    sh = Shape(dim=33, seed=33)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shifted():
    sh = Shape(seed=9, row_offset=10 ** 6)
    yield sh
    sh.close()


def random_lists(sh, B, m, seed):
    """[B][m] global rows, uniformly random: duplicates occur by chance at every m > 1 and are forced at two positions."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, sh.n, size=(B, m)).astype(np.int64) + sh.row_offset
    if m > 1:
        rows[:, m // 2] = rows[:, 0]
        rows[:, m - 1] = rows[:, 0]
    return rows


def close_to(got, want, what=""):
    """Special values (0.0 of an absent entry or a zero row, +-inf) exactly, everything else within SCORE_TOL."""
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(got).any(), f"{what}: NaN scores at {np.argwhere(np.isnan(got))[:4].tolist()}"
    special = ~np.isfinite(want) | (want == 0.0)
    assert np.array_equal(got[special], want[special]), f"{what}: special values differ at {np.argwhere(special & (got != want))[:4].tolist()}"
    err = float(np.abs(got[~special].astype(np.float64) - want[~special].astype(np.float64)).max(initial=0.0))
    print(f"{what}: largest |score - oracle| = {err}")
    assert err <= SCORE_TOL, f"{what}: scores differ by {err}"


def score_device(idx, q, rows, metric=COS, stream=None):
    """One rq_score_rows_device call over host inputs -> scores on the host."""
    import torch
    B, m = rows.shape
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        d_q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        d_r = torch.from_numpy(np.ascontiguousarray(rows, np.int64)).cuda()
        out = torch.full((B, m), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        idx.score_rows_device(d_q, B, d_r, m, metric, out, stream.cuda_stream if stream is not None else 0)
        (stream or torch.cuda.current_stream()).synchronize()
        return out.cpu().numpy()


# ---- 1. random lists against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,metric", [("wide", COS), ("wide", IP), ("narrow", COS), ("narrow", IP), ("dim33", COS), ("dim33", IP),
                                          ("shifted", COS), ("shifted", IP)])
def test_random_lists_with_duplicates_equal_the_oracle(request, shape, metric):
    sh = request.getfixturevalue(shape)
    for B in BATCHES:
        for m in LISTS:
            rows = random_lists(sh, B, m, seed=B * 10007 + m)
            got = sh.idx.score_rows(sh.q[:B], rows, metric)
            close_to(got, sh.want(B, rows, metric), f"{shape} metric {metric} B={B} m={m}")
            assert np.array_equal(got[:, 0].view(np.uint32), got[:, m - 1].view(np.uint32))         # a duplicate has the same bits


@pytest.mark.parametrize("shape", ["wide", "dim33", "shifted"])
def test_device_form_equals_the_host_form_bit_for_bit(request, shape):
    sh = request.getfixturevalue(shape)
    for B, m in ((1, 1), (3, 65), (70, 100), (64, 1500)):
        rows = random_lists(sh, B, m, seed=B + m)
        host = sh.idx.score_rows(sh.q[:B], rows)
        dev = score_device(sh.idx, sh.q[:B], rows)
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (shape, B, m)


# ---- 2. absent entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "shifted"])
def test_absent_entries_score_zero_and_leave_their_neighbours_right(request, shape):
    sh = request.getfixturevalue(shape)
    off, n = sh.row_offset, sh.n
    absent = [-1, off - 1, off + n, off + n + 12345, -(2 ** 62), 2 ** 62]
    for B, m in ((3, 7), (70, 65), (3, 100)):
        rows = random_lists(sh, B, m, seed=m)
        rows[:, 0] = off + n - 1                                       # the last stored row is present
        mask = np.zeros((B, m), dtype=bool)
        for j, a in enumerate(absent):
            pos = (j * 11 + 1) % m
            rows[:, pos] = a
            mask[:, pos] = True
        rows[B - 1, :] = np.resize(np.asarray(absent, np.int64), m)    # a list without a present entry
        mask[B - 1, :] = True
        rows[0, m - 1] = -1                                            # ... and one at the end of a list
        mask[0, m - 1] = True
        for metric in (COS, IP):
            for got in (sh.idx.score_rows(sh.q[:B], rows, metric), score_device(sh.idx, sh.q[:B], rows, metric)):
                assert not got[mask].any() and not np.signbit(got[mask]).any(), (shape, B, m)
                close_to(got, sh.want(B, rows, metric), f"{shape} absent B={B} m={m}")
                assert (got[~mask] != 0).all()


def test_an_empty_index_scores_nothing():
    idx = nat.NativeIndex(768, 0)
    q = orc.synthetic_queries(3, 768, seed=1)
    rows = np.array([[0, 1, -1, 5], [0, 0, 0, 0], [7, 8, 9, 10]], np.int64)
    assert not idx.score_rows(q, rows).any() and not score_device(idx, q, rows).any()
    assert int(idx.get_option("score_calls")) == 2 and int(idx.get_option("score_pairs")) == 24
    idx.close()


# ---- 3. the same bits as the other routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "narrow", "dim33", "shifted"])
@pytest.mark.parametrize("metric", [COS, IP])
def test_scores_have_the_bits_of_the_gather_route(request, shape, metric):
    sh = request.getfixturevalue(shape)
    allowed = np.random.default_rng(300).choice(sh.n, size=300, replace=False)
    flt = sh.idx.make_filter(allowed)
    sh.idx.set_option("filter_route", 1)
    try:
        fs, fr = sh.idx.search(sh.q[:64], 300, metric, row_filter=flt)
        assert int(sh.idx.get_option("filter_route_last")) == 1
    finally:
        sh.idx.set_option("filter_route", -1)
        flt.close()
    assert (fr >= 0).all() and all(set((r - sh.row_offset).tolist()) == set(allowed.tolist()) for r in fr)
    got = sh.idx.score_rows(sh.q[:64], fr, metric)
    assert np.array_equal(got.view(np.uint32), fs.view(np.uint32)), f"{int((got.view(np.uint32) != fs.view(np.uint32)).sum())} pairs differ"


def test_scores_have_the_bits_of_a_search():
    """rq_search's own top 100 over the fp16 rows ("scan8" = 0): the fast tail re-scores its candidates in the same summation order.
    The exact rung (and a call planned as an exact scan: fewer than 2 x (k + slack) bins) sums in another order, so the corpus is
    one the parity tests certify without it -- 30 000 Gaussian rows -- and the test asserts that no query needed it."""
    x16 = orc.synthetic_corpus(30_000, 768, seed=12)
    q = orc.synthetic_queries(16, 768, seed=13)
    idx = nat.NativeIndex(768, 0)
    idx.set_option("scan8", 0)
    idx.add_f16(x16)
    idx.reset_timing()
    for metric in (COS, IP):
        s, r = idx.search(q, 100, metric)
        t = idx.timing()
        print("timing after the search:", t)
        assert t["exact_scans"] == 0
        got = idx.score_rows(q, r, metric)
        assert np.array_equal(got.view(np.uint32), s.view(np.uint32)), f"metric {metric}: {int((got.view(np.uint32) != s.view(np.uint32)).sum())} pairs differ"
    assert idx.timing()["searches"] == 2 and idx.timing()["queries"] == 32           # a scoring call is not a search
    idx.close()


# ---- 4. special values -------------------------------------------------------------------------------------------------------------
def test_zero_rows_inf_rows_and_zero_norm_queries_on_a_70_row_index():
    x16 = orc.synthetic_corpus(70, 768, seed=70).copy()
    x16[11] = 0
    x16[40, 5] = np.float16(np.inf)
    q = orc.synthetic_queries(5, 768, seed=71)
    q[2] = 0
    sh = Shape(n=70, x16=x16, q=q)
    try:
        rng = np.random.default_rng(72)
        for m in (1, 7, 64, 65, 100, 1500):
            rows = rng.integers(0, 70, size=(5, m)).astype(np.int64)
            rows[:, 0] = 11
            if m > 2:
                rows[:, 1], rows[:, m - 1] = 40, 70                                         # the inf row; one past the end
            for metric in (COS, IP):
                want = sh.want(5, rows, metric).copy()
                want[2] = 0.0                                                               # a zero-norm query scores every present row 0.0
                for got in (sh.idx.score_rows(q, rows, metric), score_device(sh.idx, q, rows, metric)):
                    close_to(got, want, f"70 rows m={m} metric {metric}")
                    assert not got[2].any() and not got[:, 0].any()
                    if m > 2:
                        assert not got[:, m - 1].any()
                        if metric == COS:
                            assert (got[[0, 1, 3, 4], 1] == -np.inf).all()                  # inf / inf = NaN counts as -inf
                        else:
                            assert np.isinf(got[[0, 1, 3, 4], 1]).all() and np.array_equal(got[:, 1], want[:, 1])
    finally:
        sh.close()


# ---- 5. streams and deferred tails ---------------------------------------------------------------------------------------------------
def test_device_form_on_a_non_default_stream(wide):
    import torch
    s = torch.cuda.Stream()
    rows = random_lists(wide, 70, 100, seed=5)
    try:
        got = score_device(wide.idx, wide.q, rows, COS, stream=s)
        close_to(got, wide.want(70, rows), "non-default stream")
        assert np.array_equal(got.view(np.uint32), wide.idx.score_rows(wide.q, rows).view(np.uint32))
    finally:
        wide.idx.stream_release(s.cuda_stream)


def test_a_scoring_call_completes_what_the_stream_deferred(wide):
    """pipeline = 2: a fused search leaves its tail pending on the stream; the scoring call behind it completes it first, so that
    search's outputs are complete in stream order -- no flush -- and equal the oracle."""
    import torch
    idx = wide.idx
    B, k = 64, 10
    d_q = torch.from_numpy(wide.q[:B]).cuda()
    sc = torch.full((B, k), 7.0, device="cuda")
    rw = torch.full((B, k), 7, device="cuda", dtype=torch.int64)
    st = torch.full((B,), 7, device="cuda", dtype=torch.int32)
    rows = random_lists(wide, B, 100, seed=8)
    d_r = torch.from_numpy(rows).cuda()
    out = torch.full((B, 100), 7.0, device="cuda")
    torch.cuda.synchronize()
    idx.set_option("pipeline", 2)
    try:
        idx.search_device(d_q, B, k, COS, sc, rw, None, st, 0)
        idx.score_rows_device(d_q, B, d_r, 100, COS, out, 0)
        torch.cuda.synchronize()
        got_s, got_r, got_st = sc.cpu().numpy(), rw.cpu().numpy(), st.cpu().numpy()
        with pytest.raises(nat.RqError):
            idx.debug_bin_records(0, 64)                               # the stream's last call has no bin records
        idx.search_flush_device(0)
        torch.cuda.synchronize()
        assert np.array_equal(rw.cpu().numpy(), got_r) and np.array_equal(sc.cpu().numpy(), got_s)          # nothing was left to flush
    finally:
        idx.set_option("pipeline", 0)
    assert not got_st.any()
    ws, wr = orc.topk_from_scores(wide.full(COS)[:B], k)
    assert np.array_equal(got_r, wr) and float(np.abs(got_s - ws).max()) <= SCORE_TOL
    close_to(out.cpu().numpy(), wide.want(B, rows), "behind a deferred tail")


# ---- 6. appends, counters, refusals ----------------------------------------------------------------------------------------------------
def test_rows_are_scorable_after_an_append_and_the_counters_count():
    x16 = orc.synthetic_corpus(130, 100, seed=3)
    q = orc.synthetic_queries(3, 100, seed=4)
    idx = nat.NativeIndex(100, 0)
    idx.add_f16(x16[:100])
    rows = np.array([[0, 99, 100, 129], [50, 50, 128, -1], [99, 100, 101, 1]], np.int64)
    t0 = idx.timing()
    assert int(idx.get_option("score_calls")) == 0 and int(idx.get_option("score_pairs")) == 0
    close_to(idx.score_rows(q, rows), so.pairs(q, x16[:100], rows), "before the append")
    assert (int(idx.get_option("score_calls")), int(idx.get_option("score_pairs"))) == (1, 12)
    idx.add_f16(x16[100:])
    want = so.pairs(q, x16, rows)
    assert (want[:, 2] != 0).all()
    close_to(idx.score_rows(q, rows), want, "after the append")
    close_to(score_device(idx, q, rows), want, "after the append, device form")
    close_to(idx.score_rows(q[0], rows[0], IP), so.pairs(q[:1], x16, rows[:1], IP), "one query, one list")
    assert (int(idx.get_option("score_calls")), int(idx.get_option("score_pairs"))) == (4, 12 + 12 + 12 + 4)
    t1 = idx.timing()
    assert (t1["searches"], t1["queries"], t1["widened"], t1["exact_scans"]) == (t0["searches"], t0["queries"], t0["widened"], t0["exact_scans"])
    out = np.zeros(12, np.float32)
    for B, m, metric in ((3, 4, 5), (0, 4, 0), (3, 0, 0), (3, nat.MAX_SCORE_ROWS + 1, 0), (65536, 4, 0)):                   # the library's own checks: RQ_EINVAL
        assert idx._lib.rq_score_rows(idx._h, nat._ptr(q), B, nat._ptr(rows), m, metric, nat._ptr(out)) == -1
        assert idx._lib.rq_score_rows_device(idx._h, nat._ptr(q), B, nat._ptr(rows), m, metric, nat._ptr(out), None) == -1
    assert idx._lib.rq_score_rows(idx._h, nat._ptr(q), 3, None, 4, 0, nat._ptr(out)) == -1 and "null" in nat.last_error()
    assert (int(idx.get_option("score_calls")), int(idx.get_option("score_pairs"))) == (4, 40)                               # a refused call counts nothing
    idx.close()


def test_a_multi_device_index_is_refused():
    x16 = orc.synthetic_corpus(300, 768, seed=6)
    multi = nat.NativeIndex(768, devices=[0, 0])
    multi.add_f16(x16)
    q = orc.synthetic_queries(2, 768, seed=7)
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.score_rows(q, np.zeros((2, 3), np.int64))
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.score_rows_device(8, 2, 16, 3, COS, 24)                  # (refused before a pointer is looked at)
    multi.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_completed_hybrid_pools_end_to_end(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    docs = [si.Document(id=f"p{i}", text=f"passage {i} about topic {i % 7} and item {i * 31 % 101}", title=f"T{i}") for i in range(300)]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs)
    dense, bm = r.dense_index, r.bm25_index
    queries = ["passage 3 about topic 3", "item 17", docs[42].text, "topic 5 and item 99", "nothing in common"]
    filled = 0
    for pool, top in ((20, 10), (50, 100)):
        batch = r.hybrid_search_batch(queries, top_k=top, retrieval_pool_size=pool, complete_scores=True)
        single = [r.hybrid_search(q, top_k=top, retrieval_pool_size=pool, complete_scores=True) for q in queries]
        assert batch == single
        assert r.get_scores_for_router_batch(queries, top, retrieval_pool_size=pool, complete_scores=True) == \
               [r.get_scores_for_router(q, top, retrieval_pool_size=pool, complete_scores=True) for q in queries]
        assert r.hybrid_search_batch(queries, top_k=top, retrieval_pool_size=pool, complete_scores=False) == r.hybrid_search_batch(queries, top_k=top, retrieval_pool_size=pool)
        for q, res in zip(queries, single):
            found = {d: s for d, s, _ in dense.search(q, top_k=len(dense))}
            full_b = bm.get_scores(bm._tokenize(q))
            plain = {x.doc_id: x for x in r.hybrid_search(q, top_k=10 ** 6, retrieval_pool_size=pool)}
            assert res and [x.doc_id for x in res if x.doc_id not in plain] == []
            for x in res:
                assert x.dense_score == found[x.doc_id], (q, x.doc_id)
                assert x.bm25_score == full_b[bm._row_of_id()[x.doc_id]]
                filled += plain[x.doc_id].dense_score == 0.0
            assert dense.score_ids(q, [x.doc_id for x in res] + ["no such id"]) == [x.dense_score for x in res] + [0.0]
    assert filled > 10

