"""Diversified search on the MI355X (include/rq.h rq_mmr_select_device / rq_search_mmr, csrc/rq_mmr.hip): the rows a
selection returns equal the oracle's (tests/mmr_oracle.py) at EVERY step.  The gap between the best and the second-best value of a
step goes down to one fp32 ulp of a similarity, so no tolerance on v can decide a step: the comparison is path-following -- at
step t the oracle is given the device's own first t picks and must name the device's next pick -- so a failure names its step and
does not cascade.  d_mmr agrees to 1e-6 (SCORE_TOL of the parity tests, weights summing to 1); returned relevances equal the
candidates' bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_oracle as fo  # noqa: E402
import mmr_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
N_BASE = 4101                      # 65 bins, a ragged last bin
LAMBDAS = [0.0, 0.3, 0.5, 0.7, 1.0]
NQ = 70


class Shape:
    """One index with its rows, NQ queries and their canonical top RQ_MAX_K per metric (computed once, shared, never changed)."""

    def __init__(self, n=N_BASE, dim=768, seed=1234, clustered=False, options=(), row_offset=0, x16=None):
        self.n, self.dim, self.row_offset = n, dim, row_offset
        self.x16 = orc.synthetic_corpus(n, dim, seed=seed, clustered=clustered) if x16 is None else x16
        self.q = orc.synthetic_queries(NQ, dim, seed=seed + 1)
        self.idx = nat.NativeIndex(dim, 0)
        for name, v in options:
            self.idx.set_option(name, v)
        self.idx.set_option("scan8", 0)
        self.idx.add_f16(self.x16)
        if row_offset:
            self.idx.set_row_offset(row_offset)
        self._top = {}

    def top(self, metric=COS):
        if metric not in self._top:
            s, r = orc.dense_topk(self.q, self.x16, min(nat.MAX_K, self.n), metric, self.row_offset)
            s.setflags(write=False); r.setflags(write=False)
            self._top[metric] = (s, r)
        return self._top[metric]

    def cands(self, B, m, metric=COS):
        s, r = self.top(metric)
        return s[:B, :m].copy(), r[:B, :m].copy()                      # (writable copies: the shared arrays stay as they are)

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
def clustered():
    sh = Shape(seed=55, clustered=True)
    yield sh
    sh.close()


@pytest.fixture(scope="module")
def shifted():
    sh = Shape(n=1000, seed=9, row_offset=10 ** 6)
    yield sh
    sh.close()


def select(idx, rel, rows, k, lam, metric=COS, stream=0, want_mmr=True):
    """One rq_mmr_select_device call over host candidates [B][m] -> (scores, rows, mmr) on the host."""
    import torch
    B, m = rows.shape
    d_r = torch.from_numpy(np.ascontiguousarray(rows, np.int64)).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(rel, np.float32)).cuda()
    o_s = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    o_v = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.mmr_select_device(d_r, d_s, B, m, k, lam, metric, o_s, o_r, o_v if want_mmr else None, stream)
    torch.cuda.synchronize()
    return o_s.cpu().numpy(), o_r.cpu().numpy(), (o_v.cpu().numpy() if want_mmr else None)


def follows_oracle(x16, rel, rows, got, k, lam, metric=COS, row_offset=0, what=""):
    """Every query of a call: padding beyond k_eff, relevances passed through bit for bit, every step's pick equal to the oracle's
    from the same state, d_mmr within SCORE_TOL."""
    gs, gr, gv = got
    for b in range(rows.shape[0]):
        present = mo.present_mask(rel[b], rows[b], x16.shape[0], row_offset)
        k_eff = min(k, int(present.sum()))
        tag = f"{what} query {b} lambda {lam}"
        assert (gr[b, k_eff:] == -1).all() and not gs[b, k_eff:].any() and (gv is None or not gv[b, k_eff:].any()), f"{tag}: padding beyond k_eff = {k_eff}"
        pos_of = {int(r): i for i, r in enumerate(rows[b]) if present[i]}
        picks = [int(r) for r in gr[b, :k_eff]]
        assert all(r in pos_of for r in picks) and len(set(picks)) == k_eff, f"{tag}: picked rows {picks} are not distinct present candidates"
        follow = [pos_of[r] for r in picks]
        assert np.array_equal(gs[b, :k_eff].view(np.uint32), np.asarray(rel[b], np.float32)[follow].view(np.uint32)), f"{tag}: relevances were not passed through"
        if k_eff == 0:
            continue
        _, o_r, o_v, pos = mo.mmr_select(rel[b], rows[b], x16, k, lam, metric, row_offset, follow=follow)
        for t in range(k_eff):
            if pos[t] != follow[t]:
                dv = float(gv[b, t]) if gv is not None else float("nan")
                raise AssertionError(f"{tag}: step {t}: the device picked position {follow[t]} (row {picks[t]}, d_mmr {dv!r}), the oracle position {pos[t]} "
                                     f"(row {int(o_r[t])}, v {float(o_v[t])!r})")
        if gv is not None:
            err = float(np.abs(gv[b, :k_eff].astype(np.float64) - o_v[:k_eff].astype(np.float64)).max())
            assert err <= SCORE_TOL, f"{tag}: d_mmr differs by {err}"


# ---- 1. selection against the oracle -----------------------------------------------------------------------------------------
CASES = [(1, 1, 16, COS), (64, 10, 16, COS), (100, 100, 16, COS), (257, 33, 16, COS), (1024, 128, 16, COS),
         (64, 10, 1, COS), (64, 10, 70, COS), (257, 33, 70, COS), (64, 10, 16, IP), (257, 33, 16, IP)]


@pytest.mark.parametrize("m,k,B,metric", CASES)
def test_selection_follows_the_oracle(wide, m, k, B, metric):
    rel, rows = wide.cands(B, m, metric)
    for lam in LAMBDAS:
        got = select(wide.idx, rel, rows, k, lam, metric)
        follows_oracle(wide.x16, rel, rows, got, k, lam, metric, what=f"m={m} k={k} B={B} metric={metric}")


@pytest.mark.parametrize("shape", ["narrow", "dim33", "clustered"])
@pytest.mark.parametrize("m,k,B", [(64, 10, 16), (100, 100, 16), (257, 33, 70), (1024, 128, 16)])
def test_selection_on_the_narrow_layout_and_a_clustered_corpus(request, shape, m, k, B):
    sh = request.getfixturevalue(shape)
    rel, rows = sh.cands(B, m)
    for lam in LAMBDAS:
        got = select(sh.idx, rel, rows, k, lam)
        follows_oracle(sh.x16, rel, rows, got, k, lam, what=f"{shape} m={m} k={k} B={B}")


def test_lambda_zero_shows_the_similarities_and_lambda_one_the_relevance_order(wide, clustered):
    for sh in (wide, clustered):
        rel, rows = sh.cands(16, 100)
        s, r, v = select(sh.idx, rel, rows, 12, 0.0)
        assert np.array_equal(r[:, 0], rows[:, 0]) and not v[:, 0].any()                  # every v is 0: position 0
        worst = 0.0
        for b in range(16):
            for t in range(1, 12):
                sims = orc.exact_scores(sh.x16[r[b, :t]].astype(np.float32), sh.x16[r[b, t:t + 1]])[:, 0]
                worst = max(worst, abs(float(-v[b, t]) - float(sims.max())))
        print(f"lambda = 0: largest |(-d_mmr) - max sim| = {worst}")
        assert worst <= SCORE_TOL
        s, r, v = select(sh.idx, rel, rows, 100, 1.0)
        assert np.array_equal(r, rows) and np.array_equal(s.view(np.uint32), rel.view(np.uint32)) and np.array_equal(v.view(np.uint32), rel.view(np.uint32))
        s2, r2, none = select(sh.idx, rel, rows, 12, 0.5, want_mmr=False)                  # d_mmr may be NULL
        assert none is None
        follows_oracle(sh.x16, rel, rows, (s2, r2, None), 12, 0.5)


# ---- 2. lambda = 1 is the plain search -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,fetch_k", [(10, 64), (100, 100), (33, 257)])
def test_lambda_one_is_the_search_bit_for_bit(wide, k, fetch_k):
    q = wide.q[:64]
    before = int(wide.idx.get_option("mmr_calls"))
    ps, pr = wide.idx.search(q, k)
    s, r, v = wide.idx.search_mmr(q, k, fetch_k, 1.0, return_mmr=True)
    assert np.array_equal(r, pr) and np.array_equal(s.view(np.uint32), ps.view(np.uint32)) and np.array_equal(v.view(np.uint32), ps.view(np.uint32))
    flt = wide.idx.make_filter(fo.standard_masks(N_BASE)["random50"])
    fs, fr = wide.idx.search(q, k, row_filter=flt)
    s, r = wide.idx.search_mmr(q, k, fetch_k, 1.0, row_filter=flt)
    assert np.array_equal(r, fr) and np.array_equal(s.view(np.uint32), fs.view(np.uint32))
    flt.close()
    assert int(wide.idx.get_option("mmr_calls")) == before + 2


# ---- 3. absent candidates, 6. row_offset -------------------------------------------------------------------------------------
def test_absent_candidates_are_never_selected_or_read(shifted):
    off, n = shifted.row_offset, shifted.n
    rel, rows = shifted.cands(4, 16)
    rel, rows = rel.copy(), rows.copy()
    # query 0: -1 at position 0 and between present ones, the rows just outside the shard, the last stored row, a NaN relevance
    rows[0, 0] = -1; rows[0, 3] = -1; rows[0, 5] = off + n; rows[0, 6] = off - 1; rows[0, 7] = off + n - 1; rel[0, 7] = 0.5; rel[0, 9] = np.nan
    rows[0, 10] = 5; rows[0, 11] = 2 ** 40                                             # a LOCAL row number is below row_offset; far outside
    assert (rows[0] == off + n - 1).sum() == 1 and int(mo.present_mask(rel[0], rows[0], n, off).sum()) == 9
    # query 1: three present candidates for k = 8; query 2: nothing present; query 3: untouched
    rows[1, 3:] = -1
    rows[2, :] = -1; rows[2, 4] = off + n; rel[2, 0] = np.nan
    for lam in (0.0, 0.5, 1.0):
        got = select(shifted.idx, rel, rows, 8, lam)
        follows_oracle(shifted.x16, rel, rows, got, 8, lam, row_offset=off, what="absent")
        want = mo.mmr_select_batch(rel, rows, shifted.x16, 8, lam, row_offset=off)
        assert np.array_equal(got[1], want[1])
        assert (got[1][1, 3:] == -1).all() and (got[1][2] == -1).all() and not got[0][2].any() and not got[2][2].any()
        for b in range(4):
            ok = set(rows[b][mo.present_mask(rel[b], rows[b], n, off)].tolist())
            assert set(got[1][b].tolist()) - {-1} <= ok, f"query {b}: an absent candidate was selected"
        if lam > 0:
            assert off + n - 1 in got[1][0]                                                  # the last stored row is a candidate like any other


def test_row_offset_global_rows_go_in_and_come_out(shifted):
    rel, rows = shifted.cands(16, 64)
    assert rows.min() >= 10 ** 6
    for lam in (0.3, 1.0):
        got = select(shifted.idx, rel, rows, 10, lam)
        assert got[1].min() >= 10 ** 6
        follows_oracle(shifted.x16, rel, rows, got, 10, lam, row_offset=10 ** 6, what="row_offset")


# ---- 4. unsorted candidates, arbitrary relevance ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, IP])
def test_unsorted_candidates_with_arbitrary_relevance(wide, metric):
    rng = np.random.default_rng(17)
    rows = np.stack([rng.choice(N_BASE, size=200, replace=False) for _ in range(16)]).astype(np.int64)
    rel = (3.0 * rng.standard_normal((16, 200))).astype(np.float32)
    assert (rel < 0).any()
    for lam in (0.3, 0.7):
        got = select(wide.idx, rel, rows, 40, lam, metric)
        follows_oracle(wide.x16, rel, rows, got, 40, lam, metric, what="unsorted")


# ---- 5. duplicate stored rows ---------------------------------------------------------------------------------------------------
def test_duplicate_stored_rows_tie_by_position_and_are_pushed_back():
    x16 = orc.synthetic_corpus(N_BASE, 768, seed=5)
    x16[100] = x16[7]                                      # a pair
    x16[200] = x16[3000] = x16[9]                          # a triple
    sh = Shape(x16=x16, seed=5)
    q = np.stack([x16[7].astype(np.float32) + sh.q[0] / np.linalg.norm(sh.q[0]), x16[9].astype(np.float32) + sh.q[1] / np.linalg.norm(sh.q[1])])
    rel, rows = orc.dense_topk(q, x16, 64)
    assert rows[0, :2].tolist() == [7, 100] and rows[1, :3].tolist() == [9, 200, 3000] and rel[0, 0] == rel[0, 1] and rel[1, 0] == rel[1, 1] == rel[1, 2]
    for lam in (1.0, 0.5):
        want = mo.mmr_select_batch(rel, rows, x16, 10, lam)
        got = select(sh.idx, rel, rows, 10, lam)
        follows_oracle(x16, rel, rows, got, 10, lam, what="duplicates")
        assert np.array_equal(got[1], want[1])
        assert got[1][0, 0] == 7 and got[1][1, 0] == 9                                    # the lower position wins the tie
        if lam == 1.0:
            assert got[1][0, :2].tolist() == [7, 100] and got[1][1, :3].tolist() == [9, 200, 3000]
        else:
            assert 100 not in want[1][0, :5] and not {200, 3000} & set(want[1][1, :5].tolist())     # the oracle pushes the copies back ...
            assert 100 not in got[1][0, :5] and not {200, 3000} & set(got[1][1, :5].tolist())       # ... and so does the device
    sh.close()


# ---- 7. layouts ---------------------------------------------------------------------------------------------------------------
def test_row_pad_twin_is_bit_identical(narrow):
    twin = Shape(dim=384, seed=21, options=(("row_pad", 768),))
    assert narrow.idx.row_pad == 384 and twin.idx.row_pad == 768
    rel, rows = narrow.cands(16, 257)
    for lam in (0.0, 0.3, 0.7):
        a = select(narrow.idx, rel, rows, 33, lam)
        b = select(twin.idx, rel, rows, 33, lam)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    twin.close()


# ---- 8. rq_search_mmr end to end ----------------------------------------------------------------------------------------------
def _end_to_end(sh, q, k, fetch_k, lam, mask=None, flt=None, what=""):
    n_play = sh.n if mask is None else int(mask.sum())
    m = max(k, min(fetch_k, n_play))
    if mask is None:
        rel, rows = orc.dense_topk(q, sh.x16, m, COS, sh.row_offset)
    else:
        rel, rows = fo.filtered_topk(q, sh.x16, mask, m, COS, sh.row_offset)
    got = sh.idx.search_mmr(q, k, fetch_k, lam, row_filter=flt, return_mmr=True)
    # the device selects over ITS search's relevances: they must be the oracle's bit for bit for the oracle's path to apply
    ds, dr = sh.idx.search(q, m, row_filter=flt) if m <= len(sh.idx) else (rel, rows)
    print(f"{what}: candidate rows equal: {np.array_equal(dr, rows)}, relevances that differ in bits: {int((ds.view(np.uint32) != rel.view(np.uint32)).sum())} of {rel.size}")
    k_dev = min(k, n_play)
    assert (got[1][:, k_dev:] == -1).all()
    gs = got[0].copy()
    # relevances are compared to SCORE_TOL here (the parity bar of a search); the pass-through itself is checked bit for bit above
    for b in range(len(q)):
        sel = {int(r): float(s) for r, s in zip(rows[b], rel[b]) if r >= 0}
        assert all(int(r) in sel and abs(sel[int(r)] - float(s)) <= SCORE_TOL for r, s in zip(got[1][b, :k_dev], gs[b, :k_dev])), f"{what}: query {b}"
        pos = {int(r): i for i, r in enumerate(rows[b]) if r >= 0}
        gs[b, :k_dev] = [rel[b, pos[int(r)]] for r in got[1][b, :k_dev]]
    follows_oracle(sh.x16, rel, rows, (gs, got[1], got[2]), k, lam, row_offset=sh.row_offset, what=what)
    want = mo.mmr_topk(q, sh.x16, k, fetch_k, lam, COS, mask, sh.row_offset)
    assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("lam", [0.3, 0.5])
def test_search_mmr_end_to_end(wide, lam):
    q = wide.q[:16]
    _end_to_end(wide, q, 10, 64, lam, what="unfiltered")
    masks = fo.standard_masks(N_BASE)
    for name in ("random50", "five_rows", "none"):
        flt = wide.idx.make_filter(masks[name])
        _end_to_end(wide, q, 10, 64, lam, masks[name], flt, what=name)
        flt.close()


def test_search_mmr_clamps_fetch_k_and_refuses_a_stale_filter(shifted):
    _end_to_end(shifted, shifted.q[:4], 10, 1024, 0.5, what="fetch_k > N")             # 1000 rows: 1000 candidates
    x16 = orc.synthetic_corpus(300, 768, seed=3)
    idx, other = nat.NativeIndex(768, 0), nat.NativeIndex(768, 0)
    idx.add_f16(x16); other.add_f16(x16)
    flt = idx.make_filter(np.arange(0, 300, 3))
    q = orc.synthetic_queries(2, 768)
    idx.search_mmr(q, 5, 20, 0.5, row_filter=flt)
    with pytest.raises(nat.RqError, match="another index"):
        other.search_mmr(q, 5, 20, 0.5, row_filter=flt)
    idx.add_f16(x16[:10])
    with pytest.raises(nat.RqError, match="stale filter"):
        idx.search_mmr(q, 5, 20, 0.5, row_filter=flt)
    flt.close(); idx.close(); other.close()


# ---- 9. stream order ------------------------------------------------------------------------------------------------------------
def test_selection_runs_in_stream_order_behind_the_search(wide):
    import torch
    B, m, k, lam = 64, 100, 10, 0.5
    st = torch.cuda.Stream()
    d_q = torch.from_numpy(np.ascontiguousarray(wide.q[:B])).cuda()
    c_s = torch.full((B, m), 7.0, dtype=torch.float32, device="cuda")
    c_r = torch.full((B, m), 7, dtype=torch.int64, device="cuda")
    c_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    o_s = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    o_r = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    o_v = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        wide.idx.search_device(d_q, B, m, COS, c_s, c_r, None, c_st, st.cuda_stream)
        wide.idx.search_flush_device(st.cuda_stream)
        wide.idx.mmr_select_device(c_r, c_s, B, m, k, lam, COS, o_s, o_r, o_v, st.cuda_stream)      # no host synchronisation in between
        st.synchronize()
        rel, rows = c_s.cpu().numpy(), c_r.cpu().numpy()
        assert not c_st.cpu().numpy().any()
        assert np.array_equal(rows, wide.cands(B, m)[1])
        follows_oracle(wide.x16, rel, rows, (o_s.cpu().numpy(), o_r.cpu().numpy(), o_v.cpu().numpy()), k, lam, what="stream order")
    finally:
        wide.idx.stream_release(st.cuda_stream)


# ---- 10. after an append ---------------------------------------------------------------------------------------------------------
def test_selection_after_an_append(wide):
    idx = nat.NativeIndex(768, 0)
    idx.set_option("scan8", 0)
    idx.add_f16(wide.x16[:2000])
    rel, rows = orc.dense_topk(wide.q[:8], wide.x16[:2000], 64)
    follows_oracle(wide.x16[:2000], rel, rows, select(idx, rel, rows, 10, 0.5), 10, 0.5, what="before the append")
    idx.add_f16(wide.x16[2000:])
    rel, rows = wide.cands(8, 64)
    assert (rows >= 2000).any()
    follows_oracle(wide.x16, rel, rows, select(idx, rel, rows, 10, 0.5), 10, 0.5, what="after the append")
    s, r = idx.search_mmr(wide.q[:8], 10, 64, 0.5)
    assert np.array_equal(r, mo.mmr_topk(wide.q[:8], wide.x16, 10, 64, 0.5)[1])
    idx.close()


# ---- 11. the Python surface -------------------------------------------------------------------------------------------------------
def test_dense_index_and_hybrid_retriever_return_diverse_passages(tmp_path):
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import HashEmbedder
    topics = ["solar panels", "wind turbines", "river dams", "coal plants", "gas pipelines", "nuclear reactors", "tidal barrages"]
    texts = [f"report {i} on {topics[i % 7]} in region {i % 13} covering output {i * 31 % 101} and cost {i * 17 % 53}" for i in range(200)]
    texts += texts[:100]                                                     # a third of the collection: verbatim copies
    docs = [si.Document(id=f"p{i}", text=t, title=f"T{i}") for i, t in enumerate(texts)]
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "chroma"), embedder=HashEmbedder())
    r.add_documents(docs)
    emb = HashEmbedder()
    x16 = orc.prepare_rows_f32(emb.embed(texts), True)
    ids = [d.id for d in docs]
    copy_of = {f"p{i}": f"p{i + 200}" for i in range(100)}
    copy_of.update({v: k for k, v in copy_of.items()})
    queries = ["report on solar panels in region 3 covering output 93", "cost of wind turbines in region 8", "river dams output 62 and cost 34"]
    for qtext in queries:
        qv = emb.embed([qtext])
        ws, wr, _ = mo.mmr_topk(qv, x16, 10, 50, 0.5)
        plain = [ids[i] for i in orc.dense_topk(qv, x16, 5)[1][0]]
        want5 = [ids[i] for i in wr[0, :5]]
        # the precondition, on the oracle alone: the plain top 5 holds a passage AND its copy, the diversified top 5 does not
        assert any(copy_of.get(d) in plain for d in plain), qtext
        assert not any(copy_of.get(d) in want5 for d in want5), qtext
        got = r.dense_index.search_mmr(qtext, 10, 50, 0.5)
        assert [d for d, _, _ in got] == [ids[i] for i in wr[0]]
        np.testing.assert_allclose([s for _, s, _ in got], ws[0], atol=SCORE_TOL)
        assert [t for _, _, t in got] == [texts[i] for i in wr[0]]
        got5 = [d for d, _, _ in got[:5]]
        assert not any(copy_of.get(d) in got5 for d in got5)
        has = [d for d, _, _ in r.dense_index.search(qtext, 5)]
        assert has == plain and any(copy_of.get(d) in has for d in has)
        assert r.dense_index.search_mmr_batch([qtext, queries[0]], 10, 50, 0.5)[0] == got
        assert r.dense_search_mmr(qtext, 10, 50, 0.5) == [(d, s) for d, s, _ in got]
        # allowed_ids: the originals only
        allowed = ids[:200:2]
        mask = np.zeros(300, dtype=bool)
        mask[:200:2] = True
        fs, fr, _ = mo.mmr_topk(qv, x16, 10, 50, 0.5, mask=mask)
        got = r.dense_index.search_mmr(qtext, 10, 50, 0.5, allowed_ids=allowed)
        assert [d for d, _, _ in got] == [ids[i] for i in fr[0]] and {d for d, _, _ in got} <= set(allowed)
        assert r.dense_search_mmr(qtext, 10, 50, 0.5, allowed_ids=allowed) == [(d, s) for d, s, _ in got]
    r.close()


# ---- 12. error returns ------------------------------------------------------------------------------------------------------------
def test_error_returns(wide):
    import torch
    lib = nat.load_library()
    B, m, k = 2, 16, 4
    rel, rows = wide.cands(B, m)
    d_r, d_s = torch.from_numpy(rows).cuda(), torch.from_numpy(rel).cuda()
    o_s = torch.zeros((B, m), dtype=torch.float32, device="cuda")
    o_r = torch.zeros((B, m), dtype=torch.int64, device="cuda")
    P = nat._ptr
    h = wide.idx._h

    def sel(idx_h=h, cr=d_r, cs=d_s, B=B, m=m, k=k, lam=0.5, metric=COS, os_=o_s, or_=o_r):
        return lib.rq_mmr_select_device(idx_h, P(cr), P(cs), B, m, k, C.c_double(lam), metric, P(os_), P(or_), None, None)
    before = int(wide.idx.get_option("mmr_calls"))
    assert sel() == 0
    assert int(wide.idx.get_option("mmr_calls")) == before + 1
    EINVAL, EUNSUP = -1, -6
    for bad in (dict(idx_h=None), dict(cr=None), dict(cs=None), dict(os_=None), dict(or_=None), dict(B=0), dict(B=65536), dict(m=0), dict(m=nat.MAX_K + 1),
                dict(k=0), dict(k=m + 1), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")), dict(lam=float("inf")), dict(metric=2)):
        assert sel(**bad) == EINVAL, bad
    assert int(wide.idx.get_option("mmr_calls")) == before + 1
    q = np.ascontiguousarray(wide.q[:B])
    hs, hr = np.zeros((B, k), np.float32), np.zeros((B, k), np.int64)

    def srch(idx_h=h, f=None, q_=q, B=B, k=k, fetch=m, lam=0.5, metric=COS, hs_=hs, hr_=hr):
        return lib.rq_search_mmr(idx_h, f, P(q_), B, k, fetch, C.c_double(lam), metric, P(hs_), P(hr_), None)
    assert srch() == 0
    for bad in (dict(idx_h=None), dict(q_=None), dict(hs_=None), dict(hr_=None), dict(B=0), dict(k=0), dict(k=m + 1), dict(fetch=nat.MAX_K + 1), dict(fetch=0),
                dict(lam=-1.0), dict(lam=2.0), dict(lam=float("nan")), dict(metric=-1)):
        assert srch(**bad) == EINVAL, bad
    multi = nat.NativeIndex(768, devices=[0, 0])                                  # the same GPU named twice
    multi.add_f16(wide.x16[:300])
    assert sel(idx_h=multi._h) == EUNSUP and "RQ_EUNSUPPORTED" in nat.last_error()
    assert srch(idx_h=multi._h) == EUNSUP and "RQ_EUNSUPPORTED" in nat.last_error()
    with pytest.raises(nat.RqError, match="RQ_EUNSUPPORTED"):
        multi.search_mmr(q, 2, 8, 0.5)
    multi.close()
    with pytest.raises(ValueError):
        wide.idx.search_mmr(q, 5, 4, 0.5)
    with pytest.raises(ValueError):
        wide.idx.search_mmr(q, 2, 8, float("nan"))
    empty = nat.NativeIndex(768, 0)
    s, r, v = empty.search_mmr(q, 3, 8, 0.5, return_mmr=True)                       # no rows: padding
    assert (r == -1).all() and not s.any() and not v.any()
    empty.close()
