"""Masked sparse search on the device (include/rq.h rq_sparse_topk_masked*, csrc/rq_sparse.hip) against tests/sparse_masked_oracle.py:
rows identical and every score identical in its bits, no tolerance, no case left out.  tests/test_sparse_masked.py shows that the
oracle and librq_bm25.so's masked call agree bit for bit, so the device route and the host library share one definition."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_masked_oracle as mo  # noqa: E402
import sparse_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = so.cases()


def _index(ix, **options):
    sp = _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    for name, value in options.items():
        if value is not None:
            sp.set_option(name, value)
    return sp


def _by(name):
    return next(c for c in CASES if c["name"] == name)


def _check(sp, ix, q, k, masks, mask_of, tile, what=None):
    """One masked call against the oracle: rows, score bits and both tile counters, exactly."""
    B = len(q[0]) - 1
    got = sp.topk(q[0], q[1], B, k, masks=masks, mask_of=mask_of)
    want = mo.topk(ix, q[0], q[1], k, masks, mask_of)
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert so.same(got, want), (what, np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))[:5])
    masked, skipped = mo.tile_counters(ix, q[0], q[1], tile, masks, mask_of)
    assert (sp.get_option("masked_tiles_last"), sp.get_option("skipped_tiles_last")) == (masked, skipped), what
    assert sp.get_option("tiles_last") == -(-ix["n_docs"] // tile) * B
    return want


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 200])
def test_ragged_last_tile_and_a_last_mask_word_with_bits_beyond_n_docs(n_docs):
    """tile_docs = 64 with n_docs around the tile: every mask case, with the bits of the last word at or beyond n_docs set to 1 on
    purpose -- they allow nothing -- then all of them in one call with unrestricted queries between them."""
    case = _by(f"tile64_n{n_docs}")
    ix, q, k = case["ix"], (case["q_indptr"], case["q_tokens"]), case["k"]
    B = len(q[0]) - 1
    sp = _index(ix, tile_docs=64)
    try:
        keeps = mo.mask_cases(n_docs, seed=n_docs)
        plain = so.topk(ix, *q, k)
        for name, keep in keeps.items():
            want = _check(sp, ix, q, k, mo.table([keep], dirty=True), np.zeros(B, np.int32), 64, name)
            assert name != "all_ones" or so.same(want, plain)
            assert name != "empty" or ((want[0] == -1).all() and sp.get_option("masked_tiles_last") == sp.get_option("tiles_last"))
        last = np.zeros(n_docs, bool)
        last[-1] = True                                                         # the last document alone: the ragged word's highest live bit
        masks = mo.table(list(keeps.values()) + [last], dirty=True)
        _check(sp, ix, q, k, masks, ((np.arange(B) * 5) % 6 - 1).astype(np.int32), 64, "mixed")
        assert sp.get_option("masked_calls") == 5 == sp.get_option("calls")
    finally:
        sp.close()


@pytest.mark.parametrize("name", ["tile_default_n8193", "tile_max_n20000", "k1024_tile64", "order_of_additions", "batch500"])
def test_larger_indexes_under_the_four_masks(name):
    case = _by(name)
    ix, q, k = case["ix"], (case["q_indptr"], case["q_tokens"]), case["k"]
    B = len(q[0]) - 1
    tile = case["tile_docs"] or so.DEFAULT_TILE
    sp = _index(ix, tile_docs=case["tile_docs"])
    try:
        keeps = mo.mask_cases(ix["n_docs"], seed=len(name))
        masks = mo.table(list(keeps.values()), dirty=True)
        _check(sp, ix, q, k, masks, ((np.arange(B) * 3) % 5 - 1).astype(np.int32), tile)
        _check(sp, ix, q, k, masks, np.full(B, 2, np.int32), tile, "random_half")
    finally:
        sp.close()


def test_a_tile_that_holds_postings_and_allows_nothing_is_counted_as_masked():
    case = _by("tile64_n200")                                                   # 4 tiles; token 12 has postings in tile 1 only, token 8 everywhere
    ix = case["ix"]
    sp = _index(ix, tile_docs=64)
    try:
        only = lambda *tiles: np.isin(np.arange(200) // 64, tiles)              # noqa: E731
        masks = mo.table([only(0), only(1), only(3), np.zeros(200, bool)], dirty=True)
        q = so.ragged([[12], [12], [12], [8], [8, 12], [11]])
        mask_of = np.array([0, 1, -1, 2, 3, 1], np.int32)
        want = _check(sp, ix, q, 10, masks, mask_of, 64)
        assert mo.tile_counters(ix, *q, 64, masks, mask_of) == (3 + 3 + 0 + 3 + 4 + 3, 1 + 0 + 3 + 0 + 0 + 1)
        assert (want[0][0] == -1).all() and (want[0][1] >= 0).sum() == 7 and (want[0][3] >= 192).sum() == 8 and (want[0][4] == -1).all()
    finally:
        sp.close()


def test_more_positive_documents_than_k_but_fewer_allowed_ones_and_a_tie_run_cut_by_k():
    """The tie_run index: 500 rows tied at 1.25.  A mask that keeps 5 of the tied rows of one tile, at k = 37 -- the tile has more
    positive documents than k and fewer allowed positive ones: a count taken before the mask would promise candidates that the selection
    after it never writes.  Then a mask that keeps 300 of the tied rows, cut by k inside the run over several tiles."""
    case = _by("tie_run_k37")
    ix, q = case["ix"], (case["q_indptr"], case["q_tokens"])
    tied = ix["rows"][ix["indptr"][0]: ix["indptr"][1]]
    tile = np.bincount(tied // 64).argmax()                                     # the tile with the most tied rows
    in_tile = tied[tied // 64 == tile]
    assert len(in_tile) > 37 and len(tied) == 500
    five = np.zeros(700, bool)
    five[in_tile[::len(in_tile) // 5][:5]] = True
    many = np.zeros(700, bool)
    many[tied[::5]] = True
    many[tied[1::5]] = True
    many[tied[2::5]] = True
    sp = _index(ix, tile_docs=64)
    try:
        masks = mo.table([five, many], dirty=True)
        want = _check(sp, ix, q, 37, masks, np.array([0, 0, 0], np.int32), 64, "five")
        assert (want[0][0] >= 0).sum() == 5 and set(want[0][0][:5]) == set(np.flatnonzero(five))
        for k in (37, 100, 299, 300, 301):
            want = _check(sp, ix, q, k, masks, np.array([1, 1, 0], np.int32), 64, k)
            assert (want[0][0] >= 0).sum() == min(k, 300) and (want[1][0][:min(k, 300)] == 1.25).all() and (np.diff(want[0][0][:min(k, 300)]) < 0).all()
    finally:
        sp.close()


def test_k_1_and_k_1024_under_a_half_mask_and_the_specials_allowed_and_disallowed():
    case = _by("k1024_tile64")
    ix, q = case["ix"], (case["q_indptr"], case["q_tokens"])
    B = len(q[0]) - 1
    sp = _index(ix, tile_docs=64)
    try:
        half = mo.table([mo.mask_cases(ix["n_docs"], seed=1)["random_half"]], dirty=True)
        for k in (1, 1024):
            want = _check(sp, ix, q, k, half, np.zeros(B, np.int32), 64, k)
            assert k == 1 or (want[0] >= 0).sum(axis=1).max() == 1024
    finally:
        sp.close()
    case = _by("cancel_negative_nan_inf")                                       # rows 2 and 4 can be NaN, rows 3 and 4 +inf
    ix, q = case["ix"], (case["q_indptr"], case["q_tokens"])
    sp = _index(ix, tile_docs=64)
    try:
        hide = lambda *rows: ~np.isin(np.arange(140), rows)                      # noqa: E731
        masks = mo.table([hide(), hide(3), hide(2, 4), hide(3, 4, 2), ~hide(3, 4, 2), hide(9, 8, 130)], dirty=True)
        for m in range(6):
            want = _check(sp, ix, q, 10, masks, np.full(6, m, np.int32), 64, m)
            if m == 1:
                assert want[0][0].tolist()[:3] == [9, 8, -1]                    # the +inf row hidden: the next ones move up
            if m == 4:
                assert want[0][0].tolist()[:2] == [3, -1] and want[1][0][0] == np.inf
    finally:
        sp.close()


def test_a_query_of_300_tokens_under_masks():
    case = _by("query_of_300_tokens")
    ix, q = case["ix"], (case["q_indptr"], case["q_tokens"])
    sp = _index(ix, tile_docs=64)
    try:
        keeps = mo.mask_cases(300, seed=3)
        _check(sp, ix, q, case["k"], mo.table(list(keeps.values()), dirty=True), np.array([2, 3, 0, 2], np.int32), 64)
    finally:
        sp.close()


def test_a_batch_of_70_over_5_masks_in_one_three_and_seventy_rounds_and_at_four_tile_sizes():
    """mask_of in scrambled order with -1 and repeats: it is indexed by the query's position in the CALL, whatever the round."""
    ix = so.batch_index()
    q = so.queries(np.random.default_rng(70), 40, 70)
    rng = np.random.default_rng(9)
    keeps = [rng.random(2000) < p for p in (0.5, 0.1, 0.9)] + [np.arange(2000) // 250 == 3, np.arange(2000) % 7 == 0]
    masks = mo.table(keeps, dirty=True)
    mask_of = rng.integers(-1, 5, 70).astype(np.int32)
    assert set(mask_of.tolist()) == {-1, 0, 1, 2, 3, 4}
    sp = _index(ix, tile_docs=256)
    try:
        want = _check(sp, ix, q, 20, masks, mask_of, 256)
        assert sp.get_option("rounds_last") == 1 and not so.same(want, so.topk(ix, *q, 20))
        for cap, rounds in ((30 * 1920, 3), (1, 70), (0, 1)):                   # 8 tiles x 20 x 12 bytes = 1 920 bytes per query
            sp.set_option("cand_cap", cap)
            assert so.same(_check(sp, ix, q, 20, masks, mask_of, 256, cap), want) and sp.get_option("rounds_last") == rounds
        for tile in (64, 128, 4096, 8192):
            sp.set_option("tile_docs", tile)
            assert so.same(_check(sp, ix, q, 20, masks, mask_of, tile, tile), want)
    finally:
        sp.close()


def test_all_ones_is_the_unmasked_call_and_an_unmasked_call_after_a_masked_one_is_that_of_a_fresh_handle():
    case = _by("tile64_n200")
    ix, q, k = case["ix"], (case["q_indptr"], case["q_tokens"]), case["k"]
    B = len(q[0]) - 1
    fresh = _index(ix, tile_docs=64)
    sp = _index(ix, tile_docs=64)
    try:
        plain = fresh.topk(*q, B, k)
        fresh_skipped = fresh.get_option("skipped_tiles_last")
        assert fresh.get_option("masked_tiles_last") == 0 and fresh.get_option("masked_calls") == 0 and so.same(plain, so.topk(ix, *q, k))
        ones = mo.table([np.ones(200, bool)])
        assert so.same(sp.topk(*q, B, k, masks=ones, mask_of=np.zeros(B, np.int32)), plain)
        assert sp.get_option("masked_tiles_last") == 0 and sp.get_option("skipped_tiles_last") == fresh_skipped
        assert so.same(sp.topk(*q, B, k, mask_of=np.full(B, -1, np.int32)), plain)               # no table, every query unrestricted
        empty = mo.table([np.zeros(200, bool)], dirty=True)
        assert (sp.topk(*q, B, k, masks=empty, mask_of=np.zeros(B, np.int32))[0] == -1).all() and sp.get_option("masked_tiles_last") == 4 * B
        assert so.same(sp.topk(*q, B, k), plain)                                                   # the unmasked call, after masked ones
        assert sp.get_option("masked_tiles_last") == 0 and sp.get_option("skipped_tiles_last") == fresh_skipped
        assert sp.get_option("calls") == 4 and sp.get_option("masked_calls") == 3 and fresh.get_option("calls") == 1
    finally:
        sp.close()
        fresh.close()


def test_device_form_on_a_side_stream_and_an_out_of_range_mask_of_entry_is_padding():
    import torch
    case = _by("tile64_n200")
    ix = case["ix"]
    sp = _index(ix, tile_docs=64)
    try:
        q_indptr, q_tokens = so.ragged([[8, 10], [8], [9, 9], [8, 12], [], [0, 1, 2], [8]])
        B, k = 7, 10
        keeps = mo.mask_cases(200, seed=2)
        masks = mo.table([keeps["random_half"], keeps["one_row"]], dirty=True)
        mask_of = np.array([0, 2, -1, 1, 0, -2, 1 << 30], np.int32)            # 2, -2 and 2^30 are outside [-1, 2): they allow nothing
        want = mo.topk(ix, q_indptr, q_tokens, k, masks, mask_of)
        assert (want[0][[1, 5, 6]] == -1).all() and (want[1][[1, 5, 6]] == 0.0).all() and (want[0][0] >= 0).any() and (want[0][2] >= 0).any()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_ptr = torch.from_numpy(q_indptr).cuda()
            d_tok = torch.from_numpy(q_tokens).cuda()
            d_masks = torch.from_numpy(masks.view(np.int32)).cuda()
            d_mask_of = torch.from_numpy(mask_of).cuda()
            d_rows = torch.full((B, k), 77, dtype=torch.int32, device="cuda")
            d_scores = torch.full((B, k), 7.0, dtype=torch.float64, device="cuda")
            sp.topk_device(d_ptr, d_tok, B, len(q_tokens), k, d_rows, d_scores, stream=stream.cuda_stream, d_masks=d_masks, n_masks=2, d_mask_of=d_mask_of)
            got = (d_rows.cpu().numpy(), d_scores.cpu().numpy())
        stream.synchronize()
        assert so.same(got, want)
        assert (sp.get_option("masked_tiles_last"), sp.get_option("skipped_tiles_last")) == mo.tile_counters(ix, q_indptr, q_tokens, 64, masks, mask_of)
        with pytest.raises(_native.RqError, match="mask_of"):                   # which the blocking form refuses
            sp.topk(q_indptr, q_tokens, B, k, masks=masks, mask_of=mask_of)
    finally:
        sp.close()


def test_refusals():
    ix = _by("tile64_n65")["ix"]
    sp = _index(ix)
    try:
        q = so.ragged([[0, 1], [8]])
        masks = mo.table([np.ones(65, bool), np.zeros(65, bool)])
        ok = np.array([0, 1], np.int32)
        for bad in ([0, 2], [-2, 0], [5, 5]):
            with pytest.raises(_native.RqError, match="mask_of"):
                sp.topk(*q, 2, 5, masks=masks, mask_of=np.array(bad, np.int32))
        with pytest.raises(_native.RqError, match="mask_of"):
            sp.topk(*q, 2, 5, mask_of=ok)                                       # mask 0 of no table
        with pytest.raises(_native.RqError, match="one entry per query"):
            sp.topk(*q, 2, 5, masks=masks, mask_of=np.zeros(3, np.int32))
        with pytest.raises(_native.RqError, match="masks must be"):
            sp.topk(*q, 2, 5, masks=masks[:, :2], mask_of=ok)
        with pytest.raises(_native.RqError, match="without mask_of"):
            sp.topk(*q, 2, 5, masks=masks)
        for B, k in ((2, 0), (2, 1025)):
            with pytest.raises(_native.RqError, match="k "):
                sp.topk(*q, B, k, masks=masks, mask_of=ok)
        with pytest.raises(_native.RqError, match="token id"):
            sp.topk(*so.ragged([[0, ix["n_tokens"]], [1]]), 2, 5, masks=masks, mask_of=ok)
        with pytest.raises(_native.RqError, match="null mask_of"):
            _native._check(sp._lib.rq_sparse_topk_masked_device(sp._h, 1, 1, 1, 0, 1, None, 0, None, 1, 1, None), "rq_sparse_topk_masked_device")
        with pytest.raises(_native.RqError, match="masks without"):
            _native._check(sp._lib.rq_sparse_topk_masked_device(sp._h, 1, 1, 1, 0, 1, None, 2, 1, 1, 1, None), "rq_sparse_topk_masked_device")
        for name in ("masked_calls", "masked_tiles_last"):
            with pytest.raises(_native.RqError):
                sp.set_option(name, 1)
        assert sp.get_option("calls") == 0 and sp.get_option("masked_calls") == 0
        assert so.same(sp.topk(*q, 2, 5, masks=masks, mask_of=ok), mo.topk(ix, *q, 5, masks, ok))   # and the handle still answers
    finally:
        sp.close()


# ---- through the seam ----------------------------------------------------------------------------------------------------------------
def test_bm25_index_masked_gpu_backend_equals_the_host_backend():
    rng = np.random.default_rng(3)
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    bm = si.BM25Index()
    bm.add_documents([si.Document(id=f"p{i}", text=" ".join(f"w{w}" for w in rng.choice(300, rng.integers(12, 31), p=p))) for i in range(3000)])
    qs = [" ".join(f"w{w}" for w in rng.choice(300, rng.integers(1, 10), p=p)) for _ in range(38)] + ["", "zzz unknown words"]
    tenants = [{f"p{i}" for i in range(t, 3000, 4)} for t in range(4)]
    each = [[tenants[0], tenants[1], None, tenants[2], set(), tenants[3], ["p7", "ghost"]][i % 7] for i in range(40)]
    host = bm.search_batch_rows(qs, 50, backend="host", allowed_ids_each=each)
    assert (host[0] >= 0).sum() > 800
    assert so.same(bm.search_batch_rows(qs, 50, backend="gpu", allowed_ids_each=each), host)
    assert so.same(bm.search_batch_rows(qs, 50, backend="auto", allowed_ids_each=each), host)
    sp = bm._csr()["sparse"]
    assert sp.get_option("masked_calls") == 2 and sp.get_option("masked_tiles_last") == 6             # the empty set's six queries, one tile each
    assert bm.search_batch(qs, 7, backend="gpu", allowed_ids_each=each) == [bm.search(q, 7, **si._given(allowed_ids=e)) for q, e in zip(qs, each)]
    assert bm.search_batch(qs, 7, backend="gpu", allowed_ids=tenants[1]) == bm.search_batch(qs, 7, allowed_ids=tenants[1])
