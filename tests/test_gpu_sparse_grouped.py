"""Grouped sparse search on the device (include/rq.h rq_sparse_set_groups, rq_sparse_topk_grouped*, csrc/rq_sparse.hip)
against tests/sparse_grouped_oracle.py: rows, score bits and counts identical, no tolerance.  tests/test_sparse_grouped.py shows that the
oracle is BM25Index._search_distinct, so the device route and the per-query host call share one definition.  tile_docs = 64 makes a few
hundred documents many tiles."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_grouped_oracle as go  # noqa: E402
import sparse_masked_oracle as mo  # noqa: E402
import sparse_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu


def _index(ix, groups=None, **options):
    sp = _native.SparseIndex(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    for name, value in options.items():
        sp.set_option(name, value)
    if groups is not None:
        sp.set_groups(groups)
    return sp


def _check(sp, ix, q, k, groups, masks=None, mask_of=None, what=None):
    B = len(q[0]) - 1
    got = sp.topk_grouped(q[0], q[1], B, k, masks=masks, mask_of=mask_of)
    want = go.topk(ix, q[0], q[1], k, groups, masks, mask_of)
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert go.same(got, want), (what, np.argwhere(got[1].view(np.uint64) != want[1].view(np.uint64))[:5])
    return want


def _every_document(rng, n_docs, extra=()):
    """Token 0 holds every document with a random contribution; `extra` adds more posting lists."""
    return so.csr([(np.arange(n_docs), rng.uniform(0.05, 4.0, n_docs))] + list(extra), n_docs)


def test_a_group_that_spans_five_tiles_with_its_best_document_in_the_last():
    rng = np.random.default_rng(1)
    n = 300
    contrib = rng.uniform(0.05, 3.0, n)
    span = np.array([5, 70, 140, 200, 290])                                      # one document of group 7 in each of the five tiles
    contrib[span] = [3.5, 3.6, 3.7, 3.8, 9.0]                                    # all above everybody else, the best one in the last tile
    ix = so.csr([(np.arange(n), contrib)], n)
    groups = (100 + np.arange(n) // 2).astype(np.int32)
    groups[span] = 7
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, so.ragged([[0], [0, 0]]), 10, groups)
        assert want[0][0][0] == 290 and (groups[want[0][0]] == 7).sum() == 1 and want[2].tolist() == [10, 10]
        assert sp.get_option("grouped") == 1 and sp.get_option("grouped_calls") == 1 == sp.get_option("calls") and sp.get_option("masked_calls") == 0
        assert sp.get_option("final_chunks_last") == 1 and sp.get_option("tiles_last") == 5 * 2
    finally:
        sp.close()


def test_a_tile_in_which_one_group_holds_more_than_k_of_the_best_documents():
    """Group 1 holds the 30 best documents of tile 0 and k = 5 other groups of that tile score lower: without the in-tile collapse the
    tile's five candidates are all of group 1 and four winners are lost."""
    n, k = 100, 5
    contrib = np.full(n, 0.01)
    contrib[:30] = np.linspace(9.0, 8.0, 30)
    contrib[30:35] = [5.0, 4.0, 3.0, 2.0, 1.0]
    ix = so.csr([(np.arange(n), contrib)], n)
    groups = np.full(n, 1, np.int32)
    groups[30:35] = [10, 11, 12, 13, 14]
    groups[35:] = 1
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, so.ragged([[0]]), k, groups)
        assert want[0][0].tolist() == [0, 30, 31, 32, 33] and want[2][0] == 5
    finally:
        sp.close()


def test_exact_ties_between_groups_and_inside_a_group():
    """Every document is tied at 1.25 (one posting list), a second list lifts some to an exactly tied 2.5: a group's representative is
    its largest row, and tied groups come by descending row."""
    n = 200
    lists = [(np.arange(n), np.full(n, 1.25)), (np.arange(0, n, 3), np.full(len(range(0, n, 3)), 1.25))]
    ix = so.csr(lists, n)
    groups = (np.arange(n) // 7).astype(np.int32)                                # groups of seven tied rows, some across a tile boundary
    sp = _index(ix, groups, tile_docs=64)
    try:
        q = so.ragged([[0], [0, 1], [1, 1]])
        for k in (1, 20, 29, 64):
            want = _check(sp, ix, q, k, groups, what=k)
        assert want[2].tolist() == [29, 29, 29]
        assert want[0][0][:3].tolist() == [199, 195, 188]                        # the largest row of groups 28, 27, 26
        assert (want[1][1][:29] == 2.5).all() and want[0][1][0] == 198 and (np.diff(want[0][1][:29]) < 0).all()
    finally:
        sp.close()


def test_ungrouped_documents_are_never_collapsed_and_trivial_tables_are_the_ungrouped_call():
    rng = np.random.default_rng(4)
    n = 300
    ix = so.csr(so.random_lists(rng, n, 12), n)
    q = so.queries(rng, 12, 9)
    groups = np.where(np.arange(n) % 3 == 0, -1, np.arange(n) // 10).astype(np.int32)
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, q, 40, groups)
        assert (groups[want[0][want[0] >= 0]] == -1).sum() > 20 and (want[2] < (so.topk(ix, q[0], q[1], 40)[0] >= 0).sum(axis=1)).any()
        plain = sp.topk(q[0], q[1], 9, 40)
        assert so.same(plain, so.topk(ix, q[0], q[1], 40))
        for table in (np.full(n, -1, np.int32), np.arange(n, dtype=np.int32)[::-1].copy()):
            sp.set_groups(table)
            got = sp.topk_grouped(q[0], q[1], 9, 40)
            assert so.same(got[:2], plain) and np.array_equal(got[2], (plain[0] >= 0).sum(axis=1))
    finally:
        sp.close()


def test_short_results_one_group_and_no_posting():
    rng = np.random.default_rng(5)
    n = 300
    ix = _every_document(rng, n, [(np.zeros(0, np.int32), np.zeros(0)), (np.array([17, 250]), np.array([1.0, 2.0]))])
    q = so.ragged([[0], [1], [], [2], [0, 2]])
    groups = (np.arange(n) % 3).astype(np.int32)
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, q, 10, groups)
        assert want[2].tolist() == [3, 0, 0, 2, 3] and (want[0][1] == -1).all() and (want[1][0][3:] == 0.0).all()
        one = np.full(n, 5, np.int32)
        sp.set_groups(one)                                                       # a second call replaces the table
        want = _check(sp, ix, q, 10, one)
        assert want[2].tolist() == [1, 0, 0, 1, 1]
    finally:
        sp.close()


def test_k_1_and_k_1024_over_more_groups_than_k_in_more_than_one_chunk():
    """9 000 documents in 141 tiles, 1 500 groups of six documents in six different tiles: the 1 024 best candidates name fewer than
    1 024 groups, so the final kernel walks a second chunk."""
    rng = np.random.default_rng(6)
    n = 9000
    ix = _every_document(rng, n)
    groups = (np.arange(n) % 1500).astype(np.int32)
    q = so.ragged([[0], [0, 0]])
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, q, 1024, groups)
        assert want[2].tolist() == [1024, 1024] and sp.get_option("final_chunks_last") >= 2
        want = _check(sp, ix, q, 1, groups)
        assert want[2].tolist() == [1, 1] and sp.get_option("final_chunks_last") == 1
        sp.topk(q[0], q[1], 2, 5)
        assert sp.get_option("final_chunks_last") == 0
    finally:
        sp.close()


@pytest.mark.parametrize("n,tile", [(300, 64), (5000, 4096)])
def test_group_ids_that_are_adverse_for_a_power_of_two_table(n, tile):
    rng = np.random.default_rng(7)
    ix = so.csr(so.random_lists(rng, n, 10), n)
    q = so.queries(rng, 10, 6)
    r = np.arange(n)
    groups = np.where(r % 2 == 0, (r % 701) * 8192, (2 ** 31 - 1) - (r % 17)).astype(np.int64)
    assert groups.max() == 2 ** 31 - 1 and (groups >= 0).all()
    groups = groups.astype(np.int32)
    sp = _index(ix, groups, tile_docs=tile)
    try:
        _check(sp, ix, q, 50, groups)
    finally:
        sp.close()


def test_grouped_and_masked():
    """The best document of group 3 is disallowed: the next allowed one represents it; group 4 is disallowed as a whole; an all-allowing
    mask, an empty mask and an unrestricted query ride in the same call."""
    n = 200
    contrib = np.linspace(4.0, 0.5, n)
    ix = so.csr([(np.arange(n), contrib)], n)
    groups = (np.arange(n) % 10).astype(np.int32)
    custom = np.ones(n, bool)
    custom[3] = False                                                            # the best of group 3
    custom[groups == 4] = False
    masks = mo.table([custom, np.ones(n, bool), np.zeros(n, bool)], dirty=True)
    mask_of = np.array([0, 1, 2, -1], np.int32)
    q = so.ragged([[0]] * 4)
    sp = _index(ix, groups, tile_docs=64)
    try:
        want = _check(sp, ix, q, 10, groups, masks, mask_of)
        assert want[2].tolist() == [9, 10, 0, 10] and 13 in want[0][0] and 3 not in want[0][0] and not (groups[want[0][0][:9]] == 4).any()
        assert np.array_equal(want[0][1], want[0][3]) and sp.get_option("masked_calls") == 1 == sp.get_option("grouped_calls")
        free = _check(sp, ix, q, 10, groups, None, np.full(4, -1, np.int32))     # no table, every query unrestricted
        assert np.array_equal(free[0][0], want[0][3])
    finally:
        sp.close()


def test_results_do_not_depend_on_rounds_or_tile_docs():
    ix = so.batch_index()
    q = so.queries(np.random.default_rng(70), 40, 70)
    rng = np.random.default_rng(9)
    groups = rng.integers(-1, 300, 2000).astype(np.int32)
    masks = mo.table([rng.random(2000) < 0.5, np.arange(2000) % 7 == 0], dirty=True)
    mask_of = rng.integers(-1, 2, 70).astype(np.int32)
    sp = _index(ix, groups, tile_docs=256)
    try:
        want = _check(sp, ix, q, 20, groups, masks, mask_of)
        assert sp.get_option("rounds_last") == 1
        for cap, rounds in ((30 * 1920, 3), (1, 70), (0, 1)):                   # 8 tiles x 20 x 12 bytes = 1 920 bytes per query
            sp.set_option("cand_cap", cap)
            assert go.same(_check(sp, ix, q, 20, groups, masks, mask_of, cap), want) and sp.get_option("rounds_last") == rounds
        for tile, tiles in ((64, 32), (4096, 1), (8192, 1)):                    # 8 192 is clamped to 4 096 by a grouped call
            sp.set_option("tile_docs", tile)
            assert go.same(_check(sp, ix, q, 20, groups, masks, mask_of, tile), want) and sp.get_option("tiles_last") == tiles * 70
    finally:
        sp.close()


def test_device_form_clamps_tokens_and_mask_of_and_needs_a_table():
    import torch
    rng = np.random.default_rng(10)
    n = 200
    ix = so.csr(so.random_lists(rng, n, 9), n)
    groups = (np.arange(n) % 23).astype(np.int32)
    sp = _index(ix, tile_docs=64)
    try:
        q_indptr, q_tokens = so.ragged([[8, 1], [0, 99, -3], [2, 2], [1], [], [0, 1, 2], [3]])   # 99 and -3 are empty posting lists
        B, k = 7, 10
        masks = mo.table([rng.random(n) < 0.5, np.arange(n) < 5], dirty=True)
        mask_of = np.array([0, -1, 2, 1, 0, -2, 1 << 30], np.int32)             # 2, -2 and 2^30 are outside [-1, 2): they allow nothing
        with pytest.raises(_native.RqError, match="no group table"):
            sp.topk_grouped(*so.ragged([[0]]), 1, 5)
        assert sp.get_option("grouped") == 0
        sp.set_groups(groups)
        want = go.topk(ix, q_indptr, q_tokens, k, groups, masks, mask_of)
        assert want[2][[2, 4, 5, 6]].tolist() == [0, 0, 0, 0] and want[2][0] > 0 and want[2][1] > 0
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_ptr = torch.from_numpy(q_indptr).cuda()
            d_tok = torch.from_numpy(q_tokens).cuda()
            d_masks = torch.from_numpy(masks.view(np.int32)).cuda()
            d_mask_of = torch.from_numpy(mask_of).cuda()
            d_rows = torch.full((B, k), 77, dtype=torch.int32, device="cuda")
            d_scores = torch.full((B, k), 7.0, dtype=torch.float64, device="cuda")
            d_count = torch.full((B,), 55, dtype=torch.int32, device="cuda")
            sp.topk_grouped_device(d_ptr, d_tok, B, len(q_tokens), k, d_rows, d_scores, d_count, stream=stream.cuda_stream, d_masks=d_masks, n_masks=2,
                                   d_mask_of=d_mask_of)
            got = (d_rows.cpu().numpy(), d_scores.cpu().numpy(), d_count.cpu().numpy())
        stream.synchronize()
        assert go.same(got, want)
        with pytest.raises(_native.RqError, match="mask_of"):                   # which the blocking form refuses
            sp.topk_grouped(*so.ragged([[0]] * B), B, k, masks=masks, mask_of=mask_of)
        with pytest.raises(_native.RqError, match="token id"):
            sp.topk_grouped(q_indptr, q_tokens, B, k)
        for bad in (np.full(n, -2, np.int32), np.zeros(n - 1, np.int32)):
            with pytest.raises(_native.RqError):
                sp.set_groups(bad)
        assert _native.load_library().rq_sparse_set_groups(sp._h, _native._ptr(groups), n + 1) == -1
        with pytest.raises(_native.RqError, match="out_count"):
            _native._check(sp._lib.rq_sparse_topk_grouped_device(sp._h, 1, 1, 1, 0, 1, None, 0, None, 1, 1, None, None), "rq_sparse_topk_grouped_device")
        for name in ("grouped", "grouped_calls", "final_chunks_last"):
            with pytest.raises(_native.RqError):
                sp.set_option(name, 1)
    finally:
        sp.close()


# ---- through the seam ----------------------------------------------------------------------------------------------------------------
def test_bm25_index_grouped_gpu_backend_equals_the_per_query_host_search():
    rng = np.random.default_rng(3)
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    bm = si.BM25Index()
    bm.add_documents([si.Document(id=f"p{i}", title="" if i % 11 == 0 else f"t{i // 4}", text=" ".join(f"w{w}" for w in rng.choice(300, rng.integers(12, 31), p=p)))
                      for i in range(3000)])
    qs = [" ".join(f"w{w}" for w in rng.choice(300, rng.integers(1, 10), p=p)) for _ in range(22)] + ["", "zzz unknown words"]
    tenants = [{f"p{i}" for i in range(t, 3000, 3)} for t in range(3)]
    each = [[tenants[0], None, tenants[1], set(), tenants[2]][i % 5] for i in range(24)]
    want = [bm.search(q, 7, distinct_by="title") for q in qs]
    assert bm.search_batch(qs, 7, backend="gpu", distinct_by="title") == want and any(want)
    assert bm.search_batch(qs, 7, backend="auto", distinct_by="title") == want == bm.search_batch(qs, 7, distinct_by="title")
    want = [bm.search(q, 7, distinct_by="title", **si._given(allowed_ids=e)) for q, e in zip(qs, each)]
    assert bm.search_batch(qs, 7, backend="gpu", distinct_by="title", allowed_ids_each=each) == want
    assert bm.search_batch(qs, 7, backend="gpu", distinct_by="title", allowed_ids=tenants[1]) == [bm.search(q, 7, distinct_by="title", allowed_ids=tenants[1]) for q in qs]
    host = bm.search_batch_rows(qs, 50, distinct_by="title")
    assert so.same(bm.search_batch_rows(qs, 50, backend="gpu", distinct_by="title"), host) and (host[0] >= 0).sum() > 500
    sp = bm._csr()["sparse"]
    assert sp.get_option("grouped_calls") == 5 and sp.get_option("grouped") == 1
    bm.add_documents([si.Document(id="late", title="t0", text="w1 w2 w3")])    # the table goes with the device index
    assert bm.search_batch(qs, 7, backend="gpu", distinct_by="title") == [bm.search(q, 7, distinct_by="title") for q in qs]
