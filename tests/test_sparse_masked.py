"""Masked sparse search (include/rq_bm25.h rq_bm25_topk_masked, include/rq.h rq_sparse_topk_masked*), the parts that need no GPU: the
yardstick (tests/sparse_masked_oracle.py) against librq_bm25.so bit for bit on every index of sparse_oracle.cases() under four masks,
the numpy and the native branch of BM25Index.search_batch_rows, the batch call against the per-query call it is defined by, the
refusals, the masked scorer under the sanitizers as a stand-alone program, and the header.  The GPU side is tests/test_gpu_sparse_masked.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_masked_oracle as mo  # noqa: E402
import sparse_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
CASES = so.cases()


def test_header_declares_and_documents_the_masked_calls():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in ("rq_sparse_topk_masked", "rq_sparse_topk_masked_device"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES and hasattr(_native.load_library(), name)
    doc = h[h.index("sparse search: exact BM25"):h.index("typedef struct rq_sparse rq_sparse;")]
    for word in ("rq_sparse_topk_masked_device", "ALLOWED SET", "[n_masks][W]", "ceil(n_docs / 32)", "bit r % 32 of word r / 32", "rq_filter_create",
                 "at or beyond n_docs are ignored", "-1 = unrestricted", "mask_of == NULL", "outside [-1, n_masks)", "allows nothing", "BEFORE the score > 0",
                 "ORs the mask words", "before anything is counted or selected", '"masked_calls"', '"masked_tiles_last"', "0 after an unmasked call",
                 "gather route", "rq_sparse_score_rows_device", "distinct_by (it stays on the host)"):
        assert word in doc, word
    assert "Not extended: allowed_ids filters" not in h
    hybrid_doc = h[h.index("hybrid fusion: both pools"):h.index("typedef struct rq_hybrid rq_hybrid;")]
    assert "fused pool, filters" not in hybrid_doc and "distinct_by (it stays on the host)" in hybrid_doc
    b = open(os.path.join(ROOT, "include", "rq_bm25.h")).read()
    assert re.search(r"\brq_bm25_topk_masked\s*\(", re.sub(r"/\*.*?\*/", "", b, flags=re.S)) and "rq_bm25_topk_masked" in _native._BM25_SIGNATURES
    for word in ("[n_masks][W]", "-1 = unrestricted", "BEFORE the score > 0", "outside\n * [-1, n_masks)"):
        assert word in b, word


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_agrees_with_the_host_library_bit_for_bit(case):
    """Every index and query batch of sparse_oracle.cases() under an all-ones mask, an empty mask, a random half and one allowed row
    (the bits of the last word beyond n_docs set on purpose), and all four in one call with unrestricted queries between them."""
    ix = case["ix"]
    h = _native.bm25_create(ix["indptr"], ix["rows"], ix["contrib"], ix["n_tokens"], ix["n_docs"])
    try:
        B, k = len(case["q_indptr"]) - 1, case["k"]
        keeps = mo.mask_cases(ix["n_docs"], seed=len(case["name"]))
        plain = so.topk(ix, case["q_indptr"], case["q_tokens"], k)
        for name, keep in keeps.items():
            masks, mask_of = mo.table([keep], dirty=True), np.zeros(B, np.int32)
            want = mo.topk(ix, case["q_indptr"], case["q_tokens"], k, masks, mask_of)
            if name == "all_ones":
                assert so.same(want, plain)
            if name == "empty":
                assert (want[0] == -1).all()
            for n_threads in (1, 3):
                assert so.same(_native.bm25_topk(h, case["q_indptr"], case["q_tokens"], B, k, n_threads, masks=masks, mask_of=mask_of), want), (name, n_threads)
        masks = mo.table(list(keeps.values()), dirty=True)
        mask_of = ((np.arange(B) * 3) % 5 - 1).astype(np.int32)
        want = mo.topk(ix, case["q_indptr"], case["q_tokens"], k, masks, mask_of)
        assert so.same(_native.bm25_topk(h, case["q_indptr"], case["q_tokens"], B, k, 2, masks=masks, mask_of=mask_of), want)
        # every entry -1, with and without a table: the unmasked call
        free = np.full(B, -1, np.int32)
        assert so.same(_native.bm25_topk(h, case["q_indptr"], case["q_tokens"], B, k, 2, masks=masks, mask_of=free), plain)
        assert so.same(_native.bm25_topk(h, case["q_indptr"], case["q_tokens"], B, k, 2, mask_of=free), plain)
    finally:
        _native.bm25_destroy(h)


def test_the_oracle_holds_what_it_is_meant_to_hold():
    """The mask changes answers (a hidden row makes room for the next), hides a +inf row, and the tile counters tell a masked tile from
    a skipped one."""
    by = {c["name"]: c for c in CASES}
    c = by["cancel_negative_nan_inf"]
    keep = np.ones(140, bool)
    keep[3] = False                                                             # the +inf row of query 0
    rows, sc = mo.topk(c["ix"], c["q_indptr"], c["q_tokens"], c["k"], mo.table([keep]), np.zeros(6, np.int32))
    assert rows[0].tolist()[:3] == [9, 8, -1] and sc[0][0] == 1.5
    c = by["tile64_n200"]                                                       # 4 tiles; token 12 has postings in tile 1 only
    q = so.ragged([[12], [12], [12], [8]])
    only = lambda *tiles: np.isin(np.arange(200) // 64, tiles)                  # noqa: E731
    masks = mo.table([only(0), only(1), only(3)], dirty=True)
    # query 0: tile 0 allowed, no posting there -> 3 masked + 1 skipped; query 1: tile 1 -> 3 masked; query 2 unrestricted -> 3 skipped;
    # query 3: the ragged last tile alone, a token in every document -> 3 masked
    assert mo.tile_counters(c["ix"], *q, 64, masks, np.array([0, 1, -1, 2], np.int32)) == (9, 4)
    rows, _ = mo.topk(c["ix"], *q, 10, masks, np.array([0, 1, -1, 2], np.int32))
    assert (rows[0] == -1).all() and (rows[1] >= 0).sum() == 7 and (rows[3] >= 192).sum() == 8


def test_masked_scorer_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/bm25_masked_check.cpp with csrc/rq_bm25.cpp compiled into it: a stand-alone program under -fsanitize=address,undefined
    (a ragged last mask word in a table allocated exactly, 16 threads); no sanitizer is applied to code loaded into Python."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "bm25_masked_san")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "include"), os.path.join(os.path.dirname(__file__), "native", "bm25_masked_check.cpp"), os.path.join(CSRC, "rq_bm25.cpp"),
                    "-o", exe], check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- through BM25Index ---------------------------------------------------------------------------------------------------------------
def _corpus():
    rng = np.random.default_rng(8)
    p = 1.0 / np.arange(1, 61) ** 0.9
    p /= p.sum()
    docs = [si.Document(id=f"d{i}", text=" ".join(f"w{w}" for w in rng.choice(60, rng.integers(4, 12), p=p))) for i in range(150)]
    docs[40] = si.Document(id="d7", text=docs[7].text + " w1 w2")               # an id twice: the first row is the id's row
    bm = si.BM25Index()
    bm.add_documents(docs)
    qs = [" ".join(f"w{w}" for w in rng.choice(60, rng.integers(1, 7), p=p)) for _ in range(14)] + ["", "zzz unknown words"]
    return bm, qs, rng


def _entries(rng, n):
    tenant_a = {f"d{i}" for i in range(0, 150, 3)}
    tenant_b = [f"d{i}" for i in range(100, 150)] + ["ghost1", "ghost2"]        # unknown ids are ignored
    few = ("d7", "d40", "d149")
    pool = [tenant_a, tenant_b, None, set(), few, ["ghost3"], tenant_a, None]   # shared by object, an empty set, only unknown ids
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def test_batch_search_equals_the_per_query_search_it_is_defined_by():
    bm, qs, rng = _corpus()
    each = _entries(rng, len(qs))
    assert {None if e is None else id(e) for e in each} >= {None} and any(e is not None and len(e) == 0 for e in each)
    for k in (1, 5, 200):
        want = [bm.search(q, k, **si._given(allowed_ids=e)) for q, e in zip(qs, each)]
        assert any(want) and want != [bm.search(q, k) for q in qs]
        assert bm.search_batch(qs, k, allowed_ids_each=each) == want, k
        assert bm.search_batch(qs, k, allowed_ids_each=each, use_native=False) == want, k
        one = each[0] if each[0] is not None else {"d1", "d2", "d100"}
        assert bm.search_batch(qs, k, allowed_ids=one) == [bm.search(q, k, allowed_ids=one) for q in qs] == bm.search_batch(qs, k, allowed_ids_each=[one] * len(qs))
    # every entry None: the unfiltered call
    assert bm.search_batch(qs, 5, allowed_ids_each=[None] * len(qs)) == bm.search_batch(qs, 5)
    # a reusable mask, and what an add does to it
    m = bm.make_mask(each[1] or ["d3"])
    assert bm.search_batch(qs, 5, allowed_ids=m) == bm.search_batch(qs, 5, allowed_ids=each[1] or ["d3"])
    bm.add_documents([si.Document(id="late", text="w1 w2 w3")])
    with pytest.raises(_native.RqError, match="stale"):
        bm.search_batch(qs, 5, allowed_ids=m)


def test_numpy_branch_and_native_branch_agree_on_rows_and_bits():
    bm, qs, rng = _corpus()
    each = _entries(rng, len(qs))
    for k in (3, 60):
        native = bm.search_batch_rows(qs, k, allowed_ids_each=each, use_native=True)
        assert so.same(bm.search_batch_rows(qs, k, allowed_ids_each=each, use_native=False), native) and (native[0] >= 0).any()
        assert so.same(bm.search_batch_rows(qs, k, allowed_ids_each=each, n_threads=16), native)
        # and both are the oracle's answer over the index's own arrays
        c = bm._csr()
        ix = {"indptr": c["indptr"], "rows": c["rows"], "contrib": c["contrib"], "n_tokens": len(c["tid"]), "n_docs": c["n_docs"]}
        masks, mask_of = bm._mask_table(each)
        assert masks.shape == (len({id(e) for e in each if e is not None}), mo.words(150))          # one mask per distinct object
        tid = c["tid"]
        q = so.ragged([[tid[t] for t in bm._tokenize(x) if t in tid] for x in qs])
        assert so.same(native, mo.topk(ix, *q, k, masks, mask_of))


def test_refusals():
    bm, qs, _ = _corpus()
    with pytest.raises(ValueError, match="allowed_ids_each does not combine with allowed_ids"):
        bm.search_batch(qs, 3, allowed_ids={"d1"}, allowed_ids_each=[None] * len(qs))
    with pytest.raises(ValueError, match="allowed_ids_each does not combine with allowed_ids"):
        bm.search_batch_rows(qs, 3, allowed_ids={"d1"}, allowed_ids_each=[None] * len(qs))
    with pytest.raises(ValueError, match="one entry per query"):
        bm.search_batch(qs, 3, allowed_ids_each=[None] * (len(qs) - 1))
    with pytest.raises(ValueError, match="one entry per query"):
        si.BM25Index().search_batch(qs, 3, allowed_ids_each=[None])                                  # checked on an empty index too
    c = bm._csr()
    q = so.ragged([[0], [1]])
    masks = mo.table([np.ones(150, bool)])
    for bad in ([0, 1], [-2, 0], [0, 7]):
        with pytest.raises(_native.RqError, match="masked"):
            _native.bm25_topk(c["handle"], *q, 2, 3, masks=masks, mask_of=np.array(bad, np.int32))
    with pytest.raises(_native.RqError, match="one entry per query"):
        _native.bm25_topk(c["handle"], *q, 2, 3, masks=masks, mask_of=np.zeros(3, np.int32))
    with pytest.raises(_native.RqError, match="masks must be"):
        _native.bm25_topk(c["handle"], *q, 2, 3, masks=masks[:, :-1], mask_of=np.zeros(2, np.int32))
    with pytest.raises(_native.RqError, match="without mask_of"):
        _native.bm25_topk(c["handle"], *q, 2, 3, masks=masks)
    with pytest.raises(_native.RqError):
        _native.bm25_topk(c["handle"], *q, 2, 3, mask_of=np.zeros(2, np.int32))                      # mask 0 of no table
    lib = _native.load_library()
    assert lib.rq_sparse_topk_masked(None, None, None, 1, 1, None, 0, None, None, None) == -1
    assert lib.rq_sparse_topk_masked_device(None, None, None, 1, 0, 1, None, 0, None, None, None, None) == -1
