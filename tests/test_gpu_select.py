"""The workgroup top-m, the generic sorted tail, the repair ladder and its last rung (csrc/rq_select.hip, rq_exact.hip, rq_search.hip
fixup_ladder) against their host model (tests/select_oracle.py) on planted corpora (tests/select_cases.py; tests/test_select_oracle.py
shows on the CPU that every geometry is structured as named and decided, and that each assertion rejects a wrong certificate).

(a) rq_wg_topm through rq_merge_keys_device: every chunk, threshold and compaction path against the host sort.
(b) The generic tail: rq_search_device WITHOUT rq_search_fixup_device under "fast_tail" = 0 and "scan8" = 0, then rq_debug_bin_records of
    that call.  The tail is a function of those records, so per query
      (b1) unrepaired status = the model's (never undecided on a planted query)
      (b2) unrepaired rows and scores = the model's top k of the re-scored bins; status 0: = the oracle's
      (b3) the status is the certificate evaluated on the records' (nb+1)-th maximum and the kernel's OWN k-th score: no rounding left
           to argue about, so this one is decided for every query
      (b4) the widened pass, run as a call of its own ("slack_bins" = nb1 - k on the uncertified queries), says what the model says
      (b5) after rq_search_fixup_device every query equals the oracle
      (b6) "widened", "exact_scans", "repaired_queries" and the return value moved by exactly the model's counts.
(c) rq_exact_scan_kernel / rq_rescore_kernel as the exact route at the tile and query-group edges, "cu_count" = 2.
"""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat
from rag_uq_amd import distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_oracle as nfo  # noqa: E402
import select_cases as sc  # noqa: E402
import select_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6          # tests/test_gpu_parity.py
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
GUARD = 16


# ====================================================================================================================================
# (a) the workgroup top-m
# ====================================================================================================================================
def _distinct_keys(n, rng, specials=True, equal_chunk=False):
    """n distinct non-empty keys, unordered: distinct scores (never +-0.0) with +inf, -inf and -0.0 among them, distinct rows up to
    2^32 - 2.  equal_chunk: keys 1024 .. 2047 share ONE score and differ only in the row field."""
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    s = ((np.arange(n, dtype=np.float64) - n / 2 + 0.25) * 1e-3).astype(np.float32)
    s = s[rng.permutation(n)]
    if specials and n >= 3:
        s[0], s[1], s[2] = np.inf, -np.inf, -0.0
    if equal_chunk and n > 1024:
        s[1024:2048] = np.float32(0.123)
    u = np.unique(rng.integers(1, 2**32 - 2, size=2 * n + 16, dtype=np.int64))
    rows = rng.permutation(u)[:n]
    if n >= 2:
        rows[0], rows[n - 1] = 2**32 - 2, 0
    keys = dist.pack_keys(s, rows)
    assert np.unique(keys).size == n and (keys != 0).all()
    return keys


def _ordered(keys, order, rng):
    if order == "ascending":
        return np.sort(keys)
    if order == "descending":
        return np.sort(keys)[::-1].copy()
    return keys[rng.permutation(keys.size)] if order == "shuffled" else keys      # "equal chunk": as generated


def _merge_on_device(keys, k, with_keys_out, stream=None):
    """keys [B][n] uint64 -> (scores, rows, keys or None) of rq_merge_keys_device, with guard words after every output checked."""
    import torch
    B, n = keys.shape
    d_in = torch.from_numpy(np.ascontiguousarray(keys if n else np.zeros((B, 1), np.uint64)).view(np.int64)).cuda()
    d_s = torch.full((B * k + GUARD,), -777.25, device="cuda", dtype=torch.float32)
    d_r = torch.full((B * k + GUARD,), -12345, device="cuda", dtype=torch.int64)
    d_k = torch.full((B * k + GUARD,), 0x5A5A5A5A5A5A5A5A, device="cuda", dtype=torch.int64)
    torch.cuda.synchronize()
    nat.merge_keys_device(d_in, n, B, k, d_s, d_r, d_k if with_keys_out else None, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    s, r, ko = d_s.cpu().numpy(), d_r.cpu().numpy(), d_k.cpu().numpy()
    assert (s[B * k:] == np.float32(-777.25)).all() and (r[B * k:] == -12345).all() and (ko[B * k:] == 0x5A5A5A5A5A5A5A5A).all(), "guard words overwritten"
    if not with_keys_out:
        assert (ko == 0x5A5A5A5A5A5A5A5A).all()
    return s[:B * k].reshape(B, k), r[:B * k].reshape(B, k), (ko[:B * k].view(np.uint64).reshape(B, k) if with_keys_out else None)


def _check_merge(keys, k, with_keys_out, what, stream=None):
    want_s, want_r, want_k = so.merge(keys, k)
    host_s, host_r = dist.merge_keys_host(keys, k)
    assert np.array_equal(host_r, want_r) and np.array_equal(host_s.view(np.uint32), want_s.view(np.uint32)), f"{what}: merge_keys_host differs from the sort"
    s, r, ko = _merge_on_device(keys, k, with_keys_out, stream)
    assert np.array_equal(r, want_r), f"{what}: rows differ at (query, rank) {np.argwhere(r != want_r)[:4].tolist()}"
    assert np.array_equal(s.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores differ at {np.argwhere(s.view(np.uint32) != want_s.view(np.uint32))[:4].tolist()}"
    if with_keys_out:
        assert np.array_equal(ko, want_k), f"{what}: keys differ"


MERGE_N = [0, 1, 1023, 1024, 1025, 3072, 3073, 4096, 4097, 8192, 65536]
MERGE_K = [1, 2, 1023, 1024]


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled", "equal chunk"])
def test_workgroup_topm_through_the_key_merge(order):
    """ascending: every chunk passes the running threshold, the list fills to exactly 4 096 (k = 1 024) and is compacted again and again;
    descending: nothing survives the first threshold; equal chunk: 1 024 keys that differ only in their row field.  B = 3 with different
    content per query and d_keys_out given, B = 1 with d_keys_out NULL."""
    rng = np.random.default_rng(20501)
    for n in MERGE_N:
        per_q = [_ordered(_distinct_keys(n, rng, equal_chunk=(order == "equal chunk")), order, rng) for _ in range(3)]
        keys = np.stack(per_q) if n else np.zeros((3, 0), np.uint64)
        for k in MERGE_K:
            _check_merge(keys, k, True, f"{order}, n = {n}, k = {k}, B = 3")
            _check_merge(keys[1:2], k, False, f"{order}, n = {n}, k = {k}, B = 1")


def test_key_merge_with_empty_slots_and_on_a_side_stream():
    import torch
    rng = np.random.default_rng(20502)
    for n in (1025, 4097, 8192):
        keys = np.stack([_distinct_keys(n, rng)[rng.permutation(n)] for _ in range(3)])
        keys[0, ::2] = 0                                # zeros interleaved
        keys[1, :] = 0                                  # all zeros: -1 rows, 0.0 scores, empty keys
        keys[2, 7:n - 5] = 0                            # 12 non-empty keys in the first and the last chunk: fewer than k
        for k in (1, 2, 1023, 1024):
            _check_merge(keys, k, True, f"empty slots, n = {n}, k = {k}")
        s, r, _ = _merge_on_device(keys, 1024, True)
        assert (r[1] == -1).all() and (s[1] == 0).all() and (r[2, 12:] == -1).all() and (r[2, :12] >= 0).all()
    side = torch.cuda.Stream()
    keys = np.stack([np.sort(_distinct_keys(8192, rng)) for _ in range(3)])
    _check_merge(keys, 1024, True, "side stream, ascending, n = 8192, k = 1024", stream=side)
    _check_merge(keys, 1023, False, "side stream, ascending, n = 8192, k = 1023", stream=side)


# ====================================================================================================================================
# (b) the generic tail and the ladder
# ====================================================================================================================================
class Bufs:
    def __init__(self, q, k):
        import torch
        self.B, self.k = q.shape[0], k
        self.q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
        self.sc = torch.full((self.B, k), -5.5, device="cuda")
        self.rw = torch.full((self.B, k), -9, device="cuda", dtype=torch.int64)
        self.st = torch.full((self.B,), -7, device="cuda", dtype=torch.int32)

    def search(self, idx, metric, flt=None):
        idx.search_device(self.q, self.B, self.k, metric, self.sc, self.rw, None, self.st, 0, row_filter=flt)

    def fixup(self, idx, metric, flt=None):
        return idx.search_fixup_device(self.q, self.B, self.k, metric, self.sc, self.rw, None, self.st, 0, row_filter=flt)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.st.cpu().numpy().copy(), self.sc.cpu().numpy().copy(), self.rw.cpu().numpy().copy()


class Shard:
    """One index that always takes the generic tail ("fast_tail" = 0, "scan8" = 0)."""

    def __init__(self, x, row_pad=None):
        self.x = x
        self.n, self.dim = x.shape
        self.nbins = (self.n + 63) // 64
        self.idx = nat.NativeIndex(self.dim, 0)
        if row_pad:
            self.idx.set_option("row_pad", row_pad)
        self.idx.add_f16(x)
        self.idx.set_option("scan8", 0)
        self.idx.set_option("fast_tail", 0)
        self.mrn = float(self.idx.get_option("max_row_norm"))

    def eps(self, metric):
        return float(self.idx.get_option("eps_cosine" if metric == COS else "eps_ip"))

    def counters(self):
        t = self.idx.timing()
        return np.array([t["widened"], t["exact_scans"], int(self.idx.get_option("repaired_queries"))])

    def close(self):
        self.idx.close()


def _same(got_s, got_r, want_s, want_r, what):
    nfo.assert_matches(got_s, got_r, want_s, want_r, SCORE_TOL, what)


def _one_pass(sh, q, k, metric, nb, flt, allowed, what, planted=()):
    """One unrepaired call and its records against the model: (b1) - (b3).  Returns (status [B], bufs, models)."""
    bufs = Bufs(q, k)
    bufs.search(sh.idx, metric, flt)
    st, s, r = bufs.read()
    B = q.shape[0]
    assert set(np.unique(st).tolist()) <= {0, 1}, f"{what}: status {st.tolist()}"
    models = []
    if so.exact_route(nb, sh.nbins):
        assert (st == 0).all(), f"{what}: the exact route left status {st.tolist()}"
        return st, bufs, [None] * B
    rec = sh.idx.debug_bin_records(0, B)
    assert rec.shape == (B, sh.nbins, 2)
    eps = sh.eps(metric)
    for j in range(B):
        m = so.generic_tail(rec[j], sh.x, q[j], k, nb, metric, eps, sh.mrn, allowed=allowed)
        models.append(m)
        print(f"[select] {what} q{j}: status {int(st[j])} model {m['status']} ({m['why']}, margin {m['margin']} ulps)")
        assert m["status"] is not None or j not in planted, f"{what}: planted query {j} is undecided (margin {m['margin']} ulps)"
        if m["status"] is not None:
            assert int(st[j]) == m["status"], f"(b1) {what}: query {j} status {int(st[j])}, model {m['status']} ({m['why']}, margin {m['margin']} ulps)"
        _same(s[j:j + 1], r[j:j + 1], m["scores"][None, :], m["rows"][None, :], f"(b2) {what}: query {j} (unrepaired)")
        if m["why"] == "certificate":       # (b3): the records' (nb+1)-th maximum against the kernel's own k-th score
            ok, fb = so.certified(m["b"], eps, np.float32(sh.mrn * (1.0 + 1e-6)), float(np.sqrt((q[j].astype(np.float64) ** 2).sum())), metric, s[j, m["kk"] - 1])
            assert int(st[j]) == (0 if ok else 1), f"(b3) {what}: query {j} status {int(st[j])}, bound {fb!r} against the kernel's s_k {s[j, m['kk'] - 1]!r}"
    return st, bufs, models


def run_ladder(sh, q, k, metric, what, slack=-1, allowed=None, planted=(), named=None, blocking=True):
    """(b1) - (b6) for one call.  named: {query: (first status, widened status or None)}.  Returns the counts."""
    idx = sh.idx
    flt = idx.make_filter(allowed) if allowed is not None else None
    B = q.shape[0]
    if allowed is None:
        gold = orc.topk_from_scores(nfo.scores(q, sh.x, metric), k)
    else:
        gold = nfo.topk(q, sh.x, k, metric, mask=allowed)
    nb, nb1 = so.nb_default(k, slack), so.nb_widened(k, slack)
    try:
        idx.set_option("slack_bins", slack)
        st, bufs, models = _one_pass(sh, q, k, metric, nb, flt, allowed, what, planted)
        _, s, r = bufs.read()
        good = st == 0
        _same(s[good], r[good], gold[0][good], gold[1][good], f"(b2) {what}: certified queries against the oracle")
        bad = np.nonzero(st != 0)[0]
        undecided = [j for j in range(B) if models[j] is not None and models[j]["status"] is None]
        st_w = {}
        if bad.size:                                   # (b4) the widened pass as a call of its own: the same queries, the same cut into passes
            idx.set_option("slack_bins", nb1 - k)
            stw, _, _ = _one_pass(sh, q[bad], k, metric, nb1, flt, allowed, f"{what}, widened", planted=[i for i, j in enumerate(bad) if int(j) in set(planted)])
            st_w = {int(j): int(stw[i]) for i, j in enumerate(bad)}
            for i, j in enumerate(bad):
                if named and int(j) in named and named[int(j)][1] is not None:
                    assert int(stw[i]) == named[int(j)][1], f"{what}: query {j} widened status {int(stw[i])}, named {named[int(j)][1]}"
            idx.set_option("slack_bins", slack)
        for j, (first, _) in (named or {}).items():
            assert first is None or int(st[j]) == first, f"{what}: query {j} status {int(st[j])}, named {first}"
        want = so.ladder_counts(st, st_w)
        c0 = sh.counters()
        fixed = bufs.fixup(idx, metric, flt)
        c1 = sh.counters()
        st2, s, r = bufs.read()
        assert (st2 == 0).all(), f"(b5) {what}: status after the fixup {st2.tolist()}"
        _same(s, r, gold[0], gold[1], f"(b5) {what}: after the fixup")
        moved = (c1 - c0).tolist()
        print(f"[select] {what}: first-pass status {st.tolist() if B <= 16 else int(st.sum())}, widened status {st_w if B <= 16 else sum(st_w.values())}; "
              f"widened / exact_scans / repaired moved by {moved}, model {[want['widened'], want['exact_scans'], want['repaired']]}, {len(undecided)} undecided")
        assert fixed == want["repaired"] and moved == [want["widened"], want["exact_scans"], want["repaired"]], \
            f"(b6) {what}: fixup returned {fixed}, counters moved by {moved}, model {want}"
        if blocking and allowed is None:               # the blocking call: only the counters and the answers
            c0 = sh.counters()
            bs, br_ = idx.search(q, k, metric)
            moved = (sh.counters() - c0).tolist()
            _same(bs, br_, gold[0], gold[1], f"{what}: blocking rq_search")
            assert moved == [want["widened"], want["exact_scans"], want["repaired"]], f"(b6) {what}: blocking rq_search moved the counters by {moved}, model {want}"
        return want
    finally:
        idx.set_option("slack_bins", -1)
        if flt is not None:
            flt.close()


def _named(cases, metric):
    return {c["q"]: (c["status"][metric], c["widened"][metric]) for c in cases}


@pytest.mark.parametrize("dim,row_pad", [(768, None), (384, 384)], ids=["wide", "narrow"])
@pytest.mark.parametrize("metric", [COS, IP], ids=["cosine", "ip"])
def test_generic_tail_and_ladder_on_the_planted_corpora(dim, row_pad, metric):
    """Every geometry of tests/select_cases.py: separated, tied shelf (widened by one, no exact scan), wide tied shelf (one exact scan),
    ladder steps, k-th gap, tiny query; short of rows (a filter, "filter_route" 2); all-negative separated and tied shelf."""
    x, q, cases = sc.main_corpus(dim)
    sh = Shard(x, row_pad=row_pad)
    try:
        assert sh.idx.row_pad == (row_pad or 768)
        want = run_ladder(sh, q, sc.K, metric, f"planted, dim {dim}, metric {metric}", planted=range(len(cases)), named=_named(cases, metric))
        by = {c["name"]: c["q"] for c in cases}
        assert {by["tied shelf"], by["wide tied shelf"], by["k-th gap"]} <= set(want["bad"]) and by["separated"] not in want["bad"]
        assert by["wide tied shelf"] in want["exact"] and by["tied shelf"] not in want["exact"] and by["k-th gap"] not in want["exact"]
        # short of rows: 12 rows allowed, 9 of them in the bins either pass re-scores
        allowed = sc.short_filter({c["name"]: c for c in cases})
        sh.idx.set_option("filter_route", 2)
        try:
            w = run_ladder(sh, q[:1], sc.K, metric, f"short of rows, dim {dim}, metric {metric}", allowed=allowed, planted=[0], named={0: (1, 1)})
            assert int(sh.idx.get_option("filter_route_last")) == 2 and (w["widened"], w["exact_scans"]) == (1, 1)
        finally:
            sh.idx.set_option("filter_route", -1)
    finally:
        sh.close()
    for corpus in (sc.negative_separated(dim), sc.negative_shelf_corpus(dim)):
        x, q, cases = corpus
        sh = Shard(x, row_pad=row_pad)
        try:
            assert nfo.scores(q, x, metric).max() < 0
            w = run_ladder(sh, q, sc.K, metric, f"{cases[0]['name']}, dim {dim}, metric {metric}", planted=[0], named=_named(cases, metric))
            assert (w["widened"], w["exact_scans"]) == ((1, 0) if cases[0]["tie"] else (0, 0))
        finally:
            sh.close()


@pytest.mark.parametrize("dim,row_pad", [(768, None), (384, 384)], ids=["wide", "narrow"])
def test_130_queries_take_a_wide_and_a_64_query_pass(dim, row_pad):
    """Records of a 128-query pass (queries 0 .. 127) and of a 64-query pass (128, 129): the planted queries sit in the first, the tied
    shelf and the separated one once more in the second; Gaussian queries fill the rest (their status is whatever the records say)."""
    x, pq, cases = sc.main_corpus(dim)
    by = {c["name"]: c for c in cases}
    q = sc.filler_queries(130, dim)
    q[:pq.shape[0]] = pq
    q[128], q[129] = pq[by["tied shelf"]["q"]], pq[by["separated"]["q"]]
    named = _named(cases, COS)
    named[128], named[129] = named[by["tied shelf"]["q"]], named[by["separated"]["q"]]
    sh = Shard(x, row_pad=row_pad)
    sh.idx.set_option("wide_batch", 3)           # passes of 128 and 64 queries (the default cuts 130 queries into one 256-query pass)
    try:
        want = run_ladder(sh, q, sc.K, COS, f"130 queries, dim {dim}", planted=list(range(pq.shape[0])) + [128, 129], named=named, blocking=False)
        assert 128 in want["bad"] and 128 not in want["exact"] and 129 not in want["bad"]
    finally:
        sh.close()


def test_small_shards_and_small_k():
    """k = 1 and k = 3 with "slack_bins" 0 (nb = 1, nb = 3): 3 and 7 bins are the smallest shards that are not the exact route, 2 and 6 bins
    must take it and report status 0."""
    for c in sc.SMALL:
        x, q = sc.small_corpus(c["nbins"])
        sh = Shard(x)
        try:
            want = run_ladder(sh, q, c["k"], COS, f"small: k {c['k']}, {c['nbins']} bins", slack=0)
            assert want["exact_scans"] == 0 and (not c["exact"] or want["widened"] == 0)      # (the widened pass is the exact route: nothing reaches the last rung)
        finally:
            sh.close()


def test_k_321_takes_the_generic_tail_by_default():
    """k above RQ_FAST_MAX_K: the generic tail is the first pass whatever "fast_tail" says; 723 bins, nb = 361, m = 362."""
    x, q = sc.k321_corpus()
    sh = Shard(x)
    sh.idx.set_option("fast_tail", 1)
    try:
        assert sh.nbins == sc.K321_BINS
        run_ladder(sh, q, 321, COS, "k = 321")
    finally:
        sh.close()


def test_k_1024_walks_the_whole_ladder_at_its_largest_lists():
    """eps = 10: nothing certifies.  6 143 bins: the widened pass is still approximate, rq_select_bins_kernel at m = 3 072 and rq_final_kernel
    over 3 071 x 64 = 196 544 candidate keys; then the exact scan.  dim 32 under "row_pad" 384."""
    x, q = sc.k1024_corpus()
    sh = Shard(x, row_pad=384)
    sh.idx.set_option("eps", 10.0)
    try:
        assert sh.nbins == sc.K1024_BINS and so.nb_widened(1024) + 1 == 3072
        want = run_ladder(sh, q, 1024, COS, "k = 1024, eps 10", named={0: (1, 1), 1: (1, 1)}, blocking=False)
        assert (want["widened"], want["exact_scans"]) == (2, 2)
    finally:
        sh.close()


def test_certificate_at_exact_equality():
    """`<` not `<=`: with "eps" chosen so that fp32(b + eps) EQUALS the kernel's own s_k the call must not certify; one fp32 step less and it
    must.  (The scan does not read eps: the records, b and s_k are the same in every call.)"""
    x, q, cases = sc.main_corpus(768)
    qi = {c["name"]: c["q"] for c in cases}["separated"]
    sh = Shard(x)
    try:
        st, bufs, models = _one_pass(sh, q[qi:qi + 1], sc.K, COS, sc.NB, None, None, "equality, default eps", planted=[0])
        _, s, _ = bufs.read()
        b, sk = models[0]["b"], np.float32(s[0, sc.K - 1])
        assert int(st[0]) == 0 and b < sk
        base = float(sh.idx.get_option("eps"))
        flush = sh.eps(COS) - base                                   # the shard's fp16-subnormal share (rq_plan.h scan_eps)
        hit = None
        e = float(np.float64(sk) - np.float64(b)) - flush
        for _ in range(200):                                         # walk the option until the index reports an eps with fp32(b + eps) == s_k
            sh.idx.set_option("eps", e)
            fb = so.certified(b, sh.eps(COS), 1.0, 1.0, COS, sk)[1]
            if fb == sk:
                hit = e
                break
            e += (1 if fb < sk else -1) * 2e-9
        assert hit is not None, "no eps option reaches s_k"
        st_eq, bufs_eq, m_eq = _one_pass(sh, q[qi:qi + 1], sc.K, COS, sc.NB, None, None, "equality, fp32(b + eps) == s_k")
        assert m_eq[0]["b"] == b and np.float32(bufs_eq.read()[1][0, sc.K - 1]) == sk                # the same records, the same s_k
        assert int(st_eq[0]) == 1, f"certified at equality: status {int(st_eq[0])}"
        lower = None
        for step in range(1, 200):                                   # the nearest smaller eps whose fp32 bound is below s_k
            sh.idx.set_option("eps", hit - step * 2e-9)
            if so.certified(b, sh.eps(COS), 1.0, 1.0, COS, sk)[1] < sk:
                lower = step
                break
        assert lower is not None
        st_lo, _, _ = _one_pass(sh, q[qi:qi + 1], sc.K, COS, sc.NB, None, None, "equality, one step below")
        assert int(st_lo[0]) == 0
    finally:
        sh.close()


# ====================================================================================================================================
# (c) the last rung at its tile and query-group edges
# ====================================================================================================================================
EXACT_N = [1, 16, 17, 63, 65, 129, 130, 1000]
EXACT_B = [1, 31, 32, 33, 65]


@pytest.mark.parametrize("dim,row_pad", [(768, None), (385, None), (384, 768), (384, 384)], ids=["768", "385", "384-pad768", "384-pad384"])
def test_exact_scan_at_tile_and_query_group_edges(dim, row_pad):
    """"cu_count" = 2: the grid of rq_exact_scan_kernel is two workgroups, so its double-buffered tile loop iterates on a few hundred rows
    (odd and even tile counts, a partial last tile on a wrapped iteration); B around the 32-query workgroup.  These shards are the
    exact route at the first pass already (fewer than two bins per wanted bin); eps = 10 keeps any other route from certifying."""
    rng = np.random.default_rng(20601 + dim)
    xall = orc.prepare_rows_f32((rng.standard_normal((max(EXACT_N), dim)) * rng.uniform(0.5, 2.0, (max(EXACT_N), 1)) / np.sqrt(dim)).astype(np.float32), normalize=False)
    qall = (rng.standard_normal((max(EXACT_B), dim)) * 0.1).astype(np.float32)
    k = 10
    for n in EXACT_N:
        x = xall[:n]
        sh = Shard(x, row_pad=row_pad)
        sh.idx.set_option("eps", 10.0)
        sh.idx.set_option("cu_count", 2)
        try:
            assert sh.idx.row_pad == (row_pad or (384 if dim <= 384 else 768))
            for metric in (COS, IP):
                gold_all = orc.dense_topk(qall, x, k, metric)
                for B in EXACT_B:
                    rows = {}
                    for mfma in (1, 0):
                        sh.idx.set_option("exact_mfma", mfma)
                        bufs = Bufs(qall[:B], k)
                        bufs.search(sh.idx, metric)
                        st, s, r = bufs.read()
                        what = f"exact scan: dim {dim}, n {n}, B {B}, metric {metric}, exact_mfma {mfma}"
                        assert (st == 0).all(), f"{what}: status {st.tolist()}"
                        _same(s, r, gold_all[0][:B], gold_all[1][:B], what)
                        assert (r[:, min(k, n):] == -1).all() and (s[:, min(k, n):] == 0).all(), f"{what}: padding beyond n"
                        rows[mfma] = r
                    assert np.array_equal(rows[0], rows[1]), f"exact scan: dim {dim}, n {n}, B {B}: the two kernels disagree on the rows"
        finally:
            sh.close()


# ====================================================================================================================================
# (d) the repair of queries flagged by hand: which packed slot overwrites which query's answer
# ====================================================================================================================================
HAND_N, HAND_K = 2000, 10                          # 32 bins, the last one ragged
HAND_FLAGGED = [(5, [0, 3, 4]), (70, [0, 63, 64, 69])]


@pytest.mark.parametrize("dim,row_pad,metric", [(768, None, COS), (768, None, IP), (384, 384, COS)], ids=["wide-cosine", "wide-ip", "narrow-cosine"])
def test_the_fixup_repairs_exactly_the_queries_flagged_by_hand(dim, row_pad, metric):
    """rq_search_device / rq_search_filtered_device without a fixup, then on the device: status 1 for a chosen subset and garbage over
    those queries' outputs, then the fixup form.  It returns the size of the subset, the flagged queries equal the oracle (rows, scores
    within SCORE_TOL, keys made of both), every other query keeps the first call's bits, every status is 0 and the counters rose by
    the size of the subset.  With and without d_keys, with and without a filter that allows about half the rows."""
    import torch
    x = orc.synthetic_corpus(HAND_N, dim, seed=71 + dim)
    qall = orc.synthetic_queries(70, dim, seed=72 + dim)
    idx = nat.NativeIndex(dim, 0)
    if row_pad:
        idx.set_option("row_pad", row_pad)
    idx.add_f16(x)
    allowed = np.random.default_rng(73).random(HAND_N) < 0.5
    flt = idx.make_filter(allowed)
    try:
        assert idx.row_pad == (row_pad or 768)
        gold = {None: orc.topk_from_scores(nfo.scores(qall, x, metric), HAND_K), flt: nfo.topk(qall, x, HAND_K, metric, mask=allowed)}
        for (B, flagged), with_keys, f in [(bf, wk, f) for bf in HAND_FLAGGED for wk in (True, False) for f in (None, flt)]:
            what = f"by hand: dim {dim}, metric {metric}, B {B}, keys {with_keys}, filtered {f is not None}"
            q = torch.from_numpy(np.ascontiguousarray(qall[:B])).cuda()
            sc = torch.full((B, HAND_K), -5.5, device="cuda")
            rw = torch.full((B, HAND_K), -9, device="cuda", dtype=torch.int64)
            ky = torch.full((B, HAND_K), 7, device="cuda", dtype=torch.int64) if with_keys else None
            st = torch.full((B,), -7, device="cuda", dtype=torch.int32)
            idx.search_device(q, B, HAND_K, metric, sc, rw, ky, st, 0, row_filter=f)
            torch.cuda.synchronize()
            first = [t.cpu().numpy().copy() for t in (sc, rw, st) + ((ky,) if with_keys else ())]
            assert not first[2].any(), f"{what}: the first call flagged {np.nonzero(first[2])[0].tolist()} itself"
            sel = torch.tensor(flagged, device="cuda")
            st[sel] = 1
            sc[sel] = float("nan")
            rw[sel] = -7
            if with_keys:
                ky[sel] = -1                        # all ones
            before = {o: int(idx.get_option(o)) for o in ("repaired_queries", "filter_repaired")}
            n = idx.search_fixup_device(q, B, HAND_K, metric, sc, rw, ky, st, 0, row_filter=f)
            torch.cuda.synchronize()
            after = [t.cpu().numpy() for t in (sc, rw, st) + ((ky,) if with_keys else ())]
            assert n == len(flagged), f"{what}: the fixup returned {n}"
            assert not after[2].any(), f"{what}: status after the fixup {after[2].tolist()}"
            _same(after[0][flagged], after[1][flagged], gold[f][0][flagged], gold[f][1][flagged], f"{what}, flagged queries")
            if with_keys:
                assert np.array_equal(after[3].view(np.uint64)[flagged], dist.pack_keys(after[0][flagged].reshape(-1), after[1][flagged].reshape(-1)).reshape(-1, HAND_K)), \
                    f"{what}: keys of the flagged queries"
            other = np.setdiff1d(np.arange(B), flagged)
            for a, b in zip(first, after):
                assert np.array_equal(a[other].view(np.uint8), b[other].view(np.uint8)), f"{what}: an unflagged query changed"
            assert int(idx.get_option("repaired_queries")) == before["repaired_queries"] + len(flagged), what
            assert int(idx.get_option("filter_repaired")) == before["filter_repaired"] + (len(flagged) if f is not None else 0), what
    finally:
        flt.close()
        idx.close()
