"""The fast tail (csrc/rq_tail_body.h, rq_final_body.h) against its host model (tests/tail_oracle.py) on planted corpora
(tests/tail_cases.py; tests/test_tail_oracle.py shows on the CPU that every geometry is decided and structured as named).

Every call is rq_search_device on stream 0 WITHOUT rq_search_fixup_device, so d_status is the tail's own certificate; the candidate
totals come from a "tail_stop" = 5 call followed by a "tail_stop" = 0 call.  Per query:
  (a) candidate total = the model's          (b) unrepaired status = the model's
  (c) status 0: rows = the oracle's, scores within SCORE_TOL
  (d) after rq_search_fixup_device every query equals the oracle
  (e) "widened" and "repaired_queries" moved by exactly the number of status-1 queries.

Which geometry runs in which form (tail_local 0 and 1 everywhere):
  plain tail (NV = 1)                           1 spread, 2 pairs, 3 triples, 4 ties (k = 10), 5 concentrated, 8 job cap 2 048 / 2 112, 11 ranking
                                                paths 256 | 257 | 512 | 513 (k = 3); 6 all-negative, cosine and inner product; 7 mixed signs
                                                (k = 50); 9 candidate cap (70 000 rows); 10 hit cap (52 000 rows)
  riding tail of the fused kernel ("pipeline" 2: the tail of call i rides with the scan of call i + 1; the flush launches the stand-alone
  tail of the last call)                        1-5, 8 and 11; 6; 7; 10 with "fused_nv" = 4 (one chunk of 2 048 bins: 800 hits > 768)
  grid of 512 workgroups                        4 ties at k = 70
  the device's own grid                         the queries of the base shard
  192 queries (128 wide + 64 narrow grid)       1 and 5 on both sides of nwg_split
  narrow layout (dim 384, "row_pad" 384)        1-3 (plain and riding), 6 (both metrics)
  filtered tail ("filter_route" 2)              1-3 with the model run on the bitmap
  int8 scan ("scan8" 2, "thr_mult8" 2.25)       1-3 and 6: (c), (d), status 0 where the model has no overflow, total >= the fp16 model's count at T_hi
  Gaussian queries, plain tail                  the candidate total recomputed exactly from the bin records the scan wrote
"""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases as tc  # noqa: E402
import tail_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-6          # tests/test_gpu_parity.py
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP


class Bufs:
    def __init__(self, q, k):
        import torch
        self.B, self.k = q.shape[0], k
        self.q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
        self.sc = torch.empty((self.B, k), device="cuda")
        self.rw = torch.empty((self.B, k), device="cuda", dtype=torch.int64)
        self.st = torch.full((self.B,), -7, device="cuda", dtype=torch.int32)

    def search(self, idx, metric, flt=None):
        idx.search_device(self.q, self.B, self.k, metric, self.sc, self.rw, None, self.st, 0, row_filter=flt)

    def fixup(self, idx, metric, flt=None):
        return idx.search_fixup_device(self.q, self.B, self.k, metric, self.sc, self.rw, None, self.st, 0, row_filter=flt)

    def status(self):
        import torch
        torch.cuda.synchronize()
        return self.st.cpu().numpy().copy()

    def result(self):
        import torch
        torch.cuda.synchronize()
        return self.sc.cpu().numpy().copy(), self.rw.cpu().numpy().copy()


class Shard:
    """One index over a planted corpus with the scan grid pinned, its exact scores and its oracle answers."""

    def __init__(self, corpus, metric=COS, dim=768, row_pad=None):
        self.x, self.q, cases = corpus
        self.cases = {c["name"]: c for c in cases}
        self.metric = metric
        self.idx = nat.NativeIndex(dim, 0)
        if row_pad:
            self.idx.set_option("row_pad", row_pad)
        self.idx.add_f16(self.x)
        self.device_cus = int(self.idx.get_option("cu_count"))
        self.idx.set_option("scan8", 0)
        self.grid(tc.BASE_CU, tc.BASE_WG)
        self.n = self.x.shape[0]
        self.eps = float(self.idx.get_option("eps_cosine" if metric == COS else "eps_ip"))
        self.mrn = float(self.idx.get_option("max_row_norm"))
        # the model's own reading of the shard (rq_plan.h scan_eps in numpy) is what the CPU tests used
        eps_host, mrn_host = to.shard_eps(self.x, metric)
        assert abs(eps_host - self.eps) <= 1e-6 * self.eps and abs(mrn_host - self.mrn) <= 1e-9 * self.mrn, (eps_host, self.eps, mrn_host, self.mrn)
        self.e = to.tail_bound(self.eps, self.mrn, metric)
        self.unit = to.unit_scores(self.q, self.x, metric)
        self.exact = orc.exact_scores(self.q, self.x, metric)
        self.qn = np.sqrt((self.q.astype(np.float64) ** 2).sum(1))

    def grid(self, cu, wg):
        self.idx.set_option("cu_count", cu)
        self.idx.set_option("wg_per_cu", wg)
        self.cu, self.wg = cu, wg

    def G(self, wide=False):
        return to.scan_grid((self.n + 63) // 64, self.cu, 1 if wide else self.wg)

    def model(self, qi, k, tail_local, G=None, nv=1, allowed=None, scores=None):
        return to.model_query(self.unit[qi] if scores is None else scores, self.n, k, self.e, self.G() if G is None else G, nv=nv,
                              tail_local=bool(tail_local), metric=self.metric, qnorm=float(self.qn[qi]), allowed=allowed)

    def close(self):
        self.idx.close()


def measure(sh, q, k, tail_local, fused=False, flt=None, fused_nv=0):
    """The candidate totals and the unrepaired answers of one call (fused: of the riding tail AND of the twin call's flushed tail)."""
    idx = sh.idx
    idx.set_option("tail_local", tail_local)
    idx.set_option("pipeline", 2 if fused else 0)
    idx.set_option("fused_nv", fused_nv)
    out = []
    try:
        calls = [Bufs(q, k) for _ in range(2 if fused else 1)]
        for stop in (5, 0):
            idx.set_option("tail_stop", stop)
            for c in calls:
                c.search(idx, sh.metric, flt)              # fused: the second call's launch carries the first call's tail
            if fused:
                idx.search_flush_device(0)                 # ... and the flush runs the second call's tail on its own
            if stop == 5:
                totals = [c.status() for c in calls]
        for c, t in zip(calls, totals):
            s, r = c.result()
            out.append(dict(total=t, status=c.status(), scores=s, rows=r, bufs=c))
    finally:
        idx.set_option("tail_stop", 0)
        idx.set_option("pipeline", 0)
        idx.set_option("fused_nv", 0)
    return out


def check(sh, got, models, k, what, exact=None, flt=None, gold=None, int8=False):
    """(a) - (e) for one measured call; models: {query: model} for the queries the model speaks about."""
    exact = sh.exact if exact is None else exact
    gs, gr = orc.topk_from_scores(exact, k) if gold is None else gold
    rep = []
    for qi, m in sorted(models.items()):
        assert m["ambiguous"].size == 0, f"{what}: query {qi} is not decided by the oracle (bins {m['ambiguous'][:4].tolist()})"
        rep.append(f"q{qi}: total {int(got['total'][qi])} (model {m['total']}) status {int(got['status'][qi])} (model {m['status']})")
    print(f"[tail] {what}: " + "; ".join(rep))
    for qi, m in sorted(models.items()):
        if int8:    # the int8 bound is measured per shard and query: no smaller candidate set than the fp16 scan's, certified unless the model overflows
            floor = to.count_at(sh.unit[qi], sh.n, m["T_hi"])
            assert int(got["total"][qi]) >= floor, f"{what}: query {qi} candidate total {int(got['total'][qi])} below the fp16 count {floor}"
            assert m["overflow"] or int(got["status"][qi]) == 0, f"{what}: query {qi} not certified"
            continue
        if m["total"] is not None:
            assert int(got["total"][qi]) == m["total"], f"(a) {what}: query {qi} candidate total {int(got['total'][qi])}, model {m['total']}"
        assert int(got["status"][qi]) == m["status"], f"(b) {what}: query {qi} status {int(got['status'][qi])}, model {m['status']}"
    assert set(np.unique(got["status"]).tolist()) <= {0, 1}
    good = got["status"] == 0
    assert np.array_equal(got["rows"][good], gr[good]), f"(c) {what}: rows differ at {np.argwhere(got['rows'] != gr)[:4].tolist()}"
    assert float(np.abs(got["scores"][good] - gs[good]).max(initial=0.0)) <= SCORE_TOL, f"(c) {what}: scores"
    n1 = int((got["status"] == 1).sum())
    t0, r0 = sh.idx.timing(), int(sh.idx.get_option("repaired_queries"))
    fixed = got["bufs"].fixup(sh.idx, sh.metric, flt)
    s, r = got["bufs"].result()
    t1, r1 = sh.idx.timing(), int(sh.idx.get_option("repaired_queries"))
    assert np.array_equal(r, gr) and float(np.abs(s - gs).max(initial=0.0)) <= SCORE_TOL, f"(d) {what}"
    if int8:
        return
    assert fixed == n1 and r1 - r0 == n1 and t1["widened"] - t0["widened"] == n1 and 0 <= t1["exact_scans"] - t0["exact_scans"] <= n1, \
        f"(e) {what}: {n1} status-1 queries, fixup returned {fixed}, repaired {r1 - r0}, widened {t1['widened'] - t0['widened']}"


@pytest.fixture(scope="module")
def base():
    sh = Shard(tc.base_corpus())
    yield sh
    sh.close()


def _all(sh, k, tail_local, names=None, **kw):
    return {c["q"]: sh.model(c["q"], k, tail_local, **kw) for c in sh.cases.values() if c["k"] == k and (names is None or c["name"] in names)}


def _intended(sh, models, tail_local):
    """The structure the CPU tests showed, once more, on the model the kernel is held to (this shard's own bound)."""
    for c in sh.cases.values():
        if c["q"] in models:
            st = c["status"][tail_local] if isinstance(c["status"], dict) else c["status"]
            assert models[c["q"]]["status"] == st and ("total" not in c or models[c["q"]]["total"] == c["total"][tail_local]), c["name"]


@pytest.mark.parametrize("tail_local", [0, 1])
def test_plain_tail_on_the_planted_shard(base, tail_local):
    """Geometries 1-5 and 8 (the job cap at 2 048 and 2 112), one per query, NV = 1: two chunks."""
    got = measure(base, base.q, 10, tail_local)[0]
    models = _all(base, 10, tail_local)
    _intended(base, models, tail_local)
    check(base, got, models, 10, f"plain tail, tail_local {tail_local}")


@pytest.mark.parametrize("tail_local", [0, 1])
def test_riding_tail_of_the_fused_kernel(base, tail_local):
    """"pipeline" = 2: the first call's tail rides with the second call's scan (rq_scan.hip rq_scan_tail_kernel), the second
    call's tail is launched by the flush.  Both see the same bin records' contract, so both equal the model."""
    riding, flushed = measure(base, base.q, 10, tail_local, fused=True)
    models = _all(base, 10, tail_local)
    check(base, riding, models, 10, f"riding tail, tail_local {tail_local}")
    check(base, flushed, models, 10, f"flushed tail, tail_local {tail_local}")


def test_ties_at_k_70_on_512_workgroups(base):
    """Geometry 4 at k = 70: 64 identical rows and the first 6 of the next bin, ordered by row; 512 partitions (m > 64)."""
    base.grid(256, 2)
    try:
        qi = base.cases["ties"]["q"]
        q = base.q[qi:qi + 1]
        exact = base.exact[qi:qi + 1]
        for tl in (0, 1):
            m = base.model(qi, 70, tl)
            assert m["G"] == 512 and m["status"] == 0
            got = measure(base, q, 70, tl)[0]
            check(base, got, {0: m}, 70, f"ties k = 70, tail_local {tl}", exact=exact)
            assert got["rows"][0].tolist() == list(range(300 * 64, 300 * 64 + 70))
    finally:
        base.grid(tc.BASE_CU, tc.BASE_WG)


def test_the_devices_own_grid(base):
    base.grid(base.device_cus, 2)
    try:
        for tl in (0, 1):
            models = {qi: m for qi, m in _all(base, 10, tl).items() if m["ambiguous"].size == 0}    # (decided at 416, 512 and 608 workgroups)
            assert len(models) >= 6 and {base.cases[n]["q"] for n in ("spread", "ties", "jobcap32", "jobcap33")} <= set(models)
            check(base, measure(base, base.q, 10, tl)[0], models, 10, f"device grid G = {base.G()}, tail_local {tl}")
    finally:
        base.grid(tc.BASE_CU, tc.BASE_WG)


def test_192_queries_use_the_grid_of_their_own_pass(base):
    """"wide_batch" = 3: a 128-query pass on the wide grid (one workgroup per CU: 32) and a 64-query pass on the narrow one (64).
    Spread and concentrated sit at queries 0 / 1 and 128 / 129: the same vectors, two partition layouts (nwg / nwg2 past nwg_split)."""
    q = orc.synthetic_queries(192, 768, seed=20281)
    src = [base.cases["spread"]["q"], base.cases["concentrated"]["q"]]
    for off in (0, 128):
        q[off:off + 2] = base.q[src]
    exact = orc.exact_scores(q, base.x)
    base.idx.set_option("wide_batch", 3)
    try:
        for tl in (0, 1):
            models = {}
            for off, G in ((0, base.G(wide=True)), (128, base.G())):
                for j, qi in enumerate(src):
                    models[off + j] = base.model(qi, 10, tl, G=G)
            assert models[0]["G"] == 32 and models[128]["G"] == 64
            # the narrow pass wrote 64 maxima: a tail that read only the wide grid's 32 would lose five of spread's partitions
            s1 = np.pad(base.unit[src[0]], (0, 27), constant_values=-np.inf).reshape(-1, 64).max(1)
            seen = np.where(to.wg_of_quad(626, 64) < 32, s1, -np.inf)
            assert to.threshold_interval(seen, models[128]["part"], 10, base.e)[1] < models[128]["T_lo"] - 0.1
            check(base, measure(base, q, 10, tl)[0], models, 10, f"192 queries, tail_local {tl}", exact=exact)
    finally:
        base.idx.set_option("wide_batch", 1)


def test_all_negative_scores():
    """Geometry 6, cosine: every score of the shard is negative, the winners are the least negative rows (rq_up16 / rq_up26 truncate,
    the 20-bit truncation of P grows in magnitude); the best row is the last valid row of the ragged last bin."""
    sh = Shard(tc.negative_corpus())
    try:
        assert sh.exact.max() < 0
        for tl in (0, 1):
            m = {0: sh.model(0, 10, tl)}
            assert m[0]["status"] == 0 and m[0]["total"] == 10
            check(sh, measure(sh, sh.q, 10, tl)[0], m, 10, f"all negative, tail_local {tl}")
            riding, flushed = measure(sh, sh.q, 10, tl, fused=True)
            check(sh, riding, m, 10, f"all negative, riding tail, tail_local {tl}")
    finally:
        sh.close()


@pytest.mark.parametrize("tail_local", [0, 1])
def test_ranking_paths_at_their_boundaries(base, tail_local):
    """Geometry 11, k = 3.  tail_local 1: a tail workgroup ranks 256 jobs all against all and hands 257 (and 512, 513) to
    rq_select_winners; tail_local 0: rq_final_body ranks a list of 512 keys all against all and selects from 513."""
    models = _all(base, 3, tail_local)
    assert sorted(m["njob"][0] for m in models.values()) == [256, 257, 512, 513]
    _intended(base, models, tail_local)
    check(base, measure(base, base.q, 3, tail_local)[0], models, 3, f"ranking paths, tail_local {tail_local}",
          exact=base.exact)
    riding, flushed = measure(base, base.q, 3, tail_local, fused=True)
    check(base, riding, models, 3, f"ranking paths, riding tail, tail_local {tail_local}")


def test_all_negative_scores_inner_product():
    """Geometry 6, inner product: query norm 3, row norms 0.5 .. 2; the bound is eps_ip * max_row_norm."""
    sh = Shard(tc.negative_corpus(), metric=IP)
    try:
        assert sh.exact.max() < 0 and 1.9 < sh.mrn <= 2.001
        for tl in (0, 1):
            m = {0: sh.model(0, 10, tl)}
            _intended(sh, m, tl)
            check(sh, measure(sh, sh.q, 10, tl)[0], m, 10, f"all negative, inner product, tail_local {tl}")
    finally:
        sh.close()


def test_mixed_signs_in_one_candidate_list():
    """Geometry 7, k = 50: 617 keys of both signs.  tail_local 0: rq_final_body's select (n > 512); tail_local 1: the workgroup's own
    (njob > 256).  The keys' leading bits differ in bit 63 (rq_select_winners `top == 63`)."""
    sh = Shard(tc.mixed_corpus())
    try:
        for tl in (0, 1):
            m = {0: sh.model(0, 50, tl)}
            _intended(sh, m, tl)
            got = measure(sh, sh.q, 50, tl)[0]
            check(sh, got, m, 50, f"mixed signs, tail_local {tl}")
            assert (got["scores"][0] > 0).sum() == 27 and (got["scores"][0] < 0).sum() == 23
            check(sh, measure(sh, sh.q, 50, tl, fused=True)[0], m, 50, f"mixed signs, riding tail, tail_local {tl}")
    finally:
        sh.close()


def test_candidate_cap():
    """Geometry 9: three tail workgroups want 1 408 keys each: 4 224 > RQ_CAND_CAP gives up with tail_local 0, 30 keys certify with 1."""
    sh = Shard(tc.candcap_corpus())
    try:
        for tl in (0, 1):
            m = {0: sh.model(0, 10, tl)}
            _intended(sh, m, tl)
            assert m[0]["ovf_cand"] == (tl == 0) and not m[0]["ovf_job"] and not m[0]["ovf_hit"]
            check(sh, measure(sh, sh.q, 10, tl)[0], m, 10, f"candidate cap, tail_local {tl}")
    finally:
        sh.close()


def test_hit_cap():
    """Geometry 10: 800 hit bins of one row each.  Chunks of 512 bins (plain tail, flushed tail): 512 + 288 hits, certified.  One chunk
    of 2 048 bins (the riding tail with "fused_nv" = 4): 800 > RQ_TAIL_HITCAP, status 1, repaired exactly."""
    sh = Shard(tc.hitcap_corpus())
    try:
        for tl in (0, 1):
            plain, one = {0: sh.model(0, 10, tl)}, {0: sh.model(0, 10, tl, nv=4)}
            _intended(sh, plain, tl)
            assert not plain[0]["overflow"] and one[0]["ovf_hit"] and one[0]["status"] == 1
            check(sh, measure(sh, sh.q, 10, tl)[0], plain, 10, f"hit cap, plain tail, tail_local {tl}")
            riding, flushed = measure(sh, sh.q, 10, tl, fused=True, fused_nv=4)
            check(sh, riding, one, 10, f"hit cap, riding tail of 2 048 bins, tail_local {tl}")
            check(sh, flushed, plain, 10, f"hit cap, flushed tail, tail_local {tl}")
    finally:
        sh.close()


def test_narrow_layout():
    """Rows of 384 elements (dim 384, "row_pad" 384: rq_scan_narrow.hip, rq_tail_body<NV, 384>): geometries 1-3 plain and riding, 6 in both metrics."""
    sh = Shard(tc.base_corpus(384), dim=384, row_pad=384)
    names = ("spread", "pair(0, 63)", "pair(31, 32)", "triple", "triple_ragged")
    try:
        assert sh.idx.row_pad == 384
        for tl in (0, 1):
            models = _all(sh, 10, tl, names=names)
            assert len(models) == 5
            _intended(sh, models, tl)
            check(sh, measure(sh, sh.q, 10, tl)[0], models, 10, f"narrow, tail_local {tl}")
            check(sh, measure(sh, sh.q, 10, tl, fused=True)[0], models, 10, f"narrow, riding tail, tail_local {tl}")
    finally:
        sh.close()
    for metric in (COS, IP):
        sh = Shard(tc.negative_corpus(384), metric=metric, dim=384, row_pad=384)
        try:
            for tl in (0, 1):
                m = {0: sh.model(0, 10, tl)}
                _intended(sh, m, tl)
                check(sh, measure(sh, sh.q, 10, tl)[0], m, 10, f"narrow, all negative, metric {metric}, tail_local {tl}")
        finally:
            sh.close()


def test_filtered_tail(base):
    """"filter_route" = 2 (scan route: rq_tail_body<NV, DP, true>).  The filter removes the second winner of pair(0, 63), the middle
    winner of the triple and the 63 background rows of one of spread's hit bins; the model runs on the same bitmap."""
    import filter_oracle as fo
    allowed = tc.base_filter(base.n, base.cases, base.unit)
    flt = base.idx.make_filter(allowed)
    gold = fo.filtered_topk_from_scores(base.exact, allowed, 10)
    base.idx.set_option("filter_route", 2)
    try:
        for tl in (0, 1):
            models = {c["q"]: base.model(c["q"], 10, tl, allowed=allowed) for c in base.cases.values() if c["k"] == 10}
            pair, triple = base.cases["pair(0, 63)"], base.cases["triple"]
            assert models[pair["q"]]["jobs"][int(pair["winners"][0]) // 64] == 1 and models[triple["q"]]["jobs"][int(triple["winners"][0]) // 64] == 2
            got = measure(base, base.q, 10, tl, flt=flt)[0]
            assert int(base.idx.get_option("filter_route_last")) == 2
            check(base, got, models, 10, f"filtered, tail_local {tl}", flt=flt, gold=gold)
    finally:
        base.idx.set_option("filter_route", -1)
        flt.close()


def test_int8_scan(base):
    """"scan8" = 2 with "thr_mult8" = 2.25 (certified by construction like the fp16 scan): geometries 1-3 on the base shard, 6 on its own."""
    names = ("spread", "pair(0, 63)", "pair(31, 32)", "triple", "triple_ragged")
    neg = Shard(tc.negative_corpus())
    try:
        for sh, nm in ((base, names), (neg, ("negative",))):
            sh.idx.set_option("scan8", 2)
            sh.idx.set_option("thr_mult8", 2.25)
            used = int(sh.idx.get_option("scan8_used"))
            models = _all(sh, 10, 0, names=nm)
            assert len(models) == len(nm)
            check(sh, measure(sh, sh.q, 10, 0)[0], models, 10, f"int8 scan, {nm[0]} ...", int8=True)
            assert int(sh.idx.get_option("scan8_used")) > used
    finally:
        base.idx.set_option("thr_mult8", 1.25)
        base.idx.set_option("scan8", 0)
        neg.close()


def test_the_bin_records_decide_the_tail_exactly(base):
    """Beyond the model's bands: given the records the scan really wrote (rq_debug_bin_records), sections A and B are a function of
    them alone.  The workgroup maxima are the records' m1 before the 26-bit round-up, up to position bits that the 20-bit truncation
    of P drops; T follows in fp32 (the library is built with -ffp-contract=off); a bin is a hit when m1 >= T and becomes 1 / 2 / 64
    jobs by decode(c2), decode(c2 - d) >= T.  On Gaussian queries T sits at the background level, where dozens of bins lie within
    eps of it -- none of them decided by the exact scores, all of them decided by the records: a hit test that is off by a
    fraction of eps (`> T + eps` for `>= T`) changes the count."""
    B, k, nbins = 64, 10, (base.n + 63) // 64
    q = orc.synthetic_queries(B, 768, seed=20331)
    got = measure(base, q, k, 0)[0]
    rec = base.idx.debug_bin_records(0, B)
    assert rec.shape == (B, nbins, 2)
    part = to.partition_of_quad(nbins, base.G(), k)
    e = np.float32(base.eps)
    near = 0
    for j in range(B):
        x, y = rec[j, :, 0], rec[j, :, 1]
        m1 = to._f32(x & np.uint32(0xFFFFFFC0))
        # the triple's head: positive scores were rounded up by 64 ulp (rq_record_from_triple), negative ones truncated
        head = np.where(x & np.uint32(0x80000000), x & np.uint32(0xFFFFFFC0), (x & np.uint32(0xFFFFFFC0)) - np.uint32(64)).astype(np.uint32)
        keys = np.full(64 * to.npl_of(k), int(to.mono32(np.float32(-np.inf))) & 0xFFFFF000, dtype=np.uint32)
        np.maximum.at(keys, part, to.mono32(to._f32(head)) & np.uint32(0xFFFFF000))
        prefix = np.sort(keys)[::-1][k - 1]
        assert prefix > to.mono32(np.float32(-np.inf))
        T = to._threshold_fp32(to.unmono32(prefix), e, 2.25, 0.0)
        c2, d = y >> np.uint32(16), (y >> np.uint32(6)) & np.uint32(1023)
        hit = m1 >= T
        two = to.code16_value(c2) >= T
        whole = two & (to.code16_value(c2 - d) >= T)
        nj = np.where(hit, np.where(whole, 64, np.where(two, 2, 1)), 0)
        per_chunk = [int(nj[c:c + 512].sum()) for c in range(0, nbins, 512)]
        assert max(per_chunk) <= to.JOBCAP and sum(per_chunk) <= to.CAND_CAP and int(hit.sum()) <= to.HITCAP
        assert int(got["total"][j]) == sum(per_chunk), f"query {j}: candidate total {int(got['total'][j])}, the records give {sum(per_chunk)} at T = {float(T)}"
        assert int(got["status"][j]) == 0
        near += int((hit & (m1 <= T + e)).sum())
    assert near >= 8                                                       # (the test's own power: hit bins within eps above T, the ones a coarser hit test loses)
    print(f"[tail] records decide the tail: totals {got['total'].tolist()}, {near} hit bins within eps of T")
    check(base, got, {}, k, "records decide the tail", exact=orc.exact_scores(q, base.x))
