"""CPU: the host model of the generic tail (tests/select_oracle.py) and its planted corpora (tests/select_cases.py).

Records are made from EXACT scores with tests/bin_records.py records_from_scores (a scan without error), so what is shown here is
about the cases and the model, not about any kernel: every geometry is structured as named, the model's status is the named one,
every planted query that is not a tie geometry is decided with a margin of at least eps / 2 (a tie geometry is decided by the
certificate's premise alone: the (nb+1)-th bin holds a row whose exact score EQUALS s_k), and none is undecided.  Each assertion
tests/test_gpu_select.py makes about the certificate is shown to reject one emulated wrong certificate on the same inputs.
"""
import os
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bin_records as br  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402
import select_cases as sc  # noqa: E402
import select_oracle as so  # noqa: E402
import tail_oracle as to  # noqa: E402

COS, IP = so.METRIC_COSINE, so.METRIC_IP


# ---- keys --------------------------------------------------------------------------------------------------------------------------
def test_key_codec_is_the_host_twin_of_pack_keys():
    rng = np.random.default_rng(1)
    s = np.concatenate([rng.standard_normal(500).astype(np.float32), np.float32([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 3.4e38, -3.4e38])])
    r = np.concatenate([rng.integers(0, 2**32 - 1, 506), [0, 2**32 - 2]]).astype(np.int64)
    keys = so.make_key(s, r)
    assert np.array_equal(keys, dist.pack_keys(s, r))
    assert np.array_equal(so.key_index(keys), r)
    back = so.key_score(keys)
    assert np.array_equal(back, np.where(s == 0, np.float32(0.0), s)) and not np.signbit(back[s == 0]).any()
    order = np.lexsort((r, -s.astype(np.float64)))                           # score descending, row ascending
    assert np.array_equal(np.argsort(keys, kind="stable")[::-1], order)
    assert (keys != 0).all() and so.make_key(np.float32(-np.inf), 2**32 - 2) > 0       # 0 is the empty slot and nothing else
    assert so.make_key(so.sanitize(np.float32(np.nan)), 7) == so.make_key(np.float32(-np.inf), 7)


def test_topm_and_merge_are_a_sort_with_empty_slots():
    rng = np.random.default_rng(2)
    keys = so.make_key(rng.standard_normal((3, 50)).astype(np.float32), rng.permutation(150).reshape(3, 50))
    keys[0, ::3] = 0
    keys[2, 4:] = 0
    for k in (1, 4, 50, 64):
        s, r, kk = so.merge(keys, k)
        hs, hr = dist.merge_keys_host(keys, k)
        assert np.array_equal(r, hr) and np.array_equal(s, hs)
        for b in range(3):
            want = np.sort(keys[b][keys[b] != 0])[::-1][:k]
            assert np.array_equal(kk[b, :want.size], want) and (kk[b, want.size:] == 0).all()
            assert (r[b, want.size:] == -1).all() and (s[b, want.size:] == 0).all()
    assert so.topm(np.zeros(7, np.uint64), 3).size == 0 and so.topm(np.zeros(0, np.uint64), 3).size == 0


def test_ladder_arithmetic():
    assert so.nb_default(10) == 18 and so.nb_default(100) == 112 and so.nb_default(321) == 361 and so.nb_default(1024) == 1152
    assert so.nb_default(1, 0) == 1 and so.nb_default(3, 0) == 3 and so.nb_default(10, 5) == 15
    assert so.nb_widened(10) == 72 and so.nb_widened(321) == 1444 and so.nb_widened(1024) == so.NB_MAX == 3071
    assert so.exact_route(1, 2) and not so.exact_route(1, 3) and so.exact_route(3, 6) and not so.exact_route(3, 7)
    assert not so.exact_route(so.nb_default(321), sc.K321_BINS) and so.exact_route(so.nb_default(321), sc.K321_BINS - 1)
    assert so.exact_route(so.nb_widened(321), sc.K321_BINS)
    assert not so.exact_route(so.nb_widened(1024), sc.K1024_BINS) and so.exact_route(so.nb_widened(1024), sc.K1024_BINS - 1)
    for c in sc.SMALL:
        assert so.exact_route(so.nb_default(c["k"], 0), c["nbins"]) == c["exact"]
    got = so.ladder_counts([0, 1, 1, 0, 1], {1: 0, 2: 1, 4: 1})
    assert (got["repaired"], got["widened"], got["exact_scans"]) == (3, 3, 2) and got["exact"] == [2, 4]


# ---- the planted corpora -----------------------------------------------------------------------------------------------------------
class Host:
    """A corpus with the records of an error-free scan."""

    def __init__(self, corpus, metric, allowed=None):
        self.x, self.q, cases = corpus
        self.cases = {c["name"]: c for c in cases}
        self.metric, self.allowed = metric, allowed
        self.n = self.x.shape[0]
        self.eps, self.mrn = to.shard_eps(self.x, metric)
        self.unit = to.unit_scores(self.q, self.x, metric)                   # (NaN where a row holds a NaN)
        approx = self.unit.astype(np.float32)
        if allowed is not None:
            approx = np.where(allowed[None, :], approx, np.float32(np.nan))  # the filter's row scale
        self.rec = br.records_from_scores(approx, self.n)
        self.unit = np.where(np.isnan(self.unit), -np.inf, self.unit)        # (a NaN score counts as -inf)
        self.exact = nfo.scores(self.q, self.x, metric)
        self.qn = np.sqrt((self.q.astype(np.float64) ** 2).sum(1))

    def model(self, qi, k, nb, **kw):
        return so.generic_tail(self.rec[qi], self.x, self.q[qi], k, nb, self.metric, self.eps, self.mrn, allowed=self.allowed, **kw)

    def scale(self, qi):
        """eps in the units of s_k."""
        return self.eps if self.metric == COS else self.eps * self.mrn * self.qn[qi]


@pytest.fixture(scope="module", params=[(768, COS), (768, IP), (384, COS), (384, IP)], ids=["768-cos", "768-ip", "384-cos", "384-ip"])
def main(request):
    dim, metric = request.param
    return Host(sc.main_corpus(dim), metric)


def _bin_best(h, qi):
    s = np.full(((h.n + 63) // 64) * 64, -np.inf)
    s[:h.n] = np.where(np.isnan(h.unit[qi]), -np.inf, h.unit[qi])
    return s.reshape(-1, 64).max(1)


def test_geometries_are_structured_as_named(main):
    h, e = main, main.eps * (1.0 if main.metric == COS else main.mrn)        # unit-query units
    c = h.cases["separated"]
    best = _bin_best(h, c["q"])
    wb = np.asarray(c["winners"]) // 64
    assert len(set(wb.tolist())) == 10 and {0, 63} <= set((np.asarray(c["winners"]) % 64).tolist())
    kth = np.sort(h.unit[c["q"]][c["winners"]])[0]
    assert np.delete(best, wb).max() <= kth - 3 * e
    for name, nt in (("tied shelf", sc.NB + 5), ("wide tied shelf", sc.NB1 + 5)):
        c = h.cases[name]
        ex = h.exact[c["q"]]
        ties = np.nonzero(ex == ex.max())[0]
        assert np.array_equal(ties, c["ties"]) and ties.size == nt and len(set((ties // 64).tolist())) == nt
        assert {0, 63} <= set((ties % 64).tolist())
        assert name != "tied shelf" or (ties // 64).max() == (h.n - 1) // 64                            # the ragged last bin is one of them
        assert np.delete(_bin_best(h, c["q"]), ties // 64).max() <= h.unit[c["q"]].max() - 3 * e
        assert np.array_equal(orc.topk_from_scores(ex[None, :], c["k"])[1][0], ties[:c["k"]])           # the k lowest row ids among the ties
    for name in ("ladder steps", "k-th gap"):
        c = h.cases[name]
        rows = np.asarray(c["planted"])
        assert len(set((rows // 64).tolist())) == sc.NB + 5
        order = np.argsort(-h.unit[c["q"]])[:sc.NB + 5]
        assert set(order.tolist()) == set(rows.tolist())                       # the 23 best rows are the planted ones, one per bin
        s = h.unit[c["q"]][order]
        # around the k-th the planted levels are eps / 50 apart (the fp16 rounding of a row moves its cosine by a few 1e-5)
        assert s[9] - s[sc.NB + 4] < 0.5 * e and s[9] - s[sc.NB] < 0.4 * e and s[sc.NB + 4] - np.sort(h.unit[c["q"]])[::-1][sc.NB + 5] > 3 * e
        if name == "k-th gap":
            assert s[8] - s[9] > 5 * e
    assert h.qn[h.cases["tiny query"]["q"]] < so.TINY_QUERY_NORM and h.qn[h.cases["tiny query"]["q"]] > 0


def test_model_status_is_the_named_one_and_decided(main):
    h = main
    for c in h.cases.values():
        first = h.model(c["q"], c["k"], sc.NB)
        wide = h.model(c["q"], c["k"], sc.NB1)
        assert first["status"] is not None and wide["status"] is not None, f"{c['name']}: undecided (margins {first['margin']}, {wide['margin']} ulps)"
        for got, want, what in ((first, c["status"][h.metric], "first pass"), (wide, c["widened"][h.metric], "widened pass")):
            assert want is None or got["status"] == want, f"{c['name']}, {what}: model {got['status']} ({got['why']}), named {want}"
            if got["margin"] is not None and not c["tie"]:
                gap = abs(got["bound"] - got["sk"])
                assert gap >= 0.5 * h.scale(c["q"]), f"{c['name']}, {what}: bound {got['bound']} within {gap} of s_k {got['sk']}"
        if first["status"] == 0:
            assert np.array_equal(first["rows"], orc.topk_from_scores(h.exact[c["q"]][None, :], c["k"])[1][0]), c["name"]
        if c["tie"]:
            # the premise alone: the (nb+1)-th bin holds a row whose exact score equals s_k, and its record is an upper bound
            assert first["why"] == "certificate" and first["b"] >= first["sk"] - h.scale(c["q"]) and first["bound"] >= first["sk"]
            assert np.array_equal(np.sort(wide["rows"]), c["ties"][:c["k"]]) or c["widened"][h.metric] == 1
    assert h.model(h.cases["ladder steps"]["q"], sc.K, sc.NB)["status"] == 1        # (with an error-free scan: b + eps = s_k + 0.8 eps)
    t = h.model(h.cases["tiny query"]["q"], sc.K, sc.NB)
    assert t["why"] == ("tiny query" if h.metric == COS else "certificate")


@pytest.mark.parametrize("metric", [COS, IP])
def test_all_negative_forms(metric):
    for corpus, route1 in ((sc.negative_separated(), True), (sc.negative_shelf_corpus(), False)):
        h = Host(corpus, metric)
        assert np.nanmax(h.exact) < 0
        nbins = (h.n + 63) // 64
        assert so.exact_route(sc.NB1, nbins) == route1 and not so.exact_route(sc.NB, nbins)
        for c in h.cases.values():
            first, wide = h.model(0, sc.K, sc.NB), h.model(0, sc.K, sc.NB1)
            assert first["status"] == c["status"][metric] and (c["widened"][metric] is None or wide["status"] == c["widened"][metric]), c["name"]
            assert first["bound"] < 0 and first["sk"] < 0
            if c["tie"]:
                assert np.array_equal(np.nonzero(h.exact[0] == h.exact[0].max())[0], c["ties"])
                assert np.array_equal(wide["rows"], c["ties"][:sc.K])
            else:
                assert abs(first["bound"] - first["sk"]) >= 0.5 * h.scale(0)
                assert np.array_equal(first["rows"], orc.topk_from_scores(h.exact, sc.K)[1][0])


@pytest.mark.parametrize("metric", [COS, IP])
def test_short_of_rows(metric):
    corpus = sc.main_corpus()
    allowed = sc.short_filter({c["name"]: c for c in corpus[2]})
    h = Host(corpus, metric, allowed=allowed)
    assert allowed.sum() == 12 > sc.K and np.isfinite(h.unit[0][allowed]).sum() == 9 < sc.K
    for nb in (sc.NB, sc.NB1):
        m = h.model(0, sc.K, nb)
        assert m["status"] == 1 and m["why"] == "have < kk" and m["have"] == 9 and m["kk"] == 10
        assert not set(m["bins"][:nb].tolist()) & {150, 151, 152}
    full = h.model(0, sc.K, (h.n + 63) // 64)                                  # every bin: the exact route
    want = nfo.topk(h.q[:1], h.x, sc.K, metric, mask=allowed)
    assert full["status"] == 0 and np.array_equal(full["rows"], want[1][0]) and full["rows"][9] == sc.NAN_ROWS[0] and full["scores"][9] == -np.inf


def test_small_shards():
    for c in sc.SMALL:
        x, q = sc.small_corpus(c["nbins"])
        h = Host((x, q, []), COS)
        nb = so.nb_default(c["k"], 0)
        for qi in range(q.shape[0]):
            m = h.model(qi, c["k"], nb)
            if c["exact"]:
                assert m["status"] == 0 and m["why"] == "whole shard re-scored"
            else:
                assert m["why"] == "certificate" and len(m["bins"]) == nb + 1
            if m["status"] == 0:
                assert np.array_equal(m["rows"], orc.topk_from_scores(h.exact[qi][None, :], c["k"])[1][0])
            assert h.model(qi, c["k"], so.nb_widened(c["k"], 0))["why"] == "whole shard re-scored"


def test_zero_query_and_k_beyond_the_rows():
    x, q = sc.small_corpus(3)
    h = Host((x, np.zeros((1, 768), np.float32), []), COS)
    m = h.model(0, 3, 1)
    assert m["status"] == 0 and m["rows"].tolist() == [0, 1, 2] and (m["scores"] == 0).all()
    h = Host((x[:5], q[:1], []), COS)
    m = h.model(0, 8, 8)
    assert m["status"] == 0 and m["have"] == 5 and m["kk"] == 5 and (m["rows"][5:] == -1).all()


# ---- each assertion rejects a wrong certificate ------------------------------------------------------------------------------------
def test_wrong_certificates_are_rejected():
    """The assertions of tests/test_gpu_select.py (b), on the model's own inputs: status equals the model's; where the status is not
    0 the unrepaired rows equal the model's top k of the re-scored bins."""
    h = Host(sc.main_corpus(), COS)
    q = {n: c["q"] for n, c in h.cases.items()}

    def status(name, **kw):
        return h.model(q[name], sc.K, sc.NB, **kw)["status"]

    right = {n: status(n) for n in q}
    assert right == {"separated": 0, "tied shelf": 1, "wide tied shelf": 1, "ladder steps": 1, "k-th gap": 1, "tiny query": 1}
    # eps dropped: b alone is below s_k wherever the (nb+1)-th bin's best row is (ladder steps: by 0.18 eps)
    assert status("ladder steps", mutant="eps_dropped") == 0 and status("k-th gap", mutant="eps_dropped") == 0
    # the k-th score taken at kk - 2: b + eps = s_k + 0.8 eps is below s_(k-1) = s_k + 0.01
    assert status("k-th gap", mutant="kth_minus_2") == 0
    # the (nb+1)-th key of the next query's list: the wide shelf's 19th bin holds a tie, the ladder steps' (next query) a background row
    nxt = h.rec[q["ladder steps"]]
    assert q["ladder steps"] == q["wide tied shelf"] + 1
    assert h.model(q["wide tied shelf"], sc.K, sc.NB, mutant="next_query_key", next_rec=nxt)["status"] == 0
    # bin ties broken by bin descending: the tied bins' records are equal, so the other end of the shelf is re-scored -- same status,
    # other rows (assertion: unrepaired rows = the model's)
    a, b = h.model(q["tied shelf"], sc.K, sc.NB), h.model(q["tied shelf"], sc.K, sc.NB, mutant="bin_ties_descending")
    assert a["status"] == b["status"] == 1 and not np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["rows"], h.cases["tied shelf"]["ties"][:sc.K])          # (right order: the lowest bins, so the lowest rows)
    # `<=` for `<`: differs only where the fp32 bound EQUALS s_k, which the model calls undecided.  With eps chosen so that
    # fp32(b + eps) == s_k the right certificate refuses and the wrong one certifies (tests/test_gpu_select.py does this on the device
    # with the kernel's own s_k, where nothing is undecided).
    m = h.model(q["separated"], sc.K, sc.NB)
    eps_eq = equal_eps(m["b"], m["sk"])
    eq = so.generic_tail(h.rec[q["separated"]], h.x, h.q[q["separated"]], sc.K, sc.NB, COS, eps_eq, h.mrn)
    assert eq["status"] is None and eq["margin"] == 0.0
    assert so.certified(m["b"], eps_eq, 1.0, 1.0, COS, m["sk"])[0] is False
    assert so.generic_tail(h.rec[q["separated"]], h.x, h.q[q["separated"]], sc.K, sc.NB, COS, eps_eq, h.mrn, mutant="le")["status"] == 0


def equal_eps(b: float, sk: float) -> float:
    """An fp32 eps with fp32(b + eps) == s_k (b < s_k)."""
    e = np.float32(np.float64(sk) - np.float64(b))
    for _ in range(64):
        fb = so.certified(b, e, 1.0, 1.0, COS, sk)[1]
        if fb == np.float32(sk):
            return float(e)
        e = np.nextafter(e, np.float32(np.inf if fb < np.float32(sk) else -np.inf))
    raise AssertionError("no eps reaches s_k")


# ---- the paths of rq_wg_topm that tests/test_gpu_select.py (a) drives -----------------------------------------------------------------
def test_the_merge_shapes_reach_every_path_of_the_workgroup_topm():
    rng = np.random.default_rng(3)
    keys = np.sort(so.make_key(rng.standard_normal(8192).astype(np.float32), rng.permutation(8192)))
    asc = so.wg_topm_steps(keys, 1024)
    assert np.array_equal(asc["result"], so.topm(keys, 1024)) and asc["longest"] == so.SEL_L and asc["compactions"] >= 2 and asc["pruned"] == 0
    desc = so.wg_topm_steps(keys[::-1], 1024)
    assert np.array_equal(desc["result"], so.topm(keys, 1024)) and desc["compactions"] == 2 and desc["pruned"] == 8192 - 4096
    desc = so.wg_topm_steps(keys[::-1], 2)                                     # (the first 4 096 keys are cut to m, nothing later survives the threshold)
    assert desc["pruned"] == 8192 - 4096 and np.array_equal(desc["result"], so.topm(keys, 2))
    for n in (1, 1023, 1024, 1025, 3072, 3073, 4096, 4097):
        for m in (1, 2, 1023, 1024):
            for order in (keys[:n], keys[:n][::-1], keys[rng.permutation(8192)[:n]]):
                assert np.array_equal(so.wg_topm_steps(order, m)["result"], so.topm(order, m))
    # wrong selections.  The compaction test `>=` against RQ_SEL_L: at k = 1 023 an ascending list grows 1 023 + 3 x 1 024 = 4 095 keys
    # without being cut and the next chunk runs past the 4 096 slots (on the device: past the LDS array, so this one is never run there)
    assert so.wg_topm_steps(keys, 1023, compact_at=so.SEL_L)["longest"] > so.SEL_L
    assert so.wg_topm_steps(keys, 1024, compact_at=so.SEL_L)["longest"] == so.SEL_L       # (invisible at k = 1 024)
    # the threshold taken at list[m]: one rank too low, so it keeps out fewer keys and never a winner -- the result is the same for
    # every input; only the work grows
    loose = so.wg_topm_steps(keys[::-1], 2, thr_at=0)
    assert np.array_equal(loose["result"], so.topm(keys, 2)) and loose["pruned"] == desc["pruned"]
    shuf = keys[rng.permutation(8192)]
    assert np.array_equal(so.wg_topm_steps(shuf, 1023, thr_at=0)["result"], so.topm(keys, 1023))
    assert so.wg_topm_steps(shuf, 1023, thr_at=0)["pruned"] <= so.wg_topm_steps(shuf, 1023)["pruned"]
