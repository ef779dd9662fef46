"""tests/tail_oracle.py against hand-made score vectors, and every planted geometry of tests/tail_cases.py against the oracle
alone: decided (no ambiguous bin), structured as named, status as intended.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases as tc  # noqa: E402
import tail_oracle as to  # noqa: E402

E = 7e-4


# ---- self-checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nquads,G,m", [(626, 64, 10), (626, 512, 70), (10, 4, 3), (7, 7, 8), (1094, 1024, 100), (130, 128, 9)])
def test_partition_layout(nquads, G, m):
    wg = to.wg_of_quad(nquads, G)
    # the scan's own arithmetic (rq_scan_body.h:88-89), quad by quad
    for b in range(G):
        lo, hi = b * nquads // G, (b + 1) * nquads // G
        assert hi > lo and (wg[lo:hi] == b).all()
    assert wg[0] == 0 and wg[-1] == G - 1 and (np.diff(wg) >= 0).all() and (np.diff(wg) <= 1).all()
    npl = to.npl_of(m)
    assert npl == (1 if m <= 8 else 4 if m <= 64 else 8)
    part = to.partition_of_quad(nquads, G, m)
    # the tail's own loop (rq_tail_body.h:85-88): lane l, slot i reads workgroups i * 64 + l, + 64 * NPL, ...
    for i in range(npl):
        for lane in (0, 1, 63):
            for j in range(i * 64 + lane, G, 64 * npl):
                assert (part[wg == j] == i * 64 + lane).all()


def test_layout_when_the_grid_does_not_divide_the_quads():
    assert to.wg_of_quad(10, 4).tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3, 3]
    assert to.scan_grid(626, 32, 2) == 64 and to.scan_grid(626, 32, 1) == 32 and to.scan_grid(40, 256, 2) == 40 and to.scan_grid(5000, 256, 8) == 1024
    # 1100 workgroups could not exist (stride 1024); 130 workgroups at m = 9 fold onto 256 partitions one to one, at m = 8 onto 64
    assert len(set(to.partition_of_quad(130, 130, 8).tolist())) == 64 and len(set(to.partition_of_quad(130, 130, 9).tolist())) == 130


def test_negative_scores_round_the_other_way():
    f = np.float32
    for v in (f(0.3), f(0.5000123), f(1e-3), f(-0.3), f(-0.5000123), f(-1e-3)):
        # every decoded field is an UPPER bound: up16 / up26 round a positive magnitude up and truncate a negative one
        c = float(to.code16_value(to.code16(v)))
        assert v <= c <= v + 2.0 ** -7 * abs(v)
        assert (abs(c) >= abs(v)) if v > 0 else (abs(c) <= abs(v))
        u = float(to.up26(v))
        assert v <= u <= v + to.ROUND26 * abs(v)
        # ... and the 20-bit truncation of P moves DOWN for either sign: a negative P grows in magnitude
        t = float(to.trunc20(v))
        assert v - 2.0 ** -11 * abs(v) <= t <= v
        assert (abs(t) <= abs(v)) if v > 0 else (abs(t) >= abs(v))
    assert float(to.code16_value(to.code16(f(-np.inf)))) == -np.inf
    assert np.isnan(float(to.trunc20(f(-np.inf))))                        # (the kernel's guard: rq_tail_body.h:101-104)
    assert int(to.code16(f(-0.0))) == int(to.code16(f(0.0))) and float(to.up26(f(-0.0))) == 0.0    # -0.0 counts as +0.0
    # codes are monotone across zero
    vals = np.array([-0.6, -0.3, -1e-3, 0.0, 1e-3, 0.3, 0.6], dtype=np.float32)
    assert (np.diff(to.code16(vals).astype(np.int64)) > 0).all()
    # a negative threshold: scores -0.20 .. -0.29 in ten partitions, the rest at -0.5: T lies BELOW P by 2.25 e and the truncation
    s = np.full(640, -0.5); s[::64] = [-0.20 - 0.01 * i for i in range(10)]
    r = to.model_query(s, 640, 10, E, G=10)
    assert r["ambiguous"].size == 0 and r["P"] == pytest.approx(-0.29)
    assert -0.29 - 3.25 * E - 2.0 ** -11 * 0.29 - 3e-6 <= r["T_lo"] <= r["T_hi"] <= -0.29 - 1.25 * E
    assert r["hit"].sum() == 10 and (r["jobs"][r["hit"] == 1] == 1).all() and r["total"] == 10 and r["status"] == 0


def _bin_jobs(s1, s2, s3, T_at, e=E):
    """One bin with three named scores, threshold pinned near T_at by ten other bins: jobs of bin 0 (m = 1 keeps P on bin 1)."""
    s = np.full(64 * 3, -1.0)
    s[0], s[1], s[2] = s1, s2, s3
    s[64] = T_at + 2.25 * e                                                # P: with m = 2 the second largest partition maximum
    return to.model_query(s, 64 * 3, 2, e, G=3)


def test_one_two_or_sixty_four_jobs_and_a_saturated_d():
    r = _bin_jobs(0.5, 0.1, 0.05, 0.3)
    assert r["ambiguous"].size == 0 and r["jobs"][0] == 1
    r = _bin_jobs(0.5, 0.4, 0.05, 0.3)
    assert r["ambiguous"].size == 0 and r["jobs"][0] == 2
    r = _bin_jobs(0.5, 0.4, 0.35, 0.3)
    assert r["ambiguous"].size == 0 and r["jobs"][0] == 64
    assert _bin_jobs(0.5, 0.3 - 2 * E, 0.05, 0.3)["ambiguous"].tolist() == [0]       # a second score inside the bands: not decided
    # c2 - c3 > 1023 (a third score more than eight octaves below the second, or of the other sign): the record holds d = 1023 and
    # the tail tests decode(c2 - 1023) = about m2 / 256, an upper bound far above the third score itself
    c2, c3 = int(to.code16(np.float32(0.4))), int(to.code16(np.float32(1e-4)))
    assert c2 - c3 > 1023
    sat = float(to.code16_value(np.uint32(c2 - 1023)))
    assert 0.4 / 256 <= sat <= 0.4 / 256 * (1 + 2.0 ** -6)
    r = _bin_jobs(0.5, 0.4, 1e-4, sat - 8e-5, e=2e-5)                            # T below decode(c2 - 1023): whole bin although m3 << T
    assert r["ambiguous"].size == 0 and r["T_hi"] < sat and r["jobs"][0] == 64 and r["T_lo"] > 1e-4 + 2 * 2e-5
    r = _bin_jobs(0.5, 0.4, 1e-4, sat + 8e-5, e=2e-5)                            # T above it: two rows
    assert r["ambiguous"].size == 0 and r["jobs"][0] == 2
    r = _bin_jobs(0.5, 0.4, -0.2, 0.3)                                     # the other sign saturates too
    assert int(to.code16(np.float32(0.4))) - int(to.code16(np.float32(-0.2))) > 1023 and r["jobs"][0] == 2


def test_caps_and_local_topk_in_the_model():
    def tied(nb, nbins=1100, **kw):
        s = np.full(nbins * 64, 0.0)
        for b in (range(nb) if isinstance(nb, int) else nb):
            s[b * 64:(b + 1) * 64] = 0.5
        return to.model_query(s, nbins * 64, 10, E, G=nbins, **kw)
    r = tied(32)
    assert r["njob"].tolist() == [2048, 0, 0] and r["total"] == 10 and r["status"] == 0 and not r["overflow"]
    assert tied(32, tail_local=False)["total"] == 2048
    r = tied(33)
    assert r["ovf_job"] and r["total"] == 2112 and r["status"] == 1
    r = tied(list(range(30)) + list(range(512, 542)) + list(range(1024, 1049)), tail_local=False)   # 1 920 + 1 920 + 1 600 keys wanted
    assert not r["ovf_job"] and not r["ovf_hit"] and r["ovf_cand"] and r["status"] == 1
    # more than 768 hit bins of one job each in one chunk of 2 048 bins; fine in chunks of 512
    s = np.zeros(1100 * 64); s[:800 * 64:64] = 0.5
    assert to.model_query(s, s.size, 10, E, G=1024, nv=4)["total"] == 10      # (768 jobs: the workgroup publishes its own k best)
    assert to.model_query(s, s.size, 10, E, G=1024, nv=4)["ovf_hit"] and to.model_query(s, s.size, 10, E, G=1024, nv=4, tail_local=False)["total"] == 768
    r = to.model_query(s, s.size, 10, E, G=1024, nv=1)
    assert not r["overflow"] and r["nh"].tolist() == [512, 288, 0] and r["total"] == 20 and r["status"] == 0
    # fewer partitions with anything in them than m: T = -inf, every bin is taken whole
    r = to.model_query(np.linspace(0, 1, 640), 640, 10, E, G=5)
    assert r["T_hi"] == -np.inf and (r["jobs"] == 64).all() and r["total"] == 10 and r["status"] == 0
    # k beyond the rows in play (a filter that leaves 3 rows): m = 3, have = 3 = kk
    al = np.zeros(640, dtype=bool); al[[5, 70, 300]] = True
    r = to.model_query(np.linspace(0, 1, 640), 640, 10, E, G=10, allowed=al)
    assert r["m"] == 3 and r["have"] == 3 and r["status"] == 0 and r["hit"].sum() == 3
    assert to.model_query(np.ones(640), 640, 10, E, G=10, qnorm=1e-18)["status"] == 1
    assert to.model_query(np.ones(640), 640, 10, E, G=10, qnorm=0.0)["status"] == 0


def test_shard_eps_follows_scan_eps():
    x = np.zeros((3, 8), dtype=np.float16)
    x[0] = 0.25
    x[1, :4] = 0.5; x[1, 4:] = np.float16(3e-5)                            # four fp16-subnormal elements
    x[2] = 0
    eps, mrn = to.shard_eps(x, to.METRIC_COSINE)
    sub = np.sqrt(4 * float(np.float16(3e-5)) ** 2)
    nrm = np.sqrt(4 * 0.25 + sub * sub)
    assert mrn == pytest.approx(nrm) and eps == pytest.approx(7e-4 + sub / nrm, rel=1e-6)
    assert to.shard_eps(x, to.METRIC_IP)[0] == pytest.approx(7e-4 + sub / nrm, rel=1e-6)
    assert to.tail_bound(1e-3, 2.0, to.METRIC_IP) == pytest.approx(2e-3, rel=1e-5) and to.tail_bound(1e-3, 2.0, 0) == pytest.approx(1e-3, rel=1e-6)


def test_planting_reaches_its_targets_and_the_oracle_reads_the_stored_rows():
    rng = np.random.default_rng(1)
    x = np.zeros((20, 768), dtype=np.float16)
    u = to.unit(rng.standard_normal(768))
    to.plant(x, [3, 7, 11], [0.5, -0.25, 0.999], u, rng, norms=[1.0, 2.0, 0.5])
    s = to.unit_scores(u[None, :].astype(np.float32), x, to.METRIC_COSINE)[0]
    assert np.abs(s[[3, 7, 11]] - [0.5, -0.25, 0.999]).max() < 2e-4 and not s[[0, 1, 19]].any()
    ip = to.unit_scores(3 * u[None, :].astype(np.float32), x, to.METRIC_IP)[0]
    assert np.abs(ip[[3, 7, 11]] - [0.5, -0.5, 0.4995]).max() < 4e-4


# ---- the geometries ------------------------------------------------------------------------------------------------------------
def _models(corpus, metric=to.METRIC_COSINE, **kw):
    x, q, cases = corpus
    S = to.unit_scores(q, x, metric)                                       # computed once, shared, never changed
    out = {}
    for c in cases:
        for tl in (False, True):
            out[c["name"], tl] = tc.run_model(x, q, c, metric=metric, tail_local=tl, scores=S[c["q"]], **kw)
    return out, S


@pytest.fixture(scope="module")
def base():
    x, q, cases = tc.base_corpus()
    models, S = _models((x, q, cases))
    return x, q, {c["name"]: c for c in cases}, models, S


BASE_NAMES = ["spread", "pair(0, 63)", "pair(31, 32)", "triple", "triple_ragged", "ties", "concentrated", "jobcap32", "jobcap33",
              "rank256", "rank257", "rank512", "rank513"]


def _structure(c, r0, r1, s):
    """What every case names: the winners, the hit bins, the jobs of the named bins, totals and status under tail_local 0 / 1."""
    order = np.lexsort((np.arange(s.size), -s))
    if "winners" in c:
        assert sorted(order[:c["k"]].tolist()) == sorted(np.asarray(c["winners"]).tolist())
    hits = np.nonzero(r0["hit"] == 1)[0].tolist()
    if "hit_bins" in c:
        assert hits == sorted(c["hit_bins"])
    for b, nj in c.get("jobs", {}).items():
        assert r0["jobs"][b] == nj, (b, int(r0["jobs"][b]))
    st = c["status"] if isinstance(c["status"], dict) else {0: c["status"], 1: c["status"]}
    assert (r0["status"], r1["status"]) == (st[0], st[1])
    if "total" in c:
        assert (r0["total"], r1["total"]) == (c["total"][0], c["total"][1])
    if "njob0" in c:
        assert r0["njob"][0] == c["njob0"] and r0["njob"][1:].sum() == 0
    return order, hits


def test_every_geometry_is_decided(base):
    """At most 0 geometries may be ambiguous."""
    x, q, cases, models, S = base
    assert sorted(cases) == sorted(BASE_NAMES)
    amb = [(name, r["ambiguous"][:4].tolist()) for name, r in models.items() if r["ambiguous"].size]
    assert not amb, amb


@pytest.mark.parametrize("name", BASE_NAMES)
def test_geometry_has_the_claimed_structure(base, name):
    x, q, cases, models, S = base
    c = cases[name]
    r0, r1 = models[name, False], models[name, True]
    s = S[c["q"]]
    order, hits = _structure(c, r0, r1, s)
    top = s[order[:c["k"]]]
    if name == "spread":
        pos = {int(w) % 64 for w in c["winners"]}
        assert {0, 63} <= pos and {511, 512, 625} <= {int(w) // 64 for w in c["winners"]} and max(c["winners"]) == x.shape[0] - 1
        assert (r0["jobs"][hits] == 1).all() and r0["nh"].tolist() == [8, 3]
    if name.startswith("pair"):
        b = int(order[0]) // 64
        inbin = np.sort(s[b * 64:(b + 1) * 64])[::-1]
        assert int(order[1]) // 64 == b and inbin[1] > r0["T_hi"] + 0.1 and inbin[2] < r0["T_lo"] - 0.1   # third best of the bin far below T_lo
        assert {int(order[0]) % 64, int(order[1]) % 64} == ({0, 63} if name == "pair(0, 63)" else {31, 32})
    if name.startswith("triple"):
        b = int(order[0]) // 64
        assert [int(o) // 64 for o in order[:3]] == [b] * 3 and r0["jobs"][b] == 64
        assert r0["total"] == 64 + 9 and (b == 625) == (name == "triple_ragged")
        if name == "triple_ragged":
            assert r0["njob"].tolist() == [9, 64] and r1["total"] == 9 + 10 and r0["rescored"] == 9 + 37   # local top-k reserves k slots for 37 live rows
    if name == "ties":
        assert (s[300 * 64:301 * 64 + 10] == s[300 * 64]).all() and s[300 * 64] > 0.999 and s[301 * 64 + 10] < 0.3
        assert order[:10].tolist() == list(range(300 * 64, 300 * 64 + 10))
        assert order[:70].tolist() == list(range(300 * 64, 300 * 64 + 70))
    if name == "concentrated":
        wg = to.wg_of_quad(626, 64)
        assert {int(wg[int(w) // 64]) for w in c["winners"]} == {20}
        assert r0["P"] < top.min() - 0.15 and 0.32 < r0["P"] < 0.34       # P sits on the ninth shelf row, far below the winners
        assert len(hits) == 17 and r0["total"] == 19 and r1["total"] == 10
    if name.startswith("jobcap") or name.startswith("rank"):
        assert r0["ovf_job"] == (name == "jobcap33") and not r0["ovf_cand"] and not r0["ovf_hit"]
        tied = np.concatenate([s[b * 64:(b + 1) * 64] if nj == 64 else s[b * 64:(b + 1) * 64].max(keepdims=True) for b, nj in c["jobs"].items()])
        assert tied.max() - tied.min() <= 1e-4 and tied.size == c["njob0"]


def test_ties_at_k_70_on_a_grid_of_512_workgroups(base):
    x, q, cases, models, S = base
    c = dict(cases["ties"], k=70)
    r = tc.run_model(x, q, c, G=to.scan_grid(626, 256, 2), scores=S[c["q"]])
    assert r["G"] == 512 and r["ambiguous"].size == 0 and r["status"] == 0 and r["jobs"][300] == 64 and r["jobs"][301] == 64
    assert 0.30 < r["P"] < 0.32                                            # the 70th partition maximum is a shelf row
    # on the 64-workgroup grid fewer than 70 partitions hold anything: T = -inf, every bin whole, the job cap overflows
    r = tc.run_model(x, q, c, scores=S[c["q"]])
    assert r["T_hi"] == -np.inf and r["ovf_job"] and r["status"] == 1


def test_other_grids_decide_what_the_gpu_tests_ask_of_them(base):
    """The 192-query call holds spread and concentrated against the wide grid of 32 workgroups too; a card of 256 CUs runs 512."""
    x, q, cases, models, S = base
    for name in ("spread", "concentrated"):
        r = tc.run_model(x, q, cases[name], G=32, scores=S[cases[name]["q"]])
        assert r["ambiguous"].size == 0 and r["status"] == 0
    for c in cases.values():
        assert tc.run_model(x, q, c, G=512, scores=S[c["q"]])["ambiguous"].size == 0


def test_filtered_geometries_are_decided(base):
    """The filter of tests/test_gpu_tail.py: the pair loses its second winner, the triple its middle one, one of spread's hit bins
    every background row.  The pair's bin becomes one job, the triple's two, and the bin of one allowed row stays one job."""
    x, q, cases, models, S = base
    allowed = tc.base_filter(x.shape[0], cases, S)
    for name, nj in (("pair(0, 63)", 1), ("triple", 2), ("spread", 1)):
        c = cases[name]
        r = tc.run_model(x, q, c, scores=S[c["q"]], allowed=allowed)
        b = int(np.asarray(c["winners"])[0]) // 64 if name != "spread" else 77
        assert r["ambiguous"].size == 0 and r["status"] == 0 and r["jobs"][b] == nj, (name, int(r["jobs"][b]))
    assert allowed[77 * 64:78 * 64].sum() == 1 and (~allowed).sum() == 65


@pytest.mark.parametrize("dim", [768, 384])
@pytest.mark.parametrize("metric", [to.METRIC_COSINE, to.METRIC_IP])
def test_negative_geometry(dim, metric):
    xn, qn, cn = tc.negative_corpus(dim)
    c = cn[0]
    s = to.unit_scores(qn[0], xn, metric)[0]
    assert s.max() < (-0.09 if metric == to.METRIC_COSINE else -0.04) and (s < 0).all()
    r0, r1 = (tc.run_model(xn, qn, c, metric=metric, tail_local=tl, scores=s) for tl in (False, True))
    order, hits = _structure(c, r0, r1, s)
    assert int(order[0]) == xn.shape[0] - 1 and r0["T_hi"] < r0["P"] < 0 and (r0["jobs"][hits] == 1).all()


def test_narrow_corpus_is_decided():
    x, q, cases = tc.base_corpus(384)
    models, S = _models((x, q, cases))
    for c in cases:
        if c["name"] in ("spread", "pair(0, 63)", "pair(31, 32)", "triple", "triple_ragged"):
            _structure(c, models[c["name"], False], models[c["name"], True], S[c["q"]])
    assert not [n for n, r in models.items() if r["ambiguous"].size]


def test_mixed_signs_geometry():
    x, q, cases = tc.mixed_corpus()
    models, S = _models((x, q, cases))
    c, s = cases[0], S[0]
    order, hits = _structure(c, models["mixed", False], models["mixed", True], s)
    top = s[order[:50]]
    assert (top > 0).sum() == 27 and (top < 0).sum() == 23 and (s > 0).sum() == 27
    assert models["mixed", False]["njob"].tolist() == [617] and -0.43 < models["mixed", False]["P"] < -0.41


def test_candidate_and_hit_caps():
    x, q, cases = tc.candcap_corpus()
    models, S = _models((x, q, cases))
    _structure(cases[0], models["candcap", False], models["candcap", True], S[0])
    r0 = models["candcap", False]
    assert r0["njob"].tolist() == [1408] * 3 and r0["ovf_cand"] and not r0["ovf_job"] and not r0["ovf_hit"] and not models["candcap", True]["overflow"]
    x, q, cases = tc.hitcap_corpus()
    models, S = _models((x, q, cases))
    _structure(cases[0], models["hitcap", False], models["hitcap", True], S[0])
    assert models["hitcap", False]["nh"].tolist() == [512, 288] and not models["hitcap", False]["overflow"]
    one, _ = _models((x, q, cases), nv=4)                                  # one chunk of 2 048 bins: 800 hits > 768
    assert one["hitcap", True]["ovf_hit"] and one["hitcap", True]["status"] == 1 and one["hitcap", False]["status"] == 1
    assert (one["hitcap", False]["total"], one["hitcap", True]["total"]) == (768, 10)      # 768 hits of one job each keep their jobs
