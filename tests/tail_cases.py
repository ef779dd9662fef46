"""The planted corpora of tests/test_tail_oracle.py (CPU: every geometry is decided and structured as named) and
tests/test_gpu_tail.py (the kernel against tests/tail_oracle.py on the same corpora).  numpy only.

One background corpus hosts one geometry per query: a row planted for query j is background for every other query.  Each case
names the query, k, and what the oracle must find; nothing here looks at kernel output.
"""
from __future__ import annotations

import functools

import numpy as np

import tail_oracle as to

DIM = 768
BASE_N = 40_037            # 626 bins, a ragged last bin of 37 rows, two 512-bin chunks at NV = 1
BASE_CU, BASE_WG = 32, 2   # scan grid G = 64 whatever the card
NEG_N = 8_229              # 129 bins, ragged last bin of 37 rows: the all-negative corpus


class Planner:
    """Hands out bins of a corpus so that no two geometries touch the same bin, and plants rows."""

    def __init__(self, x16: np.ndarray, seed: int, G: int):
        self.x = x16
        self.n = x16.shape[0]
        self.nbins = (self.n + 63) // 64
        self.rng = np.random.default_rng(seed)
        self.used = set()
        self.G = G
        self.wg = to.wg_of_quad(self.nbins, G)

    def take(self, *bins):
        for b in bins:
            assert 0 <= b < self.nbins and b not in self.used, f"bin {b} taken twice"
            self.used.add(b)

    def free_bins(self, count: int, lo: int = 0, hi: int = None, avoid_wgs=(), step: int = 1) -> list:
        """The first `count` free bins of [lo, hi), at most one per scan workgroup (G of the planner), none in avoid_wgs."""
        hi = self.nbins - 1 if hi is None else hi          # (the ragged last bin is only taken by name)
        out, wgs = [], set(avoid_wgs)
        for b in range(lo, hi, step):
            if b in self.used or int(self.wg[b]) in wgs:
                continue
            out.append(b); wgs.add(int(self.wg[b])); self.used.add(b)
            if len(out) == count:
                return out
        raise AssertionError(f"only {len(out)} of {count} free bins in [{lo}, {hi})")

    def plant(self, u, bins, poss, cosines, norms=None):
        rows = np.asarray(bins, dtype=np.int64) * 64 + np.asarray(poss, dtype=np.int64)
        assert rows.max() < self.n
        to.plant(self.x, rows, cosines, u, self.rng, norms)
        return rows


def _gaussian_unit_rows(n, seed, dim=DIM):
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    x64 = x.astype(np.float64)
    return (x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))).astype(np.float32).astype(np.float16)


@functools.lru_cache(maxsize=None)
def base_corpus(dim: int = DIM):
    """(x16, queries [B][dim] fp32, cases): the 40 037-row Gaussian shard with geometries 1-5, 8 and 11 planted, one per query
    (dim 384: the narrow layout's own corpus, same plan)."""
    x = _gaussian_unit_rows(BASE_N, 20261 + dim, dim)
    G = to.scan_grid((BASE_N + 63) // 64, BASE_CU, BASE_WG)
    p = Planner(x, 20262, G)
    wg = p.wg
    dirs = to.unit(np.random.default_rng(20263).standard_normal((16, dim)))
    cases = []
    step = lambda n, top=0.59: [round(top - 0.01 * i, 2) for i in range(n)]

    # 1. spread: ten winners 0.59 .. 0.50 in ten bins; positions 0 and 63; bins 511 | 512 (chunk boundary); the last valid row of
    #    the ragged last bin.  At G = 64 quads 508 .. 517 belong to ONE workgroup, so bins 511 and 512 share a partition: the ten
    #    winners cover nine partitions and an eleventh planted row (0.45) holds the tenth, which is where P lands.
    sb = [3, 77, 150, 222, 290, 365, 440, 511, 512, 625]
    p.take(*sb)
    assert len({int(wg[b]) for b in sb}) == 9 and wg[511] == wg[512]
    sp = [0, 63, 17, 5, 40, 62, 1, 63, 0, BASE_N - 1 - 625 * 64]
    shelf = p.free_bins(1, lo=560, avoid_wgs=[int(wg[b]) for b in sb])
    rows = p.plant(dirs[0], sb + shelf, sp + [9], step(10) + [0.45])
    cases.append(dict(name="spread", q=0, k=10, winners=rows[:10], hit_bins=sb + shelf, jobs={b: 1 for b in sb + shelf}, total={0: 11, 1: 11}, status=0))

    # 4. ties across a bin boundary: 64 identical rows fill bin 300, bin 301 starts with 10 more.  The query is that row.  72 more
    #    rows planted 0.655, 0.650, ... (steps of 0.005) in other workgroups keep P on a planted level for k = 10 and, on a grid of
    #    more than 70 workgroups, for k = 70.
    p.take(300, 301)
    v = to.unit(dirs[5]).astype(np.float32).astype(np.float16)
    x[300 * 64:301 * 64 + 10] = v
    sh = []
    for b in range(4, 625):                      # one bin in eight, so that a grid of 512 workgroups keeps them apart too
        if b % 8 == 4 and b not in p.used and len(sh) < 72 and abs(b - 300) > 2:
            sh.append(b); p.used.add(b)
    assert len(sh) == 72
    tie_u = v.astype(np.float64)
    p.plant(tie_u, sh, [(5 * i) % 64 for i in range(72)], [0.655 - 0.005 * i for i in range(72)])
    cases.append(dict(name="ties", q=5, k=10, winners=np.arange(300 * 64, 300 * 64 + 10), jobs={300: 64, 301: 64}, status=0, query=v.astype(np.float32),
                      shelf=sh))

    # 2. pair: two winners in one bin (positions (0, 63) and (31, 32)), the bin's third best is background; eight more winners in
    #    eight other partitions and one more planted row (0.45) in a tenth.
    for qi, pp in ((1, (0, 63)), (2, (31, 32))):
        bins = p.free_bins(10, lo=20 + 7 * qi, step=3)
        rows = p.plant(dirs[qi], [bins[0]] + bins, [pp[0], pp[1]] + [11 + 3 * i for i in range(9)], step(10) + [0.45])
        cases.append(dict(name=f"pair{pp}", q=qi, k=10, winners=rows[:10], hit_bins=bins, jobs={**{b: 1 for b in bins[1:]}, bins[0]: 2}, status=0))

    # 3. triple: three winners in one bin -> the whole bin; seven more winners and two planted rows (0.45, 0.44) in nine other
    #    partitions.  Variant: the bin is the ragged last one (27 of its 64 jobs lie beyond the shard's end: key 0).
    bins = p.free_bins(10, lo=30, hi=500, step=5)
    rows = p.plant(dirs[3], [bins[0]] * 3 + bins[1:], [7, 8, 60] + [2 + 5 * i for i in range(9)], step(10) + [0.45, 0.44])
    cases.append(dict(name="triple", q=3, k=10, winners=rows[:10], hit_bins=bins, jobs={**{b: 1 for b in bins[1:]}, bins[0]: 64}, status=0))
    # (spread's winner sits in the last bin too, at row 36: other rows of the same bin, which is background for this query)
    bins = [625] + p.free_bins(9, lo=33, hi=500, step=5, avoid_wgs=[int(wg[625])])
    rows = p.plant(dirs[4], [625] * 3 + bins[1:], [0, 20, 35] + [3 + 5 * i for i in range(9)], step(10) + [0.45, 0.44])
    cases.append(dict(name="triple_ragged", q=4, k=10, winners=rows[:10], hit_bins=bins, jobs={**{b: 1 for b in bins[1:]}, 625: 64}, status=0))

    # 5. concentrated: all ten winners inside the quads of scan workgroup 20 (two bins hold two each); twelve planted rows
    #    0.41 .. 0.30 in twelve other workgroups: P is the NINTH of those, far below the winners.
    own = [b for b in range(p.nbins) if wg[b] == 20 and b not in p.used][:8]
    p.take(*own)
    assert len(own) == 8
    sh = p.free_bins(12, lo=10, hi=600, step=37, avoid_wgs=[20])   # (37 bins apart: distinct workgroups on a grid of 32 too)
    rows = p.plant(dirs[6], own + own[:2] + sh, [1, 2, 3, 4, 5, 6, 7, 8, 33, 34] + [13] * 12, step(10) + step(12, 0.41))
    cases.append(dict(name="concentrated", q=6, k=10, winners=rows[:10], one_wg=20, status=0))

    # 8. job cap: 32 (33) bins of 64 rows tied within 4e-5 (inside the issue's 1e-4), all in chunk 0, one bin per scan workgroup:
    #    exactly 2 048 jobs certify, 2 112 overflow.
    for qi, nb, name in ((7, 32, "jobcap32"), (8, 33, "jobcap33")):
        bins = p.free_bins(nb, lo=qi - 7, hi=512)
        rr = np.concatenate([np.arange(b * 64, b * 64 + 64) for b in bins])
        to.plant(x, rr, 0.5 + p.rng.uniform(0.0, 4e-5, rr.size), dirs[qi], p.rng)
        cases.append(dict(name=name, q=qi, k=10, jobs={b: 64 for b in bins}, hit_bins=bins, njob0=64 * nb,
                          total={0: 64 * nb, 1: 10 if nb == 32 else 64 * nb}, status=0 if nb == 32 else 1))

    # 11. ranking paths, k = 3 (64 partitions, so P sits on the tied level without a shelf): W whole bins of tied rows in chunk 0,
    #     one per scan workgroup, plus `extra` single tied rows in further workgroups: 256 | 257 jobs in one tail workgroup (all-pairs
    #     ranking | rq_select_winners with tail_local = 1), 512 | 513 keys in the query's list (rq_final_body with tail_local = 0).
    for qi, nb, extra in ((9, 4, 0), (10, 4, 1), (11, 8, 0), (12, 8, 1)):
        bins = p.free_bins(nb + extra, lo=qi, hi=512)
        rr = np.concatenate([np.arange(b * 64, b * 64 + 64) for b in bins[:nb]] + [np.array([b * 64 + 21], dtype=np.int64) for b in bins[nb:]])
        to.plant(x, rr, 0.5 + p.rng.uniform(0.0, 4e-5, rr.size), dirs[qi], p.rng)
        cases.append(dict(name=f"rank{64 * nb + extra}", q=qi, k=3, jobs={**{b: 64 for b in bins[:nb]}, **{b: 1 for b in bins[nb:]}}, hit_bins=bins,
                          njob0=64 * nb + extra, total={0: 64 * nb + extra, 1: 3}, status=0))

    B = 13
    q = (2.5 * dirs[:B]).astype(np.float32)
    q[5] = v.astype(np.float32)
    return x, q, cases


@functools.lru_cache(maxsize=None)
def negative_corpus(dim: int = DIM):
    """(x16, queries, cases): 8 229 rows that ALL score negative for the query 3 u: row = norm * (-c u + noise), c in 0.42 .. 0.60,
    norm in 0.5 .. 2.  14 rows of norm 0.5 are planted at cosines -0.10, -0.12, ... (inner product / |q|: -0.05, -0.06, ...) in 14
    workgroups, the best one at the last valid row of the ragged last bin: the first ten win under both metrics (geometry 6)."""
    rng = np.random.default_rng(20271 + dim)
    u = to.unit(rng.standard_normal(dim))
    x = np.empty((NEG_N, dim), dtype=np.float16)
    to.plant(x, np.arange(NEG_N), -rng.uniform(0.42, 0.60, NEG_N), u, rng, norms=rng.uniform(0.5, 2.0, NEG_N))
    G = to.scan_grid((NEG_N + 63) // 64, BASE_CU, BASE_WG)
    p = Planner(x, 20272, G)
    p.take(128)
    bins = [128] + p.free_bins(13, lo=2, step=3, avoid_wgs=[int(p.wg[128])])
    rows = p.plant(u, bins, [NEG_N - 1 - 128 * 64] + [(7 * i) % 64 for i in range(13)], [-0.10 - 0.02 * i for i in range(14)], norms=[0.5] * 14)
    cases = [dict(name="negative", q=0, k=10, winners=rows[:10], hit_bins=bins[:10], jobs={b: 1 for b in bins[:10]}, total={0: 10, 1: 10}, status=0)]
    return x, (3.0 * u[None, :]).astype(np.float32), cases


@functools.lru_cache(maxsize=None)
def mixed_corpus():
    """Geometry 7 (k = 50): background rows score -0.50 .. -0.65; 27 POSITIVE rows 0.57, 0.55, ... 0.05 sit three to a bin in nine
    workgroups (nine whole-bin jobs: 576 rows of both signs), 45 negative rows -0.02, -0.03, ... -0.46 one per bin in 45 more.  The
    top 50 are the 27 positive rows and 23 negative ones; P is the 50th partition maximum (-0.42).  617 keys of mixed sign reach
    the final select (tail_local 0) or the workgroup's own (tail_local 1): their leading bits differ in bit 63."""
    rng = np.random.default_rng(20291)
    u = to.unit(rng.standard_normal(DIM))
    x = np.empty((NEG_N, DIM), dtype=np.float16)
    to.plant(x, np.arange(NEG_N), -rng.uniform(0.50, 0.65, NEG_N), u, rng)
    p = Planner(x, 20292, to.scan_grid((NEG_N + 63) // 64, BASE_CU, BASE_WG))
    bins = p.free_bins(54, lo=0)
    pos_bins, neg_bins = bins[:9], bins[9:]
    rows = p.plant(u, [b for b in pos_bins for _ in range(3)] + neg_bins, [0, 31, 63] * 9 + [(11 * i) % 64 for i in range(45)],
                   [0.57 - 0.02 * i for i in range(27)] + [-0.02 - 0.01 * i for i in range(45)])
    cases = [dict(name="mixed", q=0, k=50, winners=rows[:50], jobs={**{b: 64 for b in pos_bins}, **{b: 1 for b in neg_bins[:41]}},
                  hit_bins=pos_bins + neg_bins[:41], total={0: 617, 1: 50}, status=0)]
    return x, (2.0 * u[None, :]).astype(np.float32), cases


def _tied_corpus(n, seed, plan):
    """A Gaussian shard of n rows with, for ONE query direction, rows tied within 4e-5 at 0.5: plan(planner) -> (whole bins, single bins)."""
    x = _gaussian_unit_rows(n, seed)
    p = Planner(x, seed + 1, to.scan_grid((n + 63) // 64, BASE_CU, BASE_WG))
    u = to.unit(np.random.default_rng(seed + 2).standard_normal(DIM))
    whole, single = plan(p)
    rr = np.concatenate([np.arange(b * 64, b * 64 + 64) for b in whole] + [np.array([b * 64 + (5 * b) % 64], dtype=np.int64) for b in single])
    to.plant(x, rr, 0.5 + p.rng.uniform(0.0, 4e-5, rr.size), u, p.rng)
    return x, (1.7 * u[None, :]).astype(np.float32), whole, single


@functools.lru_cache(maxsize=None)
def candcap_corpus():
    """Geometry 9: 70 000 rows = 1 094 bins = chunks of 512, 512 and 70 bins; 22 whole bins of tied rows in each chunk: 1 408 jobs
    per tail workgroup (below the job cap), 4 224 keys for the query's list of 4 096."""
    def plan(p):
        return p.free_bins(22, lo=0, hi=512) + p.free_bins(22, lo=512, hi=1024) + [b for b in range(1024, 1093, 3)][:22], []
    x, q, whole, _ = _tied_corpus(70_000, 20301, plan)
    cases = [dict(name="candcap", q=0, k=10, jobs={b: 64 for b in whole}, hit_bins=whole, total={0: 4224, 1: 30}, status={0: 1, 1: 0})]
    return x, q, cases


@functools.lru_cache(maxsize=None)
def hitcap_corpus():
    """Geometry 10: 52 000 rows = 813 bins; 800 bins hold one tied row each.  Chunks of 512 bins see 512 and 288 hits; ONE chunk of
    2 048 bins (the riding tail with "fused_nv" = 4) sees 800 > RQ_TAIL_HITCAP and gives up."""
    def plan(p):
        return [], list(range(800))
    x, q, _, single = _tied_corpus(52_000, 20311, plan)
    cases = [dict(name="hitcap", q=0, k=10, jobs={b: 1 for b in single}, hit_bins=single, total={0: 800, 1: 20}, status=0)]
    return x, q, cases


def base_filter(n: int, cases: dict, S: np.ndarray) -> np.ndarray:
    """Allowed rows of the filtered form: everything but the second winner of pair(0, 63), the middle winner of the triple, and the
    63 background rows of bin 77 (a hit bin of `spread`, whose winner sits at position 63)."""
    allowed = np.ones(n, dtype=bool)
    for name, rank in (("pair(0, 63)", 1), ("triple", 1)):
        s = S[cases[name]["q"]]
        order = np.lexsort((np.arange(s.size), -s))
        allowed[order[rank]] = False
    allowed[77 * 64:77 * 64 + 63] = False
    return allowed


_EPS = {}     # (corpora are cached and never changed: their bound is computed once)


def run_model(x16, q, case, metric=to.METRIC_COSINE, G=None, nv=1, tail_local=True, eps=None, allowed=None, scores=None):
    """The oracle on one case of a corpus."""
    key = (id(x16), metric)
    if key not in _EPS:
        _EPS[key] = to.shard_eps(x16, metric)
    mrn = _EPS[key][1]
    if eps is None:
        eps = _EPS[key][0]
    e = to.tail_bound(eps, mrn, metric)
    n = x16.shape[0]
    if G is None:
        G = to.scan_grid((n + 63) // 64, BASE_CU, BASE_WG)
    s = to.unit_scores(q[case["q"]], x16, metric)[0] if scores is None else scores
    qn = float(np.sqrt((q[case["q"]].astype(np.float64) ** 2).sum()))
    return to.model_query(s, n, case["k"], e, G, nv=nv, tail_local=tail_local, metric=metric, qnorm=qn, allowed=allowed)
