"""The definition of include/rq.h "router gate" restated one question at a time -- TEST INFRASTRUCTURE, the yardstick of
rag_uq_amd/router.py (host) and csrc/rq_router.hip (device).

All arithmetic is float64, every operation rounded on its own (numpy never fuses a multiply with an add):
  normalisation  "stats": nx = (x - mean) / (std + 1e-6);  "query": mean = S(x) / P, var = S((x - mean)**2) / (P - 1),
                 scale = sqrt(var) + 1e-6, with S the fixed pairwise tree over the column padded with +0.0 to a power of two
  gate           df = nd - nb; a_j = ((W0[j][0]*nb + W0[j][1]*nd) + W0[j][2]*df) + b0[j]; z += w1[j] * (a_j > 0 ? a_j : 0) in order of j;
                 z += b1; w = 1 / (1 + exp(-z))          (one layer: z = ((w1[0]*nb + w1[1]*nd) + w1[2]*df) + b1)
  rerank         h = w*d + (1 - w)*b over the positions i < count with key[i] >= 0; h descending, -0.0 as +0.0, NaN as -inf and
                 returned as it is, equal h by ascending position; padding (-1, 0, 0, 0, 0, -1)
Weights are a dict: {"layers": 1 | 2, "w0": [H][3] fp32, "b0": [H] fp32, "w1": [H] or [3] fp32, "b1": fp32}.
"""
import numpy as np

QUERY, STATS = "query", "stats"
EPS = 1e-6


def tree_sum(col):
    a = [float(v) for v in col]
    n = 1
    while n < len(a):
        n *= 2
    a = np.array(a + [0.0] * (n - len(a)), np.float64)
    while n > 1:
        n //= 2
        for i in range(n):
            a[i] = a[i] + a[i + n]
    return a[0]


def normalise(col, mode, mean=None, std=None):
    col = np.asarray(col, np.float64)
    with np.errstate(all="ignore"):
        if mode == STATS:
            return (col - np.float64(mean)) / (np.float64(std) + EPS)
        P = np.float64(len(col))
        m = np.float64(tree_sum(col)) / P
        e = col - m
        var = np.float64(tree_sum(e * e)) / (P - np.float64(1.0))
        return e / (np.sqrt(var) + EPS)


def logits(weights, b, d, mode, stats=None):
    """z [B][P]"""
    b, d = np.asarray(b, np.float64), np.asarray(d, np.float64)
    z = np.zeros(b.shape, np.float64)
    f64 = lambda k: np.asarray(weights[k], np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        for q in range(b.shape[0]):
            st = stats if stats is not None else (None,) * 4
            nb, nd = normalise(b[q], mode, st[0], st[1]), normalise(d[q], mode, st[2], st[3])
            df = nd - nb
            w1 = f64("w1").reshape(-1)
            b1 = np.float64(np.float32(weights["b1"]))
            if weights["layers"] == 1:
                z[q] = ((w1[0] * nb + w1[1] * nd) + w1[2] * df) + b1
                continue
            w0, b0 = f64("w0"), f64("b0")
            acc = np.zeros(len(nb), np.float64)
            for j in range(w0.shape[0]):
                a = ((w0[j][0] * nb + w0[j][1] * nd) + w0[j][2] * df) + b0[j]
                r = np.where(a > 0, a, 0.0)
                acc = acc + w1[j] * r
            z[q] = acc + b1
    return z


def gate(weights, b, d, mode, stats=None):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-logits(weights, b, d, mode, stats)))


def rerank_given_w(keys, b, d, w, count, top_r):
    """(keys, b, d, w, h, pos, count) of the rerank for GIVEN gate weights: everything of the definition that does not depend on exp."""
    keys, b, d, w = np.asarray(keys), np.asarray(b, np.float64), np.asarray(d, np.float64), np.asarray(w, np.float64)
    B, P = b.shape
    ok, op, oc = np.full((B, top_r), -1, np.int32), np.full((B, top_r), -1, np.int32), np.zeros(B, np.int32)
    ob, od, ow, oh = (np.zeros((B, top_r), np.float64) for _ in range(4))
    for q in range(B):
        c = min(max(int(count[q]), 0), P)
        cand = []
        for i in range(c):
            if keys[q, i] < 0:
                continue
            with np.errstate(all="ignore"):
                h = w[q, i] * d[q, i] + (np.float64(1.0) - w[q, i]) * b[q, i]
            rank = -np.inf if np.isnan(h) else (0.0 if h == 0 else float(h))
            cand.append((-rank, i, h))
        cand.sort(key=lambda t: (t[0], t[1]))
        oc[q] = min(len(cand), top_r)
        for r, (_, i, h) in enumerate(cand[:top_r]):
            ok[q, r], op[q, r], ob[q, r], od[q, r], ow[q, r], oh[q, r] = keys[q, i], i, b[q, i], d[q, i], w[q, i], h
    return ok, ob, od, ow, oh, op, oc


def rerank(weights, keys, b, d, count, top_r, mode, stats=None):
    return rerank_given_w(keys, b, d, gate(weights, b, d, mode, stats), count, top_r)


def same(got, want):
    """Bit for bit: dtype, shape and every byte (NaN payloads and the sign of zero included)."""
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def make_weights(hidden, seed, layers=2):
    rng = np.random.default_rng(seed)
    if layers == 1:
        return {"layers": 1, "w0": None, "b0": None, "w1": rng.uniform(-0.6, 0.6, 3).astype(np.float32), "b1": np.float32(rng.uniform(-0.5, 0.5))}
    lim = 1.0 / np.sqrt(hidden)
    return {"layers": 2, "w0": rng.uniform(-0.58, 0.58, (hidden, 3)).astype(np.float32), "b0": rng.uniform(-0.58, 0.58, hidden).astype(np.float32),
            "w1": rng.uniform(-lim, lim, hidden).astype(np.float32), "b1": np.float32(rng.uniform(-lim, lim))}


STEEP = {"layers": 2, "w0": np.float32([[1000, 0, 0], [-1000, 0, 0]]), "b0": np.float32([0, 0]), "w1": np.float32([10, -10]), "b1": np.float32(0)}   # z = 10 000 nb
CASE_STATS = (3.0, 2.5, 0.1, 0.4)


def _columns(B, P, seed):
    """Fused columns as get_scores_for_router pads them: BM25-like b >= 0, cosine-like d, count per question (0, below P and P all
    occur when B >= 3), (0.0, 0.0, key -1) beyond the count, and a key of -1 below the count."""
    rng = np.random.default_rng(seed)
    b = rng.gamma(2.0, 3.0, (B, P))
    d = rng.uniform(-0.2, 0.9, (B, P))
    count = rng.integers(0, P + 1, B)
    count[0] = P
    if B >= 2:
        count[1] = P // 2
    if B >= 3:
        count[2] = 0
    keys = rng.permutation(4 * P)[None, :P].repeat(B, 0).astype(np.int32) + np.arange(B, dtype=np.int32)[:, None]
    pad = np.arange(P)[None, :] >= count[:, None]
    b[pad], d[pad], keys[pad] = 0.0, 0.0, -1
    if P >= 3:
        keys[:, 1] = -1                                        # a key of -1 below count: no candidate, but normalised and weighted
    return keys, b, d, count.astype(np.int32)


def _top_rs(keys, count, P):
    q = 1 if len(count) > 1 else 0                             # (question 1 of a generated batch is the one cut at P // 2)
    c = int(((np.arange(P) < count[q]) & (keys[q] >= 0)).sum())
    return sorted({r for r in (1, c, c + 1, P) if 1 <= r <= P})


def _case(name, weights, keys, b, d, count, top_rs=None):
    P = b.shape[1]
    return {"name": name, "weights": weights, "keys": np.ascontiguousarray(keys, np.int32), "b": np.ascontiguousarray(b, np.float64),
            "d": np.ascontiguousarray(d, np.float64), "count": np.ascontiguousarray(count, np.int32), "top_rs": top_rs or _top_rs(keys, count, P), "stats": CASE_STATS}


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for P in (1, 2, 63, 64, 65, 128, 129, 256, 257, 1000, 1024):
        out.append(_case(f"p{P}_b3_h16", make_weights(16, P), *_columns(3, P, P)))
    out.append(_case("p100_b1_h64", make_weights(64, 1), *_columns(1, 100, 101)))
    out.append(_case("p100_b70_h64", make_weights(64, 2), *_columns(70, 100, 102)))
    for H in (1, 255, 256):
        out.append(_case(f"p65_b3_h{H}", make_weights(H, 10 + H), *_columns(3, 65, 65 + H)))
    out.append(_case("p129_b3_one_layer", make_weights(0, 5, layers=1), *_columns(3, 129, 77)))
    w16 = make_weights(16, 3)
    # all scores equal: std = 0, the scale is 1e-6
    P = 20
    keys = np.arange(P, dtype=np.int32)[None, :].repeat(2, 0)
    out.append(_case("all_equal", w16, keys, np.full((2, P), 2.0), np.full((2, P), 0.3), [P, 7], [1, 7, 8, P]))
    # a run of exact ties in h cut by top_r: positions 2 .. 11 hold the same (b, d)
    b, d = np.linspace(0.5, 9.0, P)[None, :].repeat(2, 0), np.linspace(0.9, -0.1, P)[None, :].repeat(2, 0)
    b[:, 2:12], d[:, 2:12] = 4.0, 0.5
    out.append(_case("tie_run_cut", w16, keys, b, d, [P, P], [1, 3, 5, 12, P]))
    # h of -0.0: b = d = -0.0 gives (-0.0) + (-0.0); it ranks with the +0.0 of its neighbours by position
    b, d = np.zeros((1, 8)), np.zeros((1, 8))
    b[0, [0, 2, 5]], d[0, [0, 2, 5]] = -0.0, -0.0
    b[0, 7], d[0, 7] = 1.0, -3.0
    out.append(_case("negative_zero_h", w16, np.arange(8, dtype=np.int32)[None, :], b, d, [8], [1, 4, 8]))
    # +-inf and NaN in b or d
    rng = np.random.default_rng(9)
    b, d = rng.gamma(2.0, 3.0, (6, 12)), rng.uniform(-0.2, 0.9, (6, 12))
    b[0, 3], d[1, 4], b[2, 5], d[3, 0], b[4, 1], d[4, 2] = np.inf, np.inf, -np.inf, -np.inf, np.nan, np.nan
    d[5, 6], d[5, 7], b[5, 8] = np.nan, np.inf, np.inf
    out.append(_case("nonfinite", w16, np.arange(12, dtype=np.int32)[None, :].repeat(6, 0), b, d, [12] * 6, [1, 6, 12]))
    # z beyond +-750 (w is exactly 1 or 0), z = +-100 and z = 0
    b = np.array([[1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.0, 0.01, -0.01, 3.0, -3.0, 0.2]])
    d = np.linspace(-1.0, 1.0, 12)[None, :]
    out.append(_case("z_beyond_750", STEEP, np.arange(12, dtype=np.int32)[None, :], b, d, [12], [1, 6, 12]))
    out[-1]["stats"] = (0.0, 1.0, 0.0, 1.0)
    _CASES = out
    return out
