"""Oracle for the encoder kernels (include/rq.h rq_nb_*, csrc/rq_encoder.hip) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain numpy, fp64 arithmetic on the fp16 inputs, no torch and no GPU: every operation the seven entry points compute, the error
bounds the GPU tier (tests/test_gpu_encoder.py) asserts, and the INPUTS of that tier.  The CPU tier (tests/test_encoder.py) builds
the same inputs with the same functions and proves on them that each bound rejects a plausible wrong kernel."""
import numpy as np

HEAD_DIM = 64
U16 = 2.0 ** -11                   # unit roundoff of fp16 (round to nearest)
U32 = 2.0 ** -24                   # ... of fp32

# The three constants that cannot be derived from the number formats alone: measured on the MI355X against this oracle and committed
# at twice the observed excess, under the caps the bounds were designed with (DESIGN 4.14 has the observed values).
ROPE_C, ROPE_C_CAP = 4.5, 8.0      # rotary table: fp32 angle error in units of 2^-24 * angle (powf decides it); observed 2.22
ATTN_T, ATTN_T_CAP = 2.0, 4.0      # attention: error in units of 2^-11 * A; 2 is derived (P to fp16, output to fp16); observed 1.36
LN_K, LN_K_CAP = 1.1, 64.0         # LayerNorm: fp32 statistics, in units of E = 2^-24 (|mean| + sigma) / sigma |gamma|; observed 0.51


# ---- the operations ------------------------------------------------------------------------------------------------------------
def rope_angles(seq, theta):
    """float64 [seq][32]: pos * theta^(-d / 32)."""
    pos = np.arange(seq, dtype=np.float64)[:, None]
    return pos * np.float64(theta) ** (-np.arange(32, dtype=np.float64) / 32.0)[None, :]


def rope_table(seq, theta):
    """float64 [seq][64]: the cosines of the 32 angles of a position, then their sines (include/rq.h rq_nb_rope_table_f32)."""
    ang = rope_angles(seq, theta)
    return np.concatenate([np.cos(ang), np.sin(ang)], axis=1)


def identity_rope(seq):
    """The table that rotates nothing (cos = 1, sin = 0): q and k reach the matrix cores unchanged."""
    t = np.zeros((seq, 64), dtype=np.float32)
    t[:, :32] = 1.0
    return t


def _rotate(x, rope):
    """Rotate-half: x [n][heads][64], rope [n][64] -> x'[d] = x[d] c - x[d + 32] s, x'[d + 32] = x[d + 32] c + x[d] s."""
    c, s = rope[:, None, :32], rope[:, None, 32:]
    lo, hi = x[..., :32], x[..., 32:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1)


def attention(qkv16, lens, rope, B, L, heads, round_qk=True):
    """qkv16 [B * L][3 * heads * 64] fp16 (q | k | v), lens [B], rope [>= L][64] (the CALLER's table) -> (ctx, A), float64
    [B * L][heads * 64].  ctx = softmax(rot(q) rot(k)^T / 8 + prefix mask j < min(len[b], L)) v per head, zero rows for
    pos >= len[b]; with `round_qk` the rotated q and k are rounded to fp16 -- they are the kernel's fp16 matrix-core operands, so
    the rounding is part of the operation.  A = sum_j p_j |v_j|: the scale of the error bound."""
    H = heads * HEAD_DIM
    x = np.asarray(qkv16).astype(np.float64).reshape(B, L, 3, heads, HEAD_DIM)
    rope = np.asarray(rope, dtype=np.float64)[:L]
    ctx = np.zeros((B, L, heads, HEAD_DIM))
    A = np.zeros_like(ctx)
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), L))
        if n == 0:
            continue
        q, k = _rotate(x[b, :n, 0], rope[:n]), _rotate(x[b, :n, 1], rope[:n])
        if round_qk:
            q, k = q.astype(np.float16).astype(np.float64), k.astype(np.float16).astype(np.float64)
        v = x[b, :n, 2]
        s = np.einsum("ihd,jhd->hij", q, k) / 8.0
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        ctx[b, :n] = np.einsum("hij,jhd->ihd", p, v)
        A[b, :n] = np.einsum("hij,jhd->ihd", p, np.abs(v))
    return ctx.reshape(B * L, H), A.reshape(B * L, H)


def packed_layout(lens, L):
    """The packed layout of a padded batch: (offsets int32 [B + 1], keep bool [B * L]); lengths clamped to 0..L first (the
    packed call documents every sequence as <= max_seq)."""
    n = np.clip(np.asarray(lens, dtype=np.int64), 0, L)
    offsets = np.zeros(len(n) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(n)
    keep = (np.arange(L)[None, :] < n[:, None]).reshape(-1)
    return offsets, keep


def add_layernorm(x16, res16, gamma16, beta16, eps):
    """LayerNorm(x + res) * gamma + beta over the last axis in fp64 -> (out [rows][width], mean [rows], sigma [rows])."""
    v = np.asarray(x16).astype(np.float64)
    if res16 is not None:
        v = v + np.asarray(res16).astype(np.float64)
    mean = v.mean(axis=1)
    d = v - mean[:, None]
    var = (d * d).mean(axis=1)
    out = d / np.sqrt(var + eps)[:, None] * np.asarray(gamma16).astype(np.float64) + np.asarray(beta16).astype(np.float64)
    return out, mean, np.sqrt(var)


def swiglu(gu16, inter):
    """gu16 [rows][2 * inter] (gate | up) -> silu(gate) * up in fp64; the sigmoid never overflows: for x < 0 it is e^x / (1 + e^x)."""
    g = np.asarray(gu16[:, :inter]).astype(np.float64)
    u = np.asarray(gu16[:, inter:]).astype(np.float64)
    e = np.exp(-np.abs(g))
    sig = np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    with np.errstate(over="ignore"):
        return g * sig * u


def mean_pool(h16, lens, L):
    """h16 [B][L][width] -> (mean over the first min(len[b], L) tokens in fp64, 0 for an empty sequence; the mean of |h| over the
    same tokens: the scale of the error bound)."""
    h = np.asarray(h16).astype(np.float64)
    out = np.zeros((h.shape[0], h.shape[2]))
    mabs = np.zeros_like(out)
    for b in range(h.shape[0]):
        n = int(min(max(int(lens[b]), 0), L))
        if n:
            out[b] = h[b, :n].sum(axis=0) / n
            mabs[b] = np.abs(h[b, :n]).sum(axis=0) / n
    return out, mabs


def fp16_rne(x64):
    """float64 -> fp16, round to nearest even, overflow to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x64, dtype=np.float64).astype(np.float16)


def ulp16_distance(a16, b16):
    """Ordinal distance between fp16 bit patterns: -0 and +0 are the same point, inf is the ordinary neighbour of 65504.  NaNs
    are the caller's to refuse first (their ordinals lie beyond inf)."""
    def ordinal(h):
        bits = np.ascontiguousarray(h, dtype=np.float16).view(np.uint16).astype(np.int64)
        mag = bits & 0x7FFF
        return np.where(bits >> 15 != 0, -mag, mag)
    return np.abs(ordinal(a16) - ordinal(b16))


# ---- the bounds ----------------------------------------------------------------------------------------------------
def rope_bound(seq, theta, c):
    """|got - ref| <= c 2^-24 ang + 2^-23 per element: an fp32 angle error (|d cos| <= |d ang|) and the last bit of cosf / sinf."""
    ang = rope_angles(seq, theta)
    return c * U32 * np.concatenate([ang, ang], axis=1) + 2.0 ** -23


def attention_bound(A, t):
    return t * U16 * A + 2.0 ** -24


def layernorm_bound(ref, mean, sigma, gamma16, K):
    """2^-11 |ref| + 2^-25 + K E with E = 2^-24 (|mean| + sigma) / sigma |gamma|; rows of sigma = 0 have no bound (inf): their
    output is beta's bits."""
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(sigma > 0, (np.abs(mean) + sigma) / sigma, np.inf)
        E = U32 * cond[:, None] * np.abs(np.asarray(gamma16).astype(np.float64))[None, :]
    E = np.where(np.isnan(E), np.inf, E)                                   # inf * 0 on a constant row
    return U16 * np.abs(ref) + 2.0 ** -25 + np.where(np.isinf(E), np.inf, K * np.where(np.isinf(E), 0.0, E))


def mean_pool_bound(ref, mabs, lens, L):
    """n 2^-24 mean_t |h| + 2^-24 |ref|: a sequential fp32 sum of n terms, then the division."""
    n = np.clip(np.asarray(lens, dtype=np.int64), 0, L).astype(np.float64)
    return n[:, None] * U32 * mabs + U32 * np.abs(ref)


# ---- the inputs of both tiers -----------------------------------------------------------------------------------------------------
ATTN_L = (1, 16, 17, 33, 64, 65, 128, 129, 288, 289, 512)     # both sides of 128 | 129 and 288 | 289, the 16- and 32-key tile edges
ATTN_HEADS = (1, 3)
ATTN_STRUCTURED = ("uniform", "ascending", "descending", "lookup", "extreme")


def attention_lens(L, variant=0):
    """Six lengths (five at L = 1): L, 0, the over-long L + 7, and three of {1, 15, 16, 17, 31, 32, 33, L - 1} that fit L, a
    different three for every `variant`, in an order that depends on it too."""
    rest = [v for v in dict.fromkeys((L - 1, 1, 15, 16, 17, 31, 32, 33)) if 0 < v < L]
    pick = [rest[(3 * variant + i) % len(rest)] for i in range(3)] if rest else [L, 0]
    lens = [L, 0, L + 7] + pick
    r = variant % len(lens)
    return np.array(lens[r:] + lens[:r], dtype=np.int32)


def random_variant(heads, theta):
    """Which three lengths the random batch of (heads, theta) takes: between them the four batches of an L take them all."""
    return heads + int(theta == 10000.0)


def structured_variant(kind, heads):
    return ATTN_STRUCTURED.index(kind) + heads


def _randn16(rng, shape, scale=1.5):
    return (scale * rng.standard_normal(shape)).astype(np.float16)


def attention_random(L, heads, variant=0):
    """1.5 randn in every row, padding included -> (qkv16 [B * L][3 H], lens)."""
    lens = attention_lens(L, variant)
    rng = np.random.default_rng(1000 * L + 10 * heads + variant)
    return _randn16(rng, (len(lens) * L, 3 * heads * HEAD_DIM)), lens


def attention_poisoned(qkv16, lens, L, heads):
    """The same batch with every row at pos >= len[b] overwritten: NaN queries, keys that would score far above every valid one
    (100 x the mean valid query of the head) and NaN values.  A kernel that never reads padding computes the same bytes."""
    H = heads * HEAD_DIM
    out = np.array(qkv16, copy=True).reshape(len(lens), L, 3 * H)
    for b, n in enumerate(np.clip(lens, 0, L)):
        if n == L:
            continue
        qbar = out[b, :n, :H].astype(np.float32).mean(axis=0) if n else np.ones(H, np.float32)
        out[b, n:, :H] = np.float16(np.nan)
        out[b, n:, H:2 * H] = np.clip(100.0 * qbar, -60000, 60000).astype(np.float16)
        out[b, n:, 2 * H:] = np.float16(np.nan)
    return out.reshape(len(lens) * L, 3 * H)


def attention_structured(kind, L, heads, variant=0):
    """One structured batch for the identity table -> (qkv16, lens, want16 or None).  want16 [B * L][H] fp16 is the exact answer
    of the kinds that have one (rows at pos >= len are zero).
      uniform     q = 0: equal weights; v_j = e_(j % 64), so ctx[d] = #{j < n: j % 64 = d} / n
      ascending   the score of key j is a_i j / 32 with a_i in 1..2: the maximum moves in every 32-key step by >= 1.44 in log2
      descending  ... a_i (L - j) / 32: the maximum never moves after step 0
      lookup      q_i = 8 * 64 * k_pi(i) over unit keys: the softmax is one-hot to fp16, ctx_i = v_pi(i); pi(0) = n - 1
      extreme     q_i = 8 * 1024 * k_pi(i), every odd key the negative of the key before it: scores from -1024 to 1024"""
    lens = attention_lens(L, variant)
    B, H = len(lens), heads * HEAD_DIM
    rng = np.random.default_rng(77000 + 1000 * L + 10 * heads + variant + 100 * ATTN_STRUCTURED.index(kind))
    x = _randn16(rng, (B, L, 3, heads, HEAD_DIM))                       # padding rows and whatever a kind leaves alone stay random
    want = None
    nv = np.clip(lens, 0, L)
    if kind == "uniform":
        x[:, :, 0] = 0
        x[:, :, 2] = 0
        j = np.arange(L)
        x[:, j, 2, :, j % 64] = 1
        want = np.zeros((B, L, heads, HEAD_DIM))
        for b, n in enumerate(nv):
            if n:
                want[b, :n] = (np.bincount(np.arange(n) % 64, minlength=64) / n)[None, None, :]
    elif kind in ("ascending", "descending"):
        j = np.arange(L, dtype=np.float64)
        ramp = (j if kind == "ascending" else L - j) / 4.0                # exact in fp16: multiples of 1/4 up to 128
        a = 1.0 + (np.arange(L) % 5) / 4.0
        x[:, :, 1] = 0
        for h in range(heads):
            d0 = (5 + 37 * h) % 64
            x[:, :, 1, h, d0] = ramp.astype(np.float16)[None, :]
            x[:, :, 0, h, d0] = a.astype(np.float16)[None, :]
    else:
        scale = 8.0 * (64.0 if kind == "lookup" else 1024.0)
        want = np.zeros((B, L, heads, HEAD_DIM))
        for b, n in enumerate(nv):
            if n == 0:
                continue
            k = rng.standard_normal((n, heads, HEAD_DIM))
            k /= np.linalg.norm(k, axis=-1, keepdims=True)
            if kind == "extreme":
                k[1::2] = -k[0:2 * (n // 2):2]
            k16 = k.astype(np.float16)
            pi = rng.permutation(n)
            pi[np.argmax(pi == n - 1)], pi[0] = pi[0], n - 1
            x[b, :n, 1] = k16
            x[b, :n, 0] = (k16[pi].astype(np.float64) * scale).astype(np.float16)      # a power of two: exact
            want[b, :n] = x[b, pi, 2].astype(np.float64)
    qkv = np.ascontiguousarray(x.reshape(B * L, 3 * H))
    return qkv, lens, (None if want is None else fp16_rne(want.reshape(B * L, H)))


LN_WIDTHS = (8, 504, 512, 520, 768, 1024, 1032, 1536)         # the edges of the three 512-element register passes
LN_ROWS = (1, 5, 1000)                                        # one wave of a workgroup, a workgroup and a quarter, many
LN_FAMILIES = ("normal", "big_residual", "offset", "constant", "huge")
LN_EPS = 1e-12


def layernorm_case(width, rows, residual):
    """-> dict(x, res, gamma, beta, family).  Row r belongs to family (r + width // 8) % 5, so that the single row of rows = 1 is a
    different family from width to width:
      normal        randn (+ randn)
      big_residual  randn + 3 randn
      offset        x + res = 1000 + k / 2, k in -2..2 (exact in fp16): |mean| ~ 1400 sigma
      constant      one value in the whole row: the output is beta's bits
      huge          +-60000 (+ the same again): x + res is beyond fp16, fine in fp32
    gamma ~ 1 + 0.1 randn with every 7th column 0 (there the output is beta's bits too), beta ~ 0.1 randn."""
    rng = np.random.default_rng(31 * width + 7 * rows + int(residual))
    fam = (np.arange(rows) + width // 8) % 5
    x = rng.standard_normal((rows, width))
    res = rng.standard_normal((rows, width))
    res[fam == 1] *= 3.0
    k = rng.integers(-2, 3, size=(rows, width)) / 2.0
    x[fam == 2] = (600.0 if residual else 1000.0) + k[fam == 2]
    res[fam == 2] = 400.0
    x[fam == 3] = 3.25
    res[fam == 3] = -1.5
    sign = rng.choice([-1.0, 1.0], size=(rows, width))
    x[fam == 4] = 60000.0 * sign[fam == 4]
    res[fam == 4] = 60000.0 * sign[fam == 4]
    gamma = 1.0 + 0.1 * rng.standard_normal(width)
    gamma[::7] = 0.0
    beta = 0.1 * rng.standard_normal(width)
    return dict(x=x.astype(np.float16), res=res.astype(np.float16) if residual else None, gamma=gamma.astype(np.float16),
                beta=beta.astype(np.float16), family=fam)


SWIGLU_UPS = (1.0, -3.0, 2.0 ** -14, 60000.0)
SWIGLU_SMALL = ((1, 8), (7, 8), (1, 776), (7, 776))           # (rows, inter)


def all_finite_fp16():
    """The 63 488 finite fp16 values as 31 rows of 2048 (both zeros and every subnormal included)."""
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    assert bits.size == 63488
    return bits.view(np.float16).reshape(31, 2048)


def swiglu_exhaustive(up):
    """[31][2 * 2048]: every finite gate against one value of up."""
    g = all_finite_fp16()
    return np.ascontiguousarray(np.concatenate([g, np.full_like(g, np.float16(up))], axis=1))


def swiglu_random(rows, inter):
    return _randn16(np.random.default_rng(rows * 10000 + inter), (rows, 2 * inter), 1.0)


POOL_WIDTHS = (8, 776, 2048)
POOL_SEQS = (1, 50, 512)


def pool_lens(seq):
    return np.array([seq, 0, 1, seq - 1, seq + 9], dtype=np.int32)


def pool_case(width, seq, offset=False):
    """-> (h16 [5][seq][width], lens).  offset: 1000 + k / 2 in every element -- at seq 512 the sum (~5e5) needs fp32."""
    rng = np.random.default_rng(width * 1000 + seq + int(offset))
    if offset:
        h = 1000.0 + rng.integers(-2, 3, size=(5, seq, width)) / 2.0
    else:
        h = rng.standard_normal((5, seq, width))
    return h.astype(np.float16), pool_lens(seq)
