"""The seven encoder entry points on the MI355X (include/rq.h rq_nb_*, csrc/rq_encoder.hip), each against the fp64 oracle
of the same operation (tests/encoder_oracle.py) at the shapes where its code takes another path, inside a per-element bound whose
derived part comes from the number formats and whose measured part is committed in the oracle file.  tests/test_encoder.py proves on
the CPU, on these very inputs, that every bound rejects a plausible wrong kernel.

Every output is allocated with guard rows behind it and filled, guard included, with a sentinel; one case of every kernel runs on a
stream of its own, as production does.  Each test prints the figure it is about to assert ("MEASURE ...")."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                          # rows behind every output that must keep the sentinel
SENTINEL = 7.0
EINVAL, EUNSUPPORTED = r"\(code -1\)", r"\(code -6\)"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(rows, cols, dtype, fill=None):
    """[rows + GUARD][cols] of the sentinel on the device; `fill` (host array [rows][cols]) goes into the rows in front."""
    import torch
    buf = torch.full((rows + GUARD, cols), SENTINEL, dtype=dtype, device="cuda")
    if fill is not None:
        buf[:rows] = _dev(fill)
    return buf


def _take(buf, rows, what=""):
    """Host copy of the rows in front; the guard behind them must be untouched."""
    host = buf.cpu().numpy()
    assert (host[rows:] == SENTINEL).all(), f"{what}: the guard rows behind the output were written"
    return host[:rows]


class _Stream:
    """`with _Stream(side) as s`: s is the raw stream to pass (0 = the default stream); leaving synchronises it."""

    def __init__(self, side):
        import torch
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream() if side else None

    def __enter__(self):
        return self.stream.cuda_stream if self.stream is not None else 0

    def __exit__(self, *exc):
        import torch
        (self.stream or torch.cuda.current_stream()).synchronize()
        torch.cuda.synchronize()


def _measure(name, value):
    print(f"MEASURE {name} {value:.4f}")


# ---- rotary table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [1000.0, 10000.0])
@pytest.mark.parametrize("seq", [1, 512, 65536])
def test_rope_table_against_fp64_angles(seq, theta):
    import torch
    buf = _guarded(seq, 64, torch.float32)
    with _Stream(seq == 512) as st:
        nat.nb_rope_table(buf, seq, theta, st)
    got = _take(buf, seq, "rope table").astype(np.float64)
    assert got[0, :32].tolist() == [1.0] * 32 and got[0, 32:].tolist() == [0.0] * 32      # position 0: exactly (1, 0)
    rows = np.unique(np.concatenate([np.arange(min(seq, 512)), np.arange(max(seq - 64, 0), seq)]))
    err = np.abs(got - eo.rope_table(seq, theta))[rows]
    ang = np.concatenate([eo.rope_angles(seq, theta)] * 2, axis=1)[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(ang > 0, (err - 2.0 ** -23) / (eo.U32 * ang), 0.0).max()
    _measure(f"rope_c seq={seq} theta={theta:g}", max(c, 0.0))
    assert eo.ROPE_C <= eo.ROPE_C_CAP
    assert (err <= eo.rope_bound(seq, theta, eo.ROPE_C)[rows]).all(), f"angle error of {c:.2f} x 2^-24 ang against c = {eo.ROPE_C}"


# ---- attention ---------------------------------------------------------------------------------------------------------------------
_tables = {}


def _table(L, theta):
    """The kernel's own table for `theta` (device tensor, host copy); None = the identity table."""
    import torch
    key = (L, theta)
    if key not in _tables:
        if theta is None:
            host = eo.identity_rope(L)
            _tables[key] = (_dev(host), host)
        else:
            t = torch.empty((L, 64), dtype=torch.float32, device="cuda")
            nat.nb_rope_table(t, L, theta)
            torch.cuda.synchronize()
            _tables[key] = (t, t.cpu().numpy())
    return _tables[key]


def _attention(qkv16, lens, d_rope, L, heads, side=False):
    """One padded call -> ctx [B * L][H] on the host."""
    import torch
    B, H = len(lens), heads * 64
    d_qkv, d_len = _dev(qkv16), _dev(np.asarray(lens, dtype=np.int32))
    ctx = _guarded(B * L, H, torch.float16)
    with _Stream(side) as st:
        nat.nb_attention(d_qkv, d_len, d_rope, ctx, B, L, heads, st)
    return _take(ctx, B * L, "attention")


def _attention_packed(qkv16, lens, d_rope, L, heads, side=False):
    """The packed call on the valid rows of the same batch -> (ctx [sum n][H], keep)."""
    import torch
    offs, keep = eo.packed_layout(lens, L)
    d_qkv, d_off = _dev(qkv16[keep]), _dev(offs)
    ctx = _guarded(int(offs[-1]), heads * 64, torch.float16)
    with _Stream(side) as st:
        nat.nb_attention_packed(d_qkv, d_off, d_rope, ctx, len(lens), L, heads, st)
    return _take(ctx, int(offs[-1]), "packed attention"), keep


def _check_padding_and_packed(got, qkv16, lens, d_rope, L, heads, side):
    offs, keep = eo.packed_layout(lens, L)
    assert not np.isnan(got).any() and np.isfinite(got).all()
    assert (got[~keep].view(np.uint16) == 0).all(), "rows at pos >= len are not +0"
    packed, _ = _attention_packed(qkv16, lens, d_rope, L, heads, side)
    assert np.array_equal(packed.view(np.uint16), got[keep].view(np.uint16)), "the packed form differs from the padded one"


def _t_of(got, ref, A):
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(A > 0, (err - 2.0 ** -24) / (eo.U16 * A), 0.0).max()), err


CASES = [(L, heads) for heads in eo.ATTN_HEADS for L in eo.ATTN_L]


@pytest.mark.parametrize("theta", [1000.0, 10000.0])
@pytest.mark.parametrize("L,heads", CASES)
def test_attention_random_within_the_bound_and_padding_never_read(L, heads, theta):
    """1.5 randn under the kernel's own table: every element within t 2^-11 A + 2^-24 of the oracle; the packed form bit-equal;
    and the same bytes again when every padding row of qkv is poison (NaN q, keys that would outscore every valid one, NaN v)."""
    variant = eo.random_variant(heads, theta)
    qkv, lens = eo.attention_random(L, heads, variant)
    d_rope, rope = _table(L, theta)
    got = _attention(qkv, lens, d_rope, L, heads)
    _check_padding_and_packed(got, qkv, lens, d_rope, L, heads, side=(theta == 1000.0))
    ref, A = eo.attention(qkv, lens, rope, len(lens), L, heads)
    t, err = _t_of(got, ref, A)
    _measure(f"attn_t random L={L} heads={heads} theta={theta:g}", t)
    poisoned = _attention(eo.attention_poisoned(qkv, lens, L, heads), lens, d_rope, L, heads, side=(theta == 10000.0))
    assert np.array_equal(poisoned.view(np.uint16), got.view(np.uint16)), "a padding row of qkv was read"
    assert eo.ATTN_T <= eo.ATTN_T_CAP
    assert (err <= eo.attention_bound(A, eo.ATTN_T)).all(), f"L {L}, heads {heads}: error of {t:.2f} x 2^-11 A against t = {eo.ATTN_T}"


@pytest.mark.parametrize("kind", eo.ATTN_STRUCTURED)
@pytest.mark.parametrize("L,heads", CASES)
def test_attention_structured_cases(L, heads, kind):
    """The identity table (q and k reach the matrix cores unchanged) and inputs built so that the answer is known or the online
    softmax takes one branch in every step (encoder_oracle.attention_structured).  uniform / lookup: the exact answer to 1 fp16 ulp
    (equal weights 1 are exact in fp16 and sum exactly, so only 1 / l, the product and the final rounding remain); extreme: the
    arg-max key's value row itself; ascending / descending: the bound of the random case."""
    variant = eo.structured_variant(kind, heads)
    qkv, lens, want16 = eo.attention_structured(kind, L, heads, variant)
    d_rope, rope = _table(L, None)
    got = _attention(qkv, lens, d_rope, L, heads, side=(kind == "lookup"))
    _check_padding_and_packed(got, qkv, lens, d_rope, L, heads, side=(kind == "ascending"))
    if kind in ("ascending", "descending"):
        ref, A = eo.attention(qkv, lens, rope, len(lens), L, heads)
        t, err = _t_of(got, ref, A)
        _measure(f"attn_t {kind} L={L} heads={heads}", t)
        assert (err <= eo.attention_bound(A, eo.ATTN_T)).all(), f"{kind}, L {L}, heads {heads}: error of {t:.2f} x 2^-11 A against t = {eo.ATTN_T}"
    else:
        d = int(eo.ulp16_distance(got, want16).max())
        _measure(f"attn_ulp {kind} L={L} heads={heads}", d)
        assert d <= (0 if kind == "extreme" else 1), f"{kind}, L {L}, heads {heads}: {d} fp16 ulp from the exact answer"


def test_attention_negative_length_is_an_empty_sequence():
    """Lengths [L, -3, 5] at L = 33 (the negative one never first): sequence 0 and everything else come out as with [L, 0, 5], bit for
    bit -- unclamped, the zero fill of sequence 1 started 3 rows early, inside sequence 0.  The mean pool gives 0 for it."""
    import torch
    L, heads = 33, 3
    qkv, _ = eo.attention_random(L, heads, variant=0)
    qkv = qkv[:3 * L]
    d_rope, _ = _table(L, 10000.0)
    want = _attention(qkv, [L, 0, 5], d_rope, L, heads)
    for side in (False, True):
        got = _attention(qkv, [L, -3, 5], d_rope, L, heads, side)
        assert np.array_equal(got[:L].view(np.uint16), want[:L].view(np.uint16)), "sequence 0 was overwritten"
        assert (got[L:2 * L].view(np.uint16) == 0).all() and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    h, _ = eo.pool_case(776, L)
    outs = []
    for lens in ([L, -3, 5], [L, 0, 5]):
        out = _guarded(3, 776, torch.float32)
        with _Stream(False) as st:
            nat.nb_mean_pool(_dev(h[:3]), _dev(np.array(lens, np.int32)), out, 3, L, 776, st)
        outs.append(_take(out, 3, "mean pool"))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)) and (outs[0][1].view(np.uint32) == 0).all()


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", eo.LN_ROWS)
@pytest.mark.parametrize("width", eo.LN_WIDTHS)
def test_add_layernorm_within_the_bound_under_every_aliasing(width, rows):
    """With and without residual; out apart, out is x, out is res (what production calls): the aliased outputs bit-equal to the
    unaliased one.  Per element 2^-11 |ref| + 2^-25 + K E; constant rows and gamma = 0 columns are beta's bits."""
    import torch
    for residual in (False, True):
        c = eo.layernorm_case(width, rows, residual)
        ref, mean, sigma = eo.add_layernorm(c["x"], c["res"], c["gamma"], c["beta"], eo.LN_EPS)
        d_g, d_b = _dev(c["gamma"]), _dev(c["beta"])
        outs = {}
        for alias in ("none", "x") + (("res",) if residual else ()):
            d_x = _guarded(rows, width, torch.float16, c["x"])
            d_r = _guarded(rows, width, torch.float16, c["res"]) if residual else None
            d_o = {"none": _guarded(rows, width, torch.float16), "x": d_x, "res": d_r}[alias]
            with _Stream(alias != "none") as st:
                nat.nb_add_layernorm(d_x, d_r, d_g, d_b, d_o, rows, width, eo.LN_EPS, st)
            outs[alias] = _take(d_o, rows, f"layernorm, out is {alias}")
            if alias != "x":
                assert np.array_equal(_take(d_x, rows), c["x"]), "x was written"
            if residual and alias != "res":
                assert np.array_equal(_take(d_r, rows), c["res"]), "res was written"
        got = outs["none"]
        for alias, o in outs.items():
            assert np.array_equal(o.view(np.uint16), got.view(np.uint16)), f"out is {alias}: differs from the unaliased call"
        assert np.isfinite(got).all()
        beta_rows = np.broadcast_to(c["beta"], got.shape)
        const = sigma == 0
        assert (c["family"] == 3)[~const].sum() == 0
        assert np.array_equal(got[const].view(np.uint16), beta_rows[const].view(np.uint16)), "a constant row is not beta"
        zero_g = c["gamma"] == 0
        assert np.array_equal(got[:, zero_g].view(np.uint16), beta_rows[:, zero_g].view(np.uint16)), "a gamma = 0 column is not beta"
        err = np.abs(got.astype(np.float64) - ref)
        base = eo.layernorm_bound(ref, mean, sigma, c["gamma"], 0.0)
        with np.errstate(invalid="ignore"):
            unit = eo.layernorm_bound(ref, mean, sigma, c["gamma"], 1.0) - base                 # (inf - inf on a constant row)
        live = np.isfinite(unit) & (unit > 0)
        K = float(((err - base)[live] / unit[live]).max(initial=0.0))
        _measure(f"ln_K width={width} rows={rows} residual={int(residual)}", max(K, 0.0))
        assert eo.LN_K <= eo.LN_K_CAP
        assert (err[~const] <= eo.layernorm_bound(ref, mean, sigma, c["gamma"], eo.LN_K)[~const]).all(), f"excess of {K:.2f} E against K = {eo.LN_K}"


# ---- SwiGLU ------------------------------------------------------------------------------------------------------------------------
def _swiglu(gu16, rows, inter, side):
    import torch
    out = _guarded(rows, inter, torch.float16)
    d_gu = _dev(gu16)
    with _Stream(side) as st:
        nat.nb_swiglu(d_gu, out, rows, inter, st)
    return _take(out, rows, "swiglu")


@pytest.mark.parametrize("up", eo.SWIGLU_UPS)
def test_swiglu_every_finite_gate_to_one_ulp(up):
    """All 63 488 finite fp16 gates against one `up`: the fp32 result is rounded once, the fp64 one once more -- at most 1 ulp apart.
    Overflowing products are the infinity of the right sign (inf is 65504's neighbour on the ordinal scale, so a wrong sign is
    ~2 x 31744 away); nothing is NaN."""
    gu = eo.swiglu_exhaustive(up)
    got = _swiglu(gu, 31, 2048, side=(up == 1.0))
    want = eo.fp16_rne(eo.swiglu(gu, 2048))
    assert not np.isnan(got).any()
    d = eo.ulp16_distance(got, want)
    _measure(f"swiglu_ulp up={up:g}", int(d.max()))
    assert d.max() <= 1, f"up {up}: gate {gu[:, :2048][d > 1][:4].tolist()} -> {got[d > 1][:4].tolist()}, want {want[d > 1][:4].tolist()}"
    ref = eo.swiglu(gu, 2048)
    over = np.abs(ref) >= 2 * 65504.0                  # far beyond the largest fp16: the infinity itself, with the product's sign
    assert np.isinf(got[over]).all() and np.array_equal(np.signbit(got[over]), np.signbit(ref[over]))


@pytest.mark.parametrize("rows,inter", eo.SWIGLU_SMALL)
def test_swiglu_small_shapes(rows, inter):
    gu = eo.swiglu_random(rows, inter)
    got = _swiglu(gu, rows, inter, side=True)
    assert not np.isnan(got).any() and eo.ulp16_distance(got, eo.fp16_rne(eo.swiglu(gu, inter))).max() <= 1


# ---- mean pool ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,seq,offset", [(w, s, False) for w in eo.POOL_WIDTHS for s in eo.POOL_SEQS] + [(8, 512, True), (776, 512, True), (2048, 512, True)])
def test_mean_pool_within_the_sequential_fp32_bound(width, seq, offset):
    """Lengths {seq, 0, 1, seq - 1, seq + 9}: n 2^-24 mean |h| + 2^-24 |ref| per element (derived: n - 1 additions of a sequential
    fp32 sum, 1 / n and the product); an empty sequence is exactly 0, an over-long one counts as seq; the packed form bit-equal."""
    import torch
    h, lens = eo.pool_case(width, seq, offset)
    B = len(lens)
    out = _guarded(B, width, torch.float32)
    d_h = _dev(h)
    with _Stream(False) as st:
        nat.nb_mean_pool(d_h, _dev(lens), out, B, seq, width, st)
    got = _take(out, B, "mean pool")
    ref, mabs = eo.mean_pool(h, lens, seq)
    err = np.abs(got.astype(np.float64) - ref)
    bound = eo.mean_pool_bound(ref, mabs, lens, seq)
    with np.errstate(divide="ignore", invalid="ignore"):
        _measure(f"pool_ratio width={width} seq={seq} offset={int(offset)}", float(np.where(bound > 0, err / bound, 0.0).max()))
    assert (got[np.clip(lens, 0, seq) == 0].view(np.uint32) == 0).all()
    assert (err <= bound).all()
    offs, keep = eo.packed_layout(lens, seq)
    out_p = _guarded(B, width, torch.float32)
    d_hp = _dev(h.reshape(B * seq, width)[keep])
    with _Stream(True) as st:
        nat.nb_mean_pool_packed(d_hp, _dev(offs), out_p, B, seq, width, st)
    assert np.array_equal(_take(out_p, B, "packed mean pool").view(np.uint32), got.view(np.uint32))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    """Real buffers, large enough for the refused shape; every output keeps its sentinel and the call raises with its code."""
    import torch
    f16, f32 = torch.float16, torch.float32
    qkv = _dev(eo.attention_random(513, 1)[0][:2 * 513])
    lens, offs = _dev(np.array([4, 4], np.int32)), _dev(np.array([0, 4, 8], np.int32))
    rope = torch.zeros((65537 + GUARD, 64), dtype=f32, device="cuda")
    ctx = _guarded(2 * 513, 64, f16)
    wide = _guarded(8, 2 * 2056, f16)                  # x / res / gate|up / h of every refused width
    vec = _dev(np.ones(2056, np.float16))
    out16, out32, table = _guarded(8, 2056, f16), _guarded(8, 2056, f32), _guarded(65537, 64, f32)
    calls = []
    for form, lengths in ((nat.nb_attention, lens), (nat.nb_attention_packed, offs)):
        calls += [(EINVAL, form, a) for a in ((None, lengths, rope, ctx, 2, 4, 1), (qkv, None, rope, ctx, 2, 4, 1), (qkv, lengths, None, ctx, 2, 4, 1),
                                              (qkv, lengths, rope, None, 2, 4, 1), (qkv, lengths, rope, ctx, 0, 4, 1), (qkv, lengths, rope, ctx, 2, 4, 0),
                                              (qkv, lengths, rope, ctx, 2, 0, 1))]
        calls += [(EUNSUPPORTED, form, (qkv, lengths, rope, ctx, 2, 513, 1))]
    ln = nat.nb_add_layernorm
    calls += [(EINVAL, ln, a) for a in ((None, wide, vec, vec, out16, 4, 768, 1e-12), (wide, wide, None, vec, out16, 4, 768, 1e-12),
                                        (wide, wide, vec, None, out16, 4, 768, 1e-12), (wide, wide, vec, vec, None, 4, 768, 1e-12),
                                        (wide, wide, vec, vec, out16, 0, 768, 1e-12), (wide, wide, vec, vec, out16, 4, 0, 1e-12),
                                        (wide, wide, vec, vec, out16, 4, 12, 1e-12), (wide, wide, vec, vec, out16, 4, 1544, 1e-12))]
    calls += [(EINVAL, nat.nb_swiglu, a) for a in ((None, out16, 4, 768), (wide, None, 4, 768), (wide, out16, 0, 768), (wide, out16, 4, 0), (wide, out16, 4, 12))]
    for form, lengths in ((nat.nb_mean_pool, lens), (nat.nb_mean_pool_packed, offs)):
        calls += [(EINVAL, form, a) for a in ((None, lengths, out32, 2, 4, 768), (wide, None, out32, 2, 4, 768), (wide, lengths, None, 2, 4, 768),
                                              (wide, lengths, out32, 0, 4, 768), (wide, lengths, out32, 2, 0, 768), (wide, lengths, out32, 2, 4, 0),
                                              (wide, lengths, out32, 2, 4, 12), (wide, lengths, out32, 2, 4, 2056))]
    calls += [(EINVAL, nat.nb_rope_table, a) for a in ((None, 4, 10000.0), (table, 0, 10000.0), (table, 65537, 10000.0), (table, 4, 1.0), (table, 4, float("nan")))]
    for side in (False, True):
        with _Stream(side) as st:
            for code, fn, args in calls:
                with pytest.raises(nat.RqError, match=code):
                    fn(*args, st)
    for buf in (ctx, out16, out32, table):
        assert bool((buf == SENTINEL).all()), "a refused call wrote to its output"
    # the same calls with the shapes put right are accepted (the refusals above are the shapes', not the buffers')
    nat.nb_attention(qkv, lens, rope, ctx, 2, 4, 1)
    nat.nb_add_layernorm(wide, None, vec, vec, out16, 4, 1536, 1e-12)
    nat.nb_swiglu(wide, out16, 4, 8)
    nat.nb_mean_pool(wide, lens, out32, 2, 4, 2048)
    nat.nb_rope_table(table, 65536, 1.5)
    torch.cuda.synchronize()
