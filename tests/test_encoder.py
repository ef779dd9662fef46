"""The encoder kernels' oracle and bounds, the parts that need no GPU: tests/encoder_oracle.py against an independent
fp64 implementation (torch.nn.functional on the CPU); the exact answers of the structured attention cases against the oracle; and,
for every bound the GPU tier (tests/test_gpu_encoder.py) asserts, one plausible wrong kernel emulated in numpy on the very inputs of
that tier, which the bound must reject at its CAP -- while a faithful fp32 emulation of the kernel passes.  Plus the header's words
about lengths outside 0..seq."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_oracle as eo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- 1. the oracle against an independent implementation -------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("L,heads,theta", [(1, 1, 1000.0), (17, 3, 1000.0), (65, 1, 10000.0), (129, 3, 10000.0)])
def test_attention_oracle_matches_torch_fp64(L, heads, theta):
    import torch
    F = torch.nn.functional
    qkv16, lens = eo.attention_random(L, heads, variant=1)
    B, H = len(lens), heads * 64
    rope = eo.rope_table(L, theta)
    got, A = eo.attention(qkv16, lens, rope, B, L, heads, round_qk=False)
    x = torch.from_numpy(qkv16.astype(np.float64)).view(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)      # [3][B][heads][L][64]
    pos = torch.arange(L, dtype=torch.float64)
    inv = torch.tensor(theta, dtype=torch.float64) ** (-torch.arange(32, dtype=torch.float64) / 32.0)
    ang = torch.cat([pos[:, None] * inv[None, :]] * 2, dim=-1)
    assert _rel(rope, torch.cat([ang[:, :32].cos(), ang[:, :32].sin()], dim=-1).numpy()) <= 1e-12

    def rot(t):
        return t * ang.cos() + torch.cat((-t[..., 32:], t[..., :32]), dim=-1) * ang.sin()
    n = torch.from_numpy(np.clip(lens, 0, L).astype(np.int64))
    keymask = torch.arange(L)[None, :] < n[:, None]
    s = (rot(x[0]) @ rot(x[1]).transpose(-1, -2)) * 0.125
    s = s.masked_fill(~keymask[:, None, None, :], float("-inf"))
    p = torch.nan_to_num(F.softmax(s, dim=-1))
    ref = ((p @ x[2]).permute(0, 2, 1, 3).reshape(B, L, H) * keymask[:, :, None]).reshape(B * L, H).numpy()
    refA = ((p @ x[2].abs()).permute(0, 2, 1, 3).reshape(B, L, H) * keymask[:, :, None]).reshape(B * L, H).numpy()
    assert _rel(got, ref) <= 1e-12 and _rel(A, refA) <= 1e-12
    assert (got.reshape(B, L, H)[~keymask.numpy()] == 0).all()
    # the packed layout keeps exactly the valid rows, in order
    offs, keep = eo.packed_layout(lens, L)
    assert np.array_equal(keep, keymask.numpy().reshape(-1)) and offs[0] == 0 and np.array_equal(np.diff(offs), n.numpy())


@pytest.mark.parametrize("width,rows,residual", [(8, 5, True), (520, 5, False), (768, 1000, True), (1536, 1, False)])
def test_layernorm_oracle_matches_torch_fp64(width, rows, residual):
    import torch
    c = eo.layernorm_case(width, rows, residual)
    got, mean, sigma = eo.add_layernorm(c["x"], c["res"], c["gamma"], c["beta"], eo.LN_EPS)
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    v = t(c["x"]) + (t(c["res"]) if residual else 0)
    ref = torch.nn.functional.layer_norm(v, (width,), t(c["gamma"]), t(c["beta"]), eo.LN_EPS).numpy()
    live = c["family"] != 3                       # a constant row is 0 / sqrt(eps): the two agree on beta, not to 1e-12 of rounding dust
    assert _rel(got[live], ref[live]) <= 1e-12 if live.any() else True
    assert np.array_equal(got[~live], np.broadcast_to(c["beta"].astype(np.float64), got.shape)[~live])
    assert np.allclose(mean, v.mean(1).numpy(), rtol=1e-12, atol=0) and np.allclose(sigma, v.std(1, unbiased=False).numpy(), rtol=1e-9, atol=1e-12)


def test_swiglu_and_mean_pool_oracles_match_torch_fp64():
    import torch
    for rows, inter in eo.SWIGLU_SMALL:
        gu = eo.swiglu_random(rows, inter)
        x = torch.from_numpy(gu.astype(np.float64))
        assert _rel(eo.swiglu(gu, inter), (torch.nn.functional.silu(x[:, :inter]) * x[:, inter:]).numpy()) <= 1e-12
    gu = eo.swiglu_exhaustive(-3.0)               # every finite gate: no overflow, no NaN, silu(x) -> x and -> -0 at the ends
    x = torch.from_numpy(gu.astype(np.float64))
    got = eo.swiglu(gu, 2048)
    ref = (torch.nn.functional.silu(x[:, :2048]) * x[:, 2048:]).numpy()
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-300)
    for width, seq in ((8, 1), (776, 50), (2048, 50)):
        h, lens = eo.pool_case(width, seq)
        got, _ = eo.mean_pool(h, lens, seq)
        n = np.clip(lens, 0, seq)
        mk = torch.from_numpy((np.arange(seq)[None, :] < n[:, None]).astype(np.float64))[:, :, None]
        ref = ((torch.from_numpy(h.astype(np.float64)) * mk).sum(1) / mk.sum(1).clamp_min(1.0)).numpy()
        assert _rel(got, ref) <= 1e-12 and (got[n == 0] == 0).all()


def test_ulp16_distance():
    h = lambda *v: np.array(v, dtype=np.float16)
    assert eo.ulp16_distance(h(0.0), h(-0.0))[0] == 0
    assert eo.ulp16_distance(h(65504.0), h(np.inf))[0] == 1 and eo.ulp16_distance(h(-65504.0), h(-np.inf))[0] == 1
    assert eo.ulp16_distance(h(1.0), h(1.0 + 2.0 ** -10))[0] == 1 and eo.ulp16_distance(h(1.0), h(1.0 - 2.0 ** -11))[0] == 1
    assert eo.ulp16_distance(h(2.0 ** -24), h(-2.0 ** -24))[0] == 2 and eo.ulp16_distance(h(2.0 ** -24), h(0.0))[0] == 1
    assert eo.ulp16_distance(h(-np.inf), h(np.inf))[0] == 2 * 0x7C00
    assert eo.fp16_rne(65519.9) == np.float16(65504) and np.isinf(eo.fp16_rne(65520.0)) and eo.fp16_rne(-1e-30) == 0 and np.signbit(eo.fp16_rne(-1e-30))
    assert eo.all_finite_fp16().shape == (31, 2048) and np.isfinite(eo.all_finite_fp16()).all()


def test_batches_cover_the_lengths_the_kernel_branches_on():
    for L in eo.ATTN_L:
        seen = set()
        for variant in sorted({eo.random_variant(h, th) for h in eo.ATTN_HEADS for th in (1000.0, 10000.0)}):     # the random batches alone
            lens = eo.attention_lens(L, variant)
            assert 5 <= len(lens) <= 6 and {L, 0, L + 7} <= set(lens.tolist())
            seen |= set(lens.tolist())
        assert {v for v in (1, 15, 16, 17, 31, 32, 33, L - 1) if 0 < v < L} <= seen, (L, seen)


# ---- 2. the structured cases have the answers their builder claims -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "lookup", "extreme"])
@pytest.mark.parametrize("L", [1, 17, 65, 129, 512])
def test_structured_cases_have_their_exact_answers(kind, L):
    qkv, lens, want16 = eo.attention_structured(kind, L, 1, eo.structured_variant(kind, 1))
    ref, _ = eo.attention(qkv, lens, eo.identity_rope(L), len(lens), L, 1)
    assert np.array_equal(eo.fp16_rne(ref), want16)
    if kind != "uniform":                         # one-hot far beyond fp16: every other key together weighs < 2^-30
        assert np.abs(ref - want16.astype(np.float64)).max() <= 2.0 ** -30 * 8
    if kind == "extreme" and L > 1:
        x = qkv.astype(np.float64).reshape(len(lens), L, 3, 64)
        b = int(np.argmax(lens == L))
        s = x[b, :, 0] @ x[b, :, 1].T / 8.0
        assert s.max() > 1000 and s.min() < -1000


@pytest.mark.parametrize("kind", ["ascending", "descending"])
def test_ramp_cases_move_the_maximum_as_they_claim(kind):
    L = 129
    qkv, lens, _ = eo.attention_structured(kind, L, 3, variant=0)
    x = qkv.astype(np.float64).reshape(len(lens), L, 3, 3, 64)
    b = int(np.argmax(lens == L))
    for h in range(3):
        s = np.einsum("id,jd->ij", x[b, :, 0, h], x[b, :, 1, h]) / 8.0 * np.log2(np.e)
        step = np.diff(s, axis=1)
        assert (step > 0).all() if kind == "ascending" else (step < 0).all()
        assert (np.abs(s[:, 32:] - s[:, :-32]) > 1.0).all()           # adjacent 32-key steps: more than 1 in the log2 domain


# ---- 3. the bounds bite: emulated kernels, right and wrong ---------------------------------------------------------------------------
def emulate_attention(qkv16, lens, rope, B, L, heads, drop_last=False, extra_key=False, no_rescale=False, swap_halves=False):
    """The kernel's arithmetic in numpy: fp16 rotated operands, fp32 scores, online softmax in 32-key steps with exp2, P rounded to
    fp16 before the PV product, fp32 running output, fp16 result.  The flags are the mutants."""
    H = heads * 64
    x = np.asarray(qkv16).reshape(B, L, 3, heads, 64)
    rope = np.asarray(rope, dtype=np.float64)
    out = np.zeros((B, L, heads, 64), dtype=np.float16)
    c = F32(0.125 * 1.4426950408889634)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            n = int(min(max(int(lens[b]), 0), L))
            if n == 0:
                continue
            nkeys = n - int(drop_last) + int(extra_key and n < L)
            nrow = max(n, nkeys)
            nk = (nrow + 31) & ~31
            q = eo._rotate(x[b, :n, 0].astype(np.float64), rope[:n]).astype(np.float16).astype(F32)
            k = np.zeros((nk, heads, 64), F32)
            v = np.zeros((nk, heads, 64), F32)
            k[:nrow] = eo._rotate(x[b, :nrow, 1].astype(np.float64), rope[:nrow]).astype(np.float16).astype(F32)
            v[:nrow] = x[b, :nrow, 2].astype(F32)
            s = np.einsum("ihd,jhd->hij", q, k).astype(F32)
            s[:, :, nkeys:] = -np.inf
            m = np.full((heads, n), -np.inf, F32)
            l = np.zeros((heads, n), F32)
            o = np.zeros((heads, n, 64), F32)
            for k0 in range(0, nk, 32):
                blk = s[:, :, k0:k0 + 32]
                mn = np.maximum(m, blk.max(axis=-1) * c)
                alpha = np.exp2(m - mn).astype(F32)
                p = np.exp2(blk * c - mn[:, :, None]).astype(F32)
                l = l * alpha + p.sum(axis=-1, dtype=F32)
                m = mn
                if not no_rescale:
                    o *= alpha[:, :, None]
                vb = v[k0:k0 + 32]
                if swap_halves:
                    vb = np.concatenate([vb[16:], vb[:16]], axis=0)
                o += np.einsum("hij,jhd->hid", p.astype(np.float16).astype(F32), vb).astype(F32)
            out[b, :n] = (o / l[:, :, None]).transpose(1, 0, 2).astype(np.float16)
    return out.reshape(B * L, H)


def _violations(got16, ref, bound, B, L):
    """Per sequence: does any element miss its bound (a NaN misses it)."""
    bad = ~(np.abs(got16.astype(np.float64) - ref) <= bound)
    return bad.reshape(B, -1).any(axis=1)


ATTN_MUTANTS = {"drop_last": lambda n, L: n >= 1, "extra_key": lambda n, L: 1 <= n < L, "no_rescale": lambda n, L: n > 32,
                "swap_halves": lambda n, L: n >= 1}


@pytest.mark.parametrize("L", eo.ATTN_L)
def test_attention_bound_accepts_the_kernels_arithmetic_and_rejects_every_mutant(L):
    """On the random batch (theta 10000) and the ascending one of the GPU tier, one head: the faithful emulation stays inside the
    bound at the committed t; each mutant misses it at the CAP in EVERY sequence it can show in (drop the last valid key: n >= 1;
    include padded key n with its true score: 1 <= n < L; never rescale: more than one 32-key step; swap the 16-key halves of V:
    n >= 1)."""
    heads = 1
    cases = []
    qkv, lens = eo.attention_random(L, heads, eo.random_variant(heads, 10000.0))
    cases.append(("random", qkv, lens, eo.rope_table(L, 10000.0).astype(F32)))
    qkv, lens, _ = eo.attention_structured("ascending", L, heads, eo.structured_variant("ascending", heads))
    cases.append(("ascending", qkv, lens, eo.identity_rope(L)))
    for name, qkv, lens, rope in cases:
        B = len(lens)
        ref, A = eo.attention(qkv, lens, rope, B, L, heads)
        nv = np.clip(lens, 0, L)
        good = emulate_attention(qkv, lens, rope, B, L, heads)
        assert not _violations(good, ref, eo.attention_bound(A, eo.ATTN_T), B, L).any(), (name, "the faithful emulation misses the bound")
        for mutant, shows in ATTN_MUTANTS.items():
            if mutant == "no_rescale" and name == "random":
                shows = lambda n, L: n >= 64           # i.i.d. scores: the maximum moves late with near certainty only over many keys
            got = emulate_attention(qkv, lens, rope, B, L, heads, **{mutant: True})
            bad = _violations(got, ref, eo.attention_bound(A, eo.ATTN_T_CAP), B, L)
            for b in range(B):
                if shows(int(nv[b]), L):
                    assert bad[b], f"{name}, L {L}, n {nv[b]}: the bound at t = {eo.ATTN_T_CAP} accepts the {mutant} mutant"


def test_uniform_case_rejects_the_swapped_halves_and_the_dropped_key():
    L = 65
    qkv, lens, want16 = eo.attention_structured("uniform", L, 1, eo.structured_variant("uniform", 1))
    B = len(lens)
    good = emulate_attention(qkv, lens, eo.identity_rope(L), B, L, 1)
    assert eo.ulp16_distance(good, want16).max() <= 1
    for mutant in ("swap_halves", "drop_last", "extra_key"):
        got = emulate_attention(qkv, lens, eo.identity_rope(L), B, L, 1, **{mutant: True})
        assert not (eo.ulp16_distance(got, want16).max() <= 1), mutant


def emulate_layernorm(c, one_pass=False, round512=False):
    """fp32 statistics as the kernel takes them (two passes over the row), fp16 result; the flags are the mutants."""
    v = c["x"].astype(F32) + (c["res"].astype(F32) if c["res"] is not None else F32(0))
    width = v.shape[1]
    div = F32(((width + 511) // 512) * 512 if round512 else width)
    mean = v.sum(axis=1, dtype=F32) / div
    if one_pass:
        var = (v * v).sum(axis=1, dtype=F32) / div - mean * mean
    else:
        d = v - mean[:, None]
        var = (d * d).sum(axis=1, dtype=F32) / div
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = F32(1) / np.sqrt(var + F32(eo.LN_EPS), dtype=F32)
        return ((v - mean[:, None]) * rstd[:, None] * c["gamma"].astype(F32) + c["beta"].astype(F32)).astype(np.float16)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("width", eo.LN_WIDTHS)
def test_layernorm_bound_accepts_two_pass_fp32_and_rejects_the_mutants(width, residual):
    """rows = 1000 (200 rows of each family).  One-pass variance E[v^2] - mean^2 in fp32: rejected at K = 64 on the |mean| >> sigma
    rows, at every width, by a factor of ~15 on the typical row.  Dividing by the width rounded up to 512: rejected wherever that is another number."""
    c = eo.layernorm_case(width, 1000, residual)
    ref, mean, sigma = eo.add_layernorm(c["x"], c["res"], c["gamma"], c["beta"], eo.LN_EPS)
    err = lambda got: np.abs(got.astype(np.float64) - ref)
    good = emulate_layernorm(c)
    assert (err(good) <= eo.layernorm_bound(ref, mean, sigma, c["gamma"], eo.LN_K)).all()
    const = c["family"] == 3
    assert np.array_equal(good[const].view(np.uint16), np.broadcast_to(c["beta"], good.shape)[const].view(np.uint16))
    cap = eo.layernorm_bound(ref, mean, sigma, c["gamma"], eo.LN_K_CAP)
    offset = c["family"] == 2
    miss = ~(err(emulate_layernorm(c, one_pass=True)) <= cap)
    # the fp32 sums of a row can come out exact by chance (often at 8 columns, now and then at any width): most such rows, not every one
    frac = miss[offset].any(axis=1).mean()
    worst = (err(emulate_layernorm(c, one_pass=True)) / cap)[offset].max()
    print(f"width {width}: one-pass variance misses the K = 64 bound on {100 * frac:.0f} % of the |mean| >> sigma rows, by up to {worst:.0f} x")
    assert frac > (0.8 if width > 8 else 0.5) and worst > 10, "one-pass variance passes on |mean| >> sigma rows"
    if width % 512:
        miss = ~(err(emulate_layernorm(c, round512=True)) <= cap)
        assert miss[sigma > 0].any(axis=1).all(), "dividing by the padded width passes"      # (8 equal signs make a +-60000 row constant too)


def emulate_swiglu(gu16, inter, swapped=False):
    g, u = gu16[:, :inter].astype(F32), gu16[:, inter:].astype(F32)
    if swapped:
        g, u = u, g
    with np.errstate(over="ignore", invalid="ignore"):
        return (g / (F32(1) + np.exp(-g, dtype=F32)) * u).astype(np.float16)


@pytest.mark.parametrize("up", eo.SWIGLU_UPS)
def test_swiglu_one_ulp_accepts_fp32_and_rejects_the_swap(up):
    gu = eo.swiglu_exhaustive(up)
    want = eo.fp16_rne(eo.swiglu(gu, 2048))
    assert not np.isnan(want).any()
    assert eo.ulp16_distance(emulate_swiglu(gu, 2048), want).max() <= 1
    bad = emulate_swiglu(gu, 2048, swapped=True)
    assert np.isnan(bad).any() or eo.ulp16_distance(bad, want).max() > 1
    if up == 60000.0:                              # the overflowing products: +-inf of the gate's sign
        g = gu[:, :2048].astype(np.float64)
        assert (want[g > 2] == np.inf).all() and np.isfinite(want[g < 0]).all()
    if up == -3.0:
        g = gu[:, :2048].astype(np.float64)
        assert (want[g > 30000] == -np.inf).all()
    for rows, inter in eo.SWIGLU_SMALL:
        gu = eo.swiglu_random(rows, inter)
        want = eo.fp16_rne(eo.swiglu(gu, inter))
        assert eo.ulp16_distance(emulate_swiglu(gu, inter), want).max() <= 1
        assert eo.ulp16_distance(emulate_swiglu(gu, inter, swapped=True), want).max() > 1


def emulate_mean_pool(h16, lens, L, acc=F32, by_L=False):
    B, _, width = h16.shape
    out = np.zeros((B, width), F32)
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), L))
        a = np.zeros(width, acc)
        with np.errstate(over="ignore"):
            for t in range(n):
                a = (a + h16[b, t].astype(acc)).astype(acc)
        out[b] = a.astype(F32) * (F32(1) / F32(L if by_L else max(n, 1)))
    return out


@pytest.mark.parametrize("width,seq,offset", [(w, s, False) for w in eo.POOL_WIDTHS for s in eo.POOL_SEQS] + [(8, 512, True), (776, 512, True)])
def test_mean_pool_bound_accepts_fp32_and_rejects_the_mutants(width, seq, offset):
    h, lens = eo.pool_case(width, seq, offset)
    ref, mabs = eo.mean_pool(h, lens, seq)
    bound = eo.mean_pool_bound(ref, mabs, lens, seq)
    err = lambda got: np.abs(got.astype(np.float64) - ref)
    assert (err(emulate_mean_pool(h, lens, seq)) <= bound).all()
    assert (bound[np.clip(lens, 0, seq) == 0] == 0).all()
    n = np.clip(lens, 0, seq)
    by_L = ~(err(emulate_mean_pool(h, lens, seq, by_L=True)) <= bound)
    assert by_L[(n > 0) & (n < seq)].any(axis=1).all() and not by_L[n == seq].any()
    half = ~(err(emulate_mean_pool(h, lens, seq, acc=np.float16)) <= bound)
    if seq >= 50:                                 # an fp16 accumulator: rejected on every sequence of more than a few tokens
        assert half[n >= 49].any(axis=1).all()
    if offset:
        assert half[n >= 49].all()                # ... and, where the sum leaves fp16 altogether, in every element


# ---- 4. the header --------------------------------------------------------------------------------------------------------------
def test_header_documents_lengths_outside_the_sequence():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in ("rq_nb_rope_table_f32", "rq_nb_attention_f16", "rq_nb_attention_packed_f16", "rq_nb_add_layernorm_f16", "rq_nb_swiglu_f16",
                 "rq_nb_mean_pool_f16", "rq_nb_mean_pool_packed_f16"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
    doc = h[h.index("ctx[b][t][:] = softmax("):h.index("int rq_nb_attention_f16(")]
    for word in ("d_len[b] > seq counts as seq", "negative d_len[b] is an empty sequence", "come out zero", "nothing else is written", "device memory"):
        assert word in re.sub(r"\s*\n \* ", " ", doc), word
    doc = h[h.index("d_out[b][:] (fp32) = mean"):h.index("int rq_nb_mean_pool_f16(")]
    for word in ("0 for an empty sequence", "d_len[b] > seq counts as seq", "negative d_len[b] is an empty sequence"):
        assert word in re.sub(r"\s*\n \* ", " ", doc), word
