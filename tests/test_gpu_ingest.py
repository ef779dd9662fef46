"""An index's stored state is a function of its rows, not of its history (MI355X), against tests/ingest_oracle.py.

The other GPU tests pin the kernels that READ the stored state; here the code that WRITES it is pinned: the two conversion kernels at
every lane edge, the row statistics that widen the certificate, the incrementally built int8 image, the NaN row scales of the ragged
end, rq_load.  Any split of the rows into appends, any mix of the four append entry points, `reserve` before or between appends,
either row_pad and a save / load in the middle must leave the same stored bits, the same statistics, the same int8 bin errors and
bit-identical search outputs as ONE add_f16 of the same fp16 rows; the statistics must equal the fp64 host model of their definition.

  (a) test_conversion_and_padding_at_every_lane_edge   9 rows at 14 dims x both layouts x six append forms
  (b) test_statistics_equal_the_model                   ~300 rows with every special row, appended in three stages
  (c) test_history_does_not_matter                      4 200 rows: six histories against one add_f16, itself against the definition
  (d) test_int8_image_*                                 an image extended inside a bin, rebuilt after a reallocation, switched off by an inf
  (e) test_ragged_end                                   appends of one row, a search after each
"""
import os
import struct
import sys

import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_oracle as ino  # noqa: E402
import nonfinite_oracle as nfo  # noqa: E402
import score_bits as sb  # noqa: E402

pytestmark = pytest.mark.gpu
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
SCORE_TOL = 1e-6
STAT_REL = 1e-12             # both sides sum <= 768 non-negative fp64 terms in different orders (768 x 2^-53 = 8.5e-14), then one or two
                             # square roots and one division: a few ulp more
STATS = ("max_row_norm", "max_sub_rel", "max_sub_abs")
ENTRIES = ("f16", "f16_device", "f32", "f32_device")


def _index(dim, row_pad=None):
    idx = nat.NativeIndex(dim, 0)
    if row_pad is not None and idx.row_pad != row_pad:
        idx.set_option("row_pad", row_pad)
    assert row_pad is None or idx.row_pad == row_pad
    return idx


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared rows are read-only)


def _append(idx, how, x16, x32=None, normalize=False):
    """x16 through one of the four entry points; the fp32 forms take x32, or the fp16 rows widened."""
    if how in ("f32", "f32_device") and x32 is None:
        x32 = x16.astype(np.float32)
    if how == "f16":
        idx.add_f16(x16)
    elif how == "f16_device":
        t = _dev(x16)
        idx.add_f16_device(t, len(x16))
    elif how == "f32":
        idx.add_f32(x32, normalize)
    else:
        t = _dev(x32)
        idx.add_f32_device(t, len(x32), normalize)


def _close(a, b, rel=STAT_REL):
    return abs(a - b) <= rel * abs(b)


def _scanned8(idx, scan8, call):
    """call() under option "scan8"; the int8 image must have been scanned by it (scan8 = 2: "scan8_used" advances; a repair may scan
    it again) or not at all (scan8 = 0, or want = False)."""
    used = int(idx.get_option("scan8_used"))
    out = call()
    now = int(idx.get_option("scan8_used"))
    assert (now > used) if scan8 else (now == used), f"scan8 = {scan8}: scan8_used went from {used} to {now}"
    return out


def _assert_stats(idx, x16, what):
    """The three statistics against the model (STAT_REL), both eps_* against the model after its fp32 cast (1 ulp of fp32)."""
    want = ino.shard_stats(x16)
    got = tuple(idx.get_option(o) for o in STATS)
    for o, g, w in zip(STATS, got, want):
        assert _close(g, w), f"{what}: {o} is {g!r}, the model says {w!r} (relative difference {abs(g - w) / max(abs(w), 1e-300):.3g})"
    for o, metric in (("eps_cosine", COS), ("eps_ip", IP)):
        g, w = np.float32(idx.get_option(o)), ino.eps(metric, want)
        assert float(g) == idx.get_option(o), f"{what}: {o} is not an fp32 value"
        assert abs(int(sb.mono(sb.bits(g))[0]) - int(sb.mono(sb.bits(w))[0])) <= 1, f"{what}: {o} is {g!r}, the model says {w!r}"
    return want


# ---- (a) conversion and padding at every lane edge ------------------------------------------------------------------------------
DIMS = [1, 3, 4, 5, 255, 256, 257, 383, 384, 385, 511, 513, 767, 768]
LAYOUTS = [(d, 384 if d <= 384 else 768) for d in DIMS] + [(d, 768) for d in DIMS if d <= 384]
LANE_ROWS = 9                 # two workgroups of four waves, one of them ragged


def _lane_rows(dim):
    """fp16 rows whose bits carry (row, element): 0x3000 + row * 768 + element (0.125 .. 14), the sign alternating: every value is
    distinct, finite and normal, and neighbours never share a sign."""
    r, i = np.meshgrid(np.arange(LANE_ROWS), np.arange(dim), indexing="ij")
    bits = (0x3000 + r * 768 + i) | (((r + i) & 1) << 15)
    return bits.astype(np.uint16).view(np.float16)


def _lane_rows_f32(x16):
    """The same rows moved off the fp16 grid by up to 3/8 of an fp16 ulp: they round back to x16, and the rounding is exercised."""
    r, i = np.meshgrid(np.arange(x16.shape[0]), np.arange(x16.shape[1]), indexing="ij")
    return (x16.astype(np.float32) * (np.float32(1) + np.float32(2.0 ** -14) * ((5 * r + 3 * i) % 7 - 3).astype(np.float32))).astype(np.float32)


@pytest.mark.parametrize("dim,row_pad", LAYOUTS, ids=[f"dim{d}-pad{p}" for d, p in LAYOUTS])
def test_conversion_and_padding_at_every_lane_edge(dim, row_pad):
    x16 = _lane_rows(dim)
    x32 = _lane_rows_f32(x16)
    assert np.array_equal(orc.prepare_rows_f32(x32, False).view(np.uint16), x16.view(np.uint16))
    q = orc.synthetic_queries(3, dim, seed=dim)
    for how, normalize in [("f16", False), ("f16_device", False), ("f32", False), ("f32", True), ("f32_device", False), ("f32_device", True)]:
        what = f"dim {dim} row_pad {row_pad} add_{how}{' normalize' if normalize else ''}"
        want = orc.prepare_rows_f32(x32, True) if normalize else x16
        idx = _index(dim, row_pad)
        _append(idx, how, x16, x32, normalize)
        assert len(idx) == LANE_ROWS, what
        got = idx.get_rows_f16(0, LANE_ROWS)
        diff = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
        assert not len(diff), f"{what}: stored bits differ at (row, element) {diff[:6].tolist()}"
        # the padding cannot be read back: junk in it would raise the largest row norm above that of the unpadded rows
        _assert_stats(idx, want, what)
        s, r = idx.search(q, 5)
        gs, gr = orc.dense_topk(q, want, 5)
        assert np.array_equal(r, gr) and float(np.abs(s - gs).max()) <= SCORE_TOL, what
        idx.close()


# ---- (b) statistics equal the model ---------------------------------------------------------------------------------------------
def _clear_subnormals(row, to):
    b = row.view(np.uint16)
    flushed = (b & 0x7C00) == 0
    b[flushed] = (b[flushed] & 0x8000) | to


def _stats_corpus(dim):
    """(rows, stage ends).  Stage 0: a NaN row, an inf row (either would win every maximum if it were counted), a row with exactly
    one subnormal element, a zero row, a row of -0.0 elements.  Stage 1: ordinary unit rows around a second NaN row and a -inf row.
    Stage 2: a row of +-65 504 (the largest norm), a row of 0x03ff beside 0x0400 (the largest absolute flushed mass: the boundary of
    the exponent test), a row of subnormals only (relative flushed mass exactly 1)."""
    rng = np.random.default_rng(1000 + dim)
    x = orc.synthetic_corpus(300, dim, seed=dim).copy()
    x[0] = np.nan
    x[1, dim // 2] = np.inf
    _clear_subnormals(x[2], 0x0400)
    x[2].view(np.uint16)[7] = 0x03FF
    x[3] = 0
    _clear_subnormals(x[4], 0x0000)
    x[4].view(np.uint16)[::5] = 0x8000
    x[150] = np.nan
    x[151, dim - 1] = -np.inf
    x[297] = np.where(np.arange(dim) % 2 == 0, 65504.0, -65504.0).astype(np.float16)
    x[298].view(np.uint16)[:] = np.where(np.arange(dim) % 2 == 0, 0x03FF, 0x8400).astype(np.uint16)
    x[299].view(np.uint16)[:] = (rng.integers(1, 0x0400, dim) | (rng.integers(0, 2, dim) << 15)).astype(np.uint16)
    return x, (5, 297, 300)


@pytest.mark.parametrize("dim,row_pad", [(768, 768), (384, 384)], ids=["dim768", "dim384-narrow"])
def test_statistics_equal_the_model(dim, row_pad):
    x, ends = _stats_corpus(dim)
    idx = _index(dim, row_pad)
    begin = 0
    for stage, end in enumerate(ends):
        idx.add_f16(x[begin:end])
        _assert_stats(idx, x[:end], f"dim {dim}, after stage {stage} ({end} rows)")
        begin = end
    assert np.array_equal(idx.get_rows_f16(0, 300).view(np.uint16), x.view(np.uint16))
    idx.close()
    # what the rows are there for, from the model: each special row decides a statistic at the end of its stage
    s0, s1, s2 = (ino.shard_stats(x[:e]) for e in ends)
    assert s0 == ino.shard_stats(x[2:3]) and s0[2] == 1023 * 2.0 ** -24, "stage 0: the row with one subnormal element decides"
    assert s2[0] == ino.row_norms(x[297:298])[0] and s2[1] == 1.0 and s2[2] == ino.shard_stats(x[298:299])[2] > s1[2]
    assert np.isfinite(s2).all() and not np.isfinite(ino.row_norms(x)[[0, 1, 150, 151]]).any()


# ---- the definition, for a handful of returned rows ------------------------------------------------------------------------------
def _assert_topk_bits(got_s, got_r, x16, q, k, metric, what, extra=32, x64=None):
    """Rows equal to the canonical top-k of the fp64 definition and scores with its bits (tests/score_bits.py), the definition being
    evaluated with exactly rounded sums over each query's k + extra best rows by plain fp64 scores (x64: the rows widened once by
    the caller).  Returns (pairs, undecided)."""
    n = len(x16)
    x64 = x16.astype(np.float64) if x64 is None else x64[:n]
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    s = q64 @ x64.T
    if metric == COS:
        s = s / (np.sqrt((q64 * q64).sum(axis=1))[:, None] * np.sqrt((x64 * x64).sum(axis=1))[None, :] + 1e-30)
    checked = und = 0
    for b in range(len(q)):
        m = min(n, k + extra)
        order = np.argsort(-s[b], kind="stable")
        assert m == n or s[b, order[k - 1]] > s[b, order[m]], f"{what}: query {b}: {extra} rows beyond k do not separate the candidates"
        cand = np.sort(order[:m])
        ref = sb.reference(x16[cand], q[b:b + 1], metric)
        _, wr, flagged = sb.canonical_topk(ref, k)
        assert not flagged.any(), f"{what}: query {b}: an undecided pair near the cut"
        wr = wr[0]
        ke = int((wr >= 0).sum())
        assert np.array_equal(got_r[b, :ke], cand[wr[:ke]]) and (got_r[b, ke:] == -1).all(), \
            f"{what}: query {b}: rows {got_r[b].tolist()}, the definition says {cand[wr[:ke]].tolist()}"
        gb = sb.mono(sb.bits(got_s[b, :ke]))
        lo, hi = sb.mono(sb.bits(ref.lo[0, wr[:ke]])), sb.mono(sb.bits(ref.hi[0, wr[:ke]]))
        assert ((gb >= lo) & (gb <= hi)).all(), f"{what}: query {b}: scores {got_s[b].tolist()} do not have the bits of the definition"
        assert not sb.bits(got_s[b, ke:]).any(), f"{what}: query {b}: padding does not score +0.0"
        checked += ke
        und += int((~ref.decided[0, wr[:ke]]).sum())
    return checked, und


# ---- (c) history does not matter ------------------------------------------------------------------------------------------------
N_C, K_C, B_C = 4_200, 10, 8          # 65 whole bins and a ragged one of 40 rows; 2 (k + 8) < 66 bins: the approximate routes, int8 included
PIECES = (1, 3, 63, 64, 65, 1000)


def _history_rows():
    """Gaussian directions at norms 0.5 .. 2 (scores of both metrics span binades), a zero row, a duplicated row, three rows that
    quantise worse; every ordinary row keeps its natural handful of fp16-subnormal elements."""
    x = sb.gaussian_rows(N_C, 768, IP, seed=61).copy()
    x[9] = 0
    x[2077] = x[3]
    x[1000:1003] = (x[1000:1003].astype(np.float32) * np.linspace(0.2, 3.0, 768, dtype=np.float32)).astype(np.float16)
    return x


def _history_queries(x16):
    q = {m: sb.queries(B_C, 768, m, seed=62).copy() for m in (COS, IP)}
    for m in (COS, IP):
        q[m][1] = x16[N_C - 1].astype(np.float32)          # a planted match in the ragged last bin
        q[m][2] = x16[3].astype(np.float32)                # ... and one that ties rows 3 and 2077
    return q


def _device_search(idx, q, k, metric):
    import torch
    d_q = _dev(q)
    d_s = torch.full((len(q), k), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((len(q), k), 7, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(q),), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_device(d_q, len(q), k, metric, d_s, d_r, None, d_st, 0)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_r.cpu().numpy(), d_st.cpu().numpy()


def _state(idx, q):
    """Everything of an index the tests can observe, as bytes, plus the blocking results per (scan8, metric)."""
    n = len(idx)
    nbins = (n + 63) // 64
    st, res = {}, {}
    st["rows"] = idx.get_rows_f16(0, n).tobytes()
    st["statistics"] = struct.pack("5d", *[idx.get_option(o) for o in STATS + ("eps_cosine", "eps_ip")])
    for scan8 in (0, 2):
        idx.set_option("scan8", scan8)
        for metric in (COS, IP):
            s, r = _scanned8(idx, scan8, lambda: idx.search(q[metric], K_C, metric))
            res[(scan8, metric)] = (s, r)
            st[f"search scan8={scan8} metric={metric}"] = s.tobytes() + r.tobytes()
        for metric in (COS, IP):
            s, r, status = _scanned8(idx, scan8, lambda: _device_search(idx, q[metric], K_C, metric))
            pooled = [idx.debug_pooled(j, nbins) for j in (0, 1)]
            assert all(len(p) == nbins for p in pooled)
            st[f"search_device scan8={scan8} metric={metric}"] = s.tobytes() + r.tobytes() + status.tobytes()
            st[f"debug_pooled scan8={scan8} metric={metric}"] = b"".join(p.tobytes() for p in pooled)
    be = idx.debug_bin_err(nbins)
    assert len(be) == nbins
    st["debug_bin_err"] = be.tobytes()
    st["scan8_row_err"] = struct.pack("d", idx.get_option("scan8_row_err"))
    return st, res


@pytest.fixture(scope="module")
def history():
    """The rows (read back once from the reference build), the queries and the state of R = one add_f16."""
    x = _history_rows()
    idx = _index(768)
    idx.add_f16(x)
    x16 = idx.get_rows_f16(0, N_C)
    assert np.array_equal(x16.view(np.uint16), x.view(np.uint16))
    x16.setflags(write=False)
    q = _history_queries(x16)
    st, res = _state(idx, q)
    yield idx, x16, q, st, res
    idx.close()


def test_reference_build_matches_the_definition_and_the_model(history):
    idx, x16, q, st, res = history
    checked = und = 0
    for (scan8, metric), (s, r) in res.items():
        c, u = _assert_topk_bits(s, r, x16, q[metric], K_C, metric, f"R, scan8 = {scan8}, metric {metric}")
        checked, und = checked + c, und + u
    print(f"score bits [reference build]: {checked} pairs checked, {und} undecided")
    assert und <= sb.CAP * checked
    assert res[(0, COS)][1][2, :2].tolist() == [3, 2077], "the duplicated row ties and orders by row id"
    assert res[(0, COS)][1][1, 0] == N_C - 1
    _assert_stats(idx, x16, "R")
    im = ino.int8_image(x16)
    be = np.frombuffer(st["debug_bin_err"], np.float32)
    want = im.bin_err.astype(np.float64)
    assert np.all(be >= want * (1 - 1e-6)) and np.all(be <= want * (1 + 1e-5) + 1e-9), float(np.abs(be - want).max())
    row_err = struct.unpack("d", st["scan8_row_err"])[0]
    assert abs(float(be.max()) - row_err) <= 1e-6 * float(be.max()) and _close(row_err, im.shard_err, 1e-9)


def _pieces(n, sizes):
    cuts, at = [], 0
    for s in sizes:
        cuts.append((at, at + s))
        at += s
    return cuts + [(at, n)]


def _build_pieces(x16, tmp_path):
    idx = _index(768)
    for b, e in _pieces(N_C, PIECES):
        idx.add_f16(x16[b:e])
    return idx


def _build_pieces_reserved(x16, tmp_path):
    idx = _index(768)
    idx.reserve(N_C + 4096)
    for b, e in _pieces(N_C, PIECES):
        idx.add_f16(x16[b:e])
    return idx


def _build_four_entry_points(x16, tmp_path):
    idx = _index(768)
    for i, b in enumerate(range(0, N_C, 100)):
        _append(idx, ENTRIES[i % 4], x16[b:b + 100])
    return idx


def _build_reserve_between(x16, tmp_path):
    idx = _index(768)
    idx.add_f16(x16[:777])
    idx.reserve(3 * N_C)
    idx.add_f16(x16[777:])
    return idx


def _build_save_load_append(x16, tmp_path):
    half = _index(768)
    half.add_f16(x16[:N_C // 2])
    half.save(str(tmp_path / "half"))
    half.close()
    idx = nat.NativeIndex.load(str(tmp_path / "half"), 0)
    assert len(idx) == N_C // 2 and idx.dim == 768
    idx.add_f16(x16[N_C // 2:])
    return idx


def _build_save_load(x16, tmp_path):
    whole = _build_pieces(x16, tmp_path)
    whole.save(str(tmp_path / "whole"))
    whole.close()
    return nat.NativeIndex.load(str(tmp_path / "whole"), 0)


HISTORIES = {"pieces": _build_pieces, "pieces-reserved": _build_pieces_reserved, "four-entry-points": _build_four_entry_points,
             "reserve-between": _build_reserve_between, "save-load-append": _build_save_load_append, "save-load": _build_save_load}


@pytest.mark.parametrize("name", list(HISTORIES))
def test_history_does_not_matter(history, name, tmp_path):
    _, x16, q, want, _ = history
    idx = HISTORIES[name](x16, tmp_path)
    assert len(idx) == N_C
    got, _ = _state(idx, q)
    idx.close()
    assert list(got) == list(want)
    differ = [key for key in want if got[key] != want[key]]
    assert not differ, f"history '{name}' differs from one add_f16 in: {differ}"


# ---- (d) the int8 image follows the index ---------------------------------------------------------------------------------------
N_D, N_WORSE, N_AFTER, CAP_D = 4_200, 37, 11, 8_192
BIN_D = N_D >> 6                       # rows 4160 .. 4223: 40 of the first launch, 24 of the second


def _image_rows():
    """4 200 unit rows | 37 rows that quantise worse (the column scaling of tests/test_gpu_parity.py) | 11 ordinary rows | 4 100 more
    (past the reserved capacity)."""
    x = orc.synthetic_corpus(N_D + N_WORSE + N_AFTER + 4_100, 768, seed=71).copy()
    w = slice(N_D, N_D + N_WORSE)
    x[w] = (x[w].astype(np.float32) * np.linspace(0.2, 3.0, 768, dtype=np.float32)).astype(np.float16)
    return x


def _exact_under_both_scans(idx, x16, q, want_used=True):
    """Blocking searches of both metrics under the int8 and the fp16 scan against the oracle; leaves "scan8" = 2."""
    for scan8 in (2, 0, 2):
        idx.set_option("scan8", scan8)
        for metric, qq in ((COS, q), (IP, 3.0 * q[:9])):
            s, r = _scanned8(idx, scan8 if want_used else 0, lambda: idx.search(qq, 10, metric))
            ws, wr = nfo.topk(qq, x16, 10, metric)
            nfo.assert_matches(s, r, ws, wr, SCORE_TOL, f"{len(x16)} rows, scan8 = {scan8}, metric {metric}")


def _assert_image(idx, x16, what):
    """debug_bin_err and scan8_row_err against the model of ALL rows, with the margins of tests/test_gpu_parity.py."""
    nbins = (len(x16) + 63) // 64
    im = ino.int8_image(x16)
    be = idx.debug_bin_err(nbins)
    assert be.shape == (nbins,), what
    want = im.bin_err.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (be >= want * (1 - 1e-6)) & (be <= want * (1 + 1e-5) + 1e-9)
    assert ok.all(), f"{what}: bins {np.nonzero(~ok)[0][:6].tolist()}: {be[~ok][:6].tolist()}, the model says {want[~ok][:6].tolist()}"
    row_err = idx.get_option("scan8_row_err")
    assert row_err == float(be.max()) or abs(float(be.max()) - row_err) <= 1e-6 * float(be.max()), (what, row_err, float(be.max()))
    return im, be


def _grown_image():
    """reserve, 4 200 rows, a search (the image covers [0, 4200)), 37 worse rows, a search, 11 ordinary rows, a search: both straddled
    bins hold the maximum over both their parts."""
    x = _image_rows()
    q = orc.synthetic_queries(16, 768, seed=72)
    idx = _index(768)
    idx.reserve(CAP_D)
    idx.set_option("scan8", 2)
    idx.add_f16(x[:N_D])
    assert idx.get_option("scan8_row_err") == -1.0
    _exact_under_both_scans(idx, x[:N_D], q)
    _assert_image(idx, x[:N_D], "first image")
    n1 = N_D + N_WORSE
    idx.add_f16_device(_dev(x[N_D:n1]), N_WORSE)
    assert idx.get_option("scan8_row_err") == -1.0, "rows appended since: the image is not up to date"
    with pytest.raises(nat.RqError):
        idx.debug_bin_err((n1 + 63) // 64)
    _exact_under_both_scans(idx, x[:n1], q)
    im, be = _assert_image(idx, x[:n1], "image extended by 37 worse rows")
    old, new = im.row_err[BIN_D * 64:N_D].max(), im.row_err[N_D:(BIN_D + 1) * 64].max()
    assert new > old * 1.0001, "the rows of the second launch were to be the worse part of the straddled bin"
    assert be[BIN_D] >= new * (1 - 1e-6) and be[BIN_D + 1] >= im.row_err[(BIN_D + 1) * 64:n1].max() * (1 - 1e-6)
    n2 = n1 + N_AFTER
    idx.add_f32(x[n1:n2].astype(np.float32), False)
    _exact_under_both_scans(idx, x[:n2], q)
    im, be = _assert_image(idx, x[:n2], "image extended by 11 ordinary rows")
    old, new = im.row_err[(BIN_D + 1) * 64:n1].max(), im.row_err[n1:n2].max()
    assert old > new * 1.0001, "the rows of the earlier launch were to be the worse part of the second straddled bin"
    assert be[BIN_D + 1] >= old * (1 - 1e-6)
    return idx, x, q, n2


def test_int8_image_is_rebuilt_after_a_reallocating_append():
    idx, x, q, n2 = _grown_image()
    idx.add_f16(x[n2:])                                        # past the reserved capacity: the shard moves, the image is dropped
    n3 = len(x)
    assert n3 > CAP_D and len(idx) == n3
    assert idx.get_option("scan8_row_err") == -1.0
    with pytest.raises(nat.RqError):
        idx.debug_bin_err((n3 + 63) // 64)
    _exact_under_both_scans(idx, x, q)
    _, be = _assert_image(idx, x, "image rebuilt after the reallocation")
    fresh = _index(768)
    fresh.set_option("scan8", 2)
    fresh.add_f16(x)
    fresh.search(q, 10)
    assert fresh.debug_bin_err((n3 + 63) // 64).tobytes() == be.tobytes(), "no value of the old image may survive"
    assert fresh.get_option("scan8_row_err") == idx.get_option("scan8_row_err")
    assert np.array_equal(fresh.get_rows_f16(0, n3).view(np.uint16), idx.get_rows_f16(0, n3).view(np.uint16))
    fresh.close(); idx.close()


def test_int8_image_is_switched_off_by_an_appended_inf():
    idx, x, q, n2 = _grown_image()
    x = x[:n2 + 1].copy()
    x[n2, 300] = np.inf
    idx.add_f16(x[n2:])                                        # within the reserved capacity: the image is extended by this row
    assert len(idx) == n2 + 1 <= CAP_D
    _exact_under_both_scans(idx, x, q, want_used=False)        # answered by the fp16 scan, under the non-finite rules
    assert idx.get_option("scan8_row_err") == np.inf
    _, be = _assert_image(idx, x, "image extended by a row with an inf")
    assert np.isinf(be[-1]) and np.isfinite(be[:-1]).all()
    assert ino.shard_stats(x) == ino.shard_stats(x[:n2])
    _assert_stats(idx, x, "after the inf row")
    idx.close()


# ---- (e) the ragged end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,dim", [(0, 768), (4_060, 768), (4_060, 384)], ids=["130-rows", "4130-rows", "4130-rows-narrow"])
def test_ragged_end(first, dim):
    """reserve, then appends of ONE row (after `first` rows in one piece); a search after each of the last 70 with the newest row as a
    query.  The pad rows of the ragged bin keep their NaN row scales: the newest row is found, no row >= n ever appears, scores have
    the bits of the definition.  130 rows take the exact route, 4 130 the scans (and cross a bin edge at 4 096)."""
    total = first + 130 if first == 0 else first + 70
    x16 = orc.synthetic_corpus(total, dim, seed=total + dim)
    q = orc.synthetic_queries(3, dim, seed=81)
    x64 = x16.astype(np.float64)
    idx = _index(dim)
    idx.reserve(total)
    if first:
        idx.add_f16(x16[:first])
    checked = und = 0
    for n in range(first + 1, total + 1):
        _append(idx, ENTRIES[n % 4], x16[n - 1:n])
        if n <= total - 70:
            continue
        q[0] = x16[n - 1].astype(np.float32)
        for metric in (COS, IP):
            s, r = idx.search(q, 5, metric)
            what = f"dim {dim}, {n} rows, metric {metric}"
            assert r.min() >= 0 and r.max() < n, f"{what}: rows {r.tolist()}"
            assert r[0, 0] == n - 1, f"{what}: the newest row is not the best match of itself: {r[0].tolist()}"
            c, u = _assert_topk_bits(s, r, x16[:n], q, 5, metric, what, x64=x64)
            checked, und = checked + c, und + u
    assert len(idx) == total and np.array_equal(idx.get_rows_f16(0, total).view(np.uint16), x16.view(np.uint16))
    _assert_stats(idx, x16, f"dim {dim}, {total} rows one at a time")
    idx.close()
    print(f"score bits [ragged end, dim {dim}, {total} rows]: {checked} pairs checked, {und} undecided")
    assert und <= sb.CAP * checked
