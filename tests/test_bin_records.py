"""tests/bin_records.py without a GPU: the numpy decoder pinned to hand-derived bit patterns of csrc/rq_device.h, the checker
against faithful synthetic records and planted faults (each must be reported by its own invariant), and a guard that every scan
variant the library builds is a case of tests/test_gpu_bin_records.py."""
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bin_records as br  # noqa: E402
import test_gpu_bin_records as gpu  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "efficient-rag-with-learned-retrieval-and-uncertainty-quantification_amd", "csrc")


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# ---- decoder ------------------------------------------------------------------------------------------------------------------
def test_decoder_pins_hand_derived_records():
    # x: 1.0 = 0x3f800000 with row 37; -2.5 = 0xc0200000 with row 63; +0 with row 0; the poison pattern
    # y: c2 = code16(1.0) = 0xbf80 (0x3f800000 | sign bit, high half), d = 1023 (saturated), p2 = 12
    #    decode: positive codes (bit 15 set) get zero low bits, k = 0xbf800000 -> float bits 0x3f800000 = 1.0 (rq_up16 rounded up already)
    #    c2 - d = 0xbb81 -> k = 0xbb810000 -> float bits 0x3b810000
    #    c2 = code16(-0.5) = 0x40ff (~0xbf000000, high half), d = 0, p2 = 0 -> k = 0x40ffffff, ~k = 0xbf000000 = -0.5
    #    c2 = 0x8000 = code16(+-0), d = 1, p2 = 63 -> decode(c2) = +0, decode(c2 - d) = decode(0x7fff) = bits ~0x7fffffff = -0
    #    c2 = 0x007f = code16(-inf) -> -inf
    rec = np.array([[0x3F800025, (0xBF80 << 16) | (1023 << 6) | 12],
                    [0xC020003F, (0x40FF << 16) | 0],
                    [0x00000000, (0x8000 << 16) | (1 << 6) | 63],
                    [0xFFFFFFFF, (0x007F << 16) | 5]], dtype=np.uint32)
    f = br.decode(rec)
    assert f["m1"][0] == 1.0 and f["m1"][1] == -2.5 and f["m1"][2] == 0.0 and np.isnan(f["m1"][3])
    assert f["p1"].tolist() == [37, 63, 0, 63] and f["p2"].tolist() == [12, 0, 63, 5]
    assert f["d"].tolist() == [1023, 0, 1, 0] and f["c2"].tolist() == [0xBF80, 0x40FF, 0x8000, 0x007F]
    assert f["c2val"][0] == 1.0 and f["c3val"][0] == np.float32(_f(0x3B810000))
    assert f["c2val"][1] == -0.5 and f["c3val"][1] == -0.5
    assert f["c2val"][2] == 0.0 and f["c3val"][2] == 0.0 and np.signbit(f["c3val"][2])
    assert np.isneginf(f["c2val"][3])
    assert br.code16(np.float32([1.0, -0.5, 0.0, -0.0, -np.inf])).tolist() == [0xBF80, 0x40FF, 0x8000, 0x8000, 0x007F]


def test_every_decoded_field_is_an_upper_bound():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(20000), rng.uniform(-1e-3, 1e-3, 5000), [0.0, -0.0, 1e-40, -1e-40]]).astype(np.float32)
    assert np.all(br.code16_value(br.code16(v)) >= v)
    trip = -np.sort(-rng.standard_normal((30000, 3)).astype(np.float32), axis=1)
    trip[:10000] *= 1e-3
    pos = rng.integers(0, 64, (30000, 3)).astype(np.uint32)
    ps = br.pos_score(trip, pos)
    f = br.decode(br.record_from_triple(ps[:, 0], ps[:, 1], ps[:, 2]))
    # bounds of the UNPERTURBED values, whose 6 low mantissa bits the positions replaced (rq_record_from_triple)
    assert np.all(f["m1"] >= trip[:, 0]) and np.all(f["c2val"] >= trip[:, 1]) and np.all(f["c3val"] >= trip[:, 2])
    assert np.all(f["m1"] - trip[:, 0] <= np.abs(trip[:, 0]) * 2.0 ** -16)
    assert np.all(f["c2val"] >= f["c3val"]) and np.all(f["d"] <= 1023)
    assert f["p1"].tolist() == pos[:, 0].tolist() and f["p2"].tolist() == pos[:, 1].tolist()


# ---- the checker: faithful records pass, each planted fault is reported by its invariant ----------------------------------------
N, B, BETA = 4101, 3, 7e-4       # 65 bins, 5 valid rows in the last


def _synthetic():
    rng = np.random.default_rng(11)
    exact = rng.uniform(-0.2, 0.2, (B, N)).astype(np.float32)
    exact[0, 7 * 64 + 5], exact[0, 7 * 64 + 40], exact[0, 7 * 64 + 61] = 0.9, 0.8, 0.7      # three strong rows in bin 7
    exact[1, 200:260] = 0.5                                                                  # ties across a bin edge
    approx = (exact + rng.uniform(-0.9, 0.9, exact.shape) * BETA).astype(np.float32)
    rec = br.records_from_scores(approx, N)
    pad = np.full((2,) + rec.shape[1:], br.POISON, np.uint32)                               # two pad slots of the pass
    return np.concatenate([rec, pad]), exact.astype(np.float64)


def _set(rec, q, b, m1=None, p1=None, c2=None, d=None, p2=None):
    x, y = int(rec[q, b, 0]), int(rec[q, b, 1])
    if m1 is not None:
        x = (struct.unpack("<I", struct.pack("<f", m1))[0] & 0xFFFFFFC0) | (x & 63)
    if p1 is not None:
        x = (x & 0xFFFFFFC0) | p1
    if c2 is not None:
        y = (c2 << 16) | (y & 0xFFFF)
    if d is not None:
        y = (y & 0xFFFF003F) | (d << 6)
    if p2 is not None:
        y = (y & 0xFFFFFFC0) | p2
    rec[q, b] = (x, y)


def test_faithful_records_pass_every_invariant():
    rec, exact = _synthetic()
    rep = br.check_records(rec, exact, N, BETA, B)
    assert not br.failures(rep), br.failures(rep)
    assert set(rep) == set(br.INVARIANTS)
    f = br.decode(rec[:B])
    assert (f["p1"][0, 7], f["p2"][0, 7]) == (5, 40)
    assert br.tightness(rec, exact, N) <= BETA
    # per-query and per-bin bounds are accepted in the same way
    assert not br.failures(br.check_records(rec, exact, N, np.full(B, BETA), B))
    assert not br.failures(br.check_records(rec, exact, N, np.full((B, 65), BETA), B))


def _fault_cases():
    c2_of = lambda v: int(br.code16(np.float32(v)))
    return {
        "I1": lambda r: r.__setitem__((1, 3), br.POISON),                              # a record nobody wrote
        "I2": lambda r: _set(r, 0, 7, m1=float(br.decode(r[0, 7])["m1"]) - 2 * BETA),  # m1 lowered by 2 beta
        "I3": lambda r: _set(r, 0, 7, m1=float(br.decode(r[0, 7])["m1"]) + 2 * BETA),  # m1 inflated
        "I4": lambda r: _set(r, 0, 7, p1=20),                                          # p1 moved to a weak row
        "I4 pad": lambda r: _set(r, 2, 64, p1=10),                                     # p1 on a pad row of the ragged last bin
        "I5": lambda r: _set(r, 0, 7, p2=5),                                           # p2 = p1
        "I6": lambda r: _set(r, 0, 7, c2=c2_of(0.8) - 2),                              # c2 below the second score - beta
        "I7": lambda r: _set(r, 0, 7, d=int(br.decode(r[0, 7])["c2"]) - c2_of(0.7) + 2),   # c3 below the third score - beta
        "I8": lambda r: r.__setitem__((4, 9), r[0, 9]),                                # a pad slot overwritten
    }


@pytest.mark.parametrize("fault", list(_fault_cases()))
def test_each_planted_fault_is_reported_by_its_invariant(fault):
    rec, exact = _synthetic()
    _fault_cases()[fault](rec)
    rep = br.check_records(rec, exact, N, BETA, B)
    inv = fault.split()[0]
    assert not rep[inv]["ok"], (fault, rep[inv])
    where = {"I1": (1, 3), "I4 pad": (2, 64), "I8": (4, 9)}.get(fault, (0, 7))
    assert rep[inv]["first"][:2] == where, (fault, rep[inv]["first"])
    if fault == "I4 pad":
        assert rep[inv]["first"][2] == 64 * 64 + 10


# ---- coverage guard: every built scan variant is a case of the GPU module ------------------------------------------------------
def _function(src, name):
    i = src.index(name + "(")
    j = src.index("\n}\n", i)
    return src[i:j]


def test_every_built_scan_variant_is_a_gpu_record_case():
    scan = _function(open(os.path.join(CSRC, "rq_scan.hip")).read(), "hipError_t rq_scan_launch")
    wide = _function(open(os.path.join(CSRC, "rq_scan_wide.hip")).read(), "hipError_t rq_scan_wide_launch")
    # rq_scan.hip: RQ_CASE(S, pf, O, ks, qw) -- the 4-wave ones by (kstage, ring, prefetch), the 8-wave one is wide_batch = 2
    defaults = dict(kstage=2, ring=3, prefetch=1)
    have64 = {(f.get("kstage", 2), f.get("ring", 3), f.get("prefetch", 1)) for f in gpu.SCAN64_FORMS}
    cases = re.findall(r"RQ_CASE\((\d+), (\d+), (\d+), (\d+), (\d+)\)", scan)
    cases = [c for c in cases if c[0] != "SS"]
    assert len(cases) >= 12
    for S, pf, _, ks, qw in cases:
        if qw == "4":
            assert (int(ks), int(S), int(pf)) in have64, f"RQ_CASE{(S, pf, ks, qw)} has no record case"
        else:
            assert qw == "8" and dict(wide_batch=2) in gpu.WIDE128_FORMS
    assert (defaults["kstage"], defaults["ring"], defaults["prefetch"]) in have64
    # the selection forms and the int8 forms of rq_scan_launch
    assert "if (epi &&" in scan and {f.get("epi", 1) for f in gpu.SCAN64_FORMS} >= {0, 1}
    i8 = {int(v) for v in re.findall(r"a\.i8 == (\d+)", scan)} | ({1} if "if (a.i8)" in scan else set())
    assert i8 == {1, 2, 3}, i8
    assert set(gpu.I8_SCAN_FORMS) >= i8
    # rq_scan_wide.hip: RQW_CASE(V, D, OCC, QW, QG, EPI, DBG, PRIO, I8) -> queries 16 QW QG; 90..95 are timing ablations
    wide128 = {f["wide128"] for f in gpu.WIDE128_FORMS if "wide128" in f}
    wide256 = {f["wide256"] for f in gpu.WIDE256_FORMS}
    for m in re.finditer(r"RQW_CASE\((\d+), (\d+), (\d+), (\d+), (\d+)((?:, \d+)*)\)", wide):
        v, qw, qg = int(m.group(1)), int(m.group(4)), int(m.group(5))
        extra = [int(t) for t in m.group(6).split(",")[1:]]
        if 90 <= v <= 95:
            continue
        is_i8 = len(extra) >= 4 and extra[3] == 1
        if is_i8:
            assert v in gpu.I8_256_VARIANTS, f"int8 wide variant {v} has no record case"
        elif 16 * qw * qg == 128:
            assert v in wide128, f"wide128 variant {v} has no record case"
        else:
            assert 16 * qw * qg == 256 and v in wide256, f"wide256 variant {v} has no record case"
    assert "variant == 8 " not in wide and "variant == 11 " not in wide       # (withdrawn)
    # the int8 32x32 form: variant == 33 and 30 <= variant <= 32
    w32 = {int(v) for v in re.findall(r"variant == (\d+)\)", wide)}
    r = re.search(r"variant >= (\d+) && variant <= (\d+)", wide)
    w32 |= set(range(int(r.group(1)), int(r.group(2)) + 1))
    assert w32 == {30, 31, 32, 33} and w32 <= set(gpu.I8_256_VARIANTS)
