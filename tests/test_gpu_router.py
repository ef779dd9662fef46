"""The router gate on the device (include/rq.h rq_router_*, csrc/rq_router.hip) against tests/router_gate_oracle.py, in both
normalisation modes.  Everything that does not depend on exp is held bit for bit: given the device's own w, every output of the
rerank equals the oracle's.  The gate itself is held to a derived tolerance: exactly 0, 1 or NaN where the oracle gives that,
elsewhere |dw| <= 2^-49 * w (3 ulp for the device library's exp -- the OpenCL bound that ocml follows --, 1 ulp for the host's, one
rounding each for the addition and the division on both sides).  tests/test_router.py shows that the oracle and the package's host
gate agree bit for bit, and pins both to the reference."""
import os
import sys

import numpy as np
import pytest

from rag_uq_amd import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import router_gate_oracle as rgo  # noqa: E402
import router_scenario as rs  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = rgo.cases()
MODES = (rgo.QUERY, rgo.STATS)
MODE_ID = {rgo.QUERY: _native.ROUTER_NORM_QUERY, rgo.STATS: _native.ROUTER_NORM_STATS}
TOL = 2.0 ** -49
_ORACLE_W = {}


def _native_gate(weights):
    return _native.RouterGate(weights["w0"], weights["b0"], weights["w1"], float(weights["b1"]), num_layers=weights["layers"])


def _oracle_w(case, mode):
    """One oracle evaluation per (case, mode), shared by the tests."""
    key = (case["name"], mode)
    if key not in _ORACLE_W:
        w = rgo.gate(case["weights"], case["b"], case["d"], mode, case["stats"] if mode == rgo.STATS else None)
        w.setflags(write=False)
        _ORACLE_W[key] = w
    return _ORACLE_W[key]


def _gate_close(got, want):
    """The gate tolerance; returns the worst relative error among the entries held to it."""
    assert got.shape == want.shape and got.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:5]       # (a NaN is a NaN: its sign is the host's or the device's default, not a value)
    exact = ((want == 0) | (want == 1)) & ~nan
    assert np.array_equal(got[exact].view(np.uint64), want[exact].view(np.uint64)), np.argwhere(exact & (got.view(np.uint64) != want.view(np.uint64)))[:5]
    exact |= nan
    err = np.abs(got[~exact] - want[~exact]) / want[~exact]
    assert (err <= TOL).all(), (float(err.max()), np.argwhere(~exact)[int(err.argmax())])
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gate_within_the_derived_tolerance_and_rerank_bit_for_bit(case, mode):
    """P of 1, 2, 63, 64, 65, 128, 129, 256, 257, 1 000, 1 024; B of 1, 3, 70; H of 1, 16, 64, 255, 256 and one layer; count 0, below P
    and at P, a key of -1 below count; top_r of 1, at the candidate count, one above, and P; all scores equal, a tie run cut by top_r,
    h of -0.0, +-inf and NaN in b or d, z beyond +-750."""
    stats = case["stats"] if mode == rgo.STATS else None
    ng = _native_gate(case["weights"])
    try:
        w = ng.gate(case["b"], case["d"], MODE_ID[mode], stats)
        worst = _gate_close(w, _oracle_w(case, mode))
        print(f"{case['name']} {mode}: worst |dw| / w = {worst / 2.0 ** -53:.2f} x 2^-53")
        calls = 1
        for top_r in case["top_rs"]:
            got = ng.rerank(case["keys"], case["b"], case["d"], case["count"], top_r, MODE_ID[mode], stats)
            want = rgo.rerank_given_w(case["keys"], case["b"], case["d"], w, case["count"], top_r)
            calls += 1
            for name, g, x in zip(("keys", "b", "d", "w", "h", "pos", "count"), got, want):
                assert rgo.same((g,), (x,)), (name, top_r, np.argwhere(g != x)[:5])
            k, _, _, gw, _, pos, cnt = got
            for q in range(len(cnt)):                                        # the rerank's w is the gate's w at that position, in its bits
                live = pos[q, :cnt[q]]
                assert np.array_equal(gw[q, :cnt[q]].view(np.uint64), w[q, live].view(np.uint64))
        assert ng.get_option("calls") == calls and ng.get_option("gate_calls") == 1 and ng.get_option("rerank_calls") == calls - 1
        assert ng.get_option("layers") == case["weights"]["layers"] and ng.get_option("hidden") == (len(case["weights"]["w1"]) if case["weights"]["layers"] == 2 else 0)
    finally:
        ng.close()


@pytest.mark.parametrize("mode", MODES)
def test_the_device_forms_on_a_side_stream(mode):
    import torch
    case = next(c for c in CASES if c["name"] == "p100_b70_h64")
    stats = case["stats"] if mode == rgo.STATS else None
    B, P, r = 70, 100, 10
    ng = _native_gate(case["weights"])
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d = {n: torch.from_numpy(case[n]).cuda() for n in ("keys", "b", "d", "count")}
            d_w = torch.full((B, P), 7.0, dtype=torch.float64, device="cuda")
            ng.gate_device(d["b"], d["d"], B, P, d_w, MODE_ID[mode], stats, stream=stream.cuda_stream)
            ok, op = (torch.full((B, r), 77, dtype=torch.int32, device="cuda") for _ in range(2))
            ob, od, ow, oh = (torch.full((B, r), 7.0, dtype=torch.float64, device="cuda") for _ in range(4))
            oc = torch.full((B,), 77, dtype=torch.int32, device="cuda")
            ng.rerank_device(d["keys"], d["b"], d["d"], d["count"], B, P, r, ok, ob, od, ow, oh, op, oc, MODE_ID[mode], stats, stream=stream.cuda_stream)
            w = d_w.cpu().numpy()
            got = tuple(t.cpu().numpy() for t in (ok, ob, od, ow, oh, op, oc))
        stream.synchronize()
        _gate_close(w, _oracle_w(case, mode))
        assert rgo.same((w,), (ng.gate(case["b"], case["d"], MODE_ID[mode], stats),))
        assert rgo.same(got, rgo.rerank_given_w(case["keys"], case["b"], case["d"], w, case["count"], r))
    finally:
        ng.close()


def test_refusals():
    case = next(c for c in CASES if c["name"] == "p65_b3_h16")
    keys, b, d, count = case["keys"], case["b"], case["d"], case["count"]
    ng = _native_gate(case["weights"])
    try:
        for top_r in (0, -1, 66):
            with pytest.raises(_native.RqError, match="top_r"):
                ng.rerank(keys, b, d, count, top_r)
        for mode in (-1, 2):
            with pytest.raises(_native.RqError, match="mode"):
                ng.gate(b, d, mode)
        with pytest.raises(_native.RqError, match="statistics"):
            ng.gate(b, d, _native.ROUTER_NORM_STATS)
        with pytest.raises(_native.RqError, match="P "):
            ng.gate(np.zeros((1, 1025)), np.zeros((1, 1025)))
        with pytest.raises(_native.RqError, match="B "):
            ng.gate(np.zeros((0, 4)), np.zeros((0, 4)))
        assert ng.get_option("no_such_option") == -1 and "unknown" in _native.last_error() and ng.get_option("calls") == 0
        w = ng.gate(b, d)                                                  # and the handle still answers
        assert rgo.same(ng.rerank(keys, b, d, count, 5), rgo.rerank_given_w(keys, b, d, w, count, 5))
    finally:
        ng.close()
    w = case["weights"]
    with pytest.raises(_native.RqError, match="num_layers"):
        _native.RouterGate(w["w0"], w["b0"], w["w1"], 0.0, num_layers=3)
    with pytest.raises(_native.RqError, match="use_batch_norm"):
        _native.RouterGate(w["w0"], w["b0"], w["w1"], 0.0, use_batch_norm=True)


def test_route_batch_on_the_device_equals_the_host_route(tmp_path):
    """3 000 passages, 70 questions, num_passages 20 and 100, with allowed_ids_each and with complete_scores, both normalisations: ids,
    b and d identical, the order identical, w within the gate tolerance and h within what that tolerance can move it:
    |dh| <= 2^-49 * w * (|b| + |d|) for the two products, plus 4 roundings of 2^-53 * (|b| + |d|) for 1 - w, the products and the sum.
    The host result is first shown to be separated (adjacent distinct h more than 1e-9 relative apart: the tolerance cannot reorder
    them; tests/test_router.py establishes the same over a host stand-in)."""
    docs, questions, each = rs.corpus()
    r = rs.retriever(tmp_path, sparse_backend="gpu", fusion_backend="gpu")
    try:
        r.add_documents(docs)
        assert r.router_backend == "host"
        for normalize in ("query", "stats"):
            gate = rs.gate(normalize)
            for P in (20, 100):
                for kw in ({"allowed_ids_each": each}, {"complete_scores": True}):
                    keywords = dict(num_passages=P, retrieval_pool_size=max(P, 50), return_weights=True, **kw)
                    r.router_backend = "host"
                    want, want_w = r.route_batch(questions, gate, 10, **keywords)
                    assert rs.separated(want) and sum(len(x) for x in want) > 500
                    r.router_backend = "gpu"
                    before = gate.native(0).get_option("rerank_calls")
                    got, got_w = r.route_batch(questions, gate, 10, **keywords)
                    assert gate.native(0).get_option("rerank_calls") == before + 1                                                 # the device branch ran
                    a, e = rs.answers(got), rs.answers(want)
                    assert [[x[:4] for x in res] for res in a] == [[x[:4] for x in res] for res in e], (normalize, P, list(kw))      # ids, texts, b, d and the order
                    _gate_close(got_w, want_w)
                    for ra, re_, w in zip(a, e, want_w):
                        for i, (x, y) in enumerate(zip(ra, re_)):
                            mag = abs(x[2]) + abs(x[3])
                            assert abs(x[4] - y[4]) <= TOL * w[i] * mag + 4 * 2.0 ** -53 * mag, (normalize, P, list(kw), x, y)
                    assert rs.answers(r.route_batch(questions, gate, 10, **{**keywords, "return_weights": False})) == a
            gate.close()
        r.router_backend = "auto"
        assert len(r.route_batch(questions[:3], rs.gate(), 5)) == 3
    finally:
        r.close()
