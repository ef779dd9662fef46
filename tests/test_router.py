"""The router gate (include/rq.h rq_router_*, rag_uq_amd/router.py, HybridRetriever.route_batch), the parts that need no GPU: the header
and the binding, the host plan (csrc/rq_router_plan.h) under the sanitizers, the package's numpy gate against the yardstick
(tests/router_gate_oracle.py) bit for bit, both pinned to the reference's RetrievalRouter as captured in tests/golden/g2_router.json,
`route_batch` on the host route against the per-question loop it replaces, and the loud failure without a device.  The GPU side is
tests/test_gpu_router.py."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rag_uq_amd import _native
from rag_uq_amd import router as rt
from rag_uq_amd import streaming_index as si

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import router_gate_oracle as rgo  # noqa: E402
import router_scenario as rs  # noqa: E402
import test_hybrid_filtered as th  # noqa: E402  (its host stand-in for the dense index, which takes filters, and its scenario)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
NEW_CALLS = ["rq_router_create", "rq_router_destroy", "rq_router_get_option", "rq_router_gate_device", "rq_router_gate", "rq_router_rerank_device", "rq_router_rerank"]
CASES = rgo.cases()
MODES = (rgo.QUERY, rgo.STATS)


def _gate_of(weights, mode, stats):
    g = rt.RouterGate(weights["w0"], weights["b0"], weights["w1"], weights["b1"], num_layers=weights["layers"])
    if mode == rgo.STATS:
        g.set_stats(*stats)
    return g


def test_header_declares_and_documents_the_router_calls():
    h = open(os.path.join(ROOT, "include", "rq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert name in _native._SIGNATURES and hasattr(_native.load_library(), name)
    assert re.search(r"#define\s+RQ_ROUTER_MAX_HIDDEN\s+256", code) and _native.ROUTER_MAX_HIDDEN == 256
    assert re.search(r"#define\s+RQ_ROUTER_NORM_STATS\s+0", code) and re.search(r"#define\s+RQ_ROUTER_NORM_QUERY\s+1", code)
    assert (_native.ROUTER_NORM_STATS, _native.ROUTER_NORM_QUERY) == (0, 1)
    doc = h[h.index("router gate: the learned gate"):h.index("typedef struct rq_router rq_router;")]
    for word in ("num_layers 1 or 2", "widened exactly", "use_batch_norm", "COPIED", "ALL P slots", "RQ_ROUTER_NORM_STATS", "RQ_ROUTER_NORM_QUERY", "+ 1e-6", "S(x) / P", "(P - 1)",
                 "0/0 = NaN", "next power of two", "does not depend on the thread count", "deliberately not offered", "df = nd - nb", "a_j > 0 ? a_j : 0", "exp(-z)",
                 "h = w*d + (1.0 - w)*b", "key[i] >= 0", "-0.0 as +0.0", "ranks as -inf", "ascending position", "min(candidates, top_r)", "(-1, 0.0, 0.0, 0.0, 0.0, -1)",
                 "2^-49", "One workgroup per query", "47 KiB", "64 KiB", "no workspace", "stream order", "RQ_EINVAL", "RQ_ENODEVICE", "no HIP device", '"gate_calls"',
                 '"rerank_calls"', '"calls"', '"hidden"', '"layers"', "Not extended", "HOST memory"):
        assert word in doc, word


def test_plan_and_validation_on_the_host(tmp_path):
    """tests/native/router_plan_check.cpp: a stand-alone host program under the address and UB sanitizers (host code only: the flags
    are given to the host compilation alone)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "router_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "router_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ---- the host gate against the yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_gate_equals_the_oracle_bit_for_bit(case, mode):
    g = _gate_of(case["weights"], mode, case["stats"])
    stats = case["stats"] if mode == rgo.STATS else None
    want_w = rgo.gate(case["weights"], case["b"], case["d"], mode, stats)
    got_w = g.gate(case["b"], case["d"])
    assert rgo.same((got_w,), (want_w,)), np.argwhere(got_w.view(np.uint64) != want_w.view(np.uint64))[:5]
    for top_r in case["top_rs"]:
        got = g.rerank(case["keys"], case["b"], case["d"], case["count"], top_r)
        want = rgo.rerank(case["weights"], case["keys"], case["b"], case["d"], case["count"], top_r, mode, stats)
        for name, x, y in zip(("keys", "b", "d", "w", "h", "pos", "count"), got, want):
            assert rgo.same((x,), (y,)), (name, top_r)
        assert rgo.same(got, rt.rerank_given_w(case["keys"], case["b"], case["d"], want_w, case["count"], top_r))


def test_the_cases_hold_what_they_are_meant_to_hold():
    by = {c["name"]: c for c in CASES}
    assert {c["b"].shape[1] for c in CASES} >= {1, 2, 63, 64, 65, 128, 129, 256, 257, 1000, 1024} and {c["b"].shape[0] for c in CASES} >= {1, 3, 70}
    assert {len(c["weights"]["w1"]) for c in CASES if c["weights"]["layers"] == 2} >= {1, 16, 64, 255, 256} and any(c["weights"]["layers"] == 1 for c in CASES)
    for c in CASES:                                                          # no logit where one side's subnormal could meet the other's 0
        for mode in MODES:
            z = np.abs(rgo.logits(c["weights"], c["b"], c["d"], mode, c["stats"]))
            assert not ((z >= 700) & (z <= 750)).any(), (c["name"], mode)
    c = by["p65_b3_h16"]
    P = 65
    assert c["count"].tolist() == [P, P // 2, 0] and (c["keys"][:, 1] == -1).all() and c["top_rs"] == [1, 31, 32, P]
    c = by["all_equal"]
    for mode in MODES:
        w = rgo.gate(c["weights"], c["b"], c["d"], mode, c["stats"])
        assert (w == w[:, :1]).all() and 0 < w[0, 0] < 1
    nb = rgo.normalise(c["b"][0], rgo.QUERY)
    assert not nb.any()                                                      # std = 0: the deviations are 0 over a scale of 1e-6
    c = by["tie_run_cut"]
    k, b, d, w, h, pos, cnt = rgo.rerank(c["weights"], c["keys"], c["b"], c["d"], c["count"], 20, rgo.QUERY)
    run = [int(np.nonzero(pos[0] == p)[0][0]) for p in range(2, 12)]
    assert run == list(range(run[0], run[0] + 10)) and len(set(h[0, run].tolist())) == 1 and any(run[0] < r <= run[-1] for r in c["top_rs"])
    c = by["negative_zero_h"]
    k, b, d, w, h, pos, cnt = rgo.rerank(c["weights"], c["keys"], c["b"], c["d"], c["count"], 8, rgo.STATS, c["stats"])
    zeros = pos[0][h[0] == 0].tolist()
    assert zeros == list(range(7)) and np.signbit(h[0][h[0] == 0]).tolist() == [True, False, True, False, False, True, False]      # -0.0 ranks as +0.0: by position
    c = by["nonfinite"]
    for mode in MODES:
        k, b, d, w, h, pos, cnt = rgo.rerank(c["weights"], c["keys"], c["b"], c["d"], c["count"], 12, mode, c["stats"])
        assert np.isnan(h).any() and (cnt == 12).all()
        for q in range(6):                                                   # a NaN h ranks as -inf: last, behind every number, by position among themselves
            nan = np.isnan(h[q])
            assert not nan[: 12 - nan.sum()].any() and (np.diff(pos[q][nan]) > 0).all()
    c = by["z_beyond_750"]
    w = rgo.gate(c["weights"], c["b"], c["d"], rgo.STATS, c["stats"])
    assert w[0].tolist()[:7] == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.5] and w[0, 7] == 1.0 and 0 < w[0, 8] < 1e-40
    w = rgo.gate(c["weights"], c["b"], c["d"], rgo.QUERY)
    assert (w == 0).any() and (w == 1).any()
    one = by["p1_b3_h16"]
    assert np.isnan(rgo.normalise(one["b"][0], rgo.QUERY)).all()            # P = 1: 0/0, as torch's unbiased std of one element


def test_tree_sum_is_the_fixed_pairwise_tree():
    x = np.array([1e16, 1.0, -1e16, 3.0, 0.5])
    assert rgo.tree_sum(x) == ((1e16 + 0.5) + -1e16) + (1.0 + 3.0) and rt._tree_sum(x[None, :])[0] == rgo.tree_sum(x)
    assert rgo.tree_sum([7.0]) == 7.0 and rgo.tree_sum([1.0, 2.0, 4.0]) == (1.0 + 4.0) + (2.0 + 0.0)
    assert np.signbit(rgo.tree_sum([-0.0, -0.0])) and not np.signbit(rgo.tree_sum([-0.0, -0.0, -0.0]))      # the padding is +0.0


# ---- pinned to the reference ----------------------------------------------------------------------------------------------------------------
def test_gate_and_rerank_match_the_reference_g2(golden_dir):
    """Against the reference's RetrievalRouter as captured in tests/golden/g2_router.json: every running-statistics case and every
    [1, P] batch-wise case (the [4, 20] and [2, 100] batch-wise cases are the whole-tensor normalisation that is not offered).  Gate
    weights within atol 2e-6 (the bound tests/test_oracle.py uses for the fp32 twin), rerank order equal up to exact ties in h."""
    g2 = json.load(open(os.path.join(golden_dir, "g2_router.json")))
    sd = g2["state_dict"]
    gate = rt.RouterGate.from_state_dict(sd, hidden=64)
    assert gate.hidden == 64 and gate.num_layers == 2 and gate.normalize == "query" and gate.stats.tolist() == [0.0, 1.0, 0.0, 1.0]
    weights = {"layers": 2, "w0": sd["scorer.0.weight"], "b0": sd["scorer.0.bias"], "w1": np.asarray(sd["scorer.3.weight"]).reshape(-1), "b1": sd["scorer.3.bias"][0]}
    used, worst = 0, 0.0
    for c in g2["cases"]:
        B, P = c["shape"]
        if not c["stats_initialized"] and B != 1:
            continue
        used += 1
        b, d = np.asarray(c["bm25"], np.float64), np.asarray(c["dense"], np.float64)
        if c["stats_initialized"]:
            gate.set_stats(**c["stats"])
            mode, stats = rgo.STATS, [c["stats"][k] for k in ("bm25_mean", "bm25_std", "dense_mean", "dense_std")]
        else:
            gate.normalize = "query"
            mode, stats = rgo.QUERY, None
        w = gate.gate(b, d)
        assert rgo.same((w,), (rgo.gate(weights, b, d, mode, stats),))
        worst = max(worst, float(np.abs(w - np.asarray(c["weights"], np.float64)).max()))
        np.testing.assert_allclose(w, np.asarray(c["weights"], np.float64), rtol=0, atol=2e-6)
        keys = np.arange(P, dtype=np.int32)[None, :].repeat(B, 0)
        h = w * d + (1.0 - w) * b

        def same_order(mine, ref, q):
            return len(mine) == len(ref) and all(m == t or h[q][m] == h[q][t] for m, t in zip(mine, ref))
        k = min(c["top_k"], P)
        pos = gate.rerank(keys, b, d, np.full(B, P), k)[5]
        full = gate.rerank(keys, b, d, np.full(B, P), P)[5]
        for q in range(B):
            assert same_order(pos[q].tolist(), c["rerank_indices"][q][:k], q), (c["shape"], q)
            if B == 1:
                assert same_order(full[q].tolist(), c["eval_loop_order"][q], q)
    print(f"g2_router: {used} cases, worst |w - golden| = {worst:.3g}")
    assert used >= 4 and any(not c["stats_initialized"] and c["shape"][0] == 1 for c in g2["cases"])


# ---- construction ------------------------------------------------------------------------------------------------------------------------------
def test_from_state_dict_and_from_module():
    import torch
    from torch import nn
    torch.manual_seed(0)

    class Router(nn.Module):
        def __init__(self, layers, batch_norm=False):
            super().__init__()
            self.scorer = nn.Sequential(*layers)
            for k, v in (("bm25_mean", 1.5), ("bm25_std", 2.0), ("dense_mean", 0.25), ("dense_std", 0.5)):
                self.register_buffer(k, torch.tensor(v))
            self.stats_initialized = False
            self.config = type("C", (), {"use_batch_norm": batch_norm})()

    two = Router([nn.Linear(3, 16), nn.ReLU(), nn.Dropout(0.1), nn.Linear(16, 1), nn.Sigmoid()]).eval()
    g = rt.RouterGate.from_module(two)
    assert (g.hidden, g.num_layers, g.normalize) == (16, 2, "query") and g.stats.tolist() == [1.5, 2.0, 0.25, 0.5]
    b, d = torch.rand(1, 20) * 10, torch.rand(1, 20)
    nb, nd = (b - b.mean()) / (b.std() + 1e-6), (d - d.mean()) / (d.std() + 1e-6)
    want = two.scorer(torch.stack([nb, nd, nd - nb], -1).reshape(-1, 3)).reshape(1, 20)
    np.testing.assert_allclose(g.gate(b.numpy(), d.numpy()), want.detach().numpy(), rtol=0, atol=2e-6)
    two.stats_initialized = True
    g = rt.RouterGate.from_module(two)
    assert g.normalize == "stats"
    nb, nd = (b - 1.5) / (2.0 + 1e-6), (d - 0.25) / (0.5 + 1e-6)
    want = two.scorer(torch.stack([nb, nd, nd - nb], -1).reshape(-1, 3)).reshape(1, 20)
    np.testing.assert_allclose(g.gate(b.numpy(), d.numpy()), want.detach().numpy(), rtol=0, atol=2e-6)
    one = Router([nn.Linear(3, 1), nn.Sigmoid()]).eval()
    g1 = rt.RouterGate.from_state_dict(one.state_dict())
    assert (g1.hidden, g1.num_layers) == (0, 1)
    np.testing.assert_allclose(g1.gate(b.numpy()[0], d.numpy()[0]), rt.RouterGate.from_module(one).gate(b.numpy(), d.numpy())[0], rtol=0, atol=0)
    with pytest.raises(ValueError, match="use_batch_norm"):
        rt.RouterGate.from_module(Router([nn.Linear(3, 8), nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.1), nn.Linear(8, 1), nn.Sigmoid()], batch_norm=True))
    with pytest.raises(ValueError, match="use_batch_norm"):
        rt.RouterGate.from_state_dict(Router([nn.Linear(3, 8), nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.1), nn.Linear(8, 1), nn.Sigmoid()]).state_dict())
    deep = Router([nn.Linear(3, 8), nn.ReLU(), nn.Dropout(0.1), nn.Linear(8, 8), nn.ReLU(), nn.Dropout(0.1), nn.Linear(8, 1), nn.Sigmoid()])
    with pytest.raises(ValueError, match="1 or 2 layers"):
        rt.RouterGate.from_module(deep)
    with pytest.raises(ValueError, match="hidden"):
        rt.RouterGate.from_state_dict(two.state_dict(), hidden=32)
    with pytest.raises(ValueError, match="hidden"):
        rt.RouterGate(np.zeros((257, 3)), np.zeros(257), np.zeros(257), 0.0)
    with pytest.raises(ValueError, match="normalize"):
        rt.RouterGate.from_state_dict(two.state_dict(), normalize="batch")
    with pytest.raises(ValueError, match="top_k"):
        g.rerank(np.zeros((1, 4), np.int32), np.zeros((1, 4)), np.zeros((1, 4)), [4], 5)


# ---- route_batch on the host route -------------------------------------------------------------------------------------------------------------
def _loop(r, gate, qs, top_k, P, pool, complete, each):
    """What a user does today, one question at a time: get_scores_for_router, the gate, the reorder, the real passages, the first top_k."""
    out, ws = [], []
    for q, e in zip(qs, each):
        b, d, ids, texts = r.get_scores_for_router(q, P, retrieval_pool_size=pool, complete_scores=complete, **si._given(allowed_ids=e))
        keys = np.array([[i if doc else -1 for i, doc in enumerate(ids)]], np.int32)
        k, ob, od, ow, oh, pos, cnt = gate.rerank(keys, [b], [d], [P], min(top_k, P))
        out.append([(ids[p], texts[p], ob[0, i], od[0, i], oh[0, i]) for i, p in enumerate(pos[0, :cnt[0]])])
        ws.append(ow[0])
    return out, np.array(ws)


@pytest.mark.parametrize("complete", [False, True], ids=["plain", "complete_scores"])
@pytest.mark.parametrize("normalize", ["query", "stats"])
def test_route_batch_on_the_host_equals_the_per_question_loop(tmp_path, normalize, complete):
    r, queries = th._scenario(tmp_path, "cosine")
    gate = rs.gate(normalize)
    tenants = [[f"p{i}" for i in range(t, 120, 3)] + [f"donly{t}"] for t in range(3)]
    each = [None if q % 4 == 1 else ([] if q == 6 else tenants[q % 3]) for q in range(len(queries))]
    assert r.router_backend == "host"
    for top_k, P, pool in ((10, 20, 50), (5, 100, 100), (7, 3, 2)):
        want, want_w = _loop(r, gate, queries, top_k, P, pool, complete, [None] * len(queries))
        got, got_w = r.route_batch(queries, gate, top_k, num_passages=P, retrieval_pool_size=pool, complete_scores=complete, return_weights=True)
        assert rs.answers(got) == want and any(want) and rgo.same((got_w,), (want_w,)), (top_k, P, pool)
        assert rs.answers(r.route_batch(queries, gate, top_k, num_passages=P, retrieval_pool_size=pool, complete_scores=complete)) == want
        want, want_w = _loop(r, gate, queries, top_k, P, pool, complete, each)
        got, got_w = r.route_batch(queries, gate, top_k, num_passages=P, retrieval_pool_size=pool, complete_scores=complete, allowed_ids_each=each, return_weights=True)
        assert rs.answers(got) == want and want[6] == [] and rgo.same((got_w,), (want_w,)), (top_k, P, pool)
        one, _ = _loop(r, gate, queries, top_k, P, pool, complete, [tenants[1]] * len(queries))
        assert rs.answers(r.route_batch(queries, gate, top_k, num_passages=P, retrieval_pool_size=pool, complete_scores=complete, allowed_ids=tenants[1])) == one
    q = queries[0]
    res, w = r.route(q, gate, 10, num_passages=20, complete_scores=complete, return_weights=True)
    want, want_w = _loop(r, gate, [q], 10, 20, 50, complete, [None])
    assert rs.answers([res]) == want and rgo.same((w,), (want_w[0],)) and rs.answers([r.route(q, gate, 10, num_passages=20, complete_scores=complete)]) == want
    assert r.route_batch([], gate) == [] and r.route_batch(queries[:2], gate, 30, num_passages=4) == r.route_batch(queries[:2], gate, 4, num_passages=4)
    hy = [x.hybrid_score for x in res]
    assert hy == sorted(hy, reverse=True) and len(res) == 10


def test_route_batch_without_a_dense_index_takes_the_per_question_columns(tmp_path, monkeypatch):
    """One side is not this module's own index class (here: no dense index at all): the columns come from the per-question path, the
    answer is still the loop's, filters included."""
    monkeypatch.setattr(si, "_gpu_backend_available", lambda: False)
    docs, questions, each = rs.corpus()
    r = rs.retriever(tmp_path)
    assert r.dense_index is None
    r.add_documents(docs[:300])
    gate = rs.gate()
    for entries in ([None] * 12, each[:12]):
        want, want_w = _loop(r, gate, questions[:12], 5, 8, 50, False, entries)
        got, got_w = r.route_batch(questions[:12], gate, 5, num_passages=8, allowed_ids_each=entries, return_weights=True)
        assert rs.answers(got) == want and sum(len(x) for x in want) > 20 and rgo.same((got_w,), (want_w,))


def test_the_gpu_scenario_is_separated_on_the_host(tmp_path):
    """The corpus tests/test_gpu_router.py routes on both backends, here over the host stand-in for the dense index: adjacent distinct
    hybrid scores of every question differ by more than 1e-9 relative, so the tolerance of the device's exp cannot reorder them."""
    docs, questions, each = rs.corpus()
    from rag_uq_amd.embedders import HashEmbedder
    emb = HashEmbedder()
    stub = th._StubNative(emb.embed([d.text for d in docs]), normalize=True)
    r = rs.retriever(tmp_path, dense_index=si.DenseIndex.from_native(stub, [d.id for d in docs], embedder=emb, metric="cosine"))
    r.bm25_index.add_documents(docs)
    for d in docs:
        r.documents[d.id] = d
    for normalize in ("query", "stats"):
        for P in (20, 100):
            for kw in ({"allowed_ids_each": each}, {"complete_scores": True}):
                out = r.route_batch(questions, rs.gate(normalize), P, num_passages=P, retrieval_pool_size=max(P, 50), **kw)
                assert rs.separated(out) and sum(len(x) for x in out) > 60 * P // 2, (normalize, P, list(kw))


# ---- keywords, no device ---------------------------------------------------------------------------------------------------------------------------
def test_router_backend_keyword_and_loud_failure_without_a_device(tmp_path):
    with pytest.raises(ValueError, match="router_backend"):
        si.HybridRetriever(bm25_persist_path=None, dense_index=object(), router_backend="cuda")
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    gate = rs.gate()
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        gate.native(0)
    w = rgo.make_weights(4, 0)
    with pytest.raises(_native.RqError, match="no HIP device|no CPU fallback"):
        _native.RouterGate(w["w0"], w["b0"], w["w1"], w["b1"])
    with pytest.raises(_native.RqError, match="num_layers"):                                                      # refused before the device is looked for
        _native.RouterGate(w["w0"], w["b0"], w["w1"], w["b1"], num_layers=3)
    with pytest.raises(_native.RqError, match="use_batch_norm"):
        _native.RouterGate(w["w0"], w["b0"], w["w1"], w["b1"], use_batch_norm=True)
    lib = _native.load_library()
    wide = np.zeros(900, np.float32)
    assert not lib.rq_router_create(0, 2, 300, 0, wide.ctypes.data, wide.ctypes.data, wide.ctypes.data, 0.0) and "hidden" in _native.last_error()
    assert not lib.rq_router_create(0, 2, 4, 0, None, None, None, 0.0) and "null" in _native.last_error()
    assert lib.rq_router_gate(None, None, None, 1, 1, 1, None, None) == -1 and lib.rq_router_gate_device(None, None, None, 1, 1, 1, None, None, None) == -1
    assert lib.rq_router_rerank(None, None, None, None, None, 1, 1, 1, None, 1, None, None, None, None, None, None, None) == -1
    assert lib.rq_router_get_option(None, b"calls") == -1.0
    lib.rq_router_destroy(None)
    r, queries = th._scenario(tmp_path, "cosine", router_backend="gpu", sparse_backend="gpu")
    with pytest.raises(_native.RqError, match="router_backend='gpu'.*no HIP device"):
        r.route_batch(queries, gate, 5)
    host, _ = th._scenario(tmp_path / "h", "cosine")
    auto, _ = th._scenario(tmp_path / "a", "cosine", router_backend="auto", sparse_backend="auto")
    assert rs.answers(auto.route_batch(queries, gate, 5)) == rs.answers(host.route_batch(queries, gate, 5))
