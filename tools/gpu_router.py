"""The router gate on the device (include/rq.h rq_router_*) beside what a user does today, in one process on the same
indexes: 500 questions, pools of 100, num_passages 100, top_k 10, over `--passages` passages (default 1M; corpus, vectors and questions
are those of tools/gpu_hybrid.py) and a seeded router of 64 hidden units, per-query normalisation.
After asserting that both routes return identical ids, b and d in identical order, with w within 2^-49 relative:
  call_ms      host clock around `--reps` calls after 2 warm-up calls, the two routes alternating; best, median, worst:
                 baseline  sparse_backend="gpu", fusion_backend="gpu": get_scores_for_router_batch + router.RouterGate.rerank (numpy) + the
                           first top_k real passages of every question as (id, text) pairs;
                 route     route_batch with router_backend="gpu": the fused pool stays in HBM, [B][top_k] come up;
               and route_batch with router_backend="host" on the same retriever, for the "auto" rule;
  rerank_us    rq_router_rerank_device alone, columns resident: HIP events around `--launches` back-to-back calls after 5 warm-up
               calls, three repetitions; at P = 100 (B = 500, the fused block of the call above) and at P = 1 024 (B = 500, seeded columns);
  gate_us      rq_router_gate_device alone, the same way.

    python tools/gpu_router.py --out profiles/gpu_router.txt [--passages 1000000] [--reps 9] [--launches 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rag_uq_amd import router as rt  # noqa: E402
from rag_uq_amd import streaming_index as si  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--passages", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()
K, DIM, NQ, TOP = 100, 768, 500, 10


def corpus(n):
    rng = np.random.default_rng(7)
    V = 50_000
    p = 1.0 / np.arange(1, V + 1) ** 0.9
    p /= p.sum()
    words = rng.choice(V, size=(n, 40), p=p)
    vocab = np.array([f"w{i}" for i in range(V)], dtype=object)
    passages = [" ".join(vocab[row].tolist()) for row in words]
    ans = rng.choice(n, size=NQ, replace=False)
    questions = [" ".join(vocab[np.concatenate([rng.choice(words[a], 8, replace=False), rng.choice(V, 4, p=p)])].tolist()) for a in ans]
    return passages, questions, ans


class TableEmbedder:
    """Questions embed to a fixed vector each (a noisy copy of their answer passage's): the embedder is not what is measured."""
    dim = DIM

    def __init__(self, table):
        self.table = table

    def embed(self, texts):
        return np.stack([self.table[t] for t in texts]).astype(np.float32)


def seeded_gate(hidden=64):
    rng = np.random.default_rng(2024)
    lim = 1.0 / np.sqrt(hidden)
    return rt.RouterGate(rng.uniform(-0.58, 0.58, (hidden, 3)), rng.uniform(-0.58, 0.58, hidden), rng.uniform(-lim, lim, hidden), rng.uniform(-lim, lim))


def spread(ms):
    return {"best": round(min(ms), 3), "median": round(float(np.median(ms)), 3), "worst": round(max(ms), 3)}


def event_us(launch, launches):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    reps = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        torch.cuda.synchronize()
        reps.append(round(e0.elapsed_time(e1) * 1e3 / launches, 1))
    return reps


def baseline(r, gate, questions):
    """What a user does today: the batch call, the host gate, the reorder, the first TOP real passages."""
    cols = r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K)
    b, d = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
    keys = np.array([[i if doc else -1 for i, doc in enumerate(c[2])] for c in cols], np.int32)
    _, ob, od, ow, oh, pos, cnt = gate.rerank(keys, b, d, np.full(len(cols), K), TOP)
    out = [[(cols[q][2][p], cols[q][3][p]) for p in pos[q, :cnt[q]]] for q in range(len(cols))]
    return out, ob, od, ow, oh


def main():
    n = args.passages
    row = {"passages": n, "questions": NQ, "pool": K, "num_passages": K, "top_k": TOP, "dim": DIM, "hidden": 64}
    passages, questions, ans = corpus(n)
    rng = np.random.default_rng(8)
    table = {}
    t0 = time.perf_counter()
    r = si.HybridRetriever(bm25_persist_path=None, chroma_persist_path="", embedder=TableEmbedder(table), sparse_backend="gpu", fusion_backend="gpu")
    dense = r.dense_index
    dense.auto_persist = False
    for lo in range(0, n, 50_000):
        hi = min(n, lo + 50_000)
        vec = rng.standard_normal((hi - lo, DIM)).astype(np.float32)
        for j in np.flatnonzero((ans >= lo) & (ans < hi)):
            table[questions[j]] = vec[ans[j] - lo] + 0.5 * rng.standard_normal(DIM).astype(np.float32)
        dense.add_vectors([f"p{i}" for i in range(lo, hi)], vec)
        docs = [si.Document(id=f"p{lo + i}", text=t) for i, t in enumerate(passages[lo:hi])]
        r.bm25_index.add_documents(docs)
        for d in docs:
            r.documents[d.id] = d
    row["index_build_s"] = round(time.perf_counter() - t0, 1)
    print(f"# indexes built in {row['index_build_s']} s", file=sys.stderr, flush=True)
    gate = seeded_gate()

    def route(backend):
        r.router_backend = backend
        return r.route_batch(questions, gate, TOP, num_passages=K, retrieval_pool_size=K, return_weights=True)

    # identical before anything is timed
    want, wb, wd, ww, wh = baseline(r, gate, questions)
    for backend in ("host", "gpu"):
        got, gw = route(backend)
        assert [[(x.doc_id, x.text) for x in res] for res in got] == want, f"router_backend={backend}: other passages or another order than the baseline"
        gb, gd, gh = (np.array([[getattr(x, f) for x in res] + [0.0] * (TOP - len(res)) for res in got]) for f in ("bm25_score", "dense_score", "hybrid_score"))
        assert np.array_equal(gb, wb) and np.array_equal(gd, wd), f"router_backend={backend}: other scores than the baseline"
        assert (np.abs(gw - ww) <= 2.0 ** -49 * ww).all(), f"router_backend={backend}: gate weights beyond 2^-49 relative"
        row[f"worst_dw_rel_{backend}"] = float((np.abs(gw - ww) / np.where(ww > 0, ww, 1.0)).max())
    row["identical"] = True
    row["results_per_question"] = round(float(np.mean([len(x) for x in want])), 1)
    ms = {"baseline": [], "route_gpu": [], "route_host": []}
    for rep in range(args.reps + 2):
        for name, call in (("baseline", lambda: baseline(r, gate, questions)), ("route_gpu", lambda: route("gpu")), ("route_host", lambda: route("host"))):
            t0 = time.perf_counter()
            call()
            if rep >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    row["call_ms"] = {k: spread(v) for k, v in ms.items()}
    # the kernels alone, columns resident
    ng = gate.native(0)
    s = torch.cuda.current_stream().cuda_stream
    launches = max(5, args.launches)
    cols = r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K)
    shapes = {"p100": (np.array([c[0] for c in cols]), np.array([c[1] for c in cols]))}
    g = np.random.default_rng(9)
    shapes["p1024"] = (g.gamma(2.0, 3.0, (NQ, 1024)), g.uniform(-0.2, 0.9, (NQ, 1024)))
    for name, (b, d) in shapes.items():
        B, P = b.shape
        d_b, d_d = torch.from_numpy(b).cuda(), torch.from_numpy(d).cuda()
        d_keys = torch.arange(P, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous()
        d_cnt = torch.full((B,), P, dtype=torch.int32, device="cuda")
        ok, op, oc = torch.empty((B, TOP), dtype=torch.int32, device="cuda"), torch.empty((B, TOP), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
        ob, od, ow, oh = (torch.empty((B, TOP), dtype=torch.float64, device="cuda") for _ in range(4))
        d_w = torch.empty((B, P), dtype=torch.float64, device="cuda")
        row[f"rerank_us_{name}"] = event_us(lambda: ng.rerank_device(d_keys, d_b, d_d, d_cnt, B, P, TOP, ok, ob, od, ow, oh, op, oc, gate.mode, None, s), launches)
        row[f"gate_us_{name}"] = event_us(lambda: ng.gate_device(d_b, d_d, B, P, d_w, gate.mode, None, s), launches)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# tools/gpu_router.py --passages {n} --reps {args.reps} --launches {args.launches}: {torch.cuda.get_device_name(0)}; call_ms: host clock, best / "
                    f"median / worst of {args.reps} calls, the routes alternating; *_us: HIP events over {launches} calls, three repetitions\n")
            f.write(json.dumps(row) + "\n")


main()
