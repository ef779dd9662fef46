"""Hybrid fusion on the device (include/rq.h rq_hybrid_*) beside the host fusion it restates, in one process on the same
indexes: 500 questions, pools of 100, top_k 100, over `--passages` passages (default 1M x 40 words over a 50 000-word Zipf vocabulary,
the generator of tools/gpu_sparse.py) with 768-dimensional random rows (a question's vector is a noisy copy of its answer passage's) --
the BASELINE.json configs[4] shape.
After asserting that both routes return identical results (complete_scores off and on):
  call_ms      HybridRetriever.get_scores_for_router_batch, fusion_backend="host" (sparse_backend="gpu": the fastest route without this
               stage) and fusion_backend="gpu", alternating, a host clock around `--reps` calls after 2 warm-up calls; best, median,
               worst; complete_scores off and on;
  fuse_us      rq_hybrid_fuse_device alone, pools and outputs resident: HIP events around `--launches` back-to-back calls after 5
               warm-up calls, three repetitions; without and with the four extra arrays;
  missing_us   rq_hybrid_missing_device alone, the same way;
  score_rows_us  rq_sparse_score_rows_device alone over the dense pool's miss list ([500][100]), the same way.

    python tools/gpu_hybrid.py --out profiles/gpu_hybrid.txt [--passages 1000000] [--reps 9] [--launches 20]
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
from rag_uq_amd import streaming_index as si  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--passages", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()
K, DIM, NQ = 100, 768, 500


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


def main():
    n = args.passages
    row = {"passages": n, "questions": NQ, "pool": K, "top_k": K, "dim": DIM}
    passages, questions, ans = corpus(n)
    rng = np.random.default_rng(8)
    table = {}
    retrievers = {}
    dense = None
    t0 = time.perf_counter()
    for fusion in ("host", "gpu"):
        r = si.HybridRetriever(bm25_persist_path=None, chroma_persist_path=None, dense_index=dense, embedder=TableEmbedder(table), sparse_backend="gpu", fusion_backend=fusion) \
            if dense is not None else si.HybridRetriever(bm25_persist_path=None, chroma_persist_path="", embedder=TableEmbedder(table), sparse_backend="gpu", fusion_backend=fusion)
        retrievers[fusion] = r
        if dense is None:                                                   # one dense index and one BM25 index serve both retrievers
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
        else:
            r.bm25_index = retrievers["host"].bm25_index
            r.documents = retrievers["host"].documents
    row["index_build_s"] = round(time.perf_counter() - t0, 1)
    print(f"# indexes built in {row['index_build_s']} s", file=sys.stderr, flush=True)
    host, gpu = retrievers["host"], retrievers["gpu"]
    for complete in (False, True):                                          # identical before anything is timed
        a, b = host._fuse_batch_rows(questions, K, K, complete), gpu._fuse_batch_rows(questions, K, K, complete)
        live = np.arange(K)[None, :] < a[4][:, None]
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[0][live], b[0][live]), "the device fusion differs from the host fusion"
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[1:4], b[1:4])), "the device fusion's scores differ in their bits"
    row["identical"] = True
    row["results_per_question"] = round(float(a[4].mean()), 1)
    for complete in (False, True):
        ms = {"host": [], "gpu": []}
        for rep in range(args.reps + 2):
            for fusion in ("host", "gpu"):
                t0 = time.perf_counter()
                retrievers[fusion].get_scores_for_router_batch(questions, K, retrieval_pool_size=K, complete_scores=complete)
                if rep >= 2:
                    ms[fusion].append((time.perf_counter() - t0) * 1e3)
        row["call_ms_complete" if complete else "call_ms"] = {"fusion_host": spread(ms["host"]), "fusion_gpu": spread(ms["gpu"])}
    # the parts the two routes share, on the host clock, once: tokenising and the texts of the answer
    bm, dn = host.bm25_index, host.dense_index
    c = bm._csr()
    t0 = time.perf_counter()
    q_ptr, q_tok = bm._query_csr(c, questions)
    row["tokenise_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    # the kernels alone, pools resident
    sp = bm._sparse_index(c)
    ks = gpu._key_space()
    hm = ks["map"]
    sp_rows, sp_scores = bm.search_batch_rows(questions, K, backend="gpu")
    de_scores, de_rows = dn.search_rows_batch(questions, K)
    dev = "cuda"
    d_sr, d_ss = torch.from_numpy(sp_rows).to(dev), torch.from_numpy(sp_scores).to(dev)
    d_dr, d_ds = torch.from_numpy(np.ascontiguousarray(de_rows)).to(dev), torch.from_numpy(np.ascontiguousarray(de_scores)).to(dev)
    d_ptr, d_tok = torch.tensor(q_ptr, dtype=torch.int64).to(dev), torch.tensor(q_tok, dtype=torch.int32).to(dev)
    B = NQ
    d_md, d_ms = torch.empty((B, K), dtype=torch.int64, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
    d_ed, d_es = torch.zeros((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.float64, device=dev)
    keys, cnt = torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    ob, od, oh = (torch.empty((B, K), dtype=torch.float64, device=dev) for _ in range(3))
    s = torch.cuda.current_stream().cuda_stream
    row["missing_us"] = event_us(lambda: hm.missing_device(d_sr, d_dr, B, K, K, d_md, d_ms, s), max(5, args.launches))
    row["missing_rows"] = {"dense": int((d_md >= 0).sum()), "sparse": int((d_ms >= 0).sum())}
    row["score_rows_us"] = event_us(lambda: sp.score_rows_device(d_ptr, d_tok, B, len(q_tok), d_ms, K, d_es, s), max(5, args.launches))
    row["fuse_us"] = event_us(lambda: hm.fuse_device(d_sr, d_ss, d_dr, d_ds, B, K, K, K, keys, ob, od, oh, None, cnt, s), max(5, args.launches))
    row["fuse_extras_us"] = event_us(lambda: hm.fuse_device(d_sr, d_ss, d_dr, d_ds, B, K, K, K, keys, ob, od, oh, None, cnt, s, d_miss_dense=d_md, d_extra_dense=d_ed,
                                                             d_miss_sparse=d_ms, d_extra_sparse=d_es), max(5, args.launches))
    # the host fusion's own share: the whole host-route call minus the two searches it starts with
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        bm.search_batch_rows(questions, K, backend="gpu")
        dn.search_rows_batch(questions, K)
        t.append((time.perf_counter() - t0) * 1e3)
    row["host_route_two_searches_ms"] = spread(t)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# tools/gpu_hybrid.py --passages {n} --reps {args.reps} --launches {args.launches}: {torch.cuda.get_device_name(0)}; call_ms: host clock, best / "
                    f"median / worst of {args.reps} calls, the two routes alternating; *_us: HIP events over {max(5, args.launches)} calls, three repetitions\n")
            f.write(json.dumps(row) + "\n")


main()
