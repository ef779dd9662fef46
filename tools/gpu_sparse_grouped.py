"""Grouped sparse search and grouped hybrid batches on the device (include/rq.h rq_sparse_topk_grouped*, rq_hybrid_fuse_grouped*; DESIGN
4.23) at 1M passages x 40 words over a 50 000-word Zipf vocabulary, 500 questions, top-100 (the generator of tools/gpu_sparse_masked.py),
titles of 4 consecutive chunks each.  One part per run (`--part`); `ungrouped` needs nothing of the grouped calls, so it also runs,
unchanged, from a checkout of the commit before them -- the yardstick of (2):
  ungrouped  (2) rq_sparse_topk_device alone and rq_hybrid_fuse_device alone (pools of 100 + 100, resident): HIP events around
             `--launches` back-to-back calls after 5 warm-up calls, `--reps` repetitions: their spread is the run-to-run spread.
  sparse     (1) rq_sparse_topk_device and rq_sparse_topk_grouped_device alternating, timed the same way, with the tile / final kernel
             split, "final_chunks_last" and the results per question; the grouped result asserted against the host definition
             (BM25Index.search_batch_rows(distinct_by=) on a sample of questions) first.
  router     (3) get_scores_for_router_batch(distinct_by="title") and route_batch(distinct_by="title") with every backend "gpu": a host
             clock around `--reps` calls after 2 warm-up calls; identical to the per-query loop on a sample asserted first.
  loop       the loop they replace, [hybrid_search(q, distinct_by="title") for q in questions], timed once over `--loop-questions`.

    python tools/gpu_sparse_grouped.py --part sparse --out profiles/gpu_sparse_grouped.txt [--passages 1000000] [--reps 5] [--launches 20]
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
from rag_uq_amd import _native as nat  # noqa: E402
from rag_uq_amd import streaming_index as si  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", required=True, choices=["ungrouped", "sparse", "router", "loop"])
ap.add_argument("--out", default="")
ap.add_argument("--passages", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--loop-questions", type=int, default=32)
args = ap.parse_args()
K, DIM, NQ, CHUNKS = 100, 768, 500, 4


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


def documents(passages, lo, hi):
    return [si.Document(id=f"p{i}", text=passages[i], title=f"T{i // CHUNKS}") for i in range(lo, hi)]


class TableEmbedder:
    """Questions embed to a fixed vector each (a noisy copy of their answer passage's): the embedder is not what is measured."""
    dim = DIM

    def __init__(self, table):
        self.table = table

    def embed(self, texts):
        return np.stack([self.table[t] for t in texts]).astype(np.float32)


def spread(ms):
    return {"best": round(min(ms), 3), "median": round(float(np.median(ms)), 3), "worst": round(max(ms), 3)}


def event_us(launches_of, launches, reps):
    """launches_of: name -> launch; the routes alternate repetition by repetition.  name -> [us per call] x reps."""
    for launch in launches_of.values():
        for _ in range(5):
            launch()
    torch.cuda.synchronize()
    out = {name: [] for name in launches_of}
    for _ in range(reps):
        for name, launch in launches_of.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(round(e0.elapsed_time(e1) * 1e3 / launches, 1))
    return out


def split(sp, launch):
    sp.set_option("profile", 1)
    launch()
    out = {"tile_kernel_us": round(sp.get_option("tile_ms_last") * 1e3, 1), "final_kernel_us": round(sp.get_option("final_ms_last") * 1e3, 1),
           "tiles": int(sp.get_option("tiles_last"))}
    sp.set_option("profile", 0)
    return out


def sparse_parts(row, passages, questions):
    n, B = len(passages), len(questions)
    bm = si.BM25Index()
    for lo in range(0, n, 50_000):
        bm.add_documents(documents(passages, lo, min(n, lo + 50_000)))
    c = bm._csr()
    sp = bm._sparse_index(c)
    q_ptr, q_tok = bm._query_csr(c, questions)
    q_ptr, q_tok = np.asarray(q_ptr, np.int64), np.asarray(q_tok, np.int32)
    row["postings"], row["query_tokens"], row["tile_docs"] = int(c["indptr"][-1]), int(len(q_tok)), int(sp.get_option("tile_docs"))
    d_ptr, d_tok = torch.from_numpy(q_ptr).cuda(), torch.from_numpy(q_tok).cuda()
    d_rows = torch.empty((B, K), dtype=torch.int32, device="cuda")
    d_scores = torch.empty((B, K), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plain = lambda: sp.topk_device(d_ptr, d_tok, B, len(q_tok), K, d_rows, d_scores, stream=s)                      # noqa: E731
    launches = max(5, args.launches)
    # the ungrouped fusion over resident pools of 100 + 100 (random rows and scores: its time does not depend on them)
    rng = np.random.default_rng(3)
    hm = nat.HybridMap(n, np.arange(n, dtype=np.int64), np.ones(n, bool))
    pools = [torch.from_numpy(x).cuda() for x in (np.stack([rng.choice(n, K, replace=False) for _ in range(B)]).astype(np.int32),
                                                   np.sort(rng.uniform(0.05, 30.0, (B, K)))[:, ::-1].copy(),
                                                   np.stack([rng.choice(n, K, replace=False) for _ in range(B)]).astype(np.int64),
                                                   np.sort(rng.uniform(-1, 1, (B, K)).astype(np.float32))[:, ::-1].copy())]
    o_keys, o_count = torch.empty((B, K), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    o_b, o_d, o_h = (torch.empty((B, K), dtype=torch.float64, device="cuda") for _ in range(3))
    fuse = lambda: hm.fuse_device(*pools, B, K, K, K, o_keys, o_b, o_d, o_h, None, o_count, s)                      # noqa: E731
    if args.part == "ungrouped":
        us = event_us({"sparse_topk": plain, "hybrid_fuse": fuse}, launches, args.reps)
        row["sparse_topk_us"], row["hybrid_fuse_us"] = us["sparse_topk"], us["hybrid_fuse"]
        row["sparse_topk_split"] = split(sp, plain)
        return
    sp = bm._sparse_index_grouped(c, "title")
    d_count = torch.empty((B,), dtype=torch.int32, device="cuda")
    grouped = lambda: sp.topk_grouped_device(d_ptr, d_tok, B, len(q_tok), K, d_rows, d_scores, d_count, stream=s)   # noqa: E731
    grouped()
    torch.cuda.synchronize()
    got = (d_rows.cpu().numpy(), d_scores.cpu().numpy(), d_count.cpu().numpy())
    m = 8                                                                   # (the host definition walks a full score vector per question)
    want = bm.search_batch_rows(questions[:m], K, distinct_by="title")
    assert np.array_equal(got[0][:m], want[0]) and np.array_equal(got[1][:m].view(np.uint64), want[1].view(np.uint64)), "the grouped call differs from the host definition"
    row["identical_on"], row["results_per_question"], row["final_chunks_last"] = m, round(float(got[2].mean()), 1), int(sp.get_option("final_chunks_last"))
    hm.set_groups((np.arange(n) // CHUNKS).astype(np.int32))
    fuse_grouped = lambda: hm.fuse_grouped_device(*pools, B, K, K, K, o_keys, o_b, o_d, o_h, None, o_count, s)      # noqa: E731
    us = event_us({"sparse_topk": plain, "sparse_topk_grouped": grouped, "hybrid_fuse": fuse, "hybrid_fuse_grouped": fuse_grouped}, launches, args.reps)
    for name, v in us.items():
        row[f"{name}_us"] = v
    row["sparse_topk_split"], row["sparse_topk_grouped_split"] = split(sp, plain), split(sp, grouped)


def hybrid_parts(row, passages, questions, ans):
    from rag_uq_amd import router as rt
    n = len(passages)
    rng = np.random.default_rng(8)
    table = {}
    r = si.HybridRetriever(bm25_persist_path=None, chroma_persist_path="", embedder=TableEmbedder(table), sparse_backend="gpu", fusion_backend="gpu", router_backend="gpu")
    dense = r.dense_index
    dense.auto_persist = False
    for lo in range(0, n, 50_000):
        hi = min(n, lo + 50_000)
        vec = rng.standard_normal((hi - lo, DIM)).astype(np.float32)
        for j in np.flatnonzero((ans >= lo) & (ans < hi)):
            table[questions[j]] = vec[ans[j] - lo] + 0.5 * rng.standard_normal(DIM).astype(np.float32)
        docs = documents(passages, lo, hi)
        dense.add_vectors([d.id for d in docs], vec, metadatas=[{"title": d.title} for d in docs])
        r.bm25_index.add_documents(docs)
        for d in docs:
            r.documents[d.id] = d
    m = min(args.loop_questions, NQ)
    if args.part == "loop":
        r.hybrid_search(questions[0], K, K, distinct_by="title")                                                   # warm-up
        t0 = time.perf_counter()
        for q in range(m):
            r.hybrid_search(questions[q], K, K, distinct_by="title")
        row["loop_ms_per_question"], row["loop_questions"] = round((time.perf_counter() - t0) * 1e3 / m, 2), m
        return
    w = np.random.default_rng(2024)
    gate = rt.RouterGate(w.standard_normal((64, 3)) * 0.5, w.standard_normal(64) * 0.1, w.standard_normal(64) * 0.3, 0.05)
    cols = r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, distinct_by="title")
    few = 4
    assert [tuple(c) for c in cols[:few]] == [tuple(r.get_scores_for_router(q, K, retrieval_pool_size=K, distinct_by="title")) for q in questions[:few]], \
        "the device route differs from the per-query calls"
    row["identical_on"], row["results_per_question"] = few, round(float(np.mean([sum(1 for d in x[2] if d) for x in cols])), 1)
    ms = {"get_scores_for_router_batch": [], "route_batch": [], "get_scores_for_router_batch_ungrouped": []}
    for rep in range(args.reps + 2):
        for name, call in (("get_scores_for_router_batch", lambda: r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, distinct_by="title")),
                           ("route_batch", lambda: r.route_batch(questions, gate, 10, num_passages=K, retrieval_pool_size=K, distinct_by="title")),
                           ("get_scores_for_router_batch_ungrouped", lambda: r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K))):
            t0 = time.perf_counter()
            call()
            if rep >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    row["batch_ms"] = {k: spread(v) for k, v in ms.items()}
    r.hybrid_search(questions[0], K, K, distinct_by="title")
    t0 = time.perf_counter()
    for q in range(m):
        r.hybrid_search(questions[q], K, K, distinct_by="title")
    row["loop_ms_per_question"], row["loop_questions"] = round((time.perf_counter() - t0) * 1e3 / m, 2), m


def main():
    row = {"part": args.part, "passages": args.passages, "questions": NQ, "k": K, "chunks_per_title": CHUNKS}
    t0 = time.perf_counter()
    passages, questions, ans = corpus(args.passages)
    if args.part in ("ungrouped", "sparse"):
        sparse_parts(row, passages, questions)
    else:
        hybrid_parts(row, passages, questions, ans)
    row["total_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(f"# tools/gpu_sparse_grouped.py --part {args.part} --passages {args.passages} --reps {args.reps} --launches {args.launches}: "
                    f"{torch.cuda.get_device_name(0)}; *_us: HIP events over {max(5, args.launches)} calls, {args.reps} repetitions; *_ms: host clock\n")
            f.write(json.dumps(row) + "\n")


main()
