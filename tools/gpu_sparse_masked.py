"""Masked sparse search and filtered hybrid batches on the device (include/rq.h rq_sparse_topk_masked*) at 1M passages x 40
words over a 50 000-word Zipf vocabulary, 500 questions, top-100 (the generator of tools/gpu_sparse.py and tools/gpu_hybrid.py).  One
part per run (`--part`), so that the parts that need nothing of the masked calls also run, unchanged, from a checkout of the commit
before them -- the yardstick of (i) and (iii):
  unmasked   rq_sparse_topk_device alone, query CSR and outputs resident: HIP events around `--launches` back-to-back calls after 5
             warm-up calls, `--reps` repetitions (their spread is the run-to-run spread of the call), and the tile / final kernel split.
             Runs on either checkout.
  masked     (i) the same call, then rq_sparse_topk_masked_device with ONE all-allowing mask for every query, alternating, timed the same
             way: the cost of the mask itself; identical results asserted first.
             (ii) 64 tenant masks of 1/64 of the corpus each, question q under mask q % 64: contiguous tenants (rows [t n/64, (t+1) n/64))
             and scattered tenants (row r belongs to tenant r % 64), with "masked_tiles_last" / "skipped_tiles_last" / "tiles_last" and the
             tile / final kernel split; results asserted against rq_bm25_topk_masked first.
  router     (iii) HybridRetriever.get_scores_for_router_batch(..., allowed_ids_each = the 64 contiguous tenants) with
             fusion_backend="gpu", ids per call and reusable make_filter results, complete_scores off and on: a host clock around `--reps`
             calls after 2 warm-up calls; identical to the host fusion asserted first.
  loop       the loop it replaces, [get_scores_for_router(q, allowed_ids=tenant_q) for q in questions], timed once over `--loop-questions`
             questions (it scores a float64 vector over every passage per question).  Runs on either checkout.

    python tools/gpu_sparse_masked.py --part masked --out profiles/gpu_sparse_masked.txt [--passages 1000000] [--reps 5] [--launches 20]
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
ap.add_argument("--part", required=True, choices=["unmasked", "masked", "router", "loop"])
ap.add_argument("--out", default="")
ap.add_argument("--passages", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--loop-questions", type=int, default=64)
args = ap.parse_args()
K, DIM, NQ, TENANTS = 100, 768, 500, 64


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
           "tiles": int(sp.get_option("tiles_last")), "skipped_tiles": int(sp.get_option("skipped_tiles_last"))}
    if sp.get_option("masked_tiles_last") >= 0:
        out["masked_tiles"] = int(sp.get_option("masked_tiles_last"))
    sp.set_option("profile", 0)
    return out


def build_bm25(passages):
    bm = si.BM25Index()
    for lo in range(0, len(passages), 50_000):
        bm.add_documents([si.Document(id=f"p{lo + i}", text=t) for i, t in enumerate(passages[lo: lo + 50_000])])
    return bm


def sparse_parts(row, passages, questions):
    n, B = len(passages), len(questions)
    bm = build_bm25(passages)
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
    if args.part == "unmasked":
        row["unmasked_us"] = event_us({"unmasked": plain}, launches, args.reps)["unmasked"]
        row["unmasked_split"] = split(sp, plain)
        return
    host = nat.bm25_topk(c["handle"], q_ptr, q_tok, B, K, 0)

    def masked_launch(masks, mask_of):
        d_masks, d_mask_of = torch.from_numpy(masks.view(np.int32)).cuda(), torch.from_numpy(mask_of).cuda()
        return lambda: sp.topk_device(d_ptr, d_tok, B, len(q_tok), K, d_rows, d_scores, stream=s, d_masks=d_masks, n_masks=len(masks), d_mask_of=d_mask_of)

    def fetched():
        torch.cuda.synchronize()
        return d_rows.cpu().numpy(), d_scores.cpu().numpy()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    # (i) one all-allowing mask against the unmasked call
    ones = nat.pack_row_masks([np.ones(n, bool)], n)
    all_allowed = masked_launch(ones, np.zeros(B, np.int32))
    all_allowed()
    assert same(fetched(), host), "the all-allowing mask changes the answer"
    us = event_us({"unmasked": plain, "all_allowing_mask": all_allowed}, launches, args.reps)
    row["unmasked_us"], row["all_allowing_mask_us"] = us["unmasked"], us["all_allowing_mask"]
    row["unmasked_split"], row["all_allowing_mask_split"] = split(sp, plain), split(sp, all_allowed)
    # (ii) 64 tenants of 1/64 of the corpus each
    mask_of = (np.arange(B) % TENANTS).astype(np.int32)
    for name, tenant_of_row in (("contiguous", np.arange(n) * TENANTS // n), ("scattered", np.arange(n) % TENANTS)):
        masks = nat.pack_row_masks([tenant_of_row == t for t in range(TENANTS)], n)
        launch = masked_launch(masks, mask_of)
        launch()
        want = nat.bm25_topk(c["handle"], q_ptr, q_tok, B, K, 0, masks=masks, mask_of=mask_of)
        assert same(fetched(), want), f"{name} tenants: the device route differs from the host library"
        row[f"tenants_{name}_us"] = event_us({name: launch}, launches, args.reps)[name]
        row[f"tenants_{name}_split"] = split(sp, launch)
        row[f"tenants_{name}_results_per_question"] = round(float((want[0] >= 0).sum(axis=1).mean()), 1)
        t = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            nat.bm25_topk(c["handle"], q_ptr, q_tok, B, K, 0, masks=masks, mask_of=mask_of)
            if rep:
                t.append((time.perf_counter() - t0) * 1e3)
        row[f"tenants_{name}_rq_bm25_topk_masked_ms"] = spread(t)


def hybrid_parts(row, passages, questions, ans):
    n = len(passages)
    rng = np.random.default_rng(8)
    table = {}
    fusions = ("host", "gpu") if args.part == "router" else ("host",)
    retrievers, dense = {}, None
    for fusion in fusions:
        kw = {"embedder": TableEmbedder(table), "sparse_backend": "gpu", "fusion_backend": fusion}
        r = si.HybridRetriever(bm25_persist_path=None, chroma_persist_path="", **kw) if dense is None else \
            si.HybridRetriever(bm25_persist_path=None, chroma_persist_path=None, dense_index=dense, **kw)
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
            r.bm25_index, r.documents = retrievers["host"].bm25_index, retrievers["host"].documents
    tenants = [[f"p{i}" for i in range(t * n // TENANTS, (t + 1) * n // TENANTS)] for t in range(TENANTS)]
    each = [tenants[q % TENANTS] for q in range(NQ)]
    if args.part == "loop":
        r, m = retrievers["host"], min(args.loop_questions, NQ)
        for complete in (False, True):
            r.get_scores_for_router(questions[0], K, retrieval_pool_size=K, allowed_ids=each[0], complete_scores=complete)      # warm-up
            t0 = time.perf_counter()
            for q in range(m):
                r.get_scores_for_router(questions[q], K, retrieval_pool_size=K, allowed_ids=each[q], complete_scores=complete)
            ms = (time.perf_counter() - t0) * 1e3
            row["loop_ms_per_question_complete" if complete else "loop_ms_per_question"] = round(ms / m, 2)
        row["loop_questions"] = m
        return
    host, gpu = retrievers["host"], retrievers["gpu"]
    t0 = time.perf_counter()
    filters = [gpu.make_filter(ids) for ids in tenants]
    row["make_64_filters_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    each_f = [filters[q % TENANTS] for q in range(NQ)]
    for complete in (False, True):                                          # identical before anything is timed
        a = host.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, complete_scores=complete, allowed_ids_each=each_f)
        assert a == gpu.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, complete_scores=complete, allowed_ids_each=each_f), "the device route differs from the host fusion"
        assert a == gpu.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, complete_scores=complete, allowed_ids_each=each), "ids and filters differ"
    row["identical"] = True
    row["results_per_question"] = round(float(np.mean([sum(1 for d in x[2] if d) for x in a])), 1)
    for complete in (False, True):
        ms = {"fusion_host_filters": [], "fusion_gpu_filters": [], "fusion_gpu_ids": []}
        for rep in range(args.reps + 2):
            for name, r, e in (("fusion_host_filters", host, each_f), ("fusion_gpu_filters", gpu, each_f), ("fusion_gpu_ids", gpu, each)):
                if name == "fusion_gpu_ids" and rep > 2:
                    continue                                                # (64 filters made and closed per call: one timed call is enough)
                t0 = time.perf_counter()
                r.get_scores_for_router_batch(questions, K, retrieval_pool_size=K, complete_scores=complete, allowed_ids_each=e)
                if rep >= 2:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        row["router_batch_ms_complete" if complete else "router_batch_ms"] = {k: spread(v) for k, v in ms.items()}
    sp, dn = gpu.bm25_index._csr()["sparse"], gpu.dense_index._index
    row["masked_tiles_last"], row["tiles_last"] = int(sp.get_option("masked_tiles_last")), int(sp.get_option("tiles_last"))
    row["filter_each_routes_last"] = int(dn.get_option("filter_each_routes_last"))


def main():
    row = {"part": args.part, "passages": args.passages, "questions": NQ, "k": K, "tenants": TENANTS}
    t0 = time.perf_counter()
    passages, questions, ans = corpus(args.passages)
    if args.part in ("unmasked", "masked"):
        sparse_parts(row, passages, questions)
    else:
        hybrid_parts(row, passages, questions, ans)
    row["total_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(f"# tools/gpu_sparse_masked.py --part {args.part} --passages {args.passages} --reps {args.reps} --launches {args.launches}: "
                    f"{torch.cuda.get_device_name(0)}; *_us: HIP events over {max(5, args.launches)} calls, {args.reps} repetitions; *_ms: host clock\n")
            f.write(json.dumps(row) + "\n")


main()
