"""Sparse search on the device (include/rq.h rq_sparse_topk) beside the host library it restates, in one process on the
same arrays, at the two recorded shapes:
  1m    1M passages x 40 words over a 50 000-word Zipf vocabulary, 500 questions, top-100 (the generator of tools/bm25_scale.py,
        profiles/r03_bm25_scale.txt);
  50k   BASELINE.json configs[4]: 50 000 passages, 500 questions, pools of 100 (tests/config_workloads.py's synthetic QA set).
Per shape, after asserting that both routes return the same rows and the same score bits:
  host_ms      BM25Index.search_batch_rows(backend="host"), n_threads auto (librq_bm25.so, at most 16 host threads): a host clock
               around `--reps` calls after 2 warm-up calls; best, median, worst;
  gpu_ms       the same call with backend="gpu" (tokenising, the staged host form rq_sparse_topk, results back on the host), timed the
               same way, alternating with the host route;
  tokenise_ms  the part of both that is neither: building the query CSR on the host (once);
  device_us    rq_sparse_topk_device alone, query CSR and outputs resident: HIP events around `--launches` back-to-back calls after 5
               warm-up calls, three repetitions, for tile_docs 2048 / 4096 / 8192;
  split        the time of the tile kernel and of the final kernel in one call (option "profile": events around each launch);
  create_ms    rq_sparse_create: validation + upload of the CSR arrays, once per corpus state.

    python tools/gpu_sparse.py --out profiles/gpu_sparse.txt [--shape both|1m|50k] [--reps 9] [--launches 20]
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
ap.add_argument("--out", default="")
ap.add_argument("--shape", default="both", choices=["both", "1m", "50k"])
ap.add_argument("--passages", type=int, default=0, help="override the number of passages (a rehearsal)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()
K = 100


def corpus_1m(n):
    rng = np.random.default_rng(7)
    V = 50_000
    p = 1.0 / np.arange(1, V + 1) ** 0.9
    p /= p.sum()
    words = rng.choice(V, size=(n, 40), p=p)
    vocab = np.array([f"w{i}" for i in range(V)], dtype=object)
    passages = [" ".join(vocab[row].tolist()) for row in words]
    ans = rng.choice(n, size=500, replace=False)
    questions = [" ".join(vocab[np.concatenate([rng.choice(words[a], 8, replace=False), rng.choice(V, 4, p=p)])].tolist()) for a in ans]
    return passages, questions


def corpus_50k(n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from config_workloads import synthetic_qa
    passages, questions, _ = synthetic_qa(n, 500)
    return passages, questions


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


def run(name, passages, questions):
    row = {"shape": name, "passages": len(passages), "questions": len(questions), "k": K}
    bm = si.BM25Index()
    t0 = time.perf_counter()
    for lo in range(0, len(passages), 50_000):
        bm.add_documents([si.Document(id=f"p{lo + i}", text=t) for i, t in enumerate(passages[lo: lo + 50_000])])
    c = bm._csr()
    row["index_build_s"] = round(time.perf_counter() - t0, 1)
    row["postings"], row["tokens"] = int(c["indptr"][-1]), len(c["tid"])
    row["device_bytes"] = row["postings"] * 12 + (row["tokens"] + 1) * 8
    t0 = time.perf_counter()
    sp = bm._sparse_index(c)
    row["create_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    # identical before anything is timed
    host = bm.search_batch_rows(questions, K, backend="host")
    gpu = bm.search_batch_rows(questions, K, backend="gpu")
    assert np.array_equal(host[0], gpu[0]) and np.array_equal(host[1].view(np.uint64), gpu[1].view(np.uint64)), "the device route differs from the host library"
    row["identical"] = True
    row["results_per_question"] = round(float((host[0] >= 0).sum(axis=1).mean()), 1)
    t0 = time.perf_counter()
    tid = c["tid"]
    q_tok, q_ptr = [], [0]
    for q in questions:
        q_tok += [tid[t] for t in bm._tokenize(q) if t in tid]
        q_ptr.append(len(q_tok))
    row["tokenise_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    q_ptr, q_tok = np.asarray(q_ptr, np.int64), np.asarray(q_tok, np.int32)
    row["query_tokens"] = int(len(q_tok))
    row["postings_walked"] = int(np.diff(c["indptr"])[q_tok].sum())
    ms = {"host": [], "gpu": []}
    for rep in range(args.reps + 2):
        for backend in ("host", "gpu"):
            t0 = time.perf_counter()
            bm.search_batch_rows(questions, K, backend=backend)
            if rep >= 2:
                ms[backend].append((time.perf_counter() - t0) * 1e3)
    row["host_ms"], row["gpu_ms"] = spread(ms["host"]), spread(ms["gpu"])
    # the library calls alone, without tokenising
    lib = {"host": [], "gpu": []}
    for rep in range(args.reps + 2):
        for backend in ("host", "gpu"):
            t0 = time.perf_counter()
            if backend == "host":
                nat.bm25_topk(c["handle"], q_ptr, q_tok, len(questions), K, 0)
            else:
                sp.topk(q_ptr, q_tok, len(questions), K)
            if rep >= 2:
                lib[backend].append((time.perf_counter() - t0) * 1e3)
    row["rq_bm25_topk_ms"], row["rq_sparse_topk_ms"] = spread(lib["host"]), spread(lib["gpu"])
    # the device form alone, per tile size
    B = len(questions)
    d_ptr, d_tok = torch.from_numpy(q_ptr).cuda(), torch.from_numpy(q_tok).cuda()
    d_rows = torch.empty((B, K), dtype=torch.int32, device="cuda")
    d_scores = torch.empty((B, K), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    launch = lambda: sp.topk_device(d_ptr, d_tok, B, len(q_tok), K, d_rows, d_scores, stream=stream)
    row["device_us"], row["split_us"] = {}, {}
    default_tile = row["tile_docs_default"] = int(sp.get_option("tile_docs"))
    for tile in (2048, 4096, 8192):
        sp.set_option("tile_docs", tile)
        row["device_us"][str(tile)] = event_us(launch, max(5, args.launches))
        assert np.array_equal(d_rows.cpu().numpy(), host[0]) and np.array_equal(d_scores.cpu().numpy().view(np.uint64), host[1].view(np.uint64)), tile
        sp.set_option("profile", 1)
        launch()
        row["split_us"][str(tile)] = {"tile_kernel": round(sp.get_option("tile_ms_last") * 1e3, 1), "final_kernel": round(sp.get_option("final_ms_last") * 1e3, 1),
                                      "tiles": int(sp.get_option("tiles_last")), "skipped_tiles": int(sp.get_option("skipped_tiles_last"))}
        sp.set_option("profile", 0)
    sp.set_option("tile_docs", default_tile)
    print(json.dumps(row), flush=True)
    bm._drop_csr()
    return row


rows = []
if args.shape in ("both", "50k"):
    rows.append(run("50k", *corpus_50k(args.passages or 50_000)))
if args.shape in ("both", "1m"):
    rows.append(run("1m", *corpus_1m(args.passages or 1_000_000)))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/gpu_sparse.py --reps {args.reps} --launches {args.launches}: {torch.cuda.get_device_name(0)}; host threads auto (at most 16); "
                f"*_ms: host clock, best / median / worst of {args.reps} calls; device_us: HIP events over {max(5, args.launches)} calls, three repetitions\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
