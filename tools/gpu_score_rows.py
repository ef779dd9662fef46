"""Scoring given rows (include/rq.h rq_score_rows_device) at bench scale: what the random whole-row gather delivers
beside the project's own yardstick for the same arithmetic (the filter's gather route) and beside the route a caller has without it.

On rows built on the device (default 1M x 768, Gaussian, unit norm), with uniformly random lists, at B x m = 64 x 100, 500 x 100 and
500 x 1 000, in one process on one index:
  score_us     one rq_score_rows_device call (query preparation + the scoring launch): HIP events around `--launches` (default 50)
               back-to-back calls after 5 warm-up calls, three repetitions (all three are reported); pairs_per_s and gathered
               bytes per second (pairs x stored row bytes) from the best repetition;
  gather_us    a filtered search of the same B queries over a filter of m random rows with "filter_route" = 1, k = 10: preparation +
               rq_gather_score_kernel over B x m pairs + the final top-k, timed the same way;
  host_ms      the route a caller has today, timed ONCE: rq_index_get_rows_f16 for every pair (one call per row) and a numpy
               float64 product per query.
The device scores are compared with that numpy product (largest absolute difference).
`--hybrid` adds the cost of `complete_scores` on the shape of BASELINE.json configs[4] (500 questions over 50 000 passages, pools
of 100, 100 passages to the router; tests/config_workloads.py's synthetic QA set): get_scores_for_router_batch with and without it,
alternating, best and median of `--hybrid-reps` calls each.

    python tools/gpu_score_rows.py --out profiles/score_rows.txt [--rows 1000000] [--launches 50] [--label tile64] [--hybrid]
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

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--label", default="")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--hybrid", action="store_true")
ap.add_argument("--hybrid-reps", type=int, default=7)
args = ap.parse_args()
dev = torch.device("cuda:0")
N, DIM, LAUNCHES = args.rows, args.dim, max(10, args.launches)
SHAPES = [(64, 100), (500, 100), (500, 1000)]


def build():
    idx = nat.NativeIndex(DIM, 0)
    idx.reserve(N)
    g = torch.Generator(device=dev); g.manual_seed(DIM)
    for lo in range(0, N, 125_000):
        m = min(125_000, N - lo)
        x = torch.nn.functional.normalize(torch.randn((m, DIM), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        del x
    idx.set_option("pipeline", 0)
    idx.set_option("scan8", 0)
    return idx


def event_us(launch):
    """microseconds per call: events around LAUNCHES back-to-back calls, after 5 warm-up calls; three repetitions"""
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    reps = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch()
        e1.record()
        torch.cuda.synchronize()
        reps.append(round(e0.elapsed_time(e1) * 1e3 / LAUNCHES, 2))
    return reps


def host_route(idx, q, rows):
    """fetch every pair's row (one call per row), then a float64 product per query; returns (seconds, scores [B][m])"""
    t0 = time.perf_counter()
    B, m = rows.shape
    out = np.empty((B, m), np.float32)
    q64 = q.astype(np.float64)
    for b in range(B):
        x = np.stack([idx.get_rows_f16(int(r), 1)[0] for r in rows[b]]).astype(np.float64)
        out[b] = ((x @ q64[b]) / (np.sqrt((x * x).sum(axis=1)) * np.sqrt((q64[b] * q64[b]).sum()) + 1e-30)).astype(np.float32)
    return time.perf_counter() - t0, out


def run_kernel_cases():
    idx = build()
    rowb = idx.row_pad * 2
    cases = []
    for B, m in SHAPES:
        rng = np.random.default_rng(B * 100003 + m)
        rows = rng.integers(0, N, size=(B, m)).astype(np.int64)
        g = torch.Generator(device=dev); g.manual_seed(1000 + B + m)
        q = torch.randn((B, DIM), device=dev, generator=g)
        d_rows = torch.from_numpy(rows).to(dev)
        d_scores = torch.empty((B, m), device=dev)
        score = lambda: idx.score_rows_device(q, B, d_rows, m, 0, d_scores, 0)
        row = {"label": args.label, "rows": N, "dim": DIM, "row_pad": idx.row_pad, "B": B, "m": m, "pairs": B * m}
        row["score_us"] = event_us(score)
        best = min(row["score_us"]) * 1e-6
        row["pairs_per_s"] = round(B * m / best)
        row["gathered_GB_per_s"] = round(B * m * rowb / best / 1e9, 1)
        # the gather route over an equal number of rows: one list of m rows shared by the B queries
        flt = idx.make_filter(np.unique(rng.integers(0, N, size=m)))
        na = flt.count
        f_s = torch.empty((B, 10), device=dev); f_r = torch.empty((B, 10), device=dev, dtype=torch.int64); f_st = torch.zeros((B,), device=dev, dtype=torch.int32)
        idx.set_option("filter_route", 1)
        gather = lambda: idx.search_device(q, B, 10, 0, f_s, f_r, None, f_st, 0, row_filter=flt)
        row["gather_us"] = event_us(gather)
        assert int(idx.get_option("filter_route_last")) == 1
        idx.set_option("filter_route", -1)
        flt.close()
        gbest = min(row["gather_us"]) * 1e-6
        row["gather_pairs"] = B * na
        row["gather_pairs_per_s"] = round(B * na / gbest)
        torch.cuda.synchronize()
        if not args.no_host:
            got = d_scores.cpu().numpy()
            sec, want = host_route(idx, q.cpu().numpy(), rows)
            row["host_ms"] = round(sec * 1e3, 1)
            row["max_abs_diff_vs_host"] = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        cases.append(row)
        print(json.dumps(row), flush=True)
    idx.close()
    return cases


def run_hybrid():
    """get_scores_for_router_batch on the configs[4] shape with and without complete_scores, alternating"""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from config_workloads import synthetic_qa
    from rag_uq_amd import streaming_index as si
    from rag_uq_amd.embedders import RandomProjectionEmbedder
    n_passages, n_questions, pool, num = 50_000, 500, 100, 100
    passages, questions, _ = synthetic_qa(n_passages, n_questions)
    tmp = tempfile.mkdtemp()
    dense = si.DenseIndex(persist_directory="", embedder=RandomProjectionEmbedder(768), load_persisted=False, auto_persist=False)
    r = si.HybridRetriever(bm25_persist_path=os.path.join(tmp, "bm25.pkl"), chroma_persist_path=os.path.join(tmp, "c"), dense_index=dense)
    r.bm25_index.persist_path = None
    docs = [si.Document(id=f"p{i}", text=t) for i, t in enumerate(passages)]
    for lo in range(0, n_passages, 5000):
        r.add_documents(docs[lo: lo + 5000], batch_size=5000)
    for flag in (False, True):
        r.get_scores_for_router_batch(questions, num_passages=num, retrieval_pool_size=pool, complete_scores=flag)
    ms = {False: [], True: []}
    for _ in range(max(3, args.hybrid_reps)):
        for flag in (False, True):
            t0 = time.perf_counter()
            out = r.get_scores_for_router_batch(questions, num_passages=num, retrieval_pool_size=pool, complete_scores=flag)
            ms[flag].append(round((time.perf_counter() - t0) * 1e3, 2))
    plain = r.get_scores_for_router_batch(questions, num_passages=num, retrieval_pool_size=pool)
    zeros = lambda arrays: int(sum(sum(1 for b, d, i in zip(a[0], a[1], a[2]) if i and (b == 0.0 or d == 0.0)) for a in arrays))
    cands = int(sum(sum(1 for i in a[2] if i) for a in plain))
    row = {"hybrid": f"{n_questions} questions x pools of {pool} over {n_passages} passages, {num} passages to the router", "candidates": cands,
           "candidates_with_a_zero_score_plain": zeros(plain), "candidates_with_a_zero_score_completed": zeros(out),
           "plain_ms": sorted(ms[False]), "completed_ms": sorted(ms[True]),
           "plain_ms_median": float(np.median(ms[False])), "completed_ms_median": float(np.median(ms[True])),
           "score_calls": int(dense._index.get_option("score_calls")), "score_pairs": int(dense._index.get_option("score_pairs"))}
    print(json.dumps(row), flush=True)
    return row


results = {"device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "cases": run_kernel_cases()}
if args.hybrid:
    results["hybrid"] = run_hybrid()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/gpu_score_rows.py --rows {N} --dim {DIM} --launches {LAUNCHES}: {results['device']}; score_us / gather_us: HIP events over {LAUNCHES} calls, three repetitions\n")
        for row in results["cases"]:
            f.write(json.dumps(row) + "\n")
        if args.hybrid:
            f.write(json.dumps(results["hybrid"]) + "\n")
print(json.dumps(results))
