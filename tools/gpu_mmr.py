"""MMR selection (include/rq.h rq_mmr_select_device) at bench scale: what the selection launch costs beside the search
that feeds it and beside the host route a caller has without it.

On rows built on the device (default 1M rows, Gaussian, unit norm), for the wide layout (dim 768) and the narrow one (dim 384), at
(B, fetch_k, k) = (64, 100, 10), (64, 1024, 100) and (1, 50, 10), lambda = 0.5, in one process on one index:
  select_us   the selection launch alone over the search's candidates: HIP events around `--launches` (default 50, at least 50)
              back-to-back launches after 5 warm-up launches, three repetitions (all three are reported);
  search_us   the plain rq_search_device of k = fetch_k that feeds it, pipeline = 0, timed the same way;
  host_ms     the route a caller has today, timed ONCE: read the candidates back, fetch their rows with rq_index_get_rows_f16 (one
              call per row), greedy selection in numpy (float64 dot products of the picked row against the candidates).
The device's picks are compared with that numpy selection (`agree`: queries whose k picks are the same rows in the same order; the
host loop rounds a similarity once, to float32, as the definition does, but sums in BLAS order).

    python tools/gpu_mmr.py --out profiles/mmr_select.txt [--rows 1000000] [--launches 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_uq_amd import _native as nat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--dims", default="768,384")
args = ap.parse_args()
dev = torch.device("cuda:0")
N, LAUNCHES, LAM = args.rows, max(50, args.launches), 0.5
SHAPES = [(64, 100, 10), (64, 1024, 100), (1, 50, 10)]


def build(dim):
    idx = nat.NativeIndex(dim, 0)
    idx.reserve(N)
    g = torch.Generator(device=dev); g.manual_seed(dim)
    for lo in range(0, N, 125_000):
        m = min(125_000, N - lo)
        x = torch.nn.functional.normalize(torch.randn((m, dim), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        del x
    idx.set_option("pipeline", 0)
    return idx


def event_us(launch):
    """microseconds per launch: events around LAUNCHES back-to-back launches, after 5 warm-up launches; three repetitions"""
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


def host_route(idx, rel, rows, k):
    """fetch the candidates' rows (one call per row), then the greedy selection in numpy; returns (seconds, picked rows [B][k])"""
    t0 = time.perf_counter()
    B, m = rows.shape
    out = np.full((B, k), -1, np.int64)
    for b in range(B):
        x = np.stack([idx.get_rows_f16(int(r), 1)[0] for r in rows[b]]).astype(np.float64)
        nrm = np.sqrt((x * x).sum(axis=1))
        pen = np.zeros(m, np.float32)
        live = np.ones(m, dtype=bool)
        for t in range(k):
            v = LAM * rel[b].astype(np.float64) - (1.0 - LAM) * pen.astype(np.float64)
            c = np.flatnonzero(live)
            p = int(c[np.argmax(v[c])])
            out[b, t] = rows[b, p]
            live[p] = False
            s = ((x @ x[p]) / (nrm * nrm[p] + 1e-30)).astype(np.float32)
            pen = s if t == 0 else np.maximum(pen, s)
    return time.perf_counter() - t0, out


results = {"rows": N, "lambda": LAM, "launches": LAUNCHES, "device": torch.cuda.get_device_name(0), "cases": []}
for dim in [int(d) for d in args.dims.split(",")]:
    idx = build(dim)
    for B, fetch_k, k in SHAPES:
        g = torch.Generator(device=dev); g.manual_seed(1000 + B + fetch_k)
        q = torch.randn((B, dim), device=dev, generator=g)
        c_s = torch.empty((B, fetch_k), device=dev); c_r = torch.empty((B, fetch_k), device=dev, dtype=torch.int64)
        c_st = torch.zeros((B,), device=dev, dtype=torch.int32)
        o_s = torch.empty((B, k), device=dev); o_r = torch.empty((B, k), device=dev, dtype=torch.int64); o_v = torch.empty((B, k), device=dev)
        search = lambda: idx.search_device(q, B, fetch_k, 0, c_s, c_r, None, c_st, 0)
        search()
        repaired = idx.search_fixup_device(q, B, fetch_k, 0, c_s, c_r, None, c_st, 0)      # exact candidates for the comparison below
        torch.cuda.synchronize()
        rel, rows = c_s.cpu().numpy(), c_r.cpu().numpy()
        d_rel, d_rows = c_s.clone(), c_r.clone()
        select = lambda: idx.mmr_select_device(d_rows, d_rel, B, fetch_k, k, LAM, 0, o_s, o_r, o_v, 0)
        row = {"dim": dim, "row_pad": idx.row_pad, "B": B, "fetch_k": fetch_k, "k": k, "repaired_before": int(repaired)}
        row["select_us"] = event_us(select)
        row["search_us"] = event_us(search)
        row["select_us_per_step"] = round(min(row["select_us"]) / k, 2)
        torch.cuda.synchronize()
        picked = o_r.cpu().numpy()
        sec, want = host_route(idx, rel, rows, k)
        row["host_ms"] = round(sec * 1e3, 1)
        row["agree"] = f"{int((picked == want).all(axis=1).sum())} of {B}"
        results["cases"].append(row)
        print(json.dumps(row), flush=True)
    idx.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/gpu_mmr.py --rows {N} --launches {LAUNCHES}: {results['device']}, lambda = {LAM}; select_us / search_us: HIP events over {LAUNCHES} launches, three repetitions\n")
        for row in results["cases"]:
            f.write(json.dumps(row) + "\n")
print(json.dumps(results))
