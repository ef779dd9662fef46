"""The blocking host-buffer forms beside rq_search (include/rq.h rq_search_filtered, rq_search_mmr, rq_score_rows; csrc/rq_stage.h): wall
clock per call, staging included.  tools/gpu_filter.py, gpu_mmr.py and gpu_score_rows.py time the DEVICE forms; this one times what a
caller with host buffers pays: allocation of the staging buffers, the copy up, the device form, the copies down, the wait, the frees.

On rows built on the device (default 250 k x 768, Gaussian, unit norm), B = 64: a filtered search at k = 10 under a 1 % filter (gather
route) and a 50 % filter (scan route), an MMR search (fetch_k 100, k 10), scoring 100 random rows per query.  Every figure is
microseconds per call over `--calls` back-to-back calls after 5 warm-up calls, `--reps` repetitions, all reported: their spread is
the yardstick when two builds are compared (run the same file from each tree, alternating).

    python tools/gpu_blocking_forms.py [--rows 250000] [--calls 50] [--reps 5] [--label parent] [--out FILE (appended to)]
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
ap.add_argument("--rows", type=int, default=250_000)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
N, DIM, B = args.rows, 768, 64

idx = nat.NativeIndex(DIM, 0)
idx.reserve(N)
g = torch.Generator(device=dev); g.manual_seed(DIM)
for lo in range(0, N, 125_000):
    n = min(125_000, N - lo)
    idx.add_f16_device(torch.nn.functional.normalize(torch.randn((n, DIM), device=dev, generator=g), dim=1).half().contiguous(), n)
idx.set_option("scan8", 0)
rng = np.random.default_rng(7)
q = rng.standard_normal((B, DIM)).astype(np.float32)
lists = rng.integers(0, N, size=(B, 100), dtype=np.int64)
f1 = idx.make_filter(rng.choice(N, size=N // 100, replace=False))
f50 = idx.make_filter(rng.choice(N, size=N // 2, replace=False))
cases = [("filtered 1 % k=10", lambda: idx.search(q, 10, row_filter=f1)),
         ("filtered 50 % k=10", lambda: idx.search(q, 10, row_filter=f50)),
         ("mmr fetch_k=100 k=10", lambda: idx.search_mmr(q, 10, 100, 0.5)),
         ("score_rows m=100", lambda: idx.score_rows(q, lists))]
lines = []
for name, call in cases:
    for _ in range(5):
        call()
    reps = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        reps.append(round((time.perf_counter() - t0) * 1e6 / args.calls, 1))
    row = {"label": args.label, "case": name, "rows": N, "B": B, "calls": args.calls, "us_per_call": reps}
    if name.startswith("filtered"):
        row["route"] = int(idx.get_option("filter_route_last"))
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
f1.close(); f50.close(); idx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
