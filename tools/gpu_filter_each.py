"""One filter per query (include/rq.h rq_search_filtered_each_device) at bench scale: the each-call against the host loop
of rq_search_filtered_device over the same groups on the same build -- until now the only way to get the result.

On rows built on the device (default 1M x 768, Gaussian, unit norm), k = 10, every figure from a warmed-up run of at least
`--min-seconds` (default 0.4) of work that ends in a device synchronise, loop and each-call alternated twice each (their spread is
the yardstick).  Every call is followed by its repair step, as in tools/gpu_filter.py.  The loop is given its sub-batches ready
made (queries already split by filter, outputs of its own): only its calls are timed.
  A  64 queries, 64 disjoint tenants of N / 64 rows (row % 64 == t): the ragged set, one query per list;
  B  256 queries, 256 tenants of N / 256 rows;
  C  64 queries, 8 tenants of N / 8 rows, 8 queries each (arranged by tenant): does the ragged order keep the cache sharing of the
     uniform gather?
  D  64 queries, 8 / 12 / 16 / 32 / 64 distinct half-allowing masks dealt interleaved: one pass per group ("filter_route" 2) against
     the shared exact route ("filter_route" 3) and the rule -- the measured crossover behind RQ_FILTER_EACH_EXACT_GROUPS.
Before a shape is timed, the each-call's rows are compared with the loop's.

    python tools/gpu_filter_each.py --out profiles/filter_each.json [--rows 1000000] [--shapes A,B,C,D]
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
ap.add_argument("--min-seconds", type=float, default=0.4)
ap.add_argument("--shapes", default="A,B,C,D")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/gpu_filter_each.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
DIM, K = 768, 10
N = args.rows


def build():
    idx = nat.NativeIndex(DIM, 0)
    idx.reserve(N)
    g = torch.Generator(device=dev); g.manual_seed(DIM)
    for lo in range(0, N, 125_000):
        m = min(125_000, N - lo)
        x = torch.nn.functional.normalize(torch.randn((m, DIM), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        del x
    idx.set_option("scan8", 0)
    idx.set_option("pipeline", 0)
    return idx


def timed(run, min_seconds):
    """run(steps) enqueues and completes `steps` calls; seconds per call over at least min_seconds of work"""
    run(2)
    t0 = time.perf_counter(); run(2); est = (time.perf_counter() - t0) / 2
    steps = max(4, int(min_seconds / max(est, 1e-7)) + 1)
    t0 = time.perf_counter(); run(steps); dt = time.perf_counter() - t0
    return dt / steps


class Batch:
    """B queries with one filter each (4 query sets in rotation), the each-call's outputs, and the same work cut into the loop's
    sub-batches: per distinct filter its queries and outputs of its own."""

    def __init__(self, filters):
        self.filters, self.B = filters, len(filters)
        g = torch.Generator(device=dev); g.manual_seed(100 + self.B)
        self.q = [torch.randn((self.B, DIM), device=dev, generator=g) for _ in range(4)]
        self.s = torch.empty((self.B, K), device=dev); self.r = torch.empty((self.B, K), device=dev, dtype=torch.int64)
        self.st = torch.zeros((self.B,), device=dev, dtype=torch.int32)
        groups = {}
        for i, f in enumerate(filters):
            groups.setdefault(id(f), (f, []))[1].append(i)
        self.groups = []
        for f, pos in groups.values():
            p = torch.tensor(pos, device=dev)
            self.groups.append({"f": f, "pos": pos, "q": [q[p].contiguous() for q in self.q], "s": torch.empty((len(pos), K), device=dev),
                                "r": torch.empty((len(pos), K), device=dev, dtype=torch.int64), "st": torch.zeros((len(pos),), device=dev, dtype=torch.int32)})
        self.repaired = 0

    def run_each(self, idx, steps):
        for i in range(steps):
            q = self.q[i % 4]
            idx.search_filtered_each_device(q, self.B, K, 0, self.s, self.r, None, self.st, self.filters, 0)
            self.repaired += idx.search_filtered_each_fixup_device(q, self.B, K, 0, self.s, self.r, None, self.st, self.filters, 0)
        torch.cuda.synchronize()

    def run_loop(self, idx, steps):
        for i in range(steps):
            for g in self.groups:
                q = g["q"][i % 4]
                idx.search_device(q, len(g["pos"]), K, 0, g["s"], g["r"], None, g["st"], 0, row_filter=g["f"])
                self.repaired += idx.search_fixup_device(q, len(g["pos"]), K, 0, g["s"], g["r"], None, g["st"], 0, row_filter=g["f"])
        torch.cuda.synchronize()

    def check(self, idx):
        """the each-call's rows against the loop's, on query set 0"""
        self.run_each(idx, 1)
        each = self.r.cpu().numpy().copy()
        self.run_loop(idx, 1)
        for g in self.groups:
            if not np.array_equal(each[g["pos"]], g["r"].cpu().numpy()):
                sys.exit("the each-call and the loop disagree")

    def us(self, idx, which):
        self.repaired = 0
        calls = [0]

        def run(n):
            calls[0] += n
            (self.run_each if which == "each" else self.run_loop)(idx, n)
        sec = timed(run, args.min_seconds)
        return round(sec * 1e6, 1), round(self.repaired / max(calls[0], 1), 2)


def each_stats(idx):
    return {nm: int(idx.get_option("filter_each_" + nm)) for nm in ("groups_last", "ragged_last", "rounds_last", "shared_exact_last", "routes_last")}


def measure(idx, name, batch, routes=(-1,)):
    rows = []
    batch.check(idx)
    for rep in range(2):
        us, rep_l = batch.us(idx, "loop")
        rows.append({"shape": name, "rep": rep, "what": "loop", "groups": len(batch.groups), "us_per_batch": us, "repaired_per_batch": rep_l})
        print(rows[-1], flush=True)
        for route in routes:
            idx.set_option("filter_route", route)
            us, rep_e = batch.us(idx, "each")
            rows.append({"shape": name, "rep": rep, "what": "each", "filter_route": route, "us_per_batch": us, "repaired_per_batch": rep_e, **each_stats(idx)})
            idx.set_option("filter_route", -1)
            print(rows[-1], flush=True)
    return rows


out = {"rows": N, "dim": DIM, "k": K, "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds, "results": []}
idx = build()
shapes = set(args.shapes.split(","))


def tenant_filters(T):
    return [idx.make_filter(np.arange(t, N, T)) for t in range(T)]


for name, T, per in (("A", 64, 1), ("B", 256, 1), ("C", 8, 8)):
    if name not in shapes:
        continue
    fl = tenant_filters(T)
    out["results"] += measure(idx, name, Batch([f for f in fl for _ in range(per)]))
    for f in fl:
        f.close()

if "D" in shapes:
    masks = [idx.make_filter(np.random.default_rng(500 + j).random(N) < 0.5) for j in range(64)]
    for nf in (8, 12, 16, 32, 64):
        out["results"] += measure(idx, f"D{nf}", Batch([masks[i % nf] for i in range(64)]), routes=(-1, 2, 3))
    for f in masks:
        f.close()

idx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
