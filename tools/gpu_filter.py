"""Filtered searches (include/rq.h rq_search_filtered_device) at bench scale: what a filter costs and where the routes cross.

On rows built on the device (default 1M x 768, Gaussian, unit norm), every figure from a warmed-up run of at least `--min-seconds`
(default 0.5) of work, filtered and unfiltered runs alternated twice each (their spread is the yardstick):
  1. scan: per-launch time of the scan kernels from "profile" events inside a filtered call (route 2) and inside an unfiltered
     pipeline = 0, scan8 = 0 call -- the same instructions over the same bytes;
  2. call: a 64-query call (k = 10) end to end, unfiltered against random masks of 50 %, 10 % and 1 % under the rule and on each
     forced route, and against the workaround the filter replaces: over-fetch k / selectivity rows and filter on the host;
  3. crossover: gather (route 1) against scan (route 2) over the allowed count na for B = 1, 64 and 256 -- the constant of the
     route rule (csrc/rq_filter_plan.h RQ_FILTER_GATHER_DIV);
  4. contiguous: one run of 10 % of the rows (one source appended together) at k = 100, B = 64: the rule's choice against each
     forced route -- the case the partition condition of the rule exists for.
Every timed call is followed by its repair step (rq_search_fixup_device / _filtered_device), so a route that cannot certify is timed
with its repairs and `repaired_per_call` says how many queries needed them.

    python tools/gpu_filter.py --out profiles/filter_routes.json [--rows 1000000] [--parts scan,call,crossover]
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
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--parts", default="scan,call,crossover,contiguous")
args = ap.parse_args()
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
    run(3)
    t0 = time.perf_counter(); run(4); est = (time.perf_counter() - t0) / 4
    steps = max(8, int(min_seconds / max(est, 1e-7)) + 1)
    t0 = time.perf_counter(); run(steps); dt = time.perf_counter() - t0
    return dt / steps, steps


class Calls:
    def __init__(self, B, k=K):
        g = torch.Generator(device=dev); g.manual_seed(100 + B)
        self.B, self.k = B, k
        self.q = [torch.randn((B, DIM), device=dev, generator=g) for _ in range(4)]
        self.s = torch.empty((B, k), device=dev); self.r = torch.empty((B, k), device=dev, dtype=torch.int64)
        self.st = torch.zeros((B,), device=dev, dtype=torch.int32)
        self.repaired = 0

    def run(self, idx, flt, steps):
        # every call with its repair step (a status copy + synchronisation, and the ladder for what came back uncertified), filtered
        # or not: a forced route that cannot certify is timed with its repairs, and "repaired" counts them
        for i in range(steps):
            q = self.q[i % 4]
            idx.search_device(q, self.B, self.k, 0, self.s, self.r, None, self.st, 0, row_filter=flt)
            self.repaired += idx.search_fixup_device(q, self.B, self.k, 0, self.s, self.r, None, self.st, 0, row_filter=flt)
        torch.cuda.synchronize()

    def us(self, idx, flt):
        """(microseconds per call, queries repaired per call) over the timed region and its warm-up"""
        self.repaired = 0
        calls = [0]

        def run(n):
            calls[0] += n
            self.run(idx, flt, n)
        sec, _ = timed(run, args.min_seconds)
        return round(sec * 1e6, 1), round(self.repaired / max(calls[0], 1), 2)


def random_filter(idx, na, seed=5):
    rows = np.random.default_rng(seed + na).choice(N, size=na, replace=False)
    return idx.make_filter(rows)


def scan_launch_us(idx, flt, B):
    c = Calls(B)
    c.run(idx, flt, 3)
    idx.set_option("profile", 1)
    idx.reset_timing()
    steps = max(8, int(args.min_seconds / 300e-6))
    c.run(idx, flt, steps)
    t = idx.timing()
    idx.set_option("profile", 0)
    idx.reset_timing()
    return round(t["scan_ms"] * 1e3 / max(t["scan_launches"], 1), 2), t["scan_launches"]


out = {"rows": N, "dim": DIM, "k": K, "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds}
idx = build()
parts = set(args.parts.split(","))

if "scan" in parts:
    half = random_filter(idx, N // 2)
    idx.set_option("filter_route", 2)
    rows = []
    for B in (64, 128, 256):
        for rep in range(2):
            rows.append({"B": B, "rep": rep, "unfiltered_us_per_launch": scan_launch_us(idx, None, B)[0], "filtered_us_per_launch": scan_launch_us(idx, half, B)[0]})
            print("scan", rows[-1], flush=True)
    idx.set_option("filter_route", -1)
    half.close()
    out["scan_launch"] = rows

if "call" in parts:
    c = Calls(64)
    rows = []
    for rep in range(2):
        rows.append({"case": "unfiltered", "rep": rep, "us_per_call": c.us(idx, None)[0]})
        print("call", rows[-1], flush=True)
        for share in (0.5, 0.1, 0.01):
            flt = random_filter(idx, int(N * share))
            for route in (-1, 1, 2, 3):
                if route == 1 and share > 0.1:
                    continue                                  # (32 M row reads per call: seconds, and not what the rule would pick)
                idx.set_option("filter_route", route)
                us, repaired = c.us(idx, flt)
                rows.append({"case": f"filtered {share:g}", "route": route, "took": int(idx.get_option("filter_route_last")), "rep": rep, "us_per_call": us,
                             "repaired_per_call": repaired})
                print("call", rows[-1], flush=True)
            idx.set_option("filter_route", -1)
            # the workaround: over-fetch k / selectivity rows (at most RQ_MAX_K), copy back, filter on the host
            kk = min(int(round(K / share)), nat.MAX_K)
            over = Calls(64, kk)
            mask = np.zeros(N, dtype=bool)
            mask[np.random.default_rng(5 + int(N * share)).choice(N, size=int(N * share), replace=False)] = True

            def overfetch(steps):
                short = 0
                for i in range(steps):
                    idx.search_device(over.q[i % 4], 64, kk, 0, over.s, over.r, None, over.st, 0)
                    torch.cuda.synchronize()
                    r = over.r.cpu().numpy()
                    keep = (r >= 0) & mask[np.maximum(r, 0)]
                    short += int((keep.sum(1) < K).sum())
                overfetch.short = short / max(steps, 1)
            sec, _ = timed(overfetch, args.min_seconds)
            rows.append({"case": f"over-fetch {share:g}", "k_fetched": kk, "rep": rep, "us_per_call": round(sec * 1e6, 1), "queries_short_of_k_per_call": overfetch.short})
            print("call", rows[-1], flush=True)
            flt.close()
    out["call_64"] = rows

if "crossover" in parts:
    rows = []
    for B in (1, 64, 256):
        c = Calls(B)
        base = c.us(idx, None)[0]
        for na in (1000, 4000, 16000, 64000, 250000):
            if B * na > 20_000_000:
                continue
            flt = random_filter(idx, na)
            row = {"B": B, "na": na, "unfiltered_us": base}
            for name, route in (("gather_us", 1), ("scan_us", 2)):
                idx.set_option("filter_route", route)
                row[name] = c.us(idx, flt)[0]
            idx.set_option("filter_route", -1)
            c.run(idx, flt, 1)
            row["rule_takes"] = int(idx.get_option("filter_route_last"))
            row["B_na_over_N"] = round(B * na / N, 4)
            rows.append(row)
            print("crossover", row, flush=True)
            flt.close()
    out["crossover"] = rows

if "contiguous" in parts:
    rows = []
    c = Calls(64, 100)
    flt = idx.make_filter(np.arange(N // 4, N // 4 + N // 10))
    for rep in range(2):
        us, _ = c.us(idx, None)
        rows.append({"case": "unfiltered k=100", "rep": rep, "us_per_call": us})
        for route in (-1, 1, 2, 3):
            idx.set_option("filter_route", route)
            us, repaired = c.us(idx, flt)
            rows.append({"case": "contiguous 10 % k=100", "route": route, "took": int(idx.get_option("filter_route_last")), "rep": rep, "us_per_call": us,
                         "repaired_per_call": repaired})
            print("contiguous", rows[-1], flush=True)
        idx.set_option("filter_route", -1)
    flt.close()
    out["contiguous"] = rows

idx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
