"""Row length 384 against 768 (include/rq.h option "row_pad"): what the narrow layout of csrc/rq_scan_narrow.hip buys and costs.

Public NativeIndex calls only, so the same script runs on a commit without the option ("row_pad" is set inside a try: there
every index is the 768-element layout, and the cases that ask for another row length are marked "row_pad_applied": false).
Per case (dim, requested row_pad, scan8) on rows built on the device:
  * microseconds per batch of the fused loop bench.py times (pipeline 2, one stream, every next batch announced), B = 64, k = 10 / 100 / 200;
  * per-launch scan time from HIP events on the dispatches (profile = 1, a run of its own), bytes per launch, fraction of 8 TB/s;
  * microseconds per blocking-free call (search_device + flush) at B = 128, 256, 512 (k = 10) and B = 500 (k = 100);
  * the 125 000-row shard on two streams (the per-rank step of a multi-GPU run).
Every figure: the shape is warmed up, then at least `--min-seconds` (default 0.5) of work is timed with the profiler off.

    python tools/gpu_row_pad.py --out profiles/row_pad_384.json [--rows 1000000] [--label branch]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_uq_amd import _native as nat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--label", default="")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--small-rows", type=int, default=125_000)
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--cases", default="", help="comma-separated case names to run (default: all)")
args = ap.parse_args()
dev = torch.device("cuda:0")
NQ = 16           # distinct query batches of a loop
PEAK = 8.0e12     # B/s


def build(dim, n, pad):
    idx = nat.NativeIndex(dim, 0)
    applied = True
    if pad is not None:
        try:
            idx.set_option("row_pad", pad)
        except nat.RqError:
            applied = False
    idx.reserve(n)
    g = torch.Generator(device=dev); g.manual_seed(dim)
    for lo in range(0, n, 125_000):
        m = min(125_000, n - lo)
        x = torch.nn.functional.normalize(torch.randn((m, dim), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        del x
    pad_now = idx.get_option("row_pad")
    return idx, applied, (int(pad_now) if pad_now == pad_now else 768)      # (NaN: a library without the option)


def timed(run, min_seconds):
    """run(steps) enqueues and completes `steps` units; returns seconds per unit over at least min_seconds of work"""
    run(8)
    t0 = time.perf_counter(); run(16); est = (time.perf_counter() - t0) / 16
    steps = max(32, int(min_seconds / max(est, 1e-7)) + 1)
    t0 = time.perf_counter(); run(steps); dt = time.perf_counter() - t0
    return dt / steps, steps


def fused_loop(idx, dim, k, nstreams, B=64):
    g = torch.Generator(device=dev); g.manual_seed(1000 + dim + k)
    qs = [torch.randn((B, dim), device=dev, generator=g) for _ in range(NQ)]
    outs = [(torch.empty((B, k), device=dev), torch.empty((B, k), device=dev, dtype=torch.int64), torch.zeros((B,), device=dev, dtype=torch.int32)) for _ in range(NQ)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(nstreams)]
    idx.set_option("pipeline", 2)

    def run(steps):
        for i in range(steps):
            s = streams[i % nstreams]; j = i % NQ
            idx.search_hint_next_device(qs[(i + nstreams) % NQ], B, s.cuda_stream)
            idx.search_device(qs[j], B, k, 0, outs[j][0], outs[j][1], None, outs[j][2], s.cuda_stream)
        for s in streams:
            idx.search_flush_device(s.cuda_stream)
        torch.cuda.synchronize()
    run(4 * NQ)                                                    # (builds the int8 image and calibrates where the library wants it)
    sec, steps = timed(run, args.min_seconds)
    unc = int(sum(int(o[2].sum()) for o in outs))
    res = {"us_per_batch": round(sec * 1e6, 2), "batches_timed": steps, "uncertified_in_last_round": unc}
    idx.reset_timing()
    idx.set_option("profile", 1)                                   # a run of its own for the per-launch figures
    run(256)
    t = idx.timing()
    idx.set_option("profile", 0)
    if t["scan_launches"]:
        per = t["scan_ms"] * 1e-3 / t["scan_launches"]
        bytes_per = t["scan_bytes"] / t["scan_launches"]
        res.update(scan_us_per_launch=round(per * 1e6, 2), scan_launches=t["scan_launches"], bytes_per_launch=int(bytes_per),
                   fraction_of_8TBs=round(bytes_per / per / PEAK, 4))
    for s in streams:
        idx.stream_release(s.cuda_stream)
    idx.set_option("pipeline", 0)
    return res


def wide_calls(idx, dim, B, k):
    g = torch.Generator(device=dev); g.manual_seed(2000 + B + k)
    qs = [torch.randn((B, dim), device=dev, generator=g) for _ in range(4)]
    sc = torch.empty((B, k), device=dev); rw = torch.empty((B, k), device=dev, dtype=torch.int64); st = torch.zeros((B,), device=dev, dtype=torch.int32)
    idx.set_option("profile", 1)
    idx.reset_timing()

    def run(steps):
        for i in range(steps):
            idx.search_device(qs[i % 4], B, k, 0, sc, rw, None, st, 0)
        idx.search_flush_device(0)
        torch.cuda.synchronize()
    run(8)
    t = idx.timing()
    passes = t["scan_launches"] / 8
    idx.set_option("profile", 0)
    sec, steps = timed(run, args.min_seconds)
    return {"us_per_call": round(sec * 1e6, 1), "calls_timed": steps, "scan_passes_per_call": passes, "uncertified_last_call": int(st.sum())}


CASES = [  # name, dim, requested row_pad, scan8 (None = the library's default), further options
    ("d384_default", 384, None, None, {}), ("d384_fp16", 384, None, 0, {}),
    ("d384_fp16_one_pass_per_batch", 384, None, 0, {"scan_ahead": 0}),      # (768-element rows: no announced batch is scanned ahead)
    ("d384_pad768_default", 384, 768, None, {}), ("d384_pad768_fp16", 384, 768, 0, {}),
    ("d32_default", 32, None, None, {}), ("d32_fp16", 32, None, 0, {}), ("d768_default", 768, None, None, {}), ("d768_fp16", 768, None, 0, {})]
want = set(c for c in args.cases.split(",") if c)
result = {"label": args.label, "rows": args.rows, "cases": {}}
built = {}
for name, dim, pad, scan8, more in CASES:
    if want and name not in want:
        continue
    key = (dim, pad)
    if key not in built:
        for k_, v_ in list(built.items()):                          # one large index at a time
            v_[0].close()
            del built[k_]
        built[key] = build(dim, args.rows, pad)
    idx, applied, pad_now = built[key]
    if scan8 is not None:
        idx.set_option("scan8", scan8)
    before = {o: idx.get_option(o) for o in more}
    for o, v in more.items():
        idx.set_option(o, v)
    case = {"dim": dim, "options": more, "row_pad_requested": pad, "row_pad_applied": applied, "row_pad": pad_now, "scan8": scan8}
    case["fused_k10"] = fused_loop(idx, dim, 10, 1)
    case["fused_k100"] = fused_loop(idx, dim, 100, 1)
    case["fused_k200"] = fused_loop(idx, dim, 200, 1)
    for B, k in ((128, 10), (256, 10), (512, 10), (500, 100)):
        case[f"call_B{B}_k{k}"] = wide_calls(idx, dim, B, k)
    case["scan8_used"] = int(idx.get_option("scan8_used"))
    case["scan8_level"] = idx.get_option("scan8_level")
    case["repaired_queries"] = int(idx.get_option("repaired_queries"))
    if scan8 is not None:
        idx.set_option("scan8", 1)
    for o, v in before.items():
        idx.set_option(o, v)
    result["cases"][name] = case
    print(name, json.dumps(case), flush=True)
for v_ in built.values():
    v_[0].close()
built.clear()
if not want or "small_shard" in want:
    small = {}
    for name, dim, pad, scan8 in (("d384_fp16", 384, None, 0), ("d384_default", 384, None, None), ("d384_pad768_fp16", 384, 768, 0)):
        idx, applied, pad_now = build(dim, args.small_rows, pad)
        if scan8 is not None:
            idx.set_option("scan8", scan8)
        small[name] = dict(fused_loop(idx, dim, 10, 2), row_pad=pad_now, row_pad_applied=applied, rows=args.small_rows, streams=2)
        idx.close()
    result["small_shard"] = small
    print("small_shard", json.dumps(small), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
