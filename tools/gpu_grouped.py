"""Grouped searches (include/rq.h rq_search_grouped_device) at bench scale: what the first rung's over-fetch costs, how
often it is not enough, and which "group_fetch" is cheapest once the repairs are paid for.

On rows built on the device (default 1M x 768), B = 64 queries, k = 10, groups of 1, 8 and 64 consecutive rows, two corpora --
"gaussian" (unit-norm Gaussian rows, random queries) and "documents" (16 consecutive rows share a document vector, the queries are
documents of the corpus plus noise: the best rows of a query sit in one or two groups) -- and "group_fetch" in {2, 3, 4, 8}:
  device_us    one rq_search_grouped_device call (the exact search for m1 = group_fetch x k rows + the collapse; no repair), between
               its own pair of HIP events;
  total_us     that call followed by rq_search_grouped_fixup_device (host clock around both; the fixup synchronises the stream):
               the time including repairs;
  flagged      queries the device form left unproven, of B: the repair rate; rounds = exclusion rounds of the fixup;
  search_us / search_total_us   the yardstick: rq_search_device with k = m1 on the same index, and with rq_search_fixup_device
               behind it -- the code path a caller over-fetching by hand takes.
Every figure is the median of `--launches` launches after 5 warm-up launches (5 launches where one takes more than 50 ms).
Each corpus is one child process under its own `timeout`, chained with `&&`: the parent never opens the GPU.  `--rocprof DIR` adds a
short run of one corpus under `rocprofv3 --kernel-trace --stats` (the collapse kernel's own time), in a process of its own.

    python tools/gpu_grouped.py --out profiles/grouped_fetch.json [--rows 1000000] [--launches 25] [--rocprof profiles/grouped_rocprof]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--launches", type=int, default=25)
ap.add_argument("--step", default="", help="(child) the corpus to measure: gaussian or documents")
ap.add_argument("--fetch", default="2,3,4,8")
ap.add_argument("--sizes", default="1,8,64")
ap.add_argument("--step-timeout", type=int, default=420)
ap.add_argument("--rocprof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of a short gaussian step")
args = ap.parse_args()
B, K = 64, 10


def parent():
    """One child per corpus, each under its own timeout, chained with &&; then the parts are merged."""
    me = os.path.abspath(__file__)
    base = args.out or os.path.join(os.getcwd(), "grouped_fetch.json")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    common = f"--rows {args.rows} --dim {args.dim} --launches {args.launches} --fetch {args.fetch} --sizes {args.sizes}"
    steps = []
    for corpus in ("gaussian", "documents"):
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --step {corpus} {common} --out {base}.{corpus}.part")
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        steps.append(f"timeout -k 10 {args.step_timeout} rocprofv3 --kernel-trace --stats --output-format csv -d {args.rocprof} -- {sys.executable} {me} --step gaussian "
                     f"--rows {args.rows} --dim {args.dim} --launches 20 --fetch 4 --sizes 8 --out {base}.rocprof.part")
    rc = subprocess.run(" && ".join(steps), shell=True).returncode
    if rc != 0:
        print(f"a step failed (exit status {rc}): nothing further was started", flush=True)
        return rc
    merged = {"rows": args.rows, "dim": args.dim, "B": B, "k": K, "launches": args.launches, "points": []}
    for corpus in ("gaussian", "documents"):
        with open(f"{base}.{corpus}.part") as f:
            part = json.load(f)
        merged["device"] = part["device"]
        merged["points"] += part["points"]
        os.remove(f"{base}.{corpus}.part")
    if args.rocprof and os.path.exists(f"{base}.rocprof.part"):
        os.remove(f"{base}.rocprof.part")
    # the choice: per group size and corpus the cheapest mean time including repairs; overall the multiplier with the lowest mean
    mean = {}
    for p in merged["points"]:
        mean.setdefault(p["group_fetch"], []).append(p["total_us"])
    merged["mean_total_us"] = {str(f): round(sum(v) / len(v), 1) for f, v in sorted(mean.items())}
    merged["choice"] = int(min(mean, key=lambda f: sum(mean[f]) / len(mean[f])))
    print(json.dumps({"mean_total_us": merged["mean_total_us"], "choice": merged["choice"]}), flush=True)
    with open(base, "w") as f:
        json.dump(merged, f, indent=1)
    return 0


def child():
    import numpy as np
    import torch
    from rag_uq_amd import _native as nat
    dev = torch.device("cuda:0")
    N, DIM, corpus = args.rows, args.dim, args.step
    g = torch.Generator(device=dev); g.manual_seed(7)
    idx = nat.NativeIndex(DIM, 0)
    idx.reserve(N)
    docs = torch.randn((N // 16 + 1, DIM), device=dev, generator=g)
    for c in range(0, N, 125_000):
        m = min(125_000, N - c)
        x = torch.randn((m, DIM), device=dev, generator=g)
        if corpus == "documents":
            x = docs[torch.arange(c, c + m, device=dev) // 16] + 0.5 * x
        idx.add_f16_device(torch.nn.functional.normalize(x, dim=1).half().contiguous(), m)
        del x
    idx.set_option("pipeline", 0)
    g.manual_seed(99)
    q = torch.randn((B, DIM), device=dev, generator=g)
    if corpus == "documents":
        q = docs[torch.randint(0, N // 16, (B,), device=dev, generator=g)] + 0.3 * q
    q = q.contiguous()
    sc = torch.empty((B, K), device=dev); rw = torch.empty((B, K), dtype=torch.int64, device=dev); gp = torch.empty((B, K), dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)

    def median(fn, launches):
        out = []
        for _ in range(launches):
            out.append(fn())
        return round(float(np.median(out)), 1), round(float(np.min(out)), 1)

    def events(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def clock(launch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    points = []
    for size in [int(s) for s in args.sizes.split(",")]:
        idx.set_groups((np.arange(N, dtype=np.int64) // size).astype(np.int32))
        for fetch in [int(f) for f in args.fetch.split(",")]:
            idx.set_option("group_fetch", fetch)
            m1 = min(fetch * K, nat.MAX_K)
            dev_call = lambda: idx.search_grouped_device(q, B, K, 0, sc, rw, gp, None, st, 0)
            flagged, rounds = [], []

            def both():
                dev_call()
                flagged.append(idx.search_grouped_fixup_device(q, B, K, 0, sc, rw, gp, None, st, 0))
                rounds.append(int(idx.get_option("group_rounds_last")) if flagged[-1] else 0)
            first = clock(both)                                     # (also the first warm-up launch)
            launches = max(20, args.launches) if first < 50_000 else 5
            for _ in range(4):
                both()
            del flagged[:], rounds[:]
            total = median(lambda: clock(both), launches)
            device = median(lambda: events(dev_call), launches)
            csc = torch.empty((B, m1), device=dev); crw = torch.empty((B, m1), dtype=torch.int64, device=dev)
            search = lambda: idx.search_device(q, B, m1, 0, csc, crw, None, st, 0)
            repaired = []

            def search_both():
                search()
                repaired.append(idx.search_fixup_device(q, B, m1, 0, csc, crw, None, st, 0))
            for _ in range(5):
                search_both()
            del repaired[:]
            s_total = median(lambda: clock(search_both), launches)
            s_device = median(lambda: events(search), launches)
            points.append({"corpus": corpus, "group_size": size, "group_fetch": fetch, "m1": m1, "launches": launches, "device_us": device[0], "device_us_min": device[1],
                           "total_us": total[0], "total_us_min": total[1], "flagged_per_call": round(float(np.mean(flagged)), 2),
                           "repair_rate": round(float(np.mean(flagged)) / B, 4), "rounds_per_call": round(float(np.mean(rounds)), 2),
                           "search_us": s_device[0], "search_total_us": s_total[0], "search_repaired_per_call": round(float(np.mean(repaired)), 2),
                           "overhead_us": round(device[0] - s_device[0], 1)})
            print(json.dumps(points[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "points": points}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(child() if args.step else parent())
