"""Group members (include/rq.h rq_search_group_members_device) at bench scale: what the fill costs on top of the grouped
search, and what building the member table costs.

On rows built on the device (default 1M x 768), B = 64 queries, k = 10, s in {1, 3, 8}, three settings -- "gaussian" rows (unit-norm
Gaussian rows, random queries) in groups of 8 and of 64 consecutive rows, and the "documents" corpus of tools/gpu_grouped.py (16
consecutive rows share a document vector and a group, the queries are documents of the corpus plus noise):
  members_us   one rq_search_group_members_device call (the grouped search, then the fill; no repair) between its own pair of HIP
               events;
  grouped_us   the yardstick: rq_search_grouped_device with the same k on the same index -- the code path before this call existed;
  overhead_us  their difference: the fill's launch, its query preparation and its row reads;
  fill_rows    members the last fill scored (option "group_fill_rows_last"), fill_bytes = fill_rows x 2 x row length;
  flagged      queries the device form left for the fixup, per call;
  table_build_ms   host clock around the first call after rq_index_set_groups minus the median later call: the host sort and the
               three uploads of the member table.
Every figure is the median of `--launches` launches after 5 warm-up launches.  Each setting is one child process under its own
`timeout`, chained with `&&`: the parent never opens the GPU.  `--rocprof DIR` adds a short run of one setting under
`rocprofv3 --kernel-trace --stats` (the fill kernel's own time), in a process of its own.

    python tools/gpu_group_members.py --out profiles/group_members.json [--rows 1000000] [--launches 25] [--rocprof profiles/group_members_rocprof]
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
ap.add_argument("--step", default="", help="(child) the setting to measure: groups8, groups64 or documents")
ap.add_argument("--sizes", default="1,3,8", help="the group sizes s")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--rocprof", default="", help="directory for a rocprofv3 --kernel-trace --stats run of a short groups8 step")
args = ap.parse_args()
B, K = 64, 10
SETTINGS = ("groups8", "groups64", "documents")


def parent():
    """One child per setting, each under its own timeout, chained with &&; then the parts are merged."""
    me = os.path.abspath(__file__)
    base = args.out or os.path.join(os.getcwd(), "group_members.json")
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    common = f"--rows {args.rows} --dim {args.dim} --launches {args.launches} --sizes {args.sizes}"
    steps = [f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --step {name} {common} --out {base}.{name}.part" for name in SETTINGS]
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        steps.append(f"timeout -k 10 {args.step_timeout} rocprofv3 --kernel-trace --stats --output-format csv -d {args.rocprof} -- {sys.executable} {me} --step groups8 "
                     f"--rows {args.rows} --dim {args.dim} --launches 20 --sizes 3 --out {base}.rocprof.part")
    rc = subprocess.run(" && ".join(steps), shell=True).returncode
    if rc != 0:
        print(f"a step failed (exit status {rc}): nothing further was started", flush=True)
        return rc
    merged = {"rows": args.rows, "dim": args.dim, "B": B, "k": K, "launches": args.launches, "points": []}
    for name in SETTINGS:
        with open(f"{base}.{name}.part") as f:
            part = json.load(f)
        merged["device"] = part["device"]
        merged["points"] += part["points"]
        os.remove(f"{base}.{name}.part")
    if args.rocprof and os.path.exists(f"{base}.rocprof.part"):
        os.remove(f"{base}.rocprof.part")
    with open(base, "w") as f:
        json.dump(merged, f, indent=1)
    return 0


def child():
    import numpy as np
    import torch
    from rag_uq_amd import _native as nat
    dev = torch.device("cuda:0")
    N, DIM, setting = args.rows, args.dim, args.step
    g = torch.Generator(device=dev); g.manual_seed(7)
    idx = nat.NativeIndex(DIM, 0)
    idx.reserve(N)
    docs = torch.randn((N // 16 + 1, DIM), device=dev, generator=g)
    for c in range(0, N, 125_000):
        m = min(125_000, N - c)
        x = torch.randn((m, DIM), device=dev, generator=g)
        if setting == "documents":
            x = docs[torch.arange(c, c + m, device=dev) // 16] + 0.5 * x
        idx.add_f16_device(torch.nn.functional.normalize(x, dim=1).half().contiguous(), m)
        del x
    idx.set_option("pipeline", 0)
    g.manual_seed(99)
    q = torch.randn((B, DIM), device=dev, generator=g)
    if setting == "documents":
        q = docs[torch.randint(0, N // 16, (B,), device=dev, generator=g)] + 0.3 * q
    q = q.contiguous()
    group_rows = {"groups8": 8, "groups64": 64, "documents": 16}[setting]
    ids = (np.arange(N, dtype=np.int64) // group_rows).astype(np.int32)
    gsc = torch.empty((B, K), device=dev); grw = torch.empty((B, K), dtype=torch.int64, device=dev)
    gp = torch.empty((B, K), dtype=torch.int32, device=dev); cnt = torch.empty((B, K), dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)

    def median(fn, launches):
        out = [fn() for _ in range(launches)]
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

    grouped = lambda: idx.search_grouped_device(q, B, K, 0, gsc, grw, gp, None, st, 0)
    points = []
    for s in [int(v) for v in args.sizes.split(",")]:
        sc = torch.empty((B, K, s), device=dev); rw = torch.empty((B, K, s), dtype=torch.int64, device=dev)
        members = lambda: idx.search_group_members_device(q, B, K, s, 0, sc, rw, gp, cnt, st, 0)
        idx.set_groups(ids)                                     # drops the member table: the next call builds it
        builds = int(idx.get_option("group_table_builds"))
        first_us = clock(members)
        assert int(idx.get_option("group_table_builds")) == builds + 1
        flagged = []
        for _ in range(5):
            members()
            flagged.append(idx.search_group_members_fixup_device(q, B, K, s, 0, sc, rw, gp, cnt, st, 0))
            grouped()
        wall = median(lambda: clock(members), args.launches)
        m_us = median(lambda: events(members), args.launches)
        g_us = median(lambda: events(grouped), args.launches)
        members()
        fill_rows = int(idx.get_option("group_fill_rows_last"))
        points.append({"setting": setting, "group_rows": group_rows, "s": s, "launches": args.launches, "members_us": m_us[0], "members_us_min": m_us[1],
                       "grouped_us": g_us[0], "grouped_us_min": g_us[1], "overhead_us": round(m_us[0] - g_us[0], 1), "fill_rows": fill_rows,
                       "fill_bytes": fill_rows * 2 * int(idx.get_option("row_pad")), "flagged_per_call": round(float(np.mean(flagged)), 2),
                       "table_build_ms": round((first_us - wall[0]) / 1e3, 2), "table_groups": int(N // group_rows), "table_rows": N})
        print(json.dumps(points[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "points": points}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(child() if args.step else parent())
