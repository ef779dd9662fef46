"""Range searches (include/rq.h rq_search_range_device) at bench scale: what the scan route costs as the number of
qualifying rows grows, beside what a caller has without it.

On rows built on the device (default 1M x 768, Gaussian, unit norm), B = 64 Gaussian queries, cap in {10, 1024}, in one process on
one index, the GPU otherwise idle:
  range_us     one rq_search_range_device call with "range_route" = 1 (query preparation + the scan pass + the range tail + the final
               select; no repair) at thresholds that about 0, 10, 1 000 and 100 000 rows per query clear;
  exact_us     the same call with "range_route" = 3 (the fp64 scan of the shard), at the 1 000-row threshold;
  topk_us      rq_search_device with k = cap over the fp16 rows ("scan8" = 0) and with the library's default ("scan8" = 1): what a
               caller does today -- fetch k rows, cut the list on the host -- which answers the question only while count <= cap.
Every figure is the median of `--launches` (default 25, at least 20) single launches, each between its own pair of HIP events, after
5 warm-up launches.  The thresholds are midpoints between neighbouring fp32 scores of a torch matrix product, so the counts the
library returns (exact) differ from the targets by a row or two: both are reported, with the (query, bin) pairs the tail re-scored
and how many queries overflowed their candidate list (status 1: rq_search_range_fixup_device would re-run them on the exact route).

    python tools/gpu_range.py --out profiles/range_routes.json [--rows 1000000] [--launches 25]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rag_uq_amd import _native as nat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--launches", type=int, default=25)
args = ap.parse_args()
dev = torch.device("cuda:0")
N, DIM, LAUNCHES, B = args.rows, args.dim, max(20, args.launches), 64
CAPS = [10, 1024]
TARGETS = [0, 10, 1_000, 100_000]


def build(q_unit):
    """The index and the fp32 score matrix [B][N] of the unit queries against the stored fp16 rows (for the thresholds only)."""
    idx = nat.NativeIndex(DIM, 0)
    idx.reserve(N)
    g = torch.Generator(device=dev); g.manual_seed(DIM)
    scores = torch.empty((B, N), device=dev)
    for lo in range(0, N, 125_000):
        m = min(125_000, N - lo)
        x = torch.nn.functional.normalize(torch.randn((m, DIM), device=dev, generator=g), dim=1).half().contiguous()
        idx.add_f16_device(x, m)
        xf = x.float()
        scores[:, lo:lo + m] = (q_unit @ xf.T) / xf.norm(dim=1)[None, :]
        del x, xf
    idx.set_option("pipeline", 0)
    return idx, scores


def median_us(launch):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(LAUNCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(float(np.median(out)), 1), round(float(np.min(out)), 1)


def main():
    g = torch.Generator(device=dev); g.manual_seed(4321)
    q = torch.randn((B, DIM), device=dev, generator=g)
    idx, scores = build(torch.nn.functional.normalize(q, dim=1))
    srt = torch.sort(scores, dim=1, descending=True).values[:, :max(TARGETS) + 1].double().cpu().numpy()
    del scores
    rows = []
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int64, device=dev)
    for cap in CAPS:
        sc = torch.empty((B, cap), device=dev)
        rw = torch.empty((B, cap), dtype=torch.int64, device=dev)
        for scan8 in (0, 1):
            idx.set_option("scan8", scan8)
            search = lambda: idx.search_device(q, B, cap, 0, sc, rw, None, st, 0)
            used0 = int(idx.get_option("scan8_used"))
            med, best = median_us(search)
            rows.append({"case": "topk", "cap": cap, "scan8": scan8, "scan8_used": int(idx.get_option("scan8_used")) > used0, "us_median": med, "us_min": best,
                         "uncertified": int(st.count_nonzero().item())})
            print(rows[-1], flush=True)
        idx.set_option("scan8", 1)
        for target in TARGETS:
            thr_h = (srt[:, 0] + 1e-3) if target == 0 else (srt[:, target - 1] + srt[:, target]) / 2
            thr = torch.from_numpy(thr_h.astype(np.float32)).to(dev)
            for route in ((1, 3) if target == 1_000 else (1,)):
                idx.set_option("range_route", route)
                call = lambda: idx.search_range_device(q, B, thr, cap, 0, sc, rw, None, cnt, st, 0)
                med, best = median_us(call)
                took = int(idx.get_option("range_route_last"))
                bins = int(idx.get_option("range_bins_last"))
                c = cnt.cpu().numpy()
                rows.append({"case": "range", "route": took, "cap": cap, "target": target, "count_median": int(np.median(c)), "count_min": int(c.min()),
                             "count_max": int(c.max()), "us_median": med, "us_min": best, "bins_rescored": bins, "bins_total": B * ((N + 63) // 64),
                             "overflowed": int(st.count_nonzero().item())})
                print(rows[-1], flush=True)
            idx.set_option("range_route", -1)
    out = {"rows": N, "dim": DIM, "B": B, "launches": LAUNCHES, "device": torch.cuda.get_device_name(0), "points": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
