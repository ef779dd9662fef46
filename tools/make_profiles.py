"""Condense rocprofv3 outputs under gpurun_out/ into the tracked summaries under profiles/.

    python tools/make_profiles.py r01

expects, in the output directory of tools/run_profiles.sh:
         prof_bench/*/*kernel_stats.csv      rocprofv3 --kernel-trace --stats -- python3 bench.py --full --no-cpu-baseline --no-extra-legs
         pmc_fetch/*/*counter_collection.csv  rocprofv3 --pmc FETCH_SIZE -- python3 bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-extra-legs
         pmc_write/*/*counter_collection.csv  rocprofv3 --pmc WRITE_SIZE -- (same)
"""
import csv, glob, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
out = os.path.join(ROOT, "profiles")
os.makedirs(out, exist_ok=True)

def first(pattern):
    g = sorted(glob.glob(os.path.join(ROOT, "gpurun_out", pattern)), key=os.path.getmtime)
    return g[-1] if g else None

ks = first("prof_bench/*/*kernel_stats.csv")
if ks:
    rows = list(csv.DictReader(open(ks)))
    keep = [r for r in rows if "rq_" in r["Name"]]
    with open(os.path.join(out, f"{tag}_bench_kernel_stats.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(keep)
    print("kernel stats:", [(r["Name"][:40], r["Calls"], round(float(r["AverageNs"]) / 1e3, 1)) for r in keep[:6]])

ks8 = first("prof_bench8/*/*kernel_stats.csv")
if ks8:
    rows = list(csv.DictReader(open(ks8)))
    with open(os.path.join(out, f"{tag}_bench_int8_kernel_stats.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows([r for r in rows if "rq_" in r["Name"]])
    print("int8 run kernel stats:", [(r["Name"][:40], r["Calls"], round(float(r["AverageNs"]) / 1e3, 1)) for r in rows if "rq_" in r["Name"]][:4])

ks1 = first("prof_bench_1s/*/*kernel_stats.csv")
if ks1:
    rows = list(csv.DictReader(open(ks1)))
    with open(os.path.join(out, f"{tag}_bench_single_stream_kernel_stats.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows([r for r in rows if "rq_" in r["Name"]])
    print("single-stream kernel stats:", [(r["Name"][:40], r["Calls"], round(float(r["AverageNs"]) / 1e3, 1)) for r in rows if "rq_" in r["Name"]][:4])
for logname in ("bench2", "bench20", "prof_bench", "prof_bench8", "prof_bench_1s"):
    lp = os.path.join(ROOT, "gpurun_out", logname + ".log")
    if os.path.exists(lp):
        lines = [l for l in open(lp, errors="replace").read().splitlines() if l.startswith('{"metric"')]
        if lines:
            open(os.path.join(out, f"{tag}_{logname}.json"), "w").write(lines[-1] + "\n")
            d = json.loads(lines[-1])
            print(logname, "value", round(d["value"]), "ms/step", round(d["ms_per_step"], 4), "scan avg us", round(d["roofline"]["avg_launch_us"], 1), "frac", round(d["roofline"]["frac"], 3))

# Two instantiations of the fused kernel at 1M rows: rq_scan_tail_kernel<true, 8, 1> (the fp16 rows: bench.py's timed region, `value`, since
# round 3) and <true, 8, 2> (the int8 image: bench.py --scan int8, the `int8_scan` leg of the default run).  Since round 3 each is profiled by
# a run of its own WITHOUT the extra legs (tools/run_profiles.sh: prof_bench / prof_bench8, pmc_*/ pmc_*8), so that the per-kernel averages are
# those of the 1M-row Gaussian loop alone and not mixed with the structured-corpus legs that launch the same kernels.
VARIANTS = (("rq_scan_tail_kernel<true, 8, 2>", "8", 768, "SQ_INSTS_VALU_MFMA_MOPS_I8", "int8 image of the fp16 shard, i8 matrix cores"),
            ("rq_scan_tail_kernel<true, 8, 1>", "", 1536, "SQ_INSTS_VALU_MFMA_MOPS_F16", "fp16 rows, f16 matrix cores"))

def kernel_avg_us(sel):
    src = ks8 if (", 2>" in sel and ks8) else ks        # each operand from the run that timed it alone
    if not src:
        return None
    for r in csv.DictReader(open(src)):
        if sel in r["Name"]:
            return float(r["AverageNs"]) / 1e3
    return None

for sel, suffix, row_bytes, mops, what in VARIANTS:
    mf = first(f"pmc_mfma{suffix}/*/*counter_collection.csv")
    if not mf:
        continue
    acc = {}
    for r in csv.DictReader(open(mf)):
        if sel in r["Kernel_Name"]:
            acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    mean = {k: sum(v) / len(v) for k, v in acc.items()}
    dur_us = kernel_avg_us(sel)
    if mops in mean and dur_us:
        ops = mean[mops] * 512.0        # one MOP = 512 operations (a 16x16x32 f16 / 16x16x64 i8 MFMA = 16384 / 32768 operations)
        algo = 2.0 * 64 * 1_000_000 * 768
        gui = mean.get("GRBM_GUI_ACTIVE", 0.0) / 8.0                # summed over the 8 XCDs
        peak = 2500.0 if row_bytes == 1536 else 5000.0             # dense fp16 TFLOP/s / dense int8 TOP/s (MI355X_MICROARCH.md)
        summ = {"kernel": sel, "workload": f"1000000x768 fp16 corpus ({what}), 64 queries per launch",
                "counters_mean_per_launch": mean, "launches": len(next(iter(acc.values()))),
                "avg_launch_us_from_kernel_stats": dur_us,
                "mfma_ops_per_launch": ops, "algorithmic_ops_per_launch": algo, "ops_over_algorithmic": ops / algo,
                "achieved_Tops": ops / (dur_us * 1e-6) / 1e12, "dense_peak_Tops": peak,
                "mfma_frac_of_peak": ops / (dur_us * 1e-6) / 1e12 / peak,
                "mfma_busy_frac": (mean.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (1024.0 * gui)) if gui else None,
                "note": "SQ_VALU_MFMA_BUSY_CYCLES is summed over the 1024 SIMDs; GRBM_GUI_ACTIVE / 8 = shader cycles of the launch.  The kernel is "
                        "HBM-bound: the matrix cores are the means not to be ALU-bound, not the roofline."}
        json.dump(summ, open(os.path.join(out, f"{tag}_pmc_mfma{suffix}.json"), "w"), indent=1)
        print("mfma", sel, {k: summ[k] for k in ("achieved_Tops", "mfma_frac_of_peak", "mfma_busy_frac", "ops_over_algorithmic")})

for sel, suffix, row_bytes, mops, what in VARIANTS:
    pmc = {}
    for name, counter in (("pmc_fetch", "FETCH_SIZE"), ("pmc_write", "WRITE_SIZE")):
        f = first(f"{name}{suffix}/*/*counter_collection.csv")
        if not f:
            continue
        vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(f)) if r["Counter_Name"] == counter and sel in r["Kernel_Name"]]
        if vals:
            pmc[counter] = {"launches": len(vals), "mean": sum(vals) / len(vals), "min": min(vals), "max": max(vals), "unit": "KiB (rocprofv3 derived counter)"}
    if "FETCH_SIZE" not in pmc:
        continue
    fetch = pmc["FETCH_SIZE"]["mean"] * 1024
    write = pmc.get("WRITE_SIZE", {"mean": 0.0})["mean"] * 1024
    summary = {
        "kernel": sel, "workload": f"1000000x768 fp16 corpus ({what}), 64 queries per launch",
        "counters": pmc,
        "correction": "MI355X_MICROARCH.md 'HBM': on gfx950 FETCH_SIZE reports exactly 1/2 of the bytes of a wide coalesced "
                      "streaming read (16 B/lane, global_load and LDS-DMA alike) -> read bytes = 2 * FETCH_SIZE * 1024; "
                      "WRITE_SIZE is taken as is (the pooled stores are 4..16 B per lane, an uncalibrated width)",
        "hbm_read_bytes_per_launch": 2 * fetch,
        "hbm_write_bytes_per_launch": write,
        "hbm_bytes_per_launch": 2 * fetch + write,
        "algorithmic_bytes_per_launch": 1_000_000 * row_bytes,
    }
    summary["traffic_over_algorithmic"] = summary["hbm_bytes_per_launch"] / summary["algorithmic_bytes_per_launch"]
    json.dump(summary, open(os.path.join(out, f"{tag}_pmc_scan{suffix}.json"), "w"), indent=1)
    print("pmc", sel, {k: summary[k] for k in ("hbm_read_bytes_per_launch", "hbm_write_bytes_per_launch", "traffic_over_algorithmic")})
