"""bench.py's command line: a plain run times exactly --steps steps and stops after the headline line (the other legs are behind
--full); --dump-outputs writes what the timed path returned in its last step, which is the exact top-k of that batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
PY = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])


def test_bench_options_and_step_count_check():
    """(argument parsing runs before torch is imported: no GPU needed)"""
    h = subprocess.run(PY + [BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    z = subprocess.run(PY + [BENCH, "--gpus", "1", "--steps", "0", "--warmup", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert z.returncode != 0 and "--steps must be at least 1" in z.stderr


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_timed_step(tmp_path):
    import torch
    from oracle import dense_oracle as orc
    rows, steps, out = 250_000, 21, tmp_path / "out"
    p = subprocess.run(PY + [BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--rows", str(rows), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["steps"] == steps and d["warmup"] == 2 and d["n_gpus"] == 1 and d["dtype"] == "f16"
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and "queries/sec" in d["metric"]
    assert abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["roofline"]["launches"] > 0 and "isolated" not in d["roofline"]
    for key in ("timed_path_vs_exact_fp64_scan", "int8_scan", "k100", "host_api", "cpu_baseline", "ids_exact", "structured"):
        assert key not in d, key                                        # --full only
    scores, got = np.load(out / "scores.npy"), np.load(out / "rows.npy")
    assert scores.dtype == np.float32 and got.dtype == np.float64 and scores.shape == got.shape == (64, 10)
    # bench.py's seeded inputs: corpus chunk c of 125 000 rows from seed 1235 + c, 16 query batches from seed 4321, step i searches batch i % 16
    dev = torch.device("cuda", 0)
    chunks = []
    for c, lo in enumerate(range(0, rows, 125_000)):
        g = torch.Generator(device=dev)
        g.manual_seed(1235 + c)
        x = torch.randn((min(125_000, rows - lo), 768), device=dev, generator=g, dtype=torch.float32)
        chunks.append(torch.nn.functional.normalize(x, dim=1).half().cpu().numpy())
    gq = torch.Generator(device=dev)
    gq.manual_seed(4321)
    queries = [torch.randn((64, 768), device=dev, generator=gq, dtype=torch.float32) for _ in range(16)]
    gs, gr = orc.dense_topk(queries[(steps - 1) % 16].cpu().numpy(), np.concatenate(chunks), 10)
    assert np.array_equal(got, gr.astype(np.float64))
    assert float(np.abs(scores - gs).max()) <= 1e-6
