"""tests/route_shapes.py -- the Python restatement of nb_default, the exact rule and the pass cutting that the GPU tests of the
scanned routes rely on -- against plan_call of csrc/rq_plan.h itself, run on the host by tests/native/plan_check.cpp.  Either side
changing without the other fails here, without a GPU."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_shapes as rs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "efficient-rag-with-learned-retrieval-and-uncertainty-quantification_amd", "csrc")


def test_the_shapes_are_what_the_gpu_tests_say_they_are():
    """Worked out by hand from the three rules, independent of the helper's own arithmetic."""
    assert rs.nbins(12_805) == 201 and 12_805 % 64 != 0 and rs.nbins(49_157) == 769 and 49_157 % 64 != 0
    assert rs.nb_default(80) == 90 and rs.nb_default(64) == 72 and rs.nb_default(330) == 371 and rs.nb_default(10) == 18
    assert not rs.is_exact(12_805, 80) and not rs.is_exact(12_805, 89) and rs.is_exact(12_805, 90)      # 180 < 201; m = 90: nb = 101, 202 >= 201
    assert not rs.is_exact(49_157, 330) and not rs.is_exact(49_157, 342) and rs.is_exact(49_157, 343)   # 742 < 769; m = 343: nb = 385, 770 >= 769
    assert rs.is_exact(4101, 25) and not rs.is_exact(4101, 24)              # the shape of the older suites: exact from m = 25 on
    assert rs.passes(130) == [256] and rs.passes(300) == [256, 64] and rs.passes(16) == [64] and rs.passes(70) == [128]
    assert rs.passes(200, narrow=True) == [128, 128] and rs.passes(130, image=True) == [256] and rs.passes(300, image=True) == [256, 64]
    # one partition maximum per workgroup of the wide grid (256): the fast tail serves a 256-query pass up to m = 256, 64 queries up to 320
    assert rs.wide_grid(49_157) == 256 and rs.wide_grid(12_805) == 201
    assert rs.shape_plan("S2", 130, 256).fast and not rs.shape_plan("S2", 130, 257).fast and not rs.shape_plan("S2", 130, 320).fast
    assert rs.shape_plan("S2", 64, 320).fast and not rs.shape_plan("S2", 130, 330).fast and not rs.shape_plan("S2", 130, 330).exact
    assert rs.plan(49_157, 200, 320, narrow=True).fast                      # rows of 384 elements: no wide grid
    assert rs.uses_image("S1i", 130, 64) and rs.uses_image("S1i", 300, 80) and not rs.uses_image("S1i", 130, 80, filtered=True) and not rs.uses_image("S1", 130, 64)
    assert rs.image_wanted(49_157, 320) and not rs.image_wanted(49_157, 321) and not rs.image_wanted(12_805, 90)
    assert rs.plan(49_157, 130, 320, image=True).fast                       # the image is read by the fast tail only
    for name, B, m in rs.FETCHES:
        p = rs.shape_plan(name, B, m)
        assert not p.exact and sum(p.pass_q) >= B > sum(p.pass_q[:-1]), (name, B, m)


def _shapes():
    """The fetches of the GPU tests, and a sweep around every edge of the three rules: batches on both sides of 64 / 128 / 256 and
    their sums, m on both sides of the exact rule of each shard, of the fast tail's range and of the wide grid's workgroups."""
    out = set()
    for name, B, m in rs.FETCHES:
        sh = rs.SHAPES[name]
        for filtered in (False, True):
            out.add((sh.rows, sh.row_pad, B, m, int(rs.uses_image(name, B, m, filtered))))
    batches = [1, 63, 64, 65, 127, 128, 129, 130, 192, 193, 200, 255, 256, 257, 300, 320, 321, 384, 385, 512, 513, 700]
    for rows in (2304, 2305, 4101, 12_805, 49_157, 1 << 20):
        edge = [m for m in range(1, 1025) if rs.is_exact(rows, m) != rs.is_exact(rows, m + 1)]
        for m in sorted({1, 7, 8, 10, 63, 64, 65, 80, 200, 201, 202, 255, 256, 257, 320, 321, 330, 1024, *edge, *(e + 1 for e in edge)}):
            for dpad in (768, 384):
                out.update((rows, dpad, B, m, 0) for B in batches)
            if rs.image_wanted(rows, m):
                out.update((rows, 768, B, m, 1) for B in batches)
    return sorted(out)


def test_the_python_rules_agree_with_plan_call_on_every_shape(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    shapes = _shapes()
    assert any(s[1] == 384 and s[2] == 200 for s in shapes) and any(s[4] == 1 and s[2] == 300 for s in shapes)
    lines = []
    for at in range(0, len(shapes), 500):
        out = subprocess.run([exe, "plan", *(":".join(map(str, s)) for s in shapes[at:at + 500])], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines += out.stdout.splitlines()
    assert len(lines) == len(shapes)
    wrong = []
    for s, line in zip(shapes, lines):
        rows, dpad, B, m, use8 = s
        p = rs.plan(rows, B, m, narrow=dpad == 384, image=bool(use8))
        wanted8 = int(dpad == 768 and rs.image_wanted(rows, m))
        want = f"{rows} {dpad} {B} {m} {use8} {int(p.exact)} {int(p.fast)} {p.nb} {p.npass} {','.join(map(str, p.pass_q))} {wanted8}"
        if line.strip() != want:
            wrong.append(f"plan_call: {line.strip()}   route_shapes: {want}")
    assert not wrong, f"{len(wrong)} of {len(shapes)} shapes differ (rows dpad B m use8 exact fast nb npass passes wanted8):\n" + "\n".join(wrong[:20])
