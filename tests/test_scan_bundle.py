"""Bundles of scanned-ahead calls (option "scan_bundle", csrc/rq_bundle_plan.h) without a device: the host plan under the
sanitizers, and what the header and the option table say.  The GPU scenarios are tests/test_gpu_scan_bundle.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-rag-with-learned-retrieval-and-uncertainty-quantification_amd")
CSRC = os.path.join(PKG, "csrc")


def test_bundle_plan_on_the_host(tmp_path):
    """tests/native/bundle_plan_check.cpp: every event sequence up to length 12 through the plan and a model of its executor -- a
    stand-alone host program under the address and UB sanitizers (host code only, no Python in the process)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "bundle_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(os.path.dirname(__file__), "native", "bundle_plan_check.cpp"), "-o", exe],
                   check=True, timeout=600, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert out.returncode == 0 and "\n0 failures" in "\n" + out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    assert "17039360 sequences" in out.stdout          # 4^12 with bundles of four + 4^9 with pairs only


def test_plan_header_is_host_only():
    src = open(os.path.join(CSRC, "rq_bundle_plan.h")).read()
    assert "#include" not in src and "hipStream" not in src and "hipError" not in src and "__global__" not in src


def test_header_documents_the_option_and_the_deferral():
    rq_h = " ".join(open(os.path.join(ROOT, "include", "rq.h")).read().split())
    for needle in ("scan_bundle", "bundles4", "up to three calls"):
        assert needle in rq_h, needle


def test_option_is_read_and_written_by_the_option_calls():
    api = open(os.path.join(CSRC, "rq_api.hip")).read()
    assert 's == "scan_bundle"' in api and "scan_bundle must be 2 or 4" in api and 's == "bundles4"' in api
