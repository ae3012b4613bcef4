"""CPU check of the vocoders' chunk planner (csrc/chunk_plan.h: plan_chunks, dense_chunk) against the loops of the two ragged entry
points it replaced: compiled for the HOST with hipcc, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_planner_matches_the_loops_it_replaced(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "chunk_plan_check")
    src = os.path.join(ROOT, "tests", "host", "chunk_plan_check.cpp")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
