"""Exactness of RequestedToCapacityRatio's host and device arithmetic
(DESIGN.md §4, §5.10), checked on the CPU by tools/rtcr_check.cpp, which
compiles the header the runtime and the kernels use
(k8s-1m_amd/csrc/ksched_fit_shape.hpp):

* the shape table against an int64 transcription of the broken-linear function
  for every two-point shape and 400,000 random shapes of 1..8 points;
* the rounding divide floor((2n + d) / (2d)) by a reciprocal multiply against
  llround((double)n / d) for every d <= 200, n <= 100 d;
* the node score as the kernel writes it against integer arithmetic, with
  zero and masked resource scores.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_exact_arith_rtcr(tmp_path):
    exe = tmp_path / "rtcr_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "include"), "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
                    str(ROOT / "tools" / "rtcr_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
