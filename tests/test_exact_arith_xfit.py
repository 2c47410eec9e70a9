"""Exactness of the arithmetic that scores listed extended resources under a
NodeResourcesFit strategy, checked on the CPU by
tools/xfit_check.cpp, which compiles the header the runtime and the kernels
use (k8s-1m_amd/csrc/ksched_fit_shape.hpp):

* one resource's score from its int64 columns, LeastAllocated and
  MostAllocated, requested up to twice the capacity and beyond: capacities
  1..1200 exhaustively, every power of two and 200,000 random ones below 2^44;
* the LeastAllocated / MostAllocated divide by a reciprocal multiply for every
  d <= 1000, n <= 100 d;
* RequestedToCapacityRatio's rounding divide against llround((double)n / d)
  over the same domain;
* the node score as the kernels compose it, for 1..3 extended resources beside
  cpu and memory over a grid of scores that holds 0.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_exact_arith_xfit(tmp_path):
    exe = tmp_path / "xfit_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "k8s-1m_amd" / "csrc"), str(ROOT / "tools" / "xfit_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
