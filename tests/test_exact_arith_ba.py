"""Exactness of the arithmetic that scores NodeResourcesBalancedAllocation over
a list of resources, checked on the CPU by
tools/ba_check.cpp, which compiles the header the runtime and the kernels use
(k8s-1m_amd/csrc/ksched_ba.hpp) and compares its sequence -- the reciprocal,
div_rn, the divides by n -- with plain `/` and sqrt:

* a scalar resource's fraction from its int64 columns: Allocatable 1..1200
  exhaustively with requested up to twice that, every power of two and 200,000
  random values below 2^44;
* x / n for n = 3..10 over the sums the grids reach and 2,000,000 random
  doubles;
* the node score over every grid of 3 and of 4 fractions k/c for c <= 12, over
  all-equal fractions for c <= 64 and n = 3..10, over 1,000,000 random lists,
  and the known answers.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_exact_arith_ba(tmp_path):
    exe = tmp_path / "ba_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
                    str(ROOT / "tools" / "ba_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
