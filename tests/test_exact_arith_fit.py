"""Exactness of the general NodeResourcesFit scorer,
checked on the host with the binary64 operation sequence the kernels use:

* tools/fit_check.cpp: MostAllocated min(req, cap) * 100 / cap as the
  truncation of fma(min(cap100 - x, cap100), RN(1/cap), 2^-45), exhaustively on
  small capacities, next to every integer quotient on random capacities up to
  2^44 and beyond capacity (the clamp); LeastAllocated's 0 for requested >
  capacity through the unsigned conversion; and the weighted division
  floor(n / d) by a reciprocal multiply for every n <= 20000, d <= 200.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_exact_arith_fit(tmp_path):
    exe = tmp_path / "fit_check"
    subprocess.run(["g++", "-O2", "-mfma", "-ffp-contract=off", str(ROOT / "tools" / "fit_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
