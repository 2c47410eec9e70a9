"""The resource-only sweep's batched wave list, checked on the
host: tools/wavelist_check.cpp runs the per-lane fold and the tuple merge the
kernel uses (ksched_dev.hpp wl_fold / wl_merge / wl_entry) at every segment
width against the sequential definition of a wave's list -- the largest
second best, then the lane bests above it picked one at a time -- over all-zero
waves, one to three candidates, the two best keys in one lane, ties at 0, keys
at the 31-bit top and two million seeded random waves.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_wavelist_check(tmp_path):
    exe = tmp_path / "wavelist_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "include"), "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
                    str(ROOT / "tools" / "wavelist_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
