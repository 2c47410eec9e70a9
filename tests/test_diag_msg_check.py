"""The host half of ks_diagnose as a stand-alone program (tools/diag_msg_check.cpp
over csrc/ksched_diag.hpp: the DiagRec -> reason rows assembly and FitError's
text, the latter also on 2,000 random histograms against the definition
restated), built with AddressSanitizer + UBSan where the host compiler links
them (plain otherwise) and run on its own: no GPU, nothing loaded into python."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_diag_msg_check(tmp_path):
    exe = tmp_path / "diag_msg_check"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", str(ROOT / "include"), "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
            str(ROOT / "tools" / "diag_msg_check.cpp"), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:  # no sanitizer runtimes to link: the same checks, uninstrumented
        subprocess.run(base, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
