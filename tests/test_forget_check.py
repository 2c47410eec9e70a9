"""ks_batch_forget's host bookkeeping as a stand-alone program
(tools/forget_check.cpp over csrc/ksched_forget.hpp: the check of the index
list -- range, order, unscheduled, forgotten already, the first offender --
and the per-batch bitmap at its word edges, on constructed and seeded random
lists against the rules restated), built with AddressSanitizer + UBSan and
run on its own: no GPU, nothing loaded into python.  Where the host compiler
has no sanitizer runtimes to link, the checks run uninstrumented and the test
warns of it; an instrumented build that fails for another reason fails the
test."""
import subprocess
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_forget_check(tmp_path):
    exe = tmp_path / "forget_check"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
            str(ROOT / "tools" / "forget_check.cpp"), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        # Only a host without the sanitizer runtimes may run the checks uninstrumented, and it says so: any
        # other failure of the instrumented build (the program's own code) fails the test.
        missing = any(w in san.stderr for w in ("cannot find -lasan", "cannot find -lubsan", "libasan", "libubsan",
                                                "unrecognized command line option", "unrecognized argument"))
        assert missing, "the AddressSanitizer + UBSan build failed:\n" + san.stderr
        warnings.warn("forget_check ran WITHOUT AddressSanitizer / UBSan: the host compiler does not link them:\n"
                      + san.stderr[-400:])
        subprocess.run(base, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "forget_check: ok" in out.stdout
