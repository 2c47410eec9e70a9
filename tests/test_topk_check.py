"""ks_explain's selection on the host: tools/topk_check.cpp
runs the staging rank, the flush rule, the pad-and-sort merge and the (best,
count) pairs of csrc/ksched_explain.hpp -- the code the kernels run -- through
both of the kernels' levels against std::partial_sort, over random key sets,
all-equal totals, strictly ascending and descending totals, fewer keys than k,
k = 1 and k = 128, at sizes around the wave, the block and the second grid
stride.  A stand-alone program built with AddressSanitizer + UBSan where the
host compiler links them (plain otherwise): no GPU, nothing loaded into python."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_topk_check(tmp_path):
    exe = tmp_path / "topk_check"
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", str(ROOT / "include"), "-I", str(ROOT / "k8s-1m_amd" / "csrc"),
            str(ROOT / "tools" / "topk_check.cpp"), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:  # no sanitizer runtimes to link: the same checks, uninstrumented
        subprocess.run(base, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches 0" in out.stdout
