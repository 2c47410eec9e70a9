"""The C-ABI additions of ks_diagnose_pods: ks_pod_diagnosis and the two new
symbols against a compiled probe of include/ksched.h (no GPU: loads and
layouts only); the ABI version stays 6 and ks_diagnosis keeps its layout."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi

ROOT = Path(__file__).resolve().parent.parent

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(ks_pod_diagnosis) O(ks_pod_diagnosis, status) O(ks_pod_diagnosis, first_reason) O(ks_pod_diagnosis, d)
  S(ks_diagnosis) S(ks_reason) S(ks_status)
  printf("KSCHED_ABI_VERSION %d\n", (int)KSCHED_ABI_VERSION);
  return 0;
}
"""


def probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in lines if line)}


def test_layouts_match_c(tmp_path):
    got = probe(tmp_path)
    types = {"ks_pod_diagnosis": _abi.KsPodDiagnosis, "ks_diagnosis": _abi.KsDiagnosis, "ks_reason": _abi.KsReason}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(types[t], f).offset == val, key
        elif key in types:
            assert C.sizeof(types[key]) == val, key
    assert got["ks_pod_diagnosis"] == 64 and got["ks_pod_diagnosis.d"] == 8
    assert got["ks_diagnosis"] == 56 and got["ks_reason"] == 16 and got["ks_status"] == 4
    assert got["KSCHED_ABI_VERSION"] == 6


def test_new_symbols_exported():
    lib = _abi.ksched_lib()
    for name in ("ks_diagnose_pods", "ks_debug_diagnose_pods"):
        assert name in _abi.KSCHED_SYMBOLS and hasattr(lib, name), name
    assert lib.ks_abi_version() == 6
    # a null context is refused before anything else
    assert lib.ks_diagnose_pods(None, None, 0, None, None, 0, None) == _abi.KS_ERR_INVALID
    assert lib.ks_debug_diagnose_pods(None, None) == _abi.KS_ERR_INVALID
    from ksched import Scheduler
    assert hasattr(Scheduler, "diagnose_many") and hasattr(Scheduler, "diagnose_pods_counters")
