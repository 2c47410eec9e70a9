"""The C-ABI additions of ks_diagnose: ks_reason, ks_diagnosis and the two new
symbols against a compiled probe of include/ksched.h (no GPU: loads and
layouts only); the ABI version stays 6 and ks_result keeps its layout."""
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
  S(ks_reason) O(ks_reason, plugin) O(ks_reason, count) O(ks_reason, reason)
  S(ks_diagnosis) O(ks_diagnosis, num_all_nodes) O(ks_diagnosis, feasible_nodes) O(ks_diagnosis, plugin_nodes)
  O(ks_diagnosis, node_ports_nodes) O(ks_diagnosis, n_reasons) O(ks_diagnosis, prefilter_msg)
  S(ks_result) S(ks_pod)
  printf("KS_NUM_FAIL_COUNTS %d\n", (int)KS_NUM_FAIL_COUNTS);
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
    types = {"ks_reason": _abi.KsReason, "ks_diagnosis": _abi.KsDiagnosis}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(types[t], f).offset == val, key
        elif key in types:
            assert C.sizeof(types[key]) == val, key
    assert got["ks_reason"] == 16 and got["ks_diagnosis"] == 56
    assert got["KS_NUM_FAIL_COUNTS"] == 8 == len(_abi.KsDiagnosis().plugin_nodes)
    assert got["ks_result"] == 64 and got["ks_pod"] == 184 and got["KSCHED_ABI_VERSION"] == 6


def test_new_symbols_exported():
    lib = _abi.ksched_lib()
    for name in ("ks_diagnose", "ks_fit_error_message"):
        assert name in _abi.KSCHED_SYMBOLS and hasattr(lib, name), name
    assert lib.ks_abi_version() == 6
    # a null context is refused before anything else
    assert lib.ks_diagnose(None, None, None, None, 0, None) == _abi.KS_ERR_INVALID
    from ksched import FitDiagnosis, Scheduler
    assert hasattr(Scheduler, "diagnose") and FitDiagnosis.__dataclass_fields__.keys() == {
        "num_all_nodes", "feasible_nodes", "plugin_nodes", "node_ports_nodes", "reasons", "prefilter_msg", "message"}
