"""ks_fit_strategy's ctypes mirror against the C header (tests/test_abi.py
checks the symbols; its layout probe lists its structs by name, so this one
is probed here), and the strategy calls' argument checks that need no device."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi

ROOT = Path(__file__).resolve().parent.parent

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
int main(void) {
  printf("size %zu\n", sizeof(ks_fit_strategy));
  printf("type %zu\n", offsetof(ks_fit_strategy, type));
  printf("weight_cpu %zu\n", offsetof(ks_fit_strategy, weight_cpu));
  printf("weight_memory %zu\n", offsetof(ks_fit_strategy, weight_memory));
  printf("_pad %zu\n", offsetof(ks_fit_strategy, _pad));
  printf("LEAST %d\n", (int)KS_FIT_LEAST_ALLOCATED);
  printf("MOST %d\n", (int)KS_FIT_MOST_ALLOCATED);
  return 0;
}
"""


def test_fit_strategy_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got.pop("size") == C.sizeof(_abi.KsFitStrategy) == 16
    assert got.pop("LEAST") == _abi.FIT_LEAST_ALLOCATED == _abi.FIT_TYPES["LeastAllocated"]
    assert got.pop("MOST") == _abi.FIT_MOST_ALLOCATED == _abi.FIT_TYPES["MostAllocated"]
    assert [f for f, _ in _abi.KsFitStrategy._fields_] == list(got)
    for field, off in got.items():
        assert getattr(_abi.KsFitStrategy, field).offset == off, field


def test_fit_strategy_calls_reject_null_arguments():
    lib = _abi.ksched_lib()
    fs = _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, 1, 1, 0)
    assert lib.ks_set_fit_strategy(None, C.byref(fs)) == _abi.KS_ERR_INVALID
    assert lib.ks_get_fit_strategy(None, C.byref(fs)) == _abi.KS_ERR_INVALID
    assert lib.ks_abi_version() == 6
