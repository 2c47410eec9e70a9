"""ks_fit_resource's ctypes mirror against the C header, the new symbols, and
the argument checks of the two calls that need no device."""
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
  printf("size %zu\n", sizeof(ks_fit_resource));
  printf("name %zu\n", offsetof(ks_fit_resource, name));
  printf("weight %zu\n", offsetof(ks_fit_resource, weight));
  printf("_pad %zu\n", offsetof(ks_fit_resource, _pad));
  return 0;
}
"""


def test_fit_resource_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got.pop("size") == C.sizeof(_abi.KsFitResource) == 16
    assert [f for f, _ in _abi.KsFitResource._fields_] == list(got)
    for field, off in got.items():
        assert getattr(_abi.KsFitResource, field).offset == off, field


def test_symbols_and_null_arguments():
    assert {"ks_set_fit_strategy_resources", "ks_get_fit_resources"} <= set(_abi.KSCHED_SYMBOLS)
    lib = _abi.ksched_lib()
    fs = _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, 1, 1, 0)
    res = (_abi.KsFitResource * 1)(_abi.KsFitResource(b"amd.com/gpu", 3, 0))
    n = C.c_uint32()
    assert lib.ks_set_fit_strategy_resources(None, C.byref(fs), None, 0, res, 1) == _abi.KS_ERR_INVALID
    assert lib.ks_get_fit_resources(None, res, 1, C.byref(n)) == _abi.KS_ERR_INVALID
    assert _abi.FIT_MAX_RESOURCES == 8
    assert lib.ks_abi_version() == 6  # additive: the version stays
