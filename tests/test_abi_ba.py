"""ks_set_balanced_resources / ks_get_balanced_resources: the symbols, the
header's declarations, and the argument checks that need no device."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi

ROOT = Path(__file__).resolve().parent.parent

C_PROBE = r"""
#include <stdio.h>
#include "ksched.h"
int main(void) {
  /* the declarations, by their types */
  ks_status (*set)(ks_ctx *, const char *const *, uint32_t) = ks_set_balanced_resources;
  ks_status (*get)(ks_ctx *, const char **, uint32_t, uint32_t *) = ks_get_balanced_resources;
  printf("%d\n", set != 0 && get != 0);
  return 0;
}
"""


def test_header_declares_the_calls(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    obj = tmp_path / "probe.o"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)


def test_symbols_and_null_arguments():
    assert {"ks_set_balanced_resources", "ks_get_balanced_resources"} <= set(_abi.KSCHED_SYMBOLS)
    lib = _abi.ksched_lib()
    names = (C.c_char_p * 3)(b"cpu", b"memory", b"amd.com/gpu")
    n = C.c_uint32()
    assert lib.ks_set_balanced_resources(None, names, 3) == _abi.KS_ERR_INVALID
    assert lib.ks_set_balanced_resources(None, None, 0) == _abi.KS_ERR_INVALID
    assert lib.ks_get_balanced_resources(None, names, 3, C.byref(n)) == _abi.KS_ERR_INVALID
    assert _abi.BALANCED_MAX_RESOURCES == 10
    assert lib.ks_abi_version() == 6  # additive: the version stays
