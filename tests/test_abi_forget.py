"""The C-ABI additions of ks_batch_forget: the two new symbols against a
compiled probe of include/ksched.h that links libksched.so (no GPU: a null
context is refused before anything else); the ABI version stays 6 and ks_pod,
ks_result and ks_container keep their sizes."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi

ROOT = Path(__file__).resolve().parent.parent

# The typed pointers make the compiler compare the header's prototypes with the
# signatures the issue declares (-Werror=incompatible-pointer-types); linking
# resolves both symbols in libksched.so; the calls check the null-context rule.
C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
int main(void) {
  ks_status (*forget)(ks_ctx *, ks_batch *, const uint32_t *, uint32_t, uint32_t *) = ks_batch_forget;
  ks_status (*debug)(ks_ctx *, uint64_t[8]) = ks_debug_forget;
  uint64_t out[8];
  uint32_t idx[1] = {0}, skipped = 7;
  printf("forget_null_ctx %d\n", (int)forget(NULL, NULL, idx, 1, &skipped));
  printf("debug_null_ctx %d\n", (int)debug(NULL, out));
  printf("KS_ERR_INVALID %d\n", (int)KS_ERR_INVALID);
  printf("ks_pod %zu\n", sizeof(ks_pod));
  printf("ks_result %zu\n", sizeof(ks_result));
  printf("ks_container %zu\n", sizeof(ks_container));
  printf("KSCHED_ABI_VERSION %d\n", (int)KSCHED_ABI_VERSION);
  printf("ks_abi_version %d\n", (int)ks_abi_version());
  return 0;
}
"""


def probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    libdir = str(_abi.KSCHED_DIR)
    subprocess.run(["gcc", "-Wall", "-Werror=incompatible-pointer-types", "-I", str(ROOT / "include"), str(src), "-o",
                    str(exe), "-L", libdir, "-lksched", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in lines if line)}


def test_symbols_link_with_declared_signatures(tmp_path):
    got = probe(tmp_path)
    assert got["forget_null_ctx"] == got["KS_ERR_INVALID"] == _abi.KS_ERR_INVALID
    assert got["debug_null_ctx"] == got["KS_ERR_INVALID"]
    assert got["KSCHED_ABI_VERSION"] == 6 and got["ks_abi_version"] == 6
    assert got["ks_pod"] == 184 == C.sizeof(_abi.KsPod)
    assert got["ks_result"] == 64 == C.sizeof(_abi.KsResult)
    assert got["ks_container"] == 64 == C.sizeof(_abi.KsContainer)


def test_python_prototypes_match():
    lib = _abi.ksched_lib()
    P, vp = C.POINTER, C.c_void_p
    for name in ("ks_batch_forget", "ks_debug_forget"):
        assert name in _abi.KSCHED_SYMBOLS and hasattr(lib, name), name
    assert lib.ks_batch_forget.argtypes == [vp, vp, P(C.c_uint32), C.c_uint32, P(C.c_uint32)]
    assert lib.ks_debug_forget.argtypes == [vp, P(C.c_uint64)]
    assert lib.ks_abi_version() == 6
    assert lib.ks_batch_forget(None, None, None, 0, None) == _abi.KS_ERR_INVALID
    assert lib.ks_debug_forget(None, None) == _abi.KS_ERR_INVALID
    from ksched import Scheduler
    assert hasattr(Scheduler, "forget") and hasattr(Scheduler, "forget_counters")
