"""The C-ABI additions of ks_capacity: the three new symbols against a compiled
probe of include/ksched.h that links libksched.so (no GPU: a null context is
refused before anything else); the struct layouts the Python mirror declares;
the ABI version stays 6 and ks_pod keeps its size.  tools/capacity_check.cpp,
the exact quotient against 128-bit division under ASan + UBSan, runs here too."""
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
  ks_status (*one)(ks_ctx *, const ks_pod *, ks_capacity *, uint32_t *) = ks_capacity_pod;
  ks_status (*many)(ks_ctx *, const ks_pod *, uint32_t, ks_pod_capacity *) = ks_capacity_pods;
  ks_status (*debug)(ks_ctx *, uint64_t[8]) = ks_debug_capacity;
  uint64_t out[8];
  ks_capacity c;
  printf("one_null_ctx %d\n", (int)one(NULL, NULL, &c, NULL));
  printf("many_null_ctx %d\n", (int)many(NULL, NULL, 0, NULL));
  printf("debug_null_ctx %d\n", (int)debug(NULL, out));
  printf("KS_ERR_INVALID %d\n", (int)KS_ERR_INVALID);
  printf("ks_capacity %zu\n", sizeof(ks_capacity));
  printf("ks_pod_capacity %zu\n", sizeof(ks_pod_capacity));
  printf("off_replicas %zu\n", offsetof(ks_capacity, replicas));
  printf("off_bound_by %zu\n", offsetof(ks_capacity, bound_by));
  printf("off_x_names %zu\n", offsetof(ks_capacity, x_names));
  printf("off_c %zu\n", offsetof(ks_pod_capacity, c));
  printf("KS_CAP_PORTS %d\n", (int)KS_CAP_PORTS);
  printf("KS_CAP_X %d\n", (int)KS_CAP_X);
  printf("KS_CAP_BOUNDS %d\n", (int)KS_CAP_BOUNDS);
  printf("ks_pod %zu\n", sizeof(ks_pod));
  printf("KSCHED_ABI_VERSION %d\n", (int)KSCHED_ABI_VERSION);
  printf("ks_abi_version %d\n", (int)ks_abi_version());
  return 0;
}
"""


def test_symbols_link_with_declared_signatures(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    libdir = str(_abi.KSCHED_DIR)
    subprocess.run(["gcc", "-Wall", "-Werror=incompatible-pointer-types", "-I", str(ROOT / "include"), str(src), "-o",
                    str(exe), "-L", libdir, "-lksched", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in lines if line)}
    assert got["one_null_ctx"] == got["many_null_ctx"] == got["debug_null_ctx"] == got["KS_ERR_INVALID"]
    assert got["ks_capacity"] == C.sizeof(_abi.KsCapacity) == 136
    assert got["ks_pod_capacity"] == C.sizeof(_abi.KsPodCapacity) == 144
    assert got["off_replicas"] == _abi.KsCapacity.replicas.offset and got["off_bound_by"] == _abi.KsCapacity.bound_by.offset
    assert got["off_x_names"] == _abi.KsCapacity.x_names.offset and got["off_c"] == _abi.KsPodCapacity.c.offset
    assert (got["KS_CAP_PORTS"], got["KS_CAP_X"], got["KS_CAP_BOUNDS"]) == (_abi.CAP_PORTS, _abi.CAP_X, _abi.CAP_BOUNDS)
    assert got["KSCHED_ABI_VERSION"] == 6 and got["ks_abi_version"] == 6
    assert got["ks_pod"] == 184 == C.sizeof(_abi.KsPod)


def test_python_prototypes_match():
    lib = _abi.ksched_lib()
    P, vp = C.POINTER, C.c_void_p
    for name in ("ks_capacity_pod", "ks_capacity_pods", "ks_debug_capacity"):
        assert name in _abi.KSCHED_SYMBOLS and hasattr(lib, name), name
    assert lib.ks_capacity_pod.argtypes == [vp, P(_abi.KsPod), P(_abi.KsCapacity), P(C.c_uint32)]
    assert lib.ks_capacity_pods.argtypes == [vp, P(_abi.KsPod), C.c_uint32, P(_abi.KsPodCapacity)]
    assert lib.ks_capacity_pods(None, None, 0, None) == _abi.KS_ERR_INVALID
    assert lib.ks_debug_capacity(None, None) == _abi.KS_ERR_INVALID
    from ksched import Scheduler
    assert hasattr(Scheduler, "capacity_many") and hasattr(Scheduler, "capacity_counters")


def test_exact_quotient_under_sanitizers(tmp_path):
    exe = tmp_path / "capacity_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "k8s-1m_amd" / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tools" / "capacity_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 wrong" in p.stdout, p.stdout
