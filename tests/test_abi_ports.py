"""The C-ABI additions of NodePorts: ks_host_port, the tail of ks_container
(ks_pod keeps its 184 bytes, which tests/test_oracle_kat.py pins),
ks_result.fail_node_ports in the former padding, and the two new symbols,
against a compiled probe of include/ksched.h (no GPU: loads and layouts only)."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi
from ksched.objects import Arena, Pod, pod_to_c

ROOT = Path(__file__).resolve().parent.parent

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(ks_host_port) O(ks_host_port, host_ip) O(ks_host_port, protocol) O(ks_host_port, host_port)
  S(ks_pod) O(ks_pod, n_namespace_labels)
  S(ks_container) O(ks_container, n_extended) O(ks_container, host_ports) O(ks_container, n_host_ports)
  S(ks_result) O(ks_result, flags) O(ks_result, fail_node_ports)
  printf("KS_STATUS_NODE_PORTS %d\n", (int)KS_STATUS_NODE_PORTS);
  printf("KS_UNMODELLED_HOST_PORTS %d\n", (int)KS_UNMODELLED_HOST_PORTS);
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
    types = {"ks_host_port": _abi.KsHostPort, "ks_pod": _abi.KsPod, "ks_result": _abi.KsResult,
             "ks_container": _abi.KsContainer}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(types[t], f).offset == val, key
        elif key in types:
            assert C.sizeof(types[key]) == val == _abi.EXPECTED_SIZES[key], key
    assert got["ks_host_port"] == 24
    # ks_container grew by exactly the 16 appended bytes: no earlier field moved; ks_pod is what it was
    assert got["ks_container"] == 64 and got["ks_container.host_ports"] == 48 and got["ks_container.n_host_ports"] == 56
    assert got["ks_container.n_extended"] == 40
    assert got["ks_pod"] == 184 and got["ks_pod.n_namespace_labels"] == 180
    # fail_node_ports sits where the padding was: the result keeps its layout
    assert got["ks_result"] == 64 and got["ks_result.fail_node_ports"] == got["ks_result.flags"] + 4 == 60
    assert got["KS_STATUS_NODE_PORTS"] == _abi.STATUS_NODE_PORTS == 8
    assert got["KS_UNMODELLED_HOST_PORTS"] == _abi.UNMODELLED["host_ports"] == 1
    assert got["KSCHED_ABI_VERSION"] == 6


def test_new_symbols_exported():
    lib = _abi.ksched_lib()
    for name in ("ks_host_ports_conflict", "ks_node_used_ports"):
        assert name in _abi.KSCHED_SYMBOLS and hasattr(lib, name), name
    assert lib.ks_abi_version() == 6
    # pure host code: callable without a context or a device
    a = _abi.KsHostPort(None, None, 80, 0)
    b = _abi.KsHostPort(b"10.0.0.1", b"TCP", 80, 0)
    assert lib.ks_host_ports_conflict(C.byref(a), C.byref(b)) == 1
    assert lib.ks_host_ports_conflict(None, C.byref(b)) == 0


def test_pod_marshalling():
    a = Arena()
    p = pod_to_c(Pod("p", host_ports=[(None, "", 9100), ("10.0.0.1", "UDP", 53), ("", None, 0)]), a)
    c = p.containers[0]  # the flattened list travels on the first container
    assert c.n_host_ports == 3
    got = [(c.host_ports[i].host_ip, c.host_ports[i].protocol, c.host_ports[i].host_port) for i in range(3)]
    assert got == [(None, b"", 9100), (b"10.0.0.1", b"UDP", 53), (b"", None, 0)]
    q = pod_to_c(Pod("q"), a).containers[0]  # a pod without ports: a zeroed tail
    assert q.n_host_ports == 0 and not q.host_ports and q._pad2 == 0
