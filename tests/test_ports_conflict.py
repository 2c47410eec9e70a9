"""ks_host_ports_conflict, the single definition the mask builder uses, against
the plain-Python HostPortInfo.CheckConflict (tests/ports_reference.py) over the
full cross product of ips, protocols and ports -- unset strings as NULL and as
"", the wildcard spelled out, an IPv6 wildcard that is no wildcard (ips are
compared as strings), a lower-case protocol that is not "TCP"."""
import ctypes as C
import itertools

from ksched import _abi
from ports_reference import HostPortInfo

IPS = [None, "", "0.0.0.0", "10.0.0.1", "10.0.0.2", "::"]
PROTOCOLS = [None, "", "TCP", "UDP", "SCTP", "tcp"]
PORTS = [-1, 0, 1, 80, 65535]


def c_port(ip, proto, port):
    return _abi.KsHostPort(None if ip is None else ip.encode(), None if proto is None else proto.encode(), port, 0)


def test_conflict_cross_product():
    lib = _abi.ksched_lib()
    triples = list(itertools.product(IPS, PROTOCOLS, PORTS))
    assert len(triples) == 180
    held = [c_port(*t) for t in triples]
    conflicts = 0
    for want in triples:
        a = c_port(*want)
        for have, b in zip(triples, held):
            node = HostPortInfo()
            node.add(*have)  # a node holding b alone (Add ignores port <= 0)
            exp = node.check_conflict(*want)
            got = lib.ks_host_ports_conflict(C.byref(a), C.byref(b))
            assert got == (1 if exp else 0), (want, have, got)
            conflicts += got
    # the table is neither empty nor full: per (protocol class, port > 0) the ip rules leave both outcomes
    assert 0 < conflicts < len(triples) ** 2 // 4
    # and a pod never conflicts through an ignored entry
    assert lib.ks_host_ports_conflict(C.byref(c_port(None, None, 0)), C.byref(c_port(None, None, 0))) == 0
