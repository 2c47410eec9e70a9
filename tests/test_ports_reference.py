"""The NodePorts reference alone (tests/ports_reference.py): the plain-Python
HostPortInfo on the semantics it restates, PortsReference on hand-derived
scenarios, and the agreement of its emulation with its mirror on the random
streams the GPU tests run (no GPU)."""
import numpy as np
import pytest

import ports_workloads as W
from helpers import res_array
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from ports_reference import HostPortInfo, PortsReference, pod_wants

Gi, Mi = 1 << 30, 1 << 20


# ------------------------------------------------------------ HostPortInfo
def test_sanitize_and_ignored_ports():
    h = HostPortInfo()
    h.add("", "", 80)       # -> 0.0.0.0 / TCP
    h.add(None, None, 80)   # the same entry
    h.add("10.0.0.1", "UDP", 0)
    h.add("10.0.0.1", "UDP", -5)
    assert h.entries() == [("0.0.0.0", "TCP", 80)]
    h.remove("0.0.0.0", "TCP", 0)  # ignored
    assert len(h) == 1
    assert not h.check_conflict("", "", 0) and not h.check_conflict("", "", -1)
    assert h.check_conflict("0.0.0.0", "TCP", 80) and h.check_conflict("10.9.9.9", None, 80)
    assert not h.check_conflict("", "tcp", 80)  # protocols are compared as strings
    assert not h.check_conflict("", "UDP", 80) and not h.check_conflict("", "", 81)


def test_wildcard_and_specific_ips():
    h = HostPortInfo()
    h.add("10.0.0.1", "TCP", 80)
    assert h.check_conflict("", "TCP", 80)              # a wildcard want against any ip's set
    assert h.check_conflict("10.0.0.1", "TCP", 80)
    assert not h.check_conflict("10.0.0.2", "TCP", 80)  # another specific ip
    assert not h.check_conflict("::", "TCP", 80)        # no IP normalisation: "::" is one more specific ip
    h.add("::", "TCP", 443)
    assert h.check_conflict("0.0.0.0", "TCP", 443) and not h.check_conflict("10.0.0.1", "TCP", 443)


def test_remove_keeps_no_reference_count():
    # two bound pods of one node hold the same triple; removing one pod clears the entry
    h = HostPortInfo()
    h.add("", "TCP", 9100)
    h.add("", "TCP", 9100)
    h.remove("", "TCP", 9100)
    assert len(h) == 0 and not h.check_conflict("", "TCP", 9100)


# --------------------------------------------------------- hand-derived scenarios
def node(name, cpu=4000, mem=8 * Gi, pods=110):
    return Node(name, {"cpu": cpu, "memory": mem, "pods": pods})


def port_pod(name, *ports, cpu=100, containers=1):
    return Pod(name, containers=[Container({"cpu": cpu, "memory": 64 * Mi}) for _ in range(containers)],
               host_ports=list(ports))


class Ref:
    def __init__(self, nodes, pairs, ips=()):
        self.a = Arena()
        self.o = PortsReference(len(nodes), pairs, ips)
        na, k = nodes_array(nodes, self.a)
        self.o.upsert(na, W.u32(range(k)), k)

    def schedule(self, pods):
        pa, m = pods_array(pods, self.a)
        return res_array(self.o.schedule(pa, m), m)

    def add(self, pods, slots, sign=1):
        pa, m = pods_array(pods, self.a)
        (self.o.add_pods if sign > 0 else self.o.remove_pods)(pa, W.u32(slots), m)


@pytest.mark.parametrize("n", [1, 5])
def test_fill(n):
    # n identical nodes, n + 3 pods wanting (TCP, 9100, ""): n distinct nodes in slot order, then NodePorts everywhere
    x = Ref([node(f"n{i}") for i in range(n)], [("TCP", 9100)])
    r = x.schedule([port_pod(f"exporter-{j}", ("", "TCP", 9100)) for j in range(n + 3)])
    assert list(r["node_index"][:n]) == list(range(n)) and (r["status"][:n] == 0).all()
    assert list(r["feasible"][:n]) == list(range(n, 0, -1)) and list(r["_pad"][:n]) == list(range(n))
    tail = r[n:]
    assert (tail["status"] == 1).all() and (tail["node_index"] == -1).all() and (tail["feasible"] == 0).all()
    assert (tail["_pad"] == n).all() and (tail["fail"] == 0).all() and (tail["evaluated"] == n).all()
    assert [x.o.used_ports(s) for s in range(n)] == [[("0.0.0.0", "TCP", 9100)]] * n


def test_wildcard_against_specific_ip_pairs():
    x = Ref([node("n0")], [("TCP", 80), ("UDP", 80), ("tcp", 80)], ["10.0.0.1", "10.0.0.2"])
    r = x.schedule([port_pod("a", ("10.0.0.1", "TCP", 80)),   # lands
                    port_pod("b", ("10.0.0.2", None, 80)),    # another ip: lands beside it
                    port_pod("c", ("", "TCP", 80)),           # the wildcard conflicts with both
                    port_pod("d", (None, "UDP", 80)),         # another protocol: lands
                    port_pod("e", ("10.0.0.1", "", 80)),      # the same ip again
                    port_pod("f", ("10.0.0.2", "UDP", 80)),   # a specific ip against the held wildcard
                    port_pod("g", ("0.0.0.0", "tcp", 80))])   # "tcp" is not "TCP"
    assert list(r["status"]) == [0, 0, 1, 0, 1, 1, 0]
    assert list(r["_pad"]) == [0, 0, 1, 0, 1, 1, 0]
    assert x.o.used_ports(0) == [("0.0.0.0", "UDP", 80), ("0.0.0.0", "tcp", 80), ("10.0.0.1", "TCP", 80),
                                 ("10.0.0.2", "TCP", 80)]


def test_node_failing_fit_and_ports_is_counted_under_ports():
    x = Ref([node("n0", cpu=1000), node("n1", cpu=1000), node("n2", cpu=8000)], [("TCP", 443)])
    x.add([port_pod("held", ("", "TCP", 443), cpu=100)], [0])
    x.add([port_pod("held2", ("", "TCP", 443), cpu=100)], [2])
    r = x.schedule([port_pod("big", ("", "TCP", 443), cpu=2000)])
    # n0 fails NodePorts and NodeResourcesFit: NodePorts', the earlier plugin; n1 fails Fit alone; n2 NodePorts alone
    assert r["status"][0] == 1 and r["_pad"][0] == 2 and list(r["fail"][0]) == [0, 0, 0, 0, 1, 0, 0, 0]


def test_two_containers_wanting_the_same_port():
    x = Ref([node("n0")], [("TCP", 8080)])
    r = x.schedule([port_pod("twice", ("", "TCP", 8080), (None, None, 8080), containers=2)])
    assert r["status"][0] == 0 and r["_pad"][0] == 0  # a pod never conflicts with itself
    assert x.o.used_ports(0) == [("0.0.0.0", "TCP", 8080)]


def test_removed_pod_frees_its_port():
    x = Ref([node("n0")], [("TCP", 9100)])
    first = port_pod("first", ("", "TCP", 9100))
    r = x.schedule([first, port_pod("second", ("", "TCP", 9100))])
    assert list(r["status"]) == [0, 1]
    x.add([first], [0], sign=-1)
    assert x.o.used_ports(0) == []
    assert x.schedule([port_pod("third", ("", "TCP", 9100))])["status"][0] == 0


def test_pod_without_ports_skips_the_plugin():
    x = Ref([node("n0")], [("TCP", 9100)])
    x.add([port_pod("held", ("", "TCP", 9100))], [0])
    pa, _ = pods_array([Pod("plain"), port_pod("ignored", ("", "TCP", 0), (None, None, -1))], x.a)
    assert pod_wants(pa) == []
    r = x.schedule([Pod("plain"), port_pod("ignored", ("", "TCP", 0), (None, None, -1))])
    assert list(r["status"]) == [0, 0] and list(r["_pad"]) == [0, 0]


def test_init_container_ports_do_not_count():
    # NodeInfo.updateUsedPorts and nodeports.PreFilter read Spec.Containers alone; every container's ports count
    x = Ref([node("n0")], [("TCP", 9100), ("TCP", 9200)])
    side = Pod("side", containers=[Container({"cpu": 100}), Container({"cpu": 100}, host_ports=[("", "TCP", 9200)])],
               init_containers=[Container({"cpu": 100}, host_ports=[("", "TCP", 9100)]),
                                Container({"cpu": 50}, True, host_ports=[("", "TCP", 9100)])])
    pa, _ = pods_array([side], x.a)
    assert pod_wants(pa) == [("0.0.0.0", "TCP", 9200)]
    r = x.schedule([side, port_pod("takes-9100", ("", "TCP", 9100)), port_pod("wants-9200", ("", "TCP", 9200))])
    assert list(r["status"]) == [0, 0, 1] and r["_pad"][2] == 1
    assert x.o.used_ports(0) == [("0.0.0.0", "TCP", 9100), ("0.0.0.0", "TCP", 9200)]


# ------------------------------------------------ the streams of the GPU tests
@pytest.mark.parametrize("n", sorted(W.SHAPES))
def test_streams_move_with_their_ports(n):
    # (PortsReference asserts the agreement of its emulation and its mirror per pod and node while it runs)
    ref = W.reference_run(n)
    r = ref["res"]
    asked, moved = W.moved(ref["placed"])
    assert asked == sum(ref["ports"]) > 0
    assert 4 * moved >= asked, (n, asked, moved)  # the condition the GPU parity tests rest on
    assert (r["_pad"] > 0).any() and (r["status"][np.array(ref["ports"])] == 0).any()
    if n >= 63:
        assert ((r["_pad"] > 0) & (r["status"] == 0)).any()  # ports narrowed a pod's choice without making it unschedulable
        assert sum(len(u) for u in ref["used"]) >= 8
