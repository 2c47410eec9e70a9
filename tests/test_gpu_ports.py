"""NodePorts on the GPU (ksched_spread.hip's PORTS filter instances and commit;
DESIGN §5.13) against PortsReference (tests/ports_reference.py), bit for bit:
every ks_result field (fail_node_ports in the former padding included),
ks_plugin_scores of probe pods, every node's state, and ks_node_used_ports of
every node against the reference's mirror.

Shapes: 1 node; 63 / 64 / 65 nodes for the wave reduction of the new counter;
1,025 and 2,049 nodes for the second and third 1,024-thread block and the
accumulation across blocks.  Each parity stream first asserts, on the
reference alone, that at least a quarter of its pods with host ports land on
another node (or on none) than they would with their ports stripped: a build
that ignored the ports could not pass.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ports_workloads as W
from fit_reference import scores_np
from helpers import res_array, states_np
from ksched import Scheduler, _abi
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from ports_reference import PortsReference
from test_gpu_spread import Pair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
CAP, UNS = _abi.KS_ERR_CAPACITY, _abi.KS_ERR_UNSUPPORTED


def assert_res(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)}/{len(want)} results differ; first at pod {i}: got {got[i]} "
                             f"want {want[i]}")


def used_ports(s, n):
    return [sorted(s.node_used_ports(slot)) for slot in range(n)]


def dump(s, pod, n, a):
    pa, _ = pods_array([pod], a)
    out = (_abi.KsNodeScore * n)()
    assert s.lib.ks_plugin_scores(s.ctx, pa, out) == 0, s.lib.ks_last_error(s.ctx)
    return scores_np(out, n)


class PortsPair(Pair):
    """libksched and PortsReference fed the same cache events."""

    def __init__(self, n, pairs=W.PAIRS, ips=W.IPS, ref=None, **cfg):
        super().__init__(n, **cfg)
        self.o.close()
        self.o = PortsReference(n, pairs, ips, **(ref or {}))

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        want = res_array(self.o.schedule(pa, m), m)
        got = res_array(self.s.schedule_raw(pa, m), m)
        assert_res(got, want, what)
        return got

    def dump_equal(self, pod, what=""):
        pa, _ = pods_array([pod], self.a)
        g, w = dump(self.s, pod, self.n, self.a), self.o.plugin_scores(pa)
        assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])
        return w

    def states_equal(self, what=""):
        assert np.array_equal(states_np(self.s.lib.ks_node_states, self.s.ctx, self.n), self.o.states()), what
        assert used_ports(self.s, self.n) == [self.o.used_ports(slot) for slot in range(self.n)], what

    def events(self, kind, pods, slots):
        """Pod events through ks_events_apply (the C5 event path) and the reference's cache."""
        pa, k = pods_array(pods, self.a)
        ev = (_abi.KsEvent * k)()
        for i in range(k):
            ev[i].kind, ev[i].slot, ev[i].pod = kind, slots[i], C.pointer(pa[i])
        assert self.s.lib.ks_events_apply(self.s.ctx, ev, k) == 0, self.s.lib.ks_last_error(self.s.ctx)
        (self.o.add_pods if kind == _abi.KS_EV_POD_ADD else self.o.remove_pods)(pa, W.u32(slots), k)

    def node_events(self, deleted, upserted):
        """KS_EV_NODE_DELETE of the slots `deleted`, then KS_EV_NODE_UPSERT of [(node, slot)], as one event log."""
        na, k = nodes_array([nd for nd, _ in upserted], self.a)
        ev = (_abi.KsEvent * (len(deleted) + k))()
        for i, slot in enumerate(deleted):
            ev[i].kind, ev[i].slot = _abi.KS_EV_NODE_DELETE, slot
        for j, (_, slot) in enumerate(upserted):
            e = ev[len(deleted) + j]
            e.kind, e.slot, e.node = _abi.KS_EV_NODE_UPSERT, slot, C.pointer(na[j])
        assert self.s.lib.ks_events_apply(self.s.ctx, ev, len(ev)) == 0, self.s.lib.ks_last_error(self.s.ctx)
        self.o.delete(W.u32(deleted), len(deleted))
        self.o.upsert(na, W.u32([slot for _, slot in upserted]), k)


# ------------------------------------------------------------ parity streams
def run_stream(n, what, **cfg):
    ref = W.reference_run(n)
    asked, moved = W.moved(ref["placed"])
    assert 4 * moved >= asked > 0, (asked, moved)  # the ports decide where these pods go
    ns, ps = W.stream(W.SEEDS[n], n)
    a = Arena()
    with Scheduler(n, pods_per_round=64, **cfg) as s:
        na, k = nodes_array(ns, a)
        s.upsert_nodes_raw(na, W.u32(range(k)), k)
        pa, m = pods_array(ps, a)
        assert_res(res_array(s.schedule_raw(pa, m), m), ref["res"], what)
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, n), ref["states"]), what
        assert used_ports(s, n) == ref["used"], what
        for p, want in zip(W.probes(n), ref["dumps"]):
            got = dump(s, p, n, a)
            assert np.array_equal(got, want), (what, p.name, np.nonzero(got != want)[0][:5])
        assert s.stats().spread_pods >= asked
    return ref


@pytest.mark.parametrize("n", sorted(W.SHAPES))
def test_stream_parity(n):
    ref = run_stream(n, f"mixed stream on {n} nodes")
    if n >= 63:  # dumps that show the new status
        assert any((d["status"] == _abi.STATUS_NODE_PORTS).any() for d in ref["dumps"])


def test_virtual_shards():
    run_stream(1025, "mixed stream on 3 virtual shards", virtual_shards=3)


def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "ports", "n": 65}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] > 0 and res["port_fails"] > 0


# every context the chain's launch tells apart (ports_workloads.CONTEXTS): the NodeResourcesFit strategies with
# and without a listed extended resource, which a third of the pods with ports request, each with and without a
# balanced list that names the GPU: the PORTS instances under GF / XF / BAL
@pytest.mark.parametrize("name,ref,cfg", [(name, ref, cfg) for name, (ref, cfg) in W.CONTEXTS.items()])
def test_context_variants(name, ref, cfg):
    n = 65
    ns, ps = W.stream(W.SEEDS[n], n)
    x = PortsPair(n, ref=dict(ref, track=True), pods_per_round=64, **cfg)
    x.upsert(ns, list(range(n)))
    r = x.schedule(ps, name)
    asked, moved = W.moved(x.o.placed)
    assert 4 * moved >= asked > 0, (asked, moved)
    assert (r["_pad"] > 0).any()
    x.states_equal(name)
    for p in W.probes(n):
        x.dump_equal(p, f"{name} {p.name}")
    x.close()


# ------------------------------------------------------- the dictionary's bits
def test_dictionary_bits_and_capacity():
    # 64 distinct triples fill the dictionary: bits 0, 31, 32 and 63 (both halves of the word) decide placements
    n = 8
    ports = list(range(2000, 2064))
    x = PortsPair(n, pairs=[("TCP", p) for p in ports], ips=[], pods_per_round=64)
    x.upsert([Node(f"n{i}", {"cpu": 64000, "memory": 64 * Gi, "pods": 200}) for i in range(n)], list(range(n)))
    holders = [Pod(f"h{i}", host_ports=[("", "TCP", p)]) for i, p in enumerate(ports)]
    x.add(holders, [i % 4 for i in range(64)])  # interned in order: triple i is bit i; nodes 4..7 hold nothing
    x.states_equal("64 holders")
    want = lambda i, name: Pod(name, containers=[Container({"cpu": 100})], host_ports=[(None, None, ports[i])])
    picks = [0, 31, 32, 63]
    r = x.schedule([want(i, f"w{i}-{j}") for j in range(7) for i in picks], "bits 0 / 31 / 32 / 63")
    # each triple has 7 free nodes (one of nodes 0..3 holds it): its first seven pods land, on distinct nodes
    assert (r["status"] == 0).all() and (r["_pad"][:4] == 1).all()
    r = x.schedule([want(i, f"x{i}") for i in picks], "the eighth pod of each")
    assert (r["status"] == 1).all() and (r["_pad"] == n).all() and (r["fail"] == 0).all()
    x.states_equal("after the fill of four triples")
    for i in picks:
        w = x.dump_equal(want(i, f"d{i}"), f"dump of bit {i}")
        assert (w["status"] == _abi.STATUS_NODE_PORTS).all()
    # the 65th distinct triple: refused for that pod alone, by name
    batch = [want(5, "ok-a"), Pod("late", host_ports=[("", "UDP", 2000)]), Pod("plain"), want(63, "ok-b")]
    pa, m = pods_array(batch, x.a)
    status = (C.c_int32 * m)()
    assert x.s.lib.ks_pods_check(x.s.ctx, pa, m, status) == CAP
    assert list(status) == [0, CAP, 0, 0]
    assert b"pod 1" in x.s.lib.ks_last_error(x.s.ctx) and b"UDP" in x.s.lib.ks_last_error(x.s.ctx)
    h = C.c_void_p()
    assert x.s.lib.ks_batch_prepare(x.s.ctx, pa, m, C.byref(h)) == CAP
    x.schedule([batch[0], batch[2], batch[3]], "the batch's other pods")
    x.states_equal("after the refusal")
    x.close()


# ------------------------------------------------------------------ the fill
def test_fill():
    n = 65
    x = PortsPair(n, pairs=[("TCP", 9100)], ips=[], pods_per_round=64)
    x.upsert([Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 110}) for i in range(n)], list(range(n)))
    r = x.schedule([Pod(f"exporter-{j}", containers=[Container({"cpu": 100})], host_ports=[("", "TCP", 9100)])
                    for j in range(n + 3)], "fill")
    assert list(r["node_index"][:n]) == list(range(n))  # n distinct nodes in slot order
    assert (r["status"][n:] == 1).all() and (r["_pad"][n:] == n).all() and (r["fail"][n:] == 0).all()
    assert list(r["_pad"][:n]) == list(range(n))
    x.states_equal("fill")
    x.close()


# ----------------------------------------------------------------- churn
def pinned(name, host, port, cpu=100):
    return Pod(name, containers=[Container({"cpu": cpu})], node_selector={"kubernetes.io/hostname": host},
               host_ports=[port])


def test_churn_between_batches():
    n = 65
    ns, ps = W.stream(W.SEEDS[n], n)
    x = PortsPair(n, pods_per_round=64)
    x.upsert(ns, list(range(n)))
    # bound pods through ks_pods_add and KS_EV_POD_ADD, one triple per node each (no double holds)
    bound = [Pod(f"b{i}", containers=[Container({"cpu": 200})], host_ports=[(W.IPS[i % 2], "TCP", 443)])
             for i in range(20)]
    x.add(bound[:10], list(range(10)))
    x.events(_abi.KS_EV_POD_ADD, bound[10:], list(range(10, 20)))
    x.states_equal("bound pods")
    r = x.schedule(ps[:30], "churn batch 0")
    # a removed pod's port frees its node for the next pod
    spot = next(i for i in range(20, n) if not ns[i].taints and ns[i].allocatable["pods"] == 110 and
                not any(e[1:] == ("UDP", 8080) for e in x.o.used_ports(i)))
    first, second, third = (pinned(f"pin{j}", f"n{spot}", ("", "UDP", 8080)) for j in range(3))
    r = x.schedule([first, second], "pinned pair")
    assert list(r["status"]) == [0, 1] and r["node_index"][0] == spot and r["_pad"][1] == 1
    x.events(_abi.KS_EV_POD_REMOVE, [first], [spot])
    x.events(_abi.KS_EV_POD_REMOVE, bound[10:15], list(range(10, 15)))
    x.add(bound[:3], [0, 1, 2], sign=-1)
    x.states_equal("after the removals")
    r = x.schedule([third] + ps[30:45], "churn batch 1")
    assert r["status"][0] == 0 and r["node_index"][0] == spot
    # a node is deleted (its used ports leave with it) and upserted again: it starts with none; an update
    # of a live node leaves its used ports alone
    busy = [s for s in range(n) if x.o.used_ports(s)]
    gone, kept = busy[0], busy[1]
    x.node_events([gone], [(ns[gone], gone), (ns[kept], kept)])
    assert x.s.node_used_ports(gone) == [] and x.s.node_used_ports(kept) != []
    x.states_equal("after delete and upsert")
    x.schedule(ps[45:], "churn batch 2")
    x.states_equal("churn end")
    x.dump_equal(W.probes(n)[0], "churn dump")
    x.close()


def test_remove_clears_an_entry_two_pods_hold():
    # HostPortInfo.Remove keeps no reference count (checked on the device column alone: PortsReference's
    # emulation counts references)
    with Scheduler(4) as s:
        s.upsert_nodes([Node("n0", {"cpu": 4000, "memory": 8 * Gi, "pods": 10})], [0])
        a, b = (Pod(nm, host_ports=[("", "TCP", 9100), ("10.0.0.1", "UDP", 53)]) for nm in "ab")
        s.add_pods([a, b], [0, 0])
        assert sorted(s.node_used_ports(0)) == [("0.0.0.0", "TCP", 9100), ("10.0.0.1", "UDP", 53)]
        s.remove_pods([a], [0])
        assert s.node_used_ports(0) == []
        r = s.schedule_pods([Pod("c", host_ports=[("", "TCP", 9100)])])
        assert r[0].suggested_host == "n0"


def test_ports_of_every_container_and_of_no_init_container():
    # the ports travel per container (ks_container.host_ports); init containers and sidecars do not count
    x = PortsPair(2, pairs=[("TCP", 9100), ("TCP", 9200)], ips=[], pods_per_round=64)
    x.upsert([Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 10}) for i in range(2)], [0, 1])
    side = Pod("side", containers=[Container({"cpu": 100}), Container({"cpu": 100}, host_ports=[("", "TCP", 9200)])],
               init_containers=[Container({"cpu": 100}, host_ports=[("", "TCP", 9100)]),
                                Container({"cpu": 50}, True, host_ports=[("", "TCP", 9100)])])
    x.add([side], [0])
    assert x.s.node_used_ports(0) == [("0.0.0.0", "TCP", 9200)]
    r = x.schedule([Pod("a", host_ports=[("", "TCP", 9100)]), Pod("b", host_ports=[("", "TCP", 9200)]),
                    Pod("c", containers=[Container(), Container(host_ports=[(None, None, 9200)])])], "containers")
    assert list(r["status"]) == [0, 0, 1] and list(r["_pad"]) == [0, 1, 2]
    x.states_equal("containers")
    x.close()


def test_used_ports_cap_convention_and_read_only_calls():
    INV = _abi.KS_ERR_INVALID
    with Scheduler(4) as s:
        node = lambda nm: Node(nm, {"cpu": 4000, "memory": 8 * Gi, "pods": 100})
        s.upsert_nodes([node("n0"), node("n1")], [0, 1])
        s.add_pods([Pod("a", host_ports=[("10.0.0.1", "TCP", 443), ("", "UDP", 53)])], [0])
        used = lambda slot, out, cap, n: s.lib.ks_node_used_ports(s.ctx, slot, out, cap, n)
        n, out = C.c_uint32(77), (_abi.KsHostPort * 2)()
        assert used(0, None, 0, C.byref(n)) == INV and n.value == 2   # no room: the count comes back
        assert used(0, out, 1, C.byref(n)) == INV and n.value == 2
        assert used(0, out, 2, C.byref(n)) == 0 and n.value == 2
        assert sorted((out[i].host_ip, out[i].protocol, out[i].host_port) for i in range(2)) == [
            (b"0.0.0.0", b"UDP", 53), (b"10.0.0.1", b"TCP", 443)]
        assert used(1, None, 0, C.byref(n)) == 0 and n.value == 0      # a node without ports needs no room
        assert used(3, None, 0, C.byref(n)) == 0 and n.value == 0      # an empty slot
        assert used(0, out, 2, None) == INV and used(0, None, 2, C.byref(n)) == INV
        assert used(4, out, 2, C.byref(n)) == _abi.KS_ERR_NOT_FOUND
        # a count without an array is refused wherever the container is read
        a = Arena()
        pa, _ = pods_array([Pod("bad"), Pod("worse", containers=[Container(), Container()])], a)
        pa[0].containers[0].n_host_ports = 2
        pa[1].containers[1].n_host_ports = 1
        status = (C.c_int32 * 2)()
        assert s.lib.ks_pods_check(s.ctx, pa, 2, status) == INV and list(status) == [INV, INV]
        assert s.lib.ks_pods_add(s.ctx, pa, (C.c_uint32 * 2)(1, 1), 2) == INV
        # the score dump is read-only: it interns nothing, and still sees a wildcard want against a held
        # specific ip although the wildcard triple is in no dictionary
        s.add_pods([Pod(f"h{i}", host_ports=[("", "TCP", 3000 + i)]) for i in range(61)], [1] * 61)  # 63 entries
        sc = s.plugin_scores(Pod("dump", host_ports=[("", "TCP", 443), ("", "TCP", 5000)]))
        assert [sc[i].status for i in range(4)] == [_abi.STATUS_NODE_PORTS, -1, -2, -2]
        assert check(s, [Pod("last", host_ports=[("", "TCP", 6000)])]) == (0, [0])  # the 64th entry is still free
        r = s.schedule_pods([Pod("last", host_ports=[("", "TCP", 6000)])])
        assert not isinstance(r[0], Exception)
        assert check(s, [Pod("dump", host_ports=[("", "TCP", 5000)])]) == (CAP, [CAP])


# --------------------------------------------------------- late interning
def test_masks_are_resolved_when_the_batch_runs():
    # batch A is prepared first; batch B then interns a specific-ip triple A's wildcard want conflicts with,
    # and runs first: A's conflict mask must be the launch's, not the prepare's
    n = 3
    x = PortsPair(n, pairs=[("TCP", 80)], ips=["10.0.0.1"], pods_per_round=64)
    x.upsert([Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 10}, labels={"kubernetes.io/hostname": f"n{i}"})
              for i in range(n)], list(range(n)))
    pa, ma = pods_array([pinned("a", "n1", ("", "TCP", 80)), Pod("a-free", host_ports=[(None, "TCP", 80)])], x.a)
    pb, mb = pods_array([pinned("b", "n1", ("10.0.0.1", "TCP", 80))], x.a)
    ha = x.s.prepare(pa, ma)
    hb = x.s.prepare(pb, mb)
    x.s.run(hb)
    x.s.run(ha)
    want = res_array(x.o.schedule(pb, mb), mb), res_array(x.o.schedule(pa, ma), ma)
    assert_res(res_array(x.s.results(hb, mb), mb), want[0], "the later batch, run first")
    got = res_array(x.s.results(ha, ma), ma)
    assert_res(got, want[1], "the earlier batch, run second")
    assert got["status"][0] == 1 and got["_pad"][0] == 1 and list(got["fail"][0][:4]) == [0, 0, 0, 2]
    assert got["status"][1] == 0 and got["node_index"][1] == 0 and got["_pad"][1] == 1
    x.s.free(ha)
    x.s.free(hb)
    x.states_equal("late interning")
    x.close()


# --------------------------------------------------------------- refusals
def check(s, pods):
    """(ks_pods_check's status, the per-pod statuses)."""
    a = Arena()
    pa, m = pods_array(pods, a)
    status = (C.c_int32 * m)()
    return s.lib.ks_pods_check(s.ctx, pa, m, status), list(status)


def test_refusals():
    node = Node("n0", {"cpu": 4000, "memory": 8 * Gi, "pods": 200})
    wants = Pod("w", host_ports=[("", "TCP", 80)])
    with Scheduler(8, percentage_of_nodes_to_score=50) as s:  # a window: pods with host ports are refused
        s.upsert_nodes([node], [0])
        assert check(s, [Pod("plain"), wants]) == (UNS, [0, UNS])
        assert b"percentage_of_nodes_to_score" in s.lib.ks_last_error(s.ctx)
        assert not isinstance(s.schedule_pods([Pod("plain")])[0], Exception)
    with Scheduler(8) as s:
        s.upsert_nodes([node], [0])
        # the caller's bit still refuses: host ports it could not express
        assert check(s, [Pod("bit", unmodelled=["host_ports"]), wants]) == (UNS, [UNS, 0])
        # a bound pod whose triple the full dictionary cannot take: every pod with host ports is refused
        # until it leaves; pods without host ports go on
        s.add_pods([Pod(f"h{i}", host_ports=[("", "TCP", 3000 + i)]) for i in range(64)], [0] * 64)
        over = Pod("over", host_ports=[("", "TCP", 3000), ("", "TCP", 4000)])
        s.add_pods([over], [0])
        assert len(s.node_used_ports(0)) == 64
        assert check(s, [wants, Pod("plain"), Pod("known", host_ports=[("", "TCP", 3001)])]) == (UNS, [UNS, 0, UNS])
        assert b"bound pod" in s.lib.ks_last_error(s.ctx)
        assert not isinstance(s.schedule_pods([Pod("plain")])[0], Exception)
        s.remove_pods([over], [0])  # (its known triple goes with it: no reference count)
        assert len(s.node_used_ports(0)) == 63
        st, each = check(s, [Pod("known", host_ports=[("", "TCP", 3000)]), wants])
        assert (st, each) == (CAP, [0, CAP])  # the dictionary stays full: a new triple is a capacity refusal
        r = s.schedule_pods([Pod("known", host_ports=[("", "TCP", 3000)]), Pod("taken", host_ports=[("", "TCP", 3001)])])
        assert r[0].suggested_host == "n0" and r[1].diagnosis.node_to_status == {"NodePorts": 1}
