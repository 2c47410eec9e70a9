"""Workloads and the twin-context driver of the ks_batch_forget tests
(tests/test_gpu_forget.py and, for two ranks, tests/forget_multirank_main.py).

The reference of every check is a twin context: it receives the same nodes and
the same batches and forgets the same pods through ks_pods_remove with the
pods' ks_pod structs and the slots of their results -- the path every earlier
ForgetPod took.  All compared values are integers; equality is exact.
"""
import ctypes as C
import random

import numpy as np

from helpers import res_array, scores_array, states_np
from ipa_cases import DB, WEB, T
from ksched import _abi
from ksched.objects import (Container, LabelSelector, Node, Pod, TopologySpreadConstraint as TSC,
                            system_default_spread)
from ports_workloads import variant_pod
from spread_cases import HOST, ZONE, pod as spread_pod
from xfit_reference import GPU, HUGE, NIC
from xfit_workloads import xfit_pod

Gi, Mi = 1 << 30, 1 << 20


def u32(xs):
    xs = [int(x) for x in xs]
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def subset(ptr, idx, T_=_abi.KsPod):
    out = (T_ * max(1, len(idx)))()
    for j, i in enumerate(idx):
        out[j] = ptr[int(i)]
    return out


def pod_at(ptr, j):
    return C.cast(C.addressof(ptr.contents) + j * C.sizeof(_abi.KsPod), C.POINTER(_abi.KsPod))


def seven_eighths(rng, res):
    """A seeded 7/8 of the placed pods of a batch, ascending: what S - 1 of S = 8 shards forget."""
    placed = [int(i) for i in np.nonzero(res["status"] == 0)[0]]
    return sorted(rng.sample(placed, (7 * len(placed)) // 8))


def raw_forget(s, batch, idx):
    """ks_batch_forget through the bare ABI: (status, skipped)."""
    skipped = C.c_uint32(0xFFFF)
    st = s.lib.ks_batch_forget(s.ctx, batch, u32(idx), len(idx), C.byref(skipped))
    return st, int(skipped.value)


class Twin:
    """A context that forgets through ks_batch_forget and its twin that
    forgets through ks_pods_remove, fed alike."""

    def __init__(self, make, capacity):
        self.cap = capacity
        self.s, self.t = make(), make()
        self.batches = []

    def both(self):
        return (self.s, self.t)

    def upsert(self, na, slots, k):
        for x in self.both():
            x.upsert_nodes_raw(na, u32(slots), k)

    def delete(self, slots):
        for x in self.both():
            x.delete_slots(list(slots))

    def add(self, pa, slots, k):
        for x in self.both():
            assert x.lib.ks_pods_add(x.ctx, pa, u32(slots), k) == 0, x.lib.ks_last_error(x.ctx)

    def run(self, pa, m, what=""):
        """One batch in the prepare / run / results form on both; the results
        must agree.  Returns (the first context's batch, still resident; results)."""
        out = []
        for x in self.both():
            b = x.prepare(pa, m)
            x.run(b)
            out.append((b, res_array(x.results(b, m), m)))
        (b, r), (bt, rt) = out
        self.t.free(bt)
        self.batches.append(b)
        assert np.array_equal(r, rt), f"{what}: the two contexts' results differ at pods {np.nonzero(r != rt)[0][:5]}"
        return b, r

    def forget(self, b, pa, res, idx, gone=()):
        """Forget pods idx of batch b: ks_batch_forget on one context,
        ks_pods_remove on the twin for the pods whose slot is not in `gone`
        (slots whose node left since the batch ran).  Returns the skipped count."""
        skipped = self.s.forget(b, idx)
        keep = [i for i in idx if int(res["node_index"][i]) not in gone]
        if keep:
            st = self.t.lib.ks_pods_remove(self.t.ctx, subset(pa, keep), u32(res["node_index"][keep]), len(keep))
            assert st == 0, self.t.lib.ks_last_error(self.t.ctx)
        ctr = self.s.forget_counters()
        assert ctr[0] == len(keep) and ctr[1] == len(idx) - len(keep) == skipped, (ctr, len(idx), len(keep), skipped)
        assert ctr[3] == (1 if keep else 0) and ctr[4:] == [0, 0, 0, 0], ctr
        return skipped

    def states(self, x=None):
        x = x or self.s
        return states_np(x.lib.ks_node_states, x.ctx, self.cap)

    def check(self, what, ports=(), probes=()):
        """ks_node_states of all slots, ks_node_used_ports of `ports`,
        ks_plugin_scores over all slots of every probe (ks_pod pointers)."""
        g, w = self.states(self.s), self.states(self.t)
        assert np.array_equal(g, w), f"{what}: node states differ at slots {np.nonzero(g != w)[0][:8]}"
        for slot in ports:
            assert sorted(self.s.node_used_ports(slot)) == sorted(self.t.node_used_ports(slot)), \
                f"{what}: used ports of slot {slot}"
        for k, p in enumerate(probes):
            d = []
            for x in self.both():
                out = (_abi.KsNodeScore * self.cap)()
                assert x.lib.ks_plugin_scores(x.ctx, p, out) == 0, x.lib.ks_last_error(x.ctx)
                d.append(scores_array(out))
            assert np.array_equal(d[0], d[1]), \
                f"{what}: score dump of probe {k} differs at slots {np.nonzero((d[0] != d[1]).any(axis=1))[0][:8]}"

    def close(self):
        for b in self.batches:
            self.s.free(b)
        for x in self.both():
            x.close()


# ------------------------------------------------------------- chain pods
def chain_nodes(n):
    """n nodes in five zones, every one with amd.com/gpu, a NIC and huge pages, every third with the disk
    label some pods of tests/xfit_workloads.py select, none with images (a pod without spread constraints,
    extended resources, host ports or affinity terms then has no one-pod program)."""
    return [Node(f"h{i}", {"cpu": 16000, "memory": 64 * Gi, "pods": 110},
                 dict({HOST: f"h{i}", ZONE: f"z{i % 5}", "rack": f"r{i % 8}"}, **({"disk": "ssd"} if i % 3 == 0 else {})),
                 [], extended={GPU: 8, NIC: 4, HUGE: 1024 * Mi}) for i in range(n)]


def plain_pod(rng, name, app=None):
    """A pod the round kernels take.  Its default label is one no selector of these workloads names: a pod
    that a bound pod's affinity term selects gets a record of that term, and with it a one-pod program."""
    return Pod(name, containers=[Container({"cpu": rng.randrange(1, 8) * 50, "memory": rng.randrange(1, 16) * 64 * Mi})],
               labels={"app": app or "batch"})


def replica_pods(name, count):
    """One deployment's replicas under the system default constraints: identical one-pod programs, which
    the replica run schedules (>= 4 in a row).  No affinity term of these workloads selects their label: the
    run kernel models programs without InterPodAffinity records."""
    sel = LabelSelector({"app": "replica"})
    return [Pod(f"{name}{j}", containers=[Container({"cpu": 250, "memory": 256 * Mi})], labels={"app": "replica"},
                topology_spread=system_default_spread(sel), spread_defaulted=True) for j in range(count)]


XFIT_KINDS = (2, 3, 4, 5, 9)  # xfit_workloads.xfit_pod's kinds without spread constraints, terms or images


def xfit_pods(rng, j0, count):
    """Pods of tests/xfit_workloads.py that request amd.com/gpu, a NIC or huge pages: one resource, two
    (two XResDev records), a NIC alone, and an init container's maximum beside a sidecar's sum."""
    return [xfit_pod(rng, 10 * (j0 + q) + XFIT_KINDS[q % len(XFIT_KINDS)]) for q in range(count)]


def xres_pod(name, requests):
    """A small pod with exactly these extended-resource requests."""
    return Pod(name, containers=[Container(dict({"cpu": 100, "memory": 64 * Mi}, **requests))], labels={"app": "x"})


# A scoring configuration under which the Requested columns of the extended resources reach the scores of
# every node (the default strategy reads them in the Fit filter only): amd.com/gpu and the NIC listed in
# NodeResourcesFit's strategy, amd.com/gpu and huge pages in BalancedAllocation's list.
LISTED = dict(fit_resource_weights={"cpu": 1, "memory": 1, GPU: 3, NIC: 2},
              balanced_resources=["cpu", "memory", GPU, HUGE])


PIN_PORT = ("", "TCP", 7777)  # a port no other pod of these workloads draws


def holds_pin_port(s, slot):
    return any(e[1] == "TCP" and e[2] == PIN_PORT[2] for e in s.node_used_ports(slot))


def pinned_port_pod(name, host):
    """A pod with a host port that only node `host` can take."""
    p = Pod(name, containers=[Container({"cpu": 100, "memory": 64 * Mi})], labels={"app": "edge"},
            node_selector={HOST: host})
    p.host_ports = [PIN_PORT]
    return p


def chain_batch(seed, tag, plain=20, pin=None):
    """A batch of every kind the one-pod chain schedules, behind `plain` pods the round kernels take.
    Returns (pods, indices of the replica run, index of the pinned port pod or None)."""
    rng = random.Random(seed)
    pods = [plain_pod(rng, f"{tag}q{j}") for j in range(plain)]
    rep0 = len(pods)
    pods += replica_pods(f"{tag}r", 8)
    reps = list(range(rep0, len(pods)))
    zone_filter = [TSC(2, ZONE, "DoNotSchedule", WEB)]
    host_score = [TSC(1, HOST, "ScheduleAnyway", LabelSelector({"app": "api"}))]
    pods += [spread_pod(f"{tag}s{j}", spread=zone_filter) for j in range(6)]
    pods += [spread_pod(f"{tag}t{j}", {"app": "api"}, spread=host_score) for j in range(6)]
    pods += [spread_pod(f"{tag}a{j}", {"app": "db"}, affinity_terms=[T(HOST, DB, kind="anti-affinity")]) for j in range(6)]
    pods += [spread_pod(f"{tag}b{j}", affinity_terms=[T(ZONE, WEB, kind="preferred-affinity", weight=50)]) for j in range(5)]
    pods += [spread_pod(f"{tag}c{j}", {"app": "front"}, affinity_terms=[T(ZONE, DB)]) for j in range(4)]
    pods += xfit_pods(rng, 1000 * seed, 16)
    pods += [variant_pod(rng, f"{tag}v{j}", True, j % 2 == 1) for j in range(8)]
    at = None
    if pin is not None:
        at = len(pods)
        pods.append(pinned_port_pod(f"{tag}pin", pin))
    return pods, reps, at


def chain_probes(seed):
    """One probe pod per kind for the score dumps."""
    rng = random.Random(seed)
    return [spread_pod("probe-s", spread=[TSC(1, ZONE, "ScheduleAnyway", WEB), TSC(2, HOST, "DoNotSchedule", WEB)]),
            spread_pod("probe-a", {"app": "db"}, affinity_terms=[T(HOST, DB, kind="anti-affinity"),
                                                                 T(ZONE, WEB, kind="preferred-affinity", weight=10)]),
            spread_pod("probe-w"),  # carries no term itself: the bound pods' terms score it
            xfit_pods(rng, 90_000, 1)[0], xres_pod("probe-x", {GPU: 1, NIC: 1, HUGE: 256 * Mi}),
            xres_pod("probe-n", {NIC: 2}), variant_pod(rng, "probe-v", True, True), plain_pod(rng, "probe-q")]
