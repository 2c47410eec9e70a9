"""Workloads of the NodePorts tests, shared by the CPU tests of the reference
(tests/test_ports_reference.py) and the GPU parity tests
(tests/test_gpu_ports.py): the CPU side picks the seeds at which the reference
alone shows that the ports move the schedule, the GPU side runs the same
streams through libksched.

The pods with host ports draw from 3 ports x 2 protocols x {wildcard, 2 ips}.
About half of them are pinned (nodeSelector) to a small pool of edge nodes,
the way ingress controllers are, and the others prefer it (preferred node
affinity, weight 100): the pool's ports run out, pinned pods become
unschedulable with NodePorts in their diagnosis, and preferring pods fall off
the pool -- which moves NodeAffinity's normaliser.  Mixed in: NoSchedule and
PreferNoSchedule taints, pods with spread constraints and a host port, pods
requesting amd.com/gpu and a host port, and plain pods that fill the nodes so
that some fail NodeResourcesFit and NodePorts at once.
"""
import ctypes as C
import functools
import itertools
import random

from fit_reference import MOST
from ksched.objects import (Arena, Container, LabelSelector, Node, NodeSelectorRequirement, NodeSelectorTerm, Pod,
                            PodAffinityTerm, PreferredSchedulingTerm, Taint, Toleration, TopologySpreadConstraint,
                            nodes_array, pods_array)
from rtcr_reference import RTCR, SHAPES as FIT_SHAPES

Gi, Mi = 1 << 30, 1 << 20
GPU = "amd.com/gpu"
PORTS, PROTOCOLS, IPS = [9100, 8080, 443], ["TCP", "UDP"], ["10.0.0.1", "10.0.0.2"]
PAIRS = list(itertools.product(PROTOCOLS, PORTS))
ZONE = "topology.kubernetes.io/zone"

# (nodes, pods, nodes of the edge pool) per node count of the GPU tests: 1 node; 63 / 64 / 65 for the
# wave reduction of the new counter; 1,025 and 2,049 for the second and third 1,024-thread block
SHAPES = {1: (1, 12, 1), 63: (63, 60, 4), 64: (64, 60, 4), 65: (65, 60, 4), 1025: (1025, 300, 12),
          2049: (2049, 150, 8)}


def nodes(rng, n, edge):
    out = []
    for i in range(n):
        labels = {"kubernetes.io/hostname": f"n{i}", ZONE: f"z{i % 3}"}
        if i % max(1, n // edge) == 0 and sum(1 for x in out if "pool" in x.labels) < edge:
            labels["pool"] = "edge"
        taints = []
        if n > 8 and rng.random() < 0.08:
            taints.append(Taint("dedicated", "infra", "NoSchedule"))
        if n > 8 and rng.random() < 0.15:
            taints.append(Taint("spot", rng.choice(["a", "b"]), "PreferNoSchedule"))
        ext = {GPU: rng.choice([2, 4])} if rng.random() < 0.3 else {}
        out.append(Node(f"n{i}", {"cpu": rng.choice([2000, 4000, 8000]), "memory": rng.choice([4, 8, 16]) * Gi,
                                  "pods": rng.choice([6, 12, 110])}, labels=labels, taints=taints, extended=ext))
    return out


def host_port(rng):
    return rng.choice([None, "", "0.0.0.0"] + 2 * IPS), rng.choice(PROTOCOLS + [None]), rng.choice(PORTS)


def prefer_edge(weight=100):
    return [PreferredSchedulingTerm(weight, NodeSelectorTerm([NodeSelectorRequirement("pool", "In", ["edge"])]))]


def pod(rng, j, ports):
    """Pod j of a mixed stream; ports: it carries host ports."""
    req = {"cpu": rng.choice([100, 250, 500, 1500]), "memory": rng.choice([128, 256, 1024]) * Mi}
    p = Pod(f"p{j}", labels={"app": rng.choice(["web", "api"])}, containers=[Container(dict(req))])
    if rng.random() < 0.3:
        p.tolerations.append(Toleration("dedicated", "Equal", "infra", "NoSchedule"))
    if rng.random() < 0.2:
        p.tolerations.append(Toleration("spot", "Exists", "", "PreferNoSchedule"))
    if not ports:
        if rng.random() < 0.25:
            p.preferred = prefer_edge(rng.choice([10, 50]))
        return p
    p.host_ports = [host_port(rng)]
    kind = rng.random()
    if kind < 0.15:  # a second container with the same port (never a conflict with itself) and an ignored entry
        p.containers.append(Container({"cpu": 50}))
        p.host_ports += [p.host_ports[0], (None, None, 0)]
    elif kind < 0.3:  # two different ports
        p.host_ports.append(host_port(rng))
    where = rng.random()
    if where < 0.5:
        p.node_selector = {"pool": "edge"}
    else:
        p.preferred = prefer_edge()
    extra = rng.random()
    if extra < 0.12:  # spread constraints and a host port
        p.topology_spread = [TopologySpreadConstraint(2, ZONE, "ScheduleAnyway",
                                                      LabelSelector({"app": p.labels["app"]}))]
    elif extra < 0.24:  # amd.com/gpu and a host port
        p.containers[0].requests[GPU] = 1
    return p


def stream(seed, n):
    """(nodes, pods) of the mixed stream at node count n: a third of the pods carry host ports."""
    k, m, edge = SHAPES[n]
    rng = random.Random(seed)
    ns = nodes(rng, k, edge)
    ps = [pod(rng, j, ports=(j % 3 == 1)) for j in range(m)]
    return ns, ps


# seeds at which PortsReference alone places at least a quarter of the pods with host ports on another node
# (or on none) than it would with their ports stripped (tests/test_ports_reference.py asserts it per shape)
SEEDS = {1: 12, 63: 11, 64: 11, 65: 12, 1025: 15, 2049: 15}


def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def probes(n):
    """Pods whose score dumps the parity tests compare at the stream's end state: with and without host ports."""
    rng = random.Random(1000 + n)
    return [pod(rng, 90_000 + j, ports=(j % 2 == 0)) for j in range(4)]


def moved(placed):
    """(pods with host ports, those placed elsewhere -- or nowhere -- than with their ports stripped)."""
    return len(placed), sum(1 for stripped, actual in placed if stripped != actual)


@functools.lru_cache(maxsize=None)
def reference_run(n):
    """The mixed stream at node count n through PortsReference alone, computed once per process: every
    result, every node's state and used ports, the probes' dumps at the end state, and where each pod
    with host ports would have gone without them."""
    from helpers import res_array
    from ports_reference import PortsReference

    ns, ps = stream(SEEDS[n], n)
    a = Arena()
    o = PortsReference(n, PAIRS, IPS, track=True)
    na, k = nodes_array(ns, a)
    o.upsert(na, u32(range(k)), k)
    pa, m = pods_array(ps, a)
    res = res_array(o.schedule(pa, m), m)
    dumps = [o.plugin_scores(pods_array([p], a)[0]) for p in probes(n)]
    out = {"res": res, "states": o.states(), "used": [o.used_ports(s) for s in range(n)], "placed": list(o.placed),
           "dumps": dumps, "ports": [bool(p.host_ports) for p in ps]}
    o.close()
    return out


def two_rank_case(cfg):
    """The mixed stream as a two-rank case (tests/chain_multirank_main.py): the one-pod chain runs replicated,
    so every rank keeps its own dictionary and used-ports column and applies every commit."""
    n = cfg["n"]
    ref = reference_run(n)
    ns, ps = stream(SEEDS[n], n)
    a = Arena()
    na, k = nodes_array(ns, a)
    sl = u32(range(k))
    half = len(ps) // 2

    def check(s):
        if [sorted(s.node_used_ports(slot)) for slot in range(n)] != ref["used"]:
            return "used ports differ from the reference's mirror"

    return dict(capacity=n, pods_per_round=64, setup=lambda s: s.upsert_nodes_raw(na, sl, k), arena=a,
                batches=[pods_array(ps[:half], a), pods_array(ps[half:], a)], want=ref["res"], states=ref["states"],
                check=check, report={"port_fails": int(ref["res"]["_pad"].sum())})


# ------------------------------------------------- the chain's launch contexts
def context(strategy=None, gpu=0, balanced=None):
    """(PortsReference's keywords, Scheduler's) of a context: MostAllocated or a RequestedToCapacityRatio
    shape by name, amd.com/gpu listed in the strategy at weight `gpu`, a balanced list."""
    ref, cfg = {}, {}
    if strategy == MOST:
        ref["strategy"], cfg["fit_strategy"] = (MOST, 1, 1), MOST
    elif strategy:
        ref["strategy"] = (FIT_SHAPES[strategy], 1, 1)
        cfg.update(fit_strategy=RTCR, fit_shape=list(FIT_SHAPES[strategy]))
    if gpu:
        ref["extended"], cfg["fit_resource_weights"] = {GPU: gpu}, {"cpu": 1, "memory": 1, GPU: gpu}
    if balanced:
        ref["balanced"], cfg["balanced_resources"] = list(balanced), list(balanced)
    return ref, cfg


# The ten contexts the chain's launch tells apart for a pod that requests amd.com/gpu: the default strategy,
# MostAllocated and RequestedToCapacityRatio (the kernels' GF 0 / 1 / 2), the latter two with and without
# the resource in the strategy (XF), each of the five with and without a balanced list that names it (BAL)
CONTEXTS = {
    "most": context(MOST),
    "most-gpu3": context(MOST, 3),
    "rtcr-binpack": context("binpack"),
    "balanced-gpu": context(balanced=["cpu", "memory", GPU]),
    "rtcr-gpu2-balanced": context("peaked", 2, [GPU, "cpu", "memory"]),
    "default": context(),
    "most-balanced": context(MOST, balanced=["cpu", "memory", GPU]),
    "most-gpu3-balanced": context(MOST, 3, [GPU, "cpu", "memory"]),
    "rtcr-binpack-balanced": context("binpack", balanced=["cpu", GPU, "memory"]),
    "rtcr-gpu2": context("peaked", 2),
}

# The chain-variant pods (tests/test_gpu_chain_variants.py): four kinds, with or without a host port and
# with or without a required anti-affinity term on kubernetes.io/hostname against their own app label.
# Each requests one amd.com/gpu, so it takes the one-pod chain under every context
KINDS = [(ports, anti) for ports in (False, True) for anti in (False, True)]
# the seed of the 16 extra pods at which, under every context, PortsReference alone schedules a pod of each
# kind and fails a pod with NodePorts (tests/test_chain_variants_reference.py asserts it)
EXTRA_SEED = 1


def variant_pod(rng, name, ports, anti):
    app = rng.choice(["web", "api"])
    p = Pod(name, labels={"app": app}, containers=[Container({"cpu": rng.choice([100, 250]), "memory": 128 * Mi, GPU: 1})])
    if ports:
        p.host_ports = [host_port(rng)]
    if anti:
        p.affinity_terms = [PodAffinityTerm("kubernetes.io/hostname", LabelSelector({"app": app}), kind="anti-affinity")]
    return p


def variant_pods(seed, j0, per_kind):
    """per_kind pods of each kind, interleaved."""
    rng = random.Random(seed)
    return [variant_pod(rng, f"v{j0 + j}", *KINDS[j % 4]) for j in range(4 * per_kind)]


@functools.lru_cache(maxsize=None)
def variants_reference(name, seed=EXTRA_SEED):
    """The 65-node mixed stream and then 4 chain-variant pods of each kind through PortsReference alone
    under the context `name`, computed once per process: the pods, every result, every node's state and
    used ports, and the dumps of one probe pod of each kind at the end state."""
    from helpers import res_array
    from ports_reference import PortsReference

    n = 65
    ns, ps = stream(SEEDS[n], n)
    ps = ps + variant_pods(seed, 80_000, 4)
    probes = variant_pods(2000 + seed, 95_000, 1)
    a = Arena()
    o = PortsReference(n, PAIRS, IPS, **CONTEXTS[name][0])
    na, k = nodes_array(ns, a)
    o.upsert(na, u32(range(k)), k)
    pa, m = pods_array(ps, a)
    res = res_array(o.schedule(pa, m), m)
    out = {"nodes": ns, "pods": ps, "probes": probes, "res": res, "states": o.states(),
           "used": [o.used_ports(s) for s in range(n)],
           "dumps": [o.plugin_scores(pods_array([p], a)[0]) for p in probes]}
    o.close()
    return out
