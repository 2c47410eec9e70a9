"""Reference for ks_capacity: how many more replicas of one pod the cluster
holds, as the closed form over a mirror of the node columns, in Python ints
throughout.  Nothing here comes from the product code.

A node is ELIGIBLE when the pod passes every filter before NodeResourcesFit
on it: tests/diag_reference.py's first-failure statuses (the existing
reference stack, NodePorts included) say feasible or NodeResourcesFit.  On an
eligible node the replicas stop at

    c = min(free pod slots, free_r // req_r for every resource r with req_r > 0)

with free pod slots = max(0, allocatable pods - pods on the node), free_r =
max(0, Allocatable_r - Requested_r) from the reference's node states (cpu,
memory) or from the node's extended allocatable less what its bound pods
request, and req_r the pod's request by resourcehelper.PodRequests
(diag_reference.pod_requests).  A pod with host ports holds one replica per
node at most.  The binding term of a node is the first that attains the
minimum in the order pods, cpu, memory, the extended resources in `xorder`
(the cluster's column order: the order its nodes first name them), ports last.

tests/test_capacity_reference.py pins this file against the reference
scheduler itself: replicas scheduled one by one until the first
unschedulable result land exactly per_node[slot] on every slot."""
import numpy as np

import diag_reference as R

CORE = ("cpu", "memory")


def has_host_ports(pod):
    ports = list(pod.host_ports)
    for c in pod.containers:
        ports += list(c.host_ports)
    return any(int(p[2]) > 0 for p in ports)


def node_capacity(slots_free, frees, reqs, ports):
    """(c, binding term) of one eligible node: frees / reqs are parallel lists
    of (name, value) in tie order, every req > 0; Python ints only."""
    c, who = max(0, int(slots_free)), "pods"
    for (name, free), (_, req) in zip(frees, reqs):
        q = max(0, int(free)) // int(req)
        if q < c:
            c, who = q, name
    if ports and c > 1:
        c, who = 1, "ports"
    return c, who


def capacity(ref, pod, xorder=None):
    """ref: a diag_reference.DiagReference fed the cluster's events.  Returns a
    dict with the fields of ksched.framework.Capacity (bound_by by term name,
    zero bins left out; per_node a uint32 array over the slots)."""
    status = ref.statuses(pod)
    states = ref.o.states()
    req = {k: int(v) for k, v in R.pod_requests(pod).items() if v > 0}
    xnames = [k for k in (xorder if xorder is not None else sorted(req)) if k in req and k not in CORE]
    assert sorted(xnames) == sorted(k for k in req if k not in CORE), (xnames, req)
    ports = has_host_ports(pod)
    per_node = np.zeros(ref.n, dtype=np.uint32)
    bound = {}
    eligible = room = biggest = total = 0
    for slot in sorted(ref.nodes):
        s = int(status[slot])
        assert s != -2, slot
        if s not in (-1, 4):
            continue
        nd, st = ref.nodes[slot], states[slot]
        eligible += 1
        frees, reqs = [], []
        if "cpu" in req:
            frees.append(("cpu", int(st["alloc_cpu"]) - int(st["req_cpu"])))
            reqs.append(("cpu", req["cpu"]))
        if "memory" in req:
            frees.append(("memory", int(st["alloc_mem"]) - int(st["req_mem"])))
            reqs.append(("memory", req["memory"]))
        if xnames:
            used = {}
            for q in ref.bound[slot]:
                for k, v in R.pod_requests(q).items():
                    used[k] = used.get(k, 0) + int(v)
            for name in xnames:
                frees.append((name, int(nd.extended.get(name, 0)) - used.get(name, 0)))
                reqs.append((name, req[name]))
        c, who = node_capacity(int(nd.allocatable.get("pods", 0)) - int(st["pod_count"]), frees, reqs, ports)
        assert (c >= 1) == (s == -1), (slot, c, s)  # room for one more: what the reference stack calls feasible
        per_node[slot] = c
        bound[who] = bound.get(who, 0) + 1
        room += c >= 1
        biggest = max(biggest, c)
        total += c
    return dict(num_all_nodes=len(ref.nodes), eligible_nodes=eligible, nodes_with_room=room, max_per_node=biggest,
                replicas=total, bound_by=bound, per_node=per_node)


def same(got, want):
    """A Capacity (ksched.framework) against this reference's dict; returns the differing fields."""
    bad = [k for k in want if k != "per_node" and getattr(got, k) != want[k]]
    if got.per_node is not None and not np.array_equal(got.per_node, want["per_node"]):
        bad.append("per_node")
    return bad


# ------------------------------------------------- clusters the tests share
Gi, Mi = 1 << 30, 1 << 20
GPU, DISK = "example.com/gpu", "ephemeral-storage"


def rand_cluster(rng, n, pods_hi=12, extended=True):
    """n nodes of mixed sizes in three zones, a fifth tainted, a few
    unschedulable or without room for pods; with `extended`, most carry the
    two extended resources (named in the order GPU, DISK: the column order)."""
    from ksched.objects import Node, Taint
    nodes = []
    for i in range(n):
        alloc = {"cpu": rng.choice([1000, 2000, 4000, 8000]), "memory": rng.choice([2, 4, 8, 16]) * Gi,
                 "pods": rng.choice([0, 3, 5, 8, pods_hi, pods_hi])}
        nd = Node(f"n{i}", alloc, {"zone": f"z{rng.randrange(3)}", "kubernetes.io/hostname": f"n{i}"},
                  [Taint("dedicated", "infra")] if rng.random() < 0.2 else [], unschedulable=rng.random() < 0.03)
        if extended and (i == 0 or rng.random() < 0.8):
            nd.extended[GPU] = rng.choice([1, 2, 4, 8])
            nd.extended[DISK] = rng.choice([10, 20, 50]) * Gi
        nodes.append(nd)
    return nodes


def rand_prefill(rng, n, per_node=1.0, extended=True):
    """Bound pods (pods, slots): some nodes end up over-committed in cpu, memory or pod count."""
    from ksched.objects import Container, Pod
    pods, slots = [], []
    for j in range(int(n * per_node)):
        req = {"cpu": rng.choice([100, 250, 500, 1500]), "memory": rng.choice([128, 512, 1024, 3072]) * Mi}
        if extended and rng.random() < 0.2:
            req[GPU] = 1
        if extended and rng.random() < 0.2:
            req[DISK] = rng.choice([1, 5]) * Gi
        pods.append(Pod(f"pre{j}", containers=[Container(req)]))
        slots.append(rng.randrange(n))
    return pods, slots


def shapes():
    """name -> pod: the shapes the fill tests place replica after replica."""
    from ksched.objects import Container, Pod, Toleration
    return {
        "resources": Pod("r", containers=[Container({"cpu": 300, "memory": 700 * Mi})]),
        "selector": Pod("s", containers=[Container({"cpu": 150, "memory": 1 * Gi})], node_selector={"zone": "z1"},
                        tolerations=[Toleration("dedicated", "Equal", "infra")]),
        "besteffort": Pod("b"),
        "extended": Pod("x", containers=[Container({"cpu": 200, "memory": 256 * Mi, GPU: 1, DISK: 3 * Gi})]),
    }


def float_divide_truncate(free, req):
    """The shortcut the exact quotient must not be: binary64 divide, truncate."""
    return int(float(max(0, free)) / float(req))
