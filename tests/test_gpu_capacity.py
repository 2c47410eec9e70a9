"""ks_capacity_pod / ks_capacity_pods on the GPU (ksched_capacity.hip, DESIGN
§5.19): every field against tests/capacity_reference.py or a closed form by
construction; the exact quotients on a table of edge nodes; fill parity (the
scheduler itself places exactly `replicas` more, `per_node[slot]` on every
slot); cross-checks against ks_diagnose; ties, refusals, no side effects, two
ranks, submitted batches.  Which path answered is read from
ks_debug_capacity: [0] the multi-pod kernel's pods, [1] the per-pod pass's,
[2] identical pods, [3] launches, [4] pods per group, [5] positions per turn."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import capacity_reference as CR
import diag_reference as R
from helpers import states_np
from ksched import FitError, Scheduler, _abi
from ksched.objects import (Arena, Container, LabelSelector, Node, Pod, PodAffinityTerm, TopologySpreadConstraint,
                            pods_array)
from test_gpu_diag import DiagPair, geometry_nodes, geometry_templates, u32
from test_gpu_diag_pods import geometry_pods
from test_gpu_spread import rand_res_nodes, rand_res_pod

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
GPU, DISK = CR.GPU, CR.DISK
XORDER = [GPU, DISK]
BIG = {"cpu": 64000, "memory": 256 * Gi, "pods": 200}
FIELDS = ("num_all_nodes", "eligible_nodes", "nodes_with_room", "max_per_node", "replicas", "bound_by")


def assert_cap(got, want, what=""):
    bad = CR.same(got, want)
    assert not bad, (what, bad, {k: (getattr(got, k), want[k]) for k in bad if k != "per_node"})


def strip(c):
    """A Capacity without its per-node array (dataclass equality on arrays is elementwise)."""
    return tuple(getattr(c, k) for k in FIELDS)


# ----------------------------------------------------------------- geometry
def geometry_want(slots, pod):
    """Closed form over the templates of test_gpu_diag.geometry_templates (slot % 7)."""
    req = R.pod_requests(pod)
    k = [sum(1 for s in slots if s % 7 == r) for r in range(7)]
    per_node = np.zeros(max(slots) + 1 if slots else 1, dtype=np.uint32)
    out = dict(num_all_nodes=len(slots), eligible_nodes=0, nodes_with_room=0, max_per_node=0, replicas=0, bound_by={})
    for r, t in enumerate(geometry_templates()):
        if r in (1, 2, 3, 4) or not k[r]:  # unschedulable, tainted, tainted, no disk=ssd
            continue
        c, who = CR.node_capacity(t.allocatable["pods"], [("cpu", t.allocatable["cpu"]), ("memory", t.allocatable["memory"])],
                                  [("cpu", req["cpu"]), ("memory", req["memory"])], False)
        out["eligible_nodes"] += k[r]
        out["nodes_with_room"] += k[r] * (c >= 1)
        out["max_per_node"] = max(out["max_per_node"], c)
        out["replicas"] += k[r] * c
        out["bound_by"][who] = out["bound_by"].get(who, 0) + k[r]
        per_node[[s for s in slots if s % 7 == r]] = c
    out["per_node"] = per_node
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_geometry(n):
    a = Arena()
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        G = s.capacity_counters()[4]
        assert G >= 2
        for m in sorted({1, 2, G - 1, G, G + 1, 2 * G + 3}):
            pods = geometry_pods(m)
            got = s.capacity_many(pods)
            assert len(got) == m
            for i, c in enumerate(got):
                assert_cap(c, geometry_want(slots, pods[i]), (n, m, i))
            ctr = s.capacity_counters()
            assert ctr[0] == m and ctr[1] == 0 and ctr[2] == 0, (n, m, ctr)
            assert ctr[3] == 1 and ctr[6] == 0 and ctr[7] == 0, (n, m, ctr)  # one launch: every pod reads the label columns
        # the single call, with the per-node counts
        pod = geometry_pods(1, first=5)[0]
        assert_cap(s.capacity(pod, per_node=True), geometry_want(slots, pod), n)
        assert s.capacity_counters()[:4] == [1, 0, 0, 1]


def test_geometry_grid_stride_second_turn():
    # just above the positions one launch covers in a turn: the loop's second step, its last wave partly past the end
    a = Arena()
    with Scheduler(1) as s0:
        turn = s0.capacity_counters()[5]
    assert 0 < turn <= 600_000
    n = turn + 100
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        pods = geometry_pods(3)
        want = [geometry_want(slots, p) for p in pods]
        for i, c in enumerate(s.capacity_many(pods)):
            assert_cap(c, want[i], i)
        ctr = s.capacity_counters()
        assert ctr[0] == 3 and ctr[1] == 0 and ctr[3] == 1 and ctr[5] == turn < n, ctr
        assert_cap(s.capacity(pods[1], per_node=True), want[1], "per node")


# ------------------------------------------------------------ quotient edges
REQS = [1, 3, 7, 100, 2 ** 20 + 1, 2 ** 43 - 1]
FREE_MAX = 2 ** 44 - 1
QS = sorted({0, 1, 2, 3, 5, 64, 109, 110, 111, 65535, 65536, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31} |
            {2 ** k + d for k in range(2, 31) for d in (-1, 0, 1)})
PODS_MAX = 2 ** 31 - 2  # the largest allocatable pod count a node may carry
PODS_ALLOC = [110, 3, PODS_MAX]
XBIG = "example.com/big"
XREQS = [3, 2 ** 23 + 1, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 52 + 1]


def edge_table():
    """[(Node, [bound Pod])], one case each: a free value next to a multiple of a request in cpu or in memory
    under each pod-slot bound; over-committed nodes; no pod slots; more pods than slots; extended values around
    2^53 and 2^62 next to multiples of the extended requests."""
    frees = set()
    for req in REQS:
        for q in QS:
            for d in (-1, 0, 1):
                f = q * req + d
                if 0 <= f <= FREE_MAX:
                    frees.add(f)
    frees |= {FREE_MAX, FREE_MAX - 1, 2 ** 43, 2 ** 43 - 2}
    cases = []
    for i, f in enumerate(sorted(frees)):
        ap = PODS_ALLOC[i % len(PODS_ALLOC)]
        cases.append((Node("", {"cpu": f, "memory": FREE_MAX, "pods": ap}), []))
        cases.append((Node("", {"cpu": FREE_MAX, "memory": f, "pods": PODS_ALLOC[(i + 1) % len(PODS_ALLOC)]}), []))
    hog = lambda cpu, mem: Pod("hog", containers=[Container({"cpu": cpu, "memory": mem})])
    cases.append((Node("", {"cpu": 1000, "memory": 8 * Gi, "pods": 110}), [hog(5000, 1 * Gi)]))          # cpu below zero
    cases.append((Node("", {"cpu": 8000, "memory": 1 * Gi, "pods": 110}), [hog(100, 3 * Gi)]))           # memory below zero
    cases.append((Node("", {"cpu": 1000, "memory": 1 * Gi, "pods": 110}), [hog(1001, 1 * Gi + 1)]))      # both by one
    cases.append((Node("", {"cpu": 8000, "memory": 8 * Gi, "pods": 0}), []))
    cases.append((Node("", {"cpu": 8000, "memory": 8 * Gi, "pods": 1}), [hog(1, 1), hog(1, 1), hog(1, 1)]))
    cases.append((Node("", {"cpu": 8000, "memory": 8 * Gi, "pods": 2}), [hog(1, 1), hog(1, 1)]))
    cases.append((Node("", {"cpu": 0, "memory": 0, "pods": 110}), []))
    xs = set()
    for req in XREQS:
        for base in (2 ** 53, 2 ** 62, 2 ** 63 - 1):
            q0 = base // req
            for q in (q0 - 1, q0, q0 + 1, 1, 2, 2 ** 31 - 1, 2 ** 31):
                for d in (-1, 0, 1):
                    v = q * req + d
                    if 0 <= v <= 2 ** 63 - 1:
                        xs.add(v)
    for i, v in enumerate(sorted(xs)):
        cases.append((Node("", {"cpu": 4000, "memory": 8 * Gi, "pods": [PODS_MAX, 110][i % 2]}, extended={XBIG: v}), []))
    for i, (nd, _) in enumerate(cases):
        nd.name = f"e{i}"
    return cases


def edge_pods():
    pods = [Pod("be")]
    for req in REQS:
        pods.append(Pod(f"c{req}", containers=[Container({"cpu": req})]))
        pods.append(Pod(f"m{req}", containers=[Container({"memory": req})]))
        pods.append(Pod(f"cm{req}", containers=[Container({"cpu": req, "memory": req})]))
    return pods


def edge_want(cases, pod):
    """The closed form in Python ints, every node eligible (no taints, no selectors)."""
    req = {k: v for k, v in R.pod_requests(pod).items() if v > 0}
    out = dict(num_all_nodes=len(cases), eligible_nodes=len(cases), nodes_with_room=0, max_per_node=0, replicas=0,
               bound_by={}, per_node=np.zeros(len(cases), dtype=np.uint32))
    for slot, (nd, bound) in enumerate(cases):
        used = {}
        for q in bound:
            for k, v in R.pod_requests(q).items():
                used[k] = used.get(k, 0) + v
        frees, reqs = [], []
        for name in ["cpu", "memory"] + sorted(k for k in req if k not in ("cpu", "memory")):
            if name in req:
                alloc = nd.allocatable[name] if name in ("cpu", "memory") else nd.extended.get(name, 0)
                frees.append((name, alloc - used.get(name, 0)))
                reqs.append((name, req[name]))
        c, who = CR.node_capacity(nd.allocatable["pods"] - len(bound), frees, reqs, False)
        out["per_node"][slot] = c
        out["nodes_with_room"] += c >= 1
        out["max_per_node"] = max(out["max_per_node"], c)
        out["replicas"] += c
        out["bound_by"][who] = out["bound_by"].get(who, 0) + 1
    return out


@pytest.fixture(scope="module")
def edges():
    cases = edge_table()
    assert 2000 <= len(cases) <= 8000, len(cases)
    n = len(cases)
    s = Scheduler(n)
    s.upsert_nodes([nd for nd, _ in cases], list(range(n)))
    for slot, (_, bound) in enumerate(cases):
        if bound:
            s.add_pods(bound, [slot] * len(bound))
    yield s, cases
    s.close()


def test_quotient_edges_the_float_shortcut_fails_on_this_table():
    cases = edge_table()
    wrong = 0
    for pod in edge_pods()[1:] + [Pod("x", containers=[Container({"cpu": 1, XBIG: r})]) for r in XREQS]:
        req = {k: v for k, v in R.pod_requests(pod).items() if v > 0}
        for nd, bound in cases:
            if bound:
                continue
            for name, r in req.items():
                free = nd.allocatable[name] if name in ("cpu", "memory") else nd.extended.get(name, 0)
                wrong += CR.float_divide_truncate(free, r) != max(0, free) // r
    assert wrong >= 10, wrong


def test_quotient_edges_multi_pod_kernel(edges):
    s, cases = edges
    pods = edge_pods()
    got = s.capacity_many(pods)
    ctr = s.capacity_counters()
    assert ctr[0] == len(pods) and ctr[1] == 0 and ctr[2] == 0 and ctr[3] == 1, ctr  # no pod reads a label column
    want = [edge_want(cases, p) for p in pods]
    for p, c, w in zip(pods, got, want):
        assert_cap(c, w, p.name)
    assert want[0]["bound_by"].keys() == {"pods"}  # the best-effort pod: slots alone
    assert any(w["max_per_node"] == PODS_MAX for w in want) and any(w["replicas"] > 2 ** 32 for w in want)
    # node by node: the single call's per-node counts
    for p, w in list(zip(pods, want))[::3]:
        assert_cap(s.capacity(p, per_node=True), w, p.name + " per node")
        assert s.capacity_counters()[:4] == [1, 0, 0, 1]


def test_quotient_edges_extended(edges):
    s, cases = edges
    pods = [Pod(f"x{r}", containers=[Container({"cpu": 1, XBIG: r})]) for r in XREQS]
    want = [edge_want(cases, p) for p in pods]
    got = s.capacity_many(pods)
    ctr = s.capacity_counters()
    assert ctr[0] == 0 and ctr[1] == len(pods) and ctr[3] == 0, ctr  # the per-pod pass
    for p, c, w in zip(pods, got, want):
        assert_cap(c, w, p.name)
        assert w["bound_by"].get(XBIG, 0) > 0 and w["bound_by"].get("pods", 0) > 0 and w["bound_by"].get("cpu", 0) > 0, w
        assert_cap(s.capacity(p, per_node=True), w, p.name + " per node")


# --------------------------------------------------------------- fill parity
PORT = ("TCP", 8080)


def port_pod():
    return Pod("h", containers=[Container({"cpu": 100, "memory": 64 * Mi}, host_ports=[(None, "TCP", 8080)])])


def fill_cluster(seed, n, **cfg):
    rng = random.Random(seed)
    x = DiagPair(n, pairs=[PORT], **cfg)
    x.upsert(CR.rand_cluster(rng, n), list(range(n)))
    pods, slots = CR.rand_prefill(rng, n)
    x.add(pods, slots)
    # a tenth of the nodes already hold the port (host ports need percentage_of_nodes_to_score 100)
    held = rng.sample(range(n), n // 10) if "percentage_of_nodes_to_score" not in cfg else []
    x.add([Pod(f"held{j}", containers=[Container({"cpu": 10}, host_ports=[(None, "TCP", 8080)])]) for j in held], held)
    return x


def fill_and_compare(x, pod, want, what):
    s, n = x.s, x.n
    got = s.capacity(pod, per_node=True)
    assert_cap(got, want, what)
    before = states_np(s.lib.ks_node_states, s.ctx, n)["pod_count"].astype(np.int64)
    placed, done = 0, False
    while not done:
        assert placed <= want["replicas"], (what, "the fill does not end")
        res = s.schedule_pods([pod] * 256)
        ok = [not isinstance(r, Exception) for r in res]
        k = ok.index(False) if False in ok else len(ok)
        assert all(ok[:k]) and not any(ok[k:]) and all(isinstance(r, FitError) for r in res[k:]), what
        placed += k
        done = k < len(ok)
    assert placed == got.replicas, what
    delta = states_np(s.lib.ks_node_states, s.ctx, n)["pod_count"].astype(np.int64) - before
    assert np.array_equal(delta, got.per_node.astype(np.int64)), (what, np.nonzero(delta != got.per_node)[0][:5])
    after = s.capacity(pod)
    assert after.replicas == 0 and after.nodes_with_room == 0 and after.max_per_node == 0, (what, after)
    assert after.eligible_nodes == (got.eligible_nodes if not CR.has_host_ports(pod) else
                                    got.eligible_nodes - got.nodes_with_room), (what, after)


def fill_shapes():
    sh = CR.shapes()
    return {"resources": sh["resources"], "selector": sh["selector"], "extended": sh["extended"], "port": port_pod()}


def reference_is_not_trivial(x, pod, want):
    """At least a quarter of the eligible nodes hold two or more (of the pod without its ports), and three binding terms."""
    plain = want
    if CR.has_host_ports(pod):
        bare = Pod("bare", containers=[Container(dict(pod.containers[0].requests))])
        plain = CR.capacity(x.ref, bare, XORDER)
        assert want["bound_by"].get("ports", 0) > 0 and want["max_per_node"] == 1, want
        assert want["eligible_nodes"] < plain["eligible_nodes"]  # the nodes holding the port are not eligible
    assert 4 * int((plain["per_node"] >= 2).sum()) >= plain["eligible_nodes"] > 0, plain
    assert len([v for v in want["bound_by"].values() if v]) >= 3, want["bound_by"]


@pytest.mark.parametrize("n", [300, 1500])
@pytest.mark.parametrize("shape", ["resources", "selector", "extended", "port"])
def test_fill_parity(shape, n):
    x = fill_cluster(100 + n, n, pods_per_round=256)
    pod = fill_shapes()[shape]
    want = CR.capacity(x.ref, pod, XORDER)
    reference_is_not_trivial(x, pod, want)
    fill_and_compare(x, pod, want, (shape, n))
    x.close()


@pytest.mark.parametrize("shape,cfg", [("resources", dict(fit_strategy="MostAllocated")),
                                       ("extended", dict(fit_strategy="MostAllocated")),
                                       ("resources", dict(percentage_of_nodes_to_score=5)),
                                       ("selector", dict(percentage_of_nodes_to_score=5))])
def test_fill_parity_does_not_depend_on_the_profile(shape, cfg):
    n = 300
    x = fill_cluster(100 + n, n, pods_per_round=256, **cfg)
    pod = fill_shapes()[shape]
    want = CR.capacity(x.ref, pod, XORDER)  # the same answer as test_fill_parity's: the reference knows no profile
    reference_is_not_trivial(x, pod, want)
    fill_and_compare(x, pod, want, (shape, cfg))
    x.close()


# -------------------------------------------------------------- cross-checks
def stream_cluster(seed, n):
    rng = random.Random(seed)
    x = DiagPair(n, pods_per_round=64)
    nodes = rand_res_nodes(rng, n)
    x.upsert(nodes, list(range(n)))
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(2 * n)]  # a crowded cluster
    for p in pre:
        p.topology_spread = []
    x.add(pre, [rng.randrange(n) for _ in pre])
    xorder = []
    for nd in nodes:  # the cluster's column order: first naming
        xorder += [k for k in nd.extended if k not in xorder]
    return rng, x, xorder


def test_random_stream_cross_checks():
    rng, x, xorder = stream_cluster(81, 400)
    s = x.s
    probes = [rand_res_pod(rng, j) for j in range(60)]
    got = s.capacity_many(probes, strict=False)
    ctr = s.capacity_counters()
    refused = [p for p, c in zip(probes, got) if c is None]
    assert ctr[0] > 0 and ctr[1] > 0 and ctr[0] + ctr[1] + ctr[2] == len(probes) - len(refused), ctr
    hard = lambda p: any(t.when_unsatisfiable == "DoNotSchedule" for t in p.topology_spread)
    assert [p.name for p in refused] == [p.name for p in probes if hard(p)] and refused
    answered = 0
    for p, c in zip(probes, got):
        if c is None:
            with pytest.raises(_abi.KschedError) as e:
                s.capacity(p)
            assert e.value.status == _abi.KS_ERR_UNSUPPORTED and "DoNotSchedule" in str(e.value)
            continue
        answered += 1
        assert c.nodes_with_room == s.diagnose(p).feasible_nodes, p.name
        assert sum(c.bound_by.values()) == c.eligible_nodes, p.name
        one = s.capacity(p, per_node=True)
        assert strip(one) == strip(c), p.name
        assert int(one.per_node.astype(np.uint64).sum()) == c.replicas and int((one.per_node >= 1).sum()) == c.nodes_with_room
        assert_cap(one, CR.capacity(x.ref, p, xorder), p.name)
    assert answered >= 30
    x.close()


def test_identical_pods_are_answered_once():
    a = Arena()
    n = 200
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        distinct = geometry_pods(5, first=1)
        copies = geometry_pods(1) * 100
        pods = copies[:30] + distinct[:2] + copies[30:70] + distinct[2:] + copies[70:]
        got = s.capacity_many(pods)
        ctr = s.capacity_counters()
        assert ctr[0] == 6 and ctr[1] == 0 and ctr[2] == 99, ctr
        for p, c in zip(pods, got):
            assert_cap(c, geometry_want(slots, p), p.name)
        # a host port no node holds leaves no trace in the compiled pod, yet it caps every node at one
        with_port = Pod("wp", containers=[Container({"cpu": 100, GPU: 1}, host_ports=[(None, "TCP", 4242)])], node_name="g0")
        without = Pod("wo", containers=[Container({"cpu": 100, GPU: 1})], node_name="g0")
        s.upsert_nodes([Node("g0", BIG, {"disk": "ssd"}, extended={GPU: 4})], [0])
        a2, b2 = s.capacity_many([with_port, without])
        assert s.capacity_counters()[1] == 2 and s.capacity_counters()[2] == 0
        assert (a2.replicas, a2.bound_by) == (1, {"ports": 1}) and (b2.replicas, b2.bound_by) == (4, {GPU: 1})


# ------------------------------------------------------- tie order of bound_by
def test_tie_order():
    pod = Pod("t", containers=[Container({"cpu": 100, "memory": 100, "aa.example/one": 1, "bb.example/two": 2})])
    ported = Pod("tp", containers=[Container(dict(pod.containers[0].requests), host_ports=[(None, "TCP", 9000)])])
    X1, X2 = "aa.example/one", "bb.example/two"
    mk = lambda pods, cpu, mem, x1, x2: Node("", {"cpu": cpu, "memory": mem, "pods": pods}, extended={X1: x1, X2: x2})
    rows = [  # (node, binding term, c): without ports
        (mk(5, 500, 500, 5, 10), "pods", 5),        # five terms tie
        (mk(6, 500, 500, 5, 10), "cpu", 5),         # four
        (mk(6, 600, 599, 5, 11), "memory", 5),      # memory and both extended tie
        (mk(6, 600, 600, 5, 10), X1, 5),            # the extended columns tie: the lower column
        (mk(6, 600, 600, 6, 11), X2, 5),
        (mk(0, 99, 99, 0, 1), "pods", 0),           # the zero minimum: all five
        (mk(3, 99, 99, 0, 1), "cpu", 0),
        (mk(3, 100, 99, 0, 1), "memory", 0),
        (mk(3, 100, 100, 0, 1), X1, 0),
        (mk(3, 100, 100, 1, 1), X2, 0),
        (mk(1, 100, 100, 1, 2), "pods", 1),         # one: ports never bind
        (mk(2, 200, 200, 2, 4), "pods", 2),         # two and more: ports bind with them
        (mk(9, 900, 200, 9, 18), "memory", 2),
    ]
    for i, (nd, _, _) in enumerate(rows):
        nd.name = f"t{i}"
    n = len(rows)
    with Scheduler(n) as s:
        s.upsert_nodes([nd for nd, _, _ in rows], list(range(n)))
        for slot, (_, who, c) in enumerate(rows):
            for p in (pod, ported):
                cc, ww = (1, "ports") if p is ported and c > 1 else (c, who)
                # one node at a time: every other node is made ineligible by name
                q = Pod(p.name, containers=p.containers, node_name=f"t{slot}")
                got = s.capacity(q, per_node=True)
                assert (got.eligible_nodes, got.replicas, got.bound_by) == (1, cc, {ww: 1}), (slot, p.name, got)
                assert got.per_node[slot] == cc and int(got.per_node.sum()) == cc
        # and all at once
        got = s.capacity(pod)
        want = {}
        for _, who, _ in rows:
            want[who] = want.get(who, 0) + 1
        assert got.bound_by == want and got.eligible_nodes == n and got.replicas == sum(c for _, _, c in rows)
        got = s.capacity(ported)
        want = {}
        for _, who, c in rows:
            w = "ports" if c > 1 else who
            want[w] = want.get(w, 0) + 1
        assert got.bound_by == want and got.replicas == sum(min(c, 1) for _, _, c in rows) and got.max_per_node == 1


# ------------------------------------------------------- refusals and edges
def test_refusals_and_edge_arguments():
    zone = "topology.kubernetes.io/zone"
    sel = LabelSelector({"app": "web"})
    nodes = [Node(f"n{i}", BIG, {zone: f"z{i % 2}", "kubernetes.io/hostname": f"n{i}"}) for i in range(6)]
    plain = lambda j: Pod(f"ok{j}", containers=[Container({"cpu": 1000 + j})])
    dns = Pod("dns", containers=[Container({"cpu": 100})], labels={"app": "web"},
              topology_spread=[TopologySpreadConstraint(1, zone, "DoNotSchedule", sel)])
    aff = Pod("aff", containers=[Container({"cpu": 100})], affinity_terms=[PodAffinityTerm(zone, sel, kind="affinity")])
    anti = Pod("anti", containers=[Container({"cpu": 100})],
               affinity_terms=[PodAffinityTerm(zone, sel, kind="anti-affinity")])
    selected = Pod("selected", containers=[Container({"cpu": 100})], labels={"app": "db"})
    guard = Pod("guard", containers=[Container({"cpu": 100})],
                affinity_terms=[PodAffinityTerm(zone, LabelSelector({"app": "db"}), kind="anti-affinity")])
    vol = Pod("vol", unmodelled=["volumes"])
    soft = Pod("soft", containers=[Container({"cpu": 1000})], labels={"app": "web"},
               topology_spread=[TopologySpreadConstraint(1, zone, "ScheduleAnyway", sel)],
               affinity_terms=[PodAffinityTerm(zone, sel, kind="preferred-affinity", weight=10),
                               PodAffinityTerm(zone, sel, kind="preferred-anti-affinity", weight=5)])
    a = Arena()
    with Scheduler(6) as s:
        s.upsert_nodes(nodes, list(range(6)))
        s.add_pods([guard], [0])
        lib, ctx = s.lib, s.ctx
        pods = [plain(0), dns, plain(1), aff, anti, selected, vol, plain(2), soft]
        pa, m = pods_array(pods, a)
        chk = (C.c_int32 * m)()
        want_st = lib.ks_pods_check(ctx, pa, m, chk)
        assert want_st == _abi.KS_ERR_UNSUPPORTED and [i for i in range(m) if chk[i]] == [6]
        out = (_abi.KsPodCapacity * m)()
        U = _abi.KS_ERR_UNSUPPORTED
        assert lib.ks_capacity_pods(ctx, pa, m, out) == U
        err = lib.ks_last_error(ctx).decode()
        assert err.startswith("pod 1:") and "DoNotSchedule" in err, err  # the first refusal, by index
        assert [o.status for o in out] == [0, U, 0, U, U, U, U, 0, 0]
        for i in (1, 3, 4, 5, 6):
            assert bytes(out[i].c) == bytes(_abi.KsCapacity()), i  # a zeroed record
        for i, cpu in ((0, 1000), (2, 1001), (7, 1002), (8, 1000)):
            want = [(64000 - 100) // cpu] + [64000 // cpu] * 5  # node 0 holds the guard's 100 millicores
            assert out[i].c.replicas == sum(want) and out[i].c.eligible_nodes == 6, i
            assert out[i].c.max_per_node == max(want) and out[i].c.bound_by[_abi.CAP_CPU] == 6, i
        # ScheduleAnyway and preferred terms only score: the same answer as with them stripped
        bare = Pod("bare", containers=[Container({"cpu": 1000})], labels={"app": "web"})
        assert strip(s.capacity(soft)) == strip(s.capacity(bare))
        # each refusal names its reason; a pod ks_pods_check refuses keeps that call's status and text
        for p, word in ((dns, "DoNotSchedule"), (aff, "required pod affinity"), (anti, "required pod anti-affinity"),
                        (selected, "bound pod's required anti-affinity")):
            with pytest.raises(_abi.KschedError) as e:
                s.capacity(p)
            assert e.value.status == U and word in str(e.value), (p.name, str(e.value))
        with pytest.raises(_abi.KschedError) as e:
            s.capacity(vol)
        assert e.value.status == want_st and "volumes" in str(e.value).lower()
        pa1, _ = pods_array([vol], a)
        one = _abi.KsCapacity()
        lib.ks_pods_check(ctx, pa1, 1, chk)
        vol_err = lib.ks_last_error(ctx).decode()
        assert lib.ks_capacity_pod(ctx, pa1, C.byref(one), None) == want_st and lib.ks_last_error(ctx).decode() == vol_err
        with pytest.raises(_abi.KschedError):
            s.capacity_many(pods)
        got = s.capacity_many(pods, strict=False)
        assert [c is None for c in got] == [False, True, False, True, True, True, True, False, False]
        # n == 0
        assert lib.ks_capacity_pods(ctx, None, 0, None) == 0 and s.capacity_many([]) == []
        # null arguments
        pa, m = pods_array([plain(0), plain(1)], a)
        out = (_abi.KsPodCapacity * m)()
        for args in ((None, pa, m, out), (ctx, None, m, out), (ctx, pa, m, None)):
            assert lib.ks_capacity_pods(*args) == _abi.KS_ERR_INVALID
        for args in ((None, pa, C.byref(one), None), (ctx, None, C.byref(one), None), (ctx, pa, None, None)):
            assert lib.ks_capacity_pod(*args) == _abi.KS_ERR_INVALID
        assert lib.ks_debug_capacity(ctx, None) == _abi.KS_ERR_INVALID and lib.ks_debug_capacity(None, None) == _abi.KS_ERR_INVALID
        # the context still answers
        assert s.capacity(plain(0)).replicas == out_replicas(64000, 100, 1000)


def out_replicas(alloc, held, cpu):
    return (alloc - held) // cpu + 5 * (alloc // cpu)


# ------------------------------------------------------------ no side effects
def test_no_side_effects():
    rng, x, xorder = stream_cluster(91, 300)
    s, n = x.s, x.n
    a = Arena()
    first = [Pod(f"f{j}", containers=[Container({"cpu": 10})]) for j in range(3)]
    x.schedule_equal(first, "first")
    # the strings of an earlier ks_diagnose
    probe = Pod("probe", containers=[Container({"cpu": 100, "memory": 64 * Gi})])
    pa1, _ = pods_array([probe], a)
    d, cnt = _abi.KsDiagnosis(), C.c_uint32(0)
    rows = (_abi.KsReason * _abi.DIAG_MAX_REASONS)()
    assert s.lib.ks_diagnose(s.ctx, pa1, C.byref(d), rows, len(rows), C.byref(cnt)) == 0 and cnt.value >= 1
    ptr = lambda r: C.c_void_p.from_buffer(r, _abi.KsReason.reason.offset).value
    text = [(ptr(rows[i]), rows[i].reason) for i in range(cnt.value)]
    before = states_np(s.lib.ks_node_states, s.ctx, n)
    start = s.next_start_index()
    probes = [rand_res_pod(rng, j) for j in range(30)]
    for p in probes:
        p.topology_spread, p.init_containers = [], []
    got = s.capacity_many(probes)
    assert [strip(s.capacity(p)) for p in probes] == [strip(c) for c in got]
    assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, n), before)
    assert s.next_start_index() == start
    assert [(ptr(rows[i]), rows[i].reason) for i in range(cnt.value)] == text
    # a following batch equals the reference's, which saw no capacity call at all
    x.schedule_equal([rand_res_pod(rng, 7000 + j) for j in range(60)], "after capacity")
    x.close()


def test_host_port_dictionary_is_not_consumed():
    port_pod_ = lambda j, port: Pod(f"p{j}", containers=[Container({"cpu": 10})], host_ports=[(None, "TCP", port)])
    with Scheduler(4) as s:
        s.upsert_nodes([Node(f"n{i}", BIG) for i in range(4)], [0, 1, 2, 3])
        s.add_pods([port_pod_(900, 8000)], [1])
        # 64 fresh triples and a held one, between plain pods, asked about only
        pods = [Pod("a", containers=[Container({"cpu": 10})])] + [port_pod_(j, 1000 + j) for j in range(64)] + \
            [port_pod_(99, 8000), Pod("b", containers=[Container({"cpu": 20})])]
        got = s.capacity_many(pods)
        assert all(c.replicas == 4 and c.bound_by == {"ports": 4} and c.eligible_nodes == 4 for c in got[1:65])
        assert got[65].eligible_nodes == 3 and got[65].replicas == 3 and got[65].bound_by == {"ports": 3}
        assert got[0].bound_by == {"pods": 4} and got[0].replicas == 199 + 3 * 200
        for j in range(64):
            assert s.capacity(port_pod_(j, 3000 + j)).replicas == 4
        assert s.node_used_ports(0) == [] and s.node_used_ports(1) == [("0.0.0.0", "TCP", 8000)]
        # the dictionary still has room for 63 more triples: none of the queried ones was interned
        res = s.schedule_pods([port_pod_(100 + j, 2000 + j) for j in range(63)])
        assert all(not isinstance(r, Exception) for r in res)


# ------------------------------------------------------------------ two ranks
def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "capacity_multirank_main.py")], capture_output=True,
                       text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["answered"] >= 30 and res["kernel_pods"] > 0 and res["chain_pods"] > 0


# ---------------------------------------------------------- submitted batches
def test_waits_for_submitted_batches():
    rng = random.Random(71)
    n = 2000
    a = Arena()
    nodes = rand_res_nodes(rng, n)
    with Scheduler(n, pods_per_round=64) as s:
        s.upsert_nodes(nodes, list(range(n)))
        batches = [[rand_res_pod(rng, b * 1000 + j) for j in range(150)] for b in range(3)]
        arrs = [pods_array(p, a) for p in batches]
        probes = [rand_res_pod(rng, 9000 + j) for j in range(20)]
        for p in probes:
            p.topology_spread = []
        hs = []
        for pa, m in arrs:
            h = s.prepare(pa, m)
            assert s.lib.ks_batch_submit(s.ctx, h) == 0, s.lib.ks_last_error(s.ctx)
            hs.append(h)
        got = s.capacity_many(probes)  # while the batches are in flight
        for h in hs:
            assert s.lib.ks_batch_wait(s.ctx, h) == 0, s.lib.ks_last_error(s.ctx)
            s.free(h)
        assert [strip(c) for c in got] == [strip(s.capacity(p)) for p in probes]
        assert any(c.replicas for c in got)
