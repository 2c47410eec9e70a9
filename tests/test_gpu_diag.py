"""ks_diagnose on the GPU (ksched_diag.hip): the reasons of every
node's status for one pod, against known answers by construction (geometry),
the hand-derived cases of tests/diag_cases.py, and tests/diag_reference.py on
random streams; agreement with what scheduling the pod reports; no side
effects; two in-process ranks; refusals."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import diag_cases as DC
import diag_reference as R
from helpers import res_array, states_np
from ksched import Scheduler, _abi
from ksched.objects import Arena, Container, Node, Pod, Taint, Toleration, nodes_array, pods_array
from test_gpu_spread import rand_ipa_pod, rand_nodes, rand_res_nodes, rand_res_pod

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
TAINT = R.TAINT


def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def assert_same(got, want, what=""):
    bad = R.same(got, want)
    assert not bad, (what, bad, {k: (getattr(got, k), want[k]) for k in bad})


def tally(s, pod, n):
    """First-failure counts from ks_plugin_scores: (plugin_nodes, NodePorts nodes, feasible nodes)."""
    st = np.array([x.status for x in s.plugin_scores(pod)[:n]])
    return [int((st == k).sum()) for k in range(8)], int((st == 8).sum()), int((st == -1).sum())


# ----------------------------------------------------------------- geometry
# The reason is a function of slot % 7, so the expected counts are closed-form:
#   0 feasible            1 unschedulable            2 one untolerated taint (a)
#   3 taints [b, a], both untolerated: b, the first in node order (the multi-taint list)
#   4 no disk=ssd label: NodeAffinity        5 no room for a pod and too little cpu: two reasons
#   6 too little memory
def geometry_templates():
    ssd = {"disk": "ssd"}
    big = {"cpu": 4000, "memory": 8 * Gi, "pods": 110}
    return [Node("t0", big, ssd), Node("t1", big, ssd, unschedulable=True),
            Node("t2", big, ssd, [Taint("a", "1")]),
            Node("t3", big, ssd, [Taint("b", "2", "NoExecute"), Taint("a", "1")]),
            Node("t4", big, {"disk": "hdd"}),
            Node("t5", {"cpu": 50, "memory": 8 * Gi, "pods": 0}, ssd),
            Node("t6", {"cpu": 4000, "memory": 64 * Mi, "pods": 110}, ssd)]


def geometry_pod():
    return Pod("p", containers=[Container({"cpu": 100, "memory": 128 * Mi})], node_selector={"disk": "ssd"})


def geometry_nodes(slots, a):
    """A ks_node per slot, the template of slot % 7 under its own name."""
    ta, _ = nodes_array(geometry_templates(), a)
    arr = (_abi.KsNode * max(1, len(slots)))()
    names = [f"g{s}".encode() for s in slots]
    for i, s in enumerate(slots):
        arr[i] = ta[s % 7]
        arr[i].name = names[i]
    a._keep.append((arr, names))
    return arr


def geometry_want(slots):
    k = [sum(1 for s in slots if s % 7 == r) for r in range(7)]
    reasons = {R.UNSCHEDULABLE: k[1], TAINT % ("a", "1"): k[2], TAINT % ("b", "2"): k[3], R.AFFINITY: k[4],
               R.TOO_MANY_PODS: k[5], R.INSUFFICIENT % "cpu": k[5], R.INSUFFICIENT % "memory": k[6]}
    reasons = {r: c for r, c in reasons.items() if c}
    return dict(num_all_nodes=len(slots), feasible_nodes=k[0], plugin_nodes=[k[1], 0, k[2] + k[3], k[4], k[5] + k[6], 0, 0, 0],
                node_ports_nodes=0, reasons=reasons, prefilter_msg=None, message=R.message(len(slots), reasons))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 2500])
def test_geometry(n):
    a = Arena()
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        assert_same(s.diagnose(geometry_pod()), geometry_want(slots), n)


def test_geometry_capacity_above_n_with_deleted_slots():
    a = Arena()
    cap = 3000
    slots = [s for s in range(2100) if s % 3 != 1]  # every third slot never filled
    with Scheduler(cap) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), len(slots))
        gone = [s_ for s_ in slots if s_ % 5 == 0 and s_ > 64]  # ... and a fifth of the rest deleted again
        s.delete_slots(gone)
        left = [s_ for s_ in slots if s_ not in set(gone)]
        assert_same(s.diagnose(geometry_pod()), geometry_want(left))


def test_geometry_more_than_one_grid_stride():
    # above 256 blocks x 1024 threads: the grid-stride loop's second step, its tail wave partly past the end
    a = Arena()
    n = 270_000
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        assert_same(s.diagnose(geometry_pod()), geometry_want(slots), n)


# ------------------------------------------------------------------- taints
def test_63_distinct_hard_taints():
    # the whole dictionary: bits 0 and 62 both decide; 70 nodes, the last 7 repeat the first taints
    n = 70
    nodes = [Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 110}, {}, [Taint(f"k{i % 63}", f"v{i % 63}")])
             for i in range(n)]
    with Scheduler(n) as s:
        s.upsert_nodes(nodes, list(range(n)))
        d = s.diagnose(Pod("p"))
        want = {TAINT % (f"k{i}", f"v{i}"): (2 if i < 7 else 1) for i in range(63)}
        assert d.reasons == want and d.plugin_nodes[2] == n and d.feasible_nodes == 0
        # tolerating the first and the last leaves their nodes feasible
        d = s.diagnose(Pod("p", tolerations=[Toleration("k0", "Equal", "v0"), Toleration("k62", "Exists")]))
        assert d.feasible_nodes == 3 and TAINT % ("k0", "v0") not in d.reasons and TAINT % ("k62", "v62") not in d.reasons
        assert d.reasons[TAINT % ("k1", "v1")] == 2 and d.reasons[TAINT % ("k61", "v61")] == 1


def test_three_taints_first_is_not_the_lowest_bit():
    big = {"cpu": 4000, "memory": 8 * Gi, "pods": 110}
    # dictionary bits follow first appearance: x 0, y 1, z 2; the last node lists them as z, x, y
    nodes = [Node("n0", big, {}, [Taint("x", "")]), Node("n1", big, {}, [Taint("y", "")]),
             Node("n2", big, {}, [Taint("z", "")]), Node("n3", big, {}, [Taint("z", ""), Taint("x", ""), Taint("y", "")])]
    with Scheduler(4) as s:
        s.upsert_nodes(nodes, [0, 1, 2, 3])
        d = s.diagnose(Pod("p"))
        assert d.reasons == {TAINT % ("x", ""): 1, TAINT % ("y", ""): 1, TAINT % ("z", ""): 2}
        # an upsert that reorders the node's taints changes its reason
        nodes[3].taints = [Taint("y", ""), Taint("z", ""), Taint("x", "")]
        s.upsert_nodes([nodes[3]], [3])
        assert s.diagnose(Pod("p")).reasons == {TAINT % ("x", ""): 1, TAINT % ("y", ""): 2, TAINT % ("z", ""): 1}


# -------------------------------------------------------- hand-derived cases
class DiagPair:
    """libksched and DiagReference fed the same cache events."""

    def __init__(self, n, pairs=(), ips=(), **cfg):
        self.n = n
        self.s = Scheduler(n, **cfg)
        self.ref = R.DiagReference(n, pairs, ips)

    def upsert(self, nodes, slots):
        self.s.upsert_nodes(nodes, slots)
        self.ref.upsert(nodes, slots)

    def delete(self, slots):
        self.s.delete_slots(slots)
        self.ref.delete(slots)

    def add(self, pods, slots, sign=1):
        if pods:
            (self.s.add_pods if sign > 0 else self.s.remove_pods)(pods, slots)
            self.ref.add(pods, slots, sign)

    def diagnose_equal(self, pod, what=""):
        d, w = self.s.diagnose(pod), self.ref.diagnose(pod)
        assert_same(d, w, what)
        assert (d.plugin_nodes, d.node_ports_nodes, d.feasible_nodes) == tally(self.s, pod, self.n), what
        return d

    def schedule_equal(self, pods, what=""):
        a = Arena()
        pa, m = pods_array(pods, a)
        got, want = res_array(self.s.schedule_raw(pa, m), m), res_array(self.ref.schedule(pods), m)
        assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:5])
        return got

    def close(self):
        self.s.close()
        self.ref.close()


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_case(name):
    nodes, bound, pod, want = DC.CASES[name]()
    ports = name == "node_ports"
    x = DiagPair(len(nodes), DC.PORT_PAIRS if ports else (), DC.PORT_IPS if ports else ())
    x.upsert(nodes, list(range(len(nodes))))
    x.add([p for p, _ in bound], [s for _, s in bound])
    d = x.s.diagnose(pod)
    for k, v in want.items():
        assert getattr(d, k) == v, (name, k, getattr(d, k), v)
    assert d.num_all_nodes == len(nodes)
    if not ports:  # (the score dump of a pod with host ports is the reference stack's business: test_gpu_ports.py)
        x.diagnose_equal(pod, name)
    else:
        assert_same(d, x.ref.diagnose(pod), name)
    x.close()


# ---------------------------------------------------- random streams, parity
def stream(x, rng, make_pod, batches, per_batch, what):
    """Every pod is diagnosed before it is scheduled; both must equal the reference's."""
    seen = set()
    for b in range(batches):
        for j in range(per_batch):
            p = make_pod(rng, b * 1000 + j)
            d = x.diagnose_equal(p, f"{what} batch {b} pod {j}")
            seen |= set(d.reasons)
            r = x.schedule_equal([p], f"{what} batch {b} pod {j}")
            # agreement with scheduling: an unschedulable pod's counts are the diagnosis'
            if r["status"][0] == 1:
                assert d.feasible_nodes == 0 and d.plugin_nodes == [int(v) for v in r["fail"][0]], (what, b, j)
    return seen


@pytest.mark.parametrize("seed,n,batches,per_batch", [(41, 300, 3, 40), (42, 1500, 2, 20)])
def test_random_stream_resources(seed, n, batches, per_batch):
    rng = random.Random(seed)
    x = DiagPair(n, pods_per_round=64)
    x.upsert(rand_res_nodes(rng, n), list(range(n)))
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(2 * n)]  # a crowded cluster: NodeResourcesFit has work
    for p in pre:
        p.topology_spread = []
    x.add(pre, [rng.randrange(n) for _ in pre])
    seen = stream(x, rng, rand_res_pod, batches, per_batch, f"seed {seed}")
    assert any(r.startswith("Insufficient ") and r not in ("Insufficient cpu", "Insufficient memory") for r in seen), seen
    assert {"Insufficient cpu", "Insufficient memory"} & seen
    x.close()


@pytest.mark.parametrize("seed,n,zones,batches,per_batch", [(51, 300, 3, 3, 40), (52, 1200, 10, 2, 20)])
def test_random_stream_affinity(seed, n, zones, batches, per_batch):
    rng = random.Random(seed)
    x = DiagPair(n, pods_per_round=64)
    x.upsert(rand_nodes(rng, n, zones), list(range(n)))
    pre = [rand_ipa_pod(rng, 10_000 + j, frac=0.15, spread_frac=0.0) for j in range(n // 2)]
    x.add(pre, [rng.randrange(n) for _ in pre])
    seen = stream(x, rng, lambda g, j: rand_ipa_pod(g, j, frac=0.6, spread_frac=0.5), batches, per_batch, f"seed {seed}")
    assert {R.IPA_AFF, R.IPA_ANTI, R.IPA_EXIST, R.SPREAD_SKEW} & seen, seen
    x.close()


# -------------------------------------------------- agreement with scheduling
def test_agrees_with_an_unschedulable_result():
    a = Arena()
    n = 200
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        # nothing fits this pod: every node fails somewhere
        p = Pod("huge", containers=[Container({"cpu": 10 ** 6, "memory": 128 * Mi})], node_selector={"disk": "ssd"})
        r = s.schedule_raw(pods_array([p], a)[0], 1)[0]
        assert r.status == 1
        d = s.diagnose(p)
        assert d.plugin_nodes == [int(v) for v in r.fail_counts] and d.node_ports_nodes == r.fail_node_ports
        assert d.feasible_nodes == 0 and d.num_all_nodes == r.evaluated_nodes == n
        assert sum(d.plugin_nodes) == n and d.message.startswith(f"0/{n} nodes are available: ")


def test_agrees_with_node_ports_result():
    nodes, bound, pod, _ = DC.CASES["node_ports"]()
    nodes[2].allocatable["cpu"] = 50  # the last free node is too small: unschedulable, NodePorts and Fit both blamed
    a = Arena()
    with Scheduler(3) as s:
        s.upsert_nodes(nodes, [0, 1, 2])
        s.add_pods([p for p, _ in bound], [sl for _, sl in bound])
        d = s.diagnose(pod)
        r = s.schedule_raw(pods_array([pod], a)[0], 1)[0]
        assert r.status == 1 and r.fail_node_ports == d.node_ports_nodes == 2
        assert d.plugin_nodes == [int(v) for v in r.fail_counts] == [0, 0, 0, 0, 1, 0, 0, 0]
        assert d.reasons == {R.PORTS: 2, "Insufficient cpu": 1}


# ------------------------------------------------------------ no side effects
def test_no_side_effects_and_window_does_not_matter():
    rng = random.Random(61)
    n = 400
    nodes = rand_res_nodes(rng, n)
    for nd in nodes:
        nd.images = []
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(n)]
    for p in pre:
        p.topology_spread, p.init_containers = [], []
    where = [rng.randrange(n) for _ in pre]
    probes = [rand_res_pod(rng, j) for j in range(12)]
    x100, x5 = DiagPair(n), DiagPair(n, percentage_of_nodes_to_score=5)
    for x in (x100, x5):
        x.upsert(nodes, list(range(n)))
        x.add(pre, where)
    # move nextStartNodeIndex off zero on the pct-5 context
    first = [Pod(f"f{j}", containers=[Container({"cpu": 10})]) for j in range(3)]
    x5.s.schedule_pods(first)
    x100.s.schedule_pods(first)
    start = x5.s.next_start_index()
    assert start != 0
    before100 = states_np(x100.s.lib.ks_node_states, x100.s.ctx, n)
    before5 = states_np(x5.s.lib.ks_node_states, x5.s.ctx, n)
    for p in probes:
        d100, d5 = x100.s.diagnose(p), x5.s.diagnose(p)
        assert d100 == d5, p.name  # a FitError is over every present node, whatever the window
    assert x5.s.next_start_index() == start
    assert np.array_equal(states_np(x100.s.lib.ks_node_states, x100.s.ctx, n), before100)
    assert np.array_equal(states_np(x5.s.lib.ks_node_states, x5.s.ctx, n), before5)
    # a following batch equals the reference's (which saw no diagnose call at all)
    x100.ref.schedule(first)
    x100.schedule_equal([rand_res_pod(rng, 7000 + j) for j in range(60)], "after diagnose")
    for x in (x100, x5):
        x.close()


def test_host_port_dictionary_is_not_consumed():
    big = {"cpu": 64000, "memory": 256 * Gi, "pods": 200}
    port_pod = lambda j, port: Pod(f"p{j}", containers=[Container({"cpu": 10})], host_ports=[(None, "TCP", port)])
    with Scheduler(4) as s:
        s.upsert_nodes([Node(f"n{i}", big) for i in range(4)], [0, 1, 2, 3])
        s.add_pods([port_pod(900, 8000)], [1])
        for j in range(64):  # 64 fresh triples, diagnosed only
            d = s.diagnose(port_pod(j, 1000 + j))
            assert d.feasible_nodes == 4 and d.reasons == {}
        d = s.diagnose(port_pod(99, 8000))  # a held port is seen
        assert d.reasons == {R.PORTS: 1} and d.node_ports_nodes == 1 and d.feasible_nodes == 3
        assert s.node_used_ports(0) == [] and s.node_used_ports(1) == [("0.0.0.0", "TCP", 8000)]
        # the dictionary still has room for 63 more triples: none of the diagnosed ones was interned
        res = s.schedule_pods([port_pod(100 + j, 2000 + j) for j in range(63)])
        assert all(not isinstance(r, Exception) for r in res)


# ------------------------------------------------------------------ two ranks
def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "diag_multirank_main.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["diagnosed"] >= 10 and res["reasons"] >= 8


# ------------------------------------------------------------------ refusals
def test_refusals():
    a = Arena()
    n = 70
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        lib, ctx = s.lib, s.ctx
        # a pod ks_pods_check refuses: the same status and text
        vol = Pod("v", unmodelled=["volumes"])
        pa, _ = pods_array([vol], a)
        st = (C.c_int32 * 1)()
        want_st = lib.ks_pods_check(ctx, pa, 1, st)
        want_err = lib.ks_last_error(ctx).decode()
        assert want_st == _abi.KS_ERR_UNSUPPORTED and "volumes" in want_err.lower()
        with pytest.raises(_abi.KschedError) as e:
            s.diagnose(vol)
        assert e.value.status == want_st and lib.ks_last_error(ctx).decode() == want_err
        # cap too small: KS_ERR_INVALID with *n (and the diagnosis) set
        pa, _ = pods_array([geometry_pod()], a)
        d, cnt = _abi.KsDiagnosis(), C.c_uint32(0)
        out = (_abi.KsReason * 16)()
        assert lib.ks_diagnose(ctx, pa, C.byref(d), out, 2, C.byref(cnt)) == _abi.KS_ERR_INVALID
        assert cnt.value == d.n_reasons == 7 and d.num_all_nodes == n
        assert lib.ks_diagnose(ctx, pa, C.byref(d), None, 0, C.byref(cnt)) == _abi.KS_ERR_INVALID and cnt.value == 7
        assert lib.ks_diagnose(ctx, pa, C.byref(d), out, 7, C.byref(cnt)) == 0 and cnt.value == 7
        assert sorted(out[i].plugin for i in range(7)) == [0, 2, 2, 3, 4, 4, 4]
        # null arguments
        for args in ((None, pa, C.byref(d), out, 16, C.byref(cnt)), (ctx, None, C.byref(d), out, 16, C.byref(cnt)),
                     (ctx, pa, None, out, 16, C.byref(cnt)), (ctx, pa, C.byref(d), out, 16, None),
                     (ctx, pa, C.byref(d), None, 16, C.byref(cnt))):
            assert lib.ks_diagnose(*args) == _abi.KS_ERR_INVALID
        # the context still answers
        assert_same(s.diagnose(geometry_pod()), geometry_want(slots))
