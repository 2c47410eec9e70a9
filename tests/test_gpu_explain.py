"""ks_explain on the GPU (ksched_explain.hip): a pod's k best
feasible nodes with their per-plugin scores, the best TotalScore and the size
of its tie set.  The reference of every test is ks_plugin_scores on the same
context immediately before the call (other tests pin it against the oracle):
its feasible records sorted by (-total_score, slot), the first k of them.
Geometry by construction, field-for-field equality on random clusters, explain
then schedule, no side effects, two in-process ranks, refusals."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from helpers import res_array, states_np
from ksched import Scheduler, _abi
from ksched.objects import (Arena, Container, Node, NodeSelectorRequirement, NodeSelectorTerm, Pod,
                            PreferredSchedulingTerm, Taint, Toleration, nodes_array, pods_array)
from test_gpu_spread import rand_ipa_pod, rand_nodes, rand_pod, rand_res_nodes, rand_res_pod

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
GPU = "nvidia.com/gpu"
KS = [1, 2, 64, 128]
SCORE_DT = np.dtype([(f, "<i4") for f, _ in _abi.KsNodeScore._fields_[:-1]] + [("total_score", "<i8")])
assert SCORE_DT.itemsize == C.sizeof(_abi.KsNodeScore)


def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def dump(s, pa):
    """ks_plugin_scores of the marshalled pod: one record per slot, as numpy."""
    out = (_abi.KsNodeScore * s.capacity)()
    assert s.lib.ks_plugin_scores(s.ctx, pa, out) == 0, s.lib.ks_last_error(s.ctx)
    return np.frombuffer(C.string_at(C.addressof(out), C.sizeof(out)), dtype=SCORE_DT)


def explain_raw(s, pa, k):
    e = _abi.KsExplanation()
    out = (_abi.KsCandidate * k)()
    assert s.lib.ks_explain(s.ctx, pa, k, C.byref(e), out) == 0, s.lib.ks_last_error(s.ctx)
    slots = [int(out[i].slot) for i in range(e.n_candidates)]
    recs = np.frombuffer(b"".join(bytes(out[i].score) for i in range(e.n_candidates)), dtype=SCORE_DT)
    return e, slots, recs


def order_of(sc):
    """Slots of the feasible records by (-total_score, slot)."""
    feas = np.nonzero(sc["status"] == -1)[0]
    return feas[np.lexsort((feas, -sc["total_score"][feas]))]


def assert_explains(s, pa, ks, what="", sc=None):
    """ks_explain at every k against want(k) of the dump `sc` (taken here unless given)."""
    if sc is None:
        sc = dump(s, pa)
    order = order_of(sc)
    present = int((sc["status"] != -2).sum())
    top = int(sc["total_score"][order[0]]) if len(order) else 0
    ties = int((sc["total_score"][order] == top).sum()) if len(order) else 0
    for k in ks:
        e, slots, recs = explain_raw(s, pa, k)
        w = order[:k]
        assert (e.num_all_nodes, e.feasible_nodes, e.n_candidates) == (present, len(order), len(w)), (what, k)
        assert (e.top_score, e.top_score_nodes) == (top, ties), (what, k, e.top_score, e.top_score_nodes, top, ties)
        assert slots == [int(x) for x in w], (what, k, slots[:8], w[:8])
        assert np.array_equal(recs, sc[w]), (what, k, [i for i in range(len(w)) if recs[i] != sc[w][i]][:4])
    return sc, order


# ----------------------------------------------------------------- geometry
# A node of level L (0..99) scores L under LeastAllocated for the pod below and
# 100 under BalancedAllocation (its cpu and memory fractions are equal), so a
# node's TotalScore rises with its level and nothing else: "rich" nodes are
# level 90 among "poor" ones of level 10.
POOR, RICH = 10, 90


def level_templates(a):
    nodes = []
    for lv in range(100):
        cpu = -(-100_000 // (100 - lv))
        nodes.append(Node(f"l{lv}", {"cpu": cpu, "memory": cpu * Mi, "pods": 110}))
    nodes.append(Node("cordoned", {"cpu": 10 ** 6, "memory": 10 ** 6 * Mi, "pods": 110}, unschedulable=True))
    return nodes_array(nodes, a)[0]


def level_nodes(ta, slots, levels, a):
    """A ks_node per slot at its level (100: a cordoned node) under its own name."""
    arr = (_abi.KsNode * max(1, len(slots)))()
    names = [f"g{s}".encode() for s in slots]
    for i, lv in enumerate(levels):
        arr[i] = ta[lv]
        arr[i].name = names[i]
    a._keep.append((arr, names))
    return arr


def level_pod():
    return Pod("p", containers=[Container({"cpu": 1000, "memory": 1000 * Mi})])


def placements(n):
    """{name: level of slot i} for n slots."""
    w0 = n // 2 // 64 * 64
    last = (n - 1) // 64 * 64
    return {
        "one wave": [RICH if w0 <= i < w0 + 64 else POOR for i in range(n)],
        "one per block": [RICH if i % 1024 == min(17, n - 1) else POOR for i in range(n)],
        "last wave": [RICH if i >= last else POOR for i in range(n)],
        "ascending": [i * 100 // n for i in range(n)],
        "descending": [99 - i * 100 // n for i in range(n)],
        "identical": [50] * n,
        "ties above k": [RICH if i % 7 == 3 else POOR for i in range(n)],
    }


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 2500])
def test_geometry(n):
    a = Arena()
    ta = level_templates(a)
    slots = list(range(n))
    pa, _ = pods_array([level_pod()], a)
    with Scheduler(n) as s:
        for name, levels in placements(n).items():
            s.upsert_nodes_raw(level_nodes(ta, slots, levels, a), u32(slots), n)
            sc, order = assert_explains(s, pa, KS, f"n {n} {name}")
            tot = sc["total_score"]
            assert len(order) == n
            # the placement is what its name says (from the reference's own totals)
            if name == "ascending":  # strictly while the 100 levels last, in level steps beyond
                assert np.all(np.diff(tot) > 0) if n <= 100 else (np.all(np.diff(tot) >= 0) and len(set(tot)) == 100)
            elif name == "descending":
                assert np.all(np.diff(tot) < 0) if n <= 100 else (np.all(np.diff(tot) <= 0) and len(set(tot)) == 100)
            elif name == "identical":
                assert len(set(tot)) == 1 and list(order[:128]) == slots[:128]
            else:
                rich = [i for i in slots if levels[i] == RICH]
                assert list(order[:len(rich)]) == rich
                assert len(rich) in (0, n) or tot[rich[0]] > tot[order[len(rich)]]
                if name == "ties above k" and n >= 1023:
                    assert len(rich) > 128


def test_geometry_capacity_above_n_with_deleted_and_cordoned_slots():
    a = Arena()
    ta = level_templates(a)
    cap = 3000
    slots = [s_ for s_ in range(2100) if s_ % 3 != 1]  # every third slot never filled
    levels = [100 if s_ % 11 == 5 else (s_ * 37) % 100 for s_ in slots]  # a cordoned node now and then
    pa, _ = pods_array([level_pod()], a)
    with Scheduler(cap) as s:
        s.upsert_nodes_raw(level_nodes(ta, slots, levels, a), u32(slots), len(slots))
        gone = {s_ for s_ in slots if s_ % 5 == 0 and s_ > 64}  # ... and a fifth of the rest deleted again
        s.delete_slots(sorted(gone))
        sc, order = assert_explains(s, pa, KS, "capacity above n")
        left = [(s_, lv) for s_, lv in zip(slots, levels) if s_ not in gone]
        assert int((sc["status"] != -2).sum()) == len(left)
        assert len(order) == sum(1 for _, lv in left if lv != 100)


def test_geometry_more_than_one_grid_stride():
    # above 256 blocks x 1024 threads (one position per thread per step): the
    # grid-stride loop's second step, its tail wave partly past the end; the
    # best nodes sit in both strides
    a = Arena()
    ta = level_templates(a)
    n = 270_000
    slots = list(range(n))
    levels = [RICH if (i % 4099 == 7 or i >= n - 40) else (i * 13) % 80 for i in range(n)]
    pa, _ = pods_array([level_pod()], a)
    with Scheduler(n) as s:
        s.upsert_nodes_raw(level_nodes(ta, slots, levels, a), u32(slots), n)
        _, order = assert_explains(s, pa, [1, 128], "two strides")
        assert order[0] == 7 and order[105] >= n - 40  # 66 rich nodes by the stride-4099 rule, then the tail's


# ------------------------------------------- field for field, random clusters
def soften(rng, nodes):
    """PreferNoSchedule taints (TaintToleration's normaliser) on some nodes."""
    for nd in nodes:
        for key in ("soft-a", "soft-b", "soft-c"):
            if rng.random() < 0.25:
                nd.taints = nd.taints + [Taint(key, "1", "PreferNoSchedule")]
    return nodes


def pref_pod(rng, j):
    """A label / taint / preferred-affinity pod: both normalisers non-trivial."""
    p = rand_pod(rng, j, spread_frac=0.0)
    p.preferred = [PreferredSchedulingTerm(rng.randint(1, 100), NodeSelectorTerm(
        [NodeSelectorRequirement("disk", "In", ["ssd"])])), PreferredSchedulingTerm(rng.randint(1, 100), NodeSelectorTerm(
            [NodeSelectorRequirement("rack", "In", rng.sample([f"r{q}" for q in range(8)], 3))]))]
    if rng.random() < 0.5:
        p.tolerations = p.tolerations + [Toleration("soft-a", "Exists", "", "PreferNoSchedule")]
    return p


def cluster(s, rng, nodes, bound):
    n = len(nodes)
    s.upsert_nodes(nodes, list(range(n)))
    if bound:
        s.add_pods(bound, [rng.randrange(n) for _ in bound])


def equal_on(s, pods, ks=(16,), what=""):
    """Every pod explained against its dump; returns the feasible records of all the dumps
    (what the cluster gave the plugins to score: the callers check it is not trivial)."""
    a = Arena()
    seen = np.zeros(0, dtype=SCORE_DT)
    for j, p in enumerate(pods):
        pa, _ = pods_array([p], a)
        sc, order = assert_explains(s, pa, ks, f"{what} pod {j}")
        seen = np.concatenate([seen, sc[order]])
    return seen


def test_fields_plain_and_normalised_pods():
    rng = random.Random(71)
    n = 700
    with Scheduler(n) as s:
        cluster(s, rng, soften(rng, rand_nodes(rng, n, 5)), [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n)])
        seen = equal_on(s, [rand_pod(rng, j, spread_frac=0.0) for j in range(6)], (16, 128), "plain")
        seen = equal_on(s, [pref_pod(rng, 100 + j) for j in range(10)], (16, 128), "normalised")
        assert len(set(seen["taint_score"])) > 1 and len(set(seen["affinity_score"])) > 1
        assert seen["taint_raw"].any() and seen["affinity_raw"].any()


def test_fields_spread_pods():
    rng = random.Random(72)
    n = 900
    with Scheduler(n) as s:
        cluster(s, rng, rand_nodes(rng, n, 6), [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n)])
        pods = [rand_pod(rng, j, spread_frac=1.0) for j in range(16)]
        kinds = {c.when_unsatisfiable for p in pods for c in p.topology_spread}
        assert kinds == {"DoNotSchedule", "ScheduleAnyway"}
        seen = equal_on(s, pods, (16,), "spread")
        assert seen["spread_raw"].any() and len(set(seen["spread_score"])) > 1


def test_fields_inter_pod_affinity():
    rng = random.Random(73)
    n = 600
    with Scheduler(n) as s:
        # bound pods carry terms of their own: preferred terms of existing pods score too
        cluster(s, rng, rand_nodes(rng, n, 4), [rand_ipa_pod(rng, 10_000 + j, frac=0.4, spread_frac=0.0) for j in range(n // 2)])
        seen = equal_on(s, [rand_ipa_pod(rng, j, frac=1.0) for j in range(14)], (16,), "ipa")
        seen2 = equal_on(s, [rand_ipa_pod(rng, 50 + j, frac=0.0, spread_frac=0.0) for j in range(6)], (16,), "ipa existing")
        assert seen["affinity_pod_raw"].any() and seen2["affinity_pod_raw"].any()
        assert len(set(seen["affinity_pod_score"])) > 1


def test_fields_images_extended_resources():
    rng = random.Random(74)
    n = 1200
    with Scheduler(n) as s:
        pre = [rand_res_pod(rng, 50_000 + j) for j in range(n // 2)]
        for p in pre:
            p.topology_spread = []
        cluster(s, rng, rand_res_nodes(rng, n), pre)
        seen = equal_on(s, [rand_res_pod(rng, j) for j in range(24)], (16, 128), "resources")
        assert seen["image_locality"].any()


def test_fields_host_ports():
    rng = random.Random(75)
    n = 300
    with Scheduler(n) as s:
        held = [Pod(f"h{j}", containers=[Container({"cpu": 100})], host_ports=[(None, "TCP", 8000 + j % 3)]) for j in range(200)]
        cluster(s, rng, rand_nodes(rng, n, 3), held)
        for j in range(4):
            p = Pod(f"p{j}", containers=[Container({"cpu": 200, "memory": 256 * Mi})],
                    host_ports=[(None, "TCP", 8000 + j % 3), ("10.0.0.1", "UDP", 53)])
            pa, _ = pods_array([p], Arena())
            sc, order = assert_explains(s, pa, (16, 128), f"ports pod {j}")
            assert (sc["status"] == _abi.STATUS_NODE_PORTS).any() and len(order)


def gpu_pod(rng, j):
    p = rand_res_pod(rng, j)
    p.containers[0].requests[GPU] = rng.choice([1, 2])
    return p


@pytest.mark.parametrize("cfg", [
    dict(fit_strategy="MostAllocated", fit_resource_weights={"cpu": 3, "memory": 1}),
    dict(fit_strategy="RequestedToCapacityRatio", fit_resource_weights={"cpu": 2, "memory": 1},
         fit_shape=[(0, 0), (40, 7), (100, 10)]),
    dict(fit_strategy="LeastAllocated", fit_resource_weights={"cpu": 1, "memory": 1, GPU: 3}),
    dict(fit_strategy="RequestedToCapacityRatio", fit_resource_weights={"cpu": 1, "memory": 1, GPU: 3},
         fit_shape=[(0, 0), (100, 10)]),
    dict(balanced_resources=["cpu", "memory", GPU]),
    dict(fit_strategy="MostAllocated", fit_resource_weights={"cpu": 1, "memory": 2, GPU: 2},
         balanced_resources=[GPU, "cpu", "memory"]),
], ids=["most", "rtcr", "least-x", "rtcr-x", "balanced-x", "most-x-balanced-x"])
def test_fields_strategies(cfg):
    rng = random.Random(76)
    n = 500
    with Scheduler(n, **cfg) as s:
        pre = [rand_res_pod(rng, 50_000 + j) for j in range(n)]
        for p in pre:
            p.topology_spread = []
        cluster(s, rng, rand_res_nodes(rng, n), pre)
        # pods that request the listed scalar resource, and pods that do not
        seen = equal_on(s, [gpu_pod(rng, j) for j in range(6)] + [rand_res_pod(rng, 100 + j) for j in range(6)], (16,), str(cfg))
        assert len(set(seen["least_allocated"])) > 1 and len(set(seen["balanced_allocation"])) > 1


# ------------------------------------------------------ explain, then schedule
def test_explain_then_schedule():
    rng = random.Random(81)
    n = 500
    nodes = rand_res_nodes(rng, n)
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(2 * n)]  # crowded: some pods will not fit
    for p in pre:
        p.topology_spread = []
    where = [rng.randrange(n) for _ in pre]
    pods = [(rand_ipa_pod(rng, j, frac=0.5) if j % 3 == 0 else rand_res_pod(rng, j)) for j in range(160)]
    pods.append(Pod("huge", containers=[Container({"cpu": 10 ** 7})]))
    a = Arena()
    with Scheduler(n) as s, Scheduler(n) as only:
        for x in (s, only):
            x.upsert_nodes(nodes, list(range(n)))
            x.add_pods(pre, where)
        unsched = ties = 0
        for j, p in enumerate(pods):
            pa, _ = pods_array([p], a)
            e, slots, recs = explain_raw(s, pa, 4)
            r = res_array(s.schedule_raw(pa, 1), 1)[0]
            r2 = res_array(only.schedule_raw(pa, 1), 1)[0]
            assert r == r2, (j, r, r2)
            assert r["status"] in (0, 1), (j, r)
            assert e.feasible_nodes == r["feasible"], (j, e.feasible_nodes, r)
            if r["status"] == 1:
                assert e.feasible_nodes == 0 and e.n_candidates == 0 and e.top_score == 0 and e.top_score_nodes == 0
                unsched += 1
                continue
            assert r["node_index"] == slots[0], (j, r, slots)
            if not r["flags"] & 1:  # KS_RESULT_SINGLE_FEASIBLE: upstream skips scoring
                assert r["total_score"] == recs["total_score"][0] == e.top_score, (j, r, e.top_score)
            ties += e.top_score_nodes > 1
        assert unsched >= 1 and ties >= 1 and len(pods) - unsched >= 100
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, n), states_np(only.lib.ks_node_states, only.ctx, n))


# ------------------------------------------------------------ no side effects
def test_no_side_effects_and_window_does_not_matter():
    rng = random.Random(82)
    n = 400
    nodes = rand_res_nodes(rng, n)
    for nd in nodes:
        nd.images = []
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(n)]
    for p in pre:
        p.topology_spread, p.init_containers = [], []
    where = [rng.randrange(n) for _ in pre]
    probes = [rand_res_pod(rng, j) for j in range(12)]
    batch = [rand_res_pod(rng, 7000 + j) for j in range(60)]
    first = [Pod(f"f{j}", containers=[Container({"cpu": 10})]) for j in range(3)]
    a = Arena()
    with Scheduler(n) as x100, Scheduler(n, percentage_of_nodes_to_score=5) as x5, Scheduler(n) as never:
        for x in (x100, x5, never):
            x.upsert_nodes(nodes, list(range(n)))
            x.add_pods(pre, where)
            x.schedule_pods(first)  # moves nextStartNodeIndex off zero on the pct-5 context
        start = x5.next_start_index()
        assert start != 0
        before = [states_np(x.lib.ks_node_states, x.ctx, n) for x in (x100, x5)]
        ports = [[x.node_used_ports(sl) for sl in range(0, n, 37)] for x in (x100, x5)]
        for p in probes:
            pa, _ = pods_array([p], a)
            # the answer on the pct-5 context is want(k) over the whole list, whatever the window
            # (its cache differs from the pct-100 context's by where the first pods went)
            assert_explains(x5, pa, (16,), f"pct 5 {p.name}")
            assert_explains(x100, pa, (16,), f"pct 100 {p.name}")
        assert x5.next_start_index() == start
        for x, b, pt in zip((x100, x5), before, ports):
            assert np.array_equal(states_np(x.lib.ks_node_states, x.ctx, n), b)
            assert [x.node_used_ports(sl) for sl in range(0, n, 37)] == pt
        # a following batch equals the same batch on a context that never explained
        pa, m = pods_array(batch, a)
        assert np.array_equal(res_array(x100.schedule_raw(pa, m), m), res_array(never.schedule_raw(pa, m), m))
        assert np.array_equal(states_np(x100.lib.ks_node_states, x100.ctx, n), states_np(never.lib.ks_node_states, never.ctx, n))


def test_host_port_dictionary_is_not_consumed():
    big = {"cpu": 64000, "memory": 256 * Gi, "pods": 200}
    port_pod = lambda j, port: Pod(f"p{j}", containers=[Container({"cpu": 10})], host_ports=[(None, "TCP", port)])
    with Scheduler(4) as s:
        s.upsert_nodes([Node(f"n{i}", big) for i in range(4)], [0, 1, 2, 3])
        s.add_pods([port_pod(900, 8000)], [1])
        for j in range(64):  # 64 fresh triples, explained only
            e = s.explain(port_pod(j, 1000 + j), 4)
            assert e.feasible_nodes == 4 and sorted(c.slot for c in e.candidates) == [0, 1, 2, 3]
        e = s.explain(port_pod(99, 8000), 4)  # a held port is seen
        assert e.feasible_nodes == 3 and [c.slot for c in e.candidates] == [0, 2, 3] and e.top_score_nodes == 3
        assert s.node_used_ports(0) == [] and s.node_used_ports(1) == [("0.0.0.0", "TCP", 8000)]
        # the dictionary still has room for 63 more triples: none of the explained ones was interned
        res = s.schedule_pods([port_pod(100 + j, 2000 + j) for j in range(63)])
        assert all(not isinstance(r, Exception) for r in res)


# ------------------------------------------------------------- python surface
def test_python_explanation():
    from ksched import Explanation
    from ksched.framework import DEFAULT_WEIGHTS
    rng = random.Random(83)
    n = 300
    with Scheduler(n) as s:
        cluster(s, rng, soften(rng, rand_nodes(rng, n, 3)), [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n)])
        p = pref_pod(rng, 1)
        sc = s.plugin_scores(p)
        e = s.explain(p)
        assert isinstance(e, Explanation) and len(e.candidates) == min(16, e.feasible_nodes) and e.num_all_nodes == n
        for c in e.candidates:
            assert c.name == s.names[c.slot] and c.total_score == sc[c.slot].total_score == c.raw.total_score
            assert [x.name for x in c.scores] == list(DEFAULT_WEIGHTS)
            # the default weights applied to the plugins' scores give the total
            assert sum(DEFAULT_WEIGHTS[x.name] * x.score for x in c.scores) == c.total_score
        assert e.candidates[0].total_score == e.top_score


# ------------------------------------------------------------------ two ranks
def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "explain_multirank_main.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["explained"] >= 8 and res["candidates"] >= 100


# ------------------------------------------------------------------ refusals
def test_refusals():
    a = Arena()
    ta = level_templates(a)
    n = 70
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(level_nodes(ta, slots, [i % 100 for i in slots], a), u32(slots), n)
        lib, ctx = s.lib, s.ctx
        # a pod ks_pods_check refuses: the same status and text
        vol = Pod("v", unmodelled=["volumes"])
        pa, _ = pods_array([vol], a)
        st = (C.c_int32 * 1)()
        want_st = lib.ks_pods_check(ctx, pa, 1, st)
        want_err = lib.ks_last_error(ctx).decode()
        assert want_st == _abi.KS_ERR_UNSUPPORTED and "volumes" in want_err.lower()
        with pytest.raises(_abi.KschedError) as err:
            s.explain(vol)
        assert err.value.status == want_st and lib.ks_last_error(ctx).decode() == want_err
        # k out of range, null arguments
        pa, _ = pods_array([level_pod()], a)
        e = _abi.KsExplanation()
        out = (_abi.KsCandidate * 129)()
        assert _abi.EXPLAIN_MAX_CANDIDATES == 128
        for k in (0, 129, 1 << 31):
            assert lib.ks_explain(ctx, pa, k, C.byref(e), out) == _abi.KS_ERR_INVALID
        for args in ((None, pa, 4, C.byref(e), out), (ctx, None, 4, C.byref(e), out), (ctx, pa, 4, None, out),
                     (ctx, pa, 4, C.byref(e), None)):
            assert lib.ks_explain(*args) == _abi.KS_ERR_INVALID
        # the context still answers
        assert_explains(s, pa, [1, 128], "after refusals")
