"""ks_batch_forget: Cache.ForgetPod for pods a batch placed, from the data the
batch keeps resident.

The reference is a twin context (forget_workloads.Twin): the same nodes and
batches, the same pods forgotten through ks_pods_remove.  After every forget
and after the following batch the two contexts' ks_node_states of all slots,
ks_node_used_ports of the slots touched, the next batch's results and the
ks_plugin_scores of probe pods over all slots must be equal -- the dumps read
the extended-resource, selector-class and term-class columns, which have no
read-back of their own.  For the synthetic resource and label streams the CPU
oracle is checked too, as tests/test_gpu_permit.py does.  Integers throughout:
every comparison is exact.
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import forget_workloads as W
from xfit_reference import GPU, HUGE, NIC
from xfit_workloads import requests_extended
import pyoracle
from helpers import res_array, states_np
from ksched import Scheduler, _abi, synth
from ksched.objects import Arena, Container, LabelSelector, Node, Pod, TopologySpreadConstraint as TSC, nodes_array, \
    pods_array
from spread_cases import HOST, ZONE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20


# ------------------------------------------------ 1. resource and label streams
@pytest.mark.parametrize("kind", [synth.HETERO, synth.LABELED])
def test_streams_vs_twin_and_oracle(kind):
    n, m = 4000, 1500
    ns = synth.nodes(kind, n, 31)
    ps = synth.pods(kind, 4 * m + 1, 32)
    slots = synth.slot_array(n)
    x = W.Twin(lambda: Scheduler(n, pods_per_round=256), n)
    o = pyoracle.Oracle(n)
    try:
        for t in x.both():
            t.upsert_nodes_raw(ns.nodes, slots, n)
        o.upsert(ns.nodes, slots, n)
        probe = [ps.pods_at(4 * m)]
        rng = random.Random(33)
        for b in range(3):
            arr = ps.pods_at(b * m)
            batch, r = x.run(arr, m, f"batch {b}")
            assert np.array_equal(r, res_array(o.schedule(arr, m), m)), f"batch {b} against the oracle"
            lost = W.seven_eighths(rng, r)
            assert x.forget(batch, arr, r, lost) == 0
            assert x.s.forget_counters()[:4] == [len(lost), 0, 0, 1]
            o.remove_pods(W.subset(arr, lost), W.u32(r["node_index"][lost]), len(lost))
            x.check(f"after forgetting {len(lost)} pods of batch {b}", probes=probe)
            assert np.array_equal(x.states(), states_np(o.L.oracle_node_states, o.o, n)), \
                f"node tables after forgetting batch {b} against the oracle"
            # ks_batch_results stays valid and unchanged
            assert np.array_equal(res_array(x.s.results(batch, m), m), r)
        # the batch that follows the last forget
        arr = ps.pods_at(3 * m)
        _, r = x.run(arr, m, "batch 3")
        assert np.array_equal(r, res_array(o.schedule(arr, m), m)), "batch 3 against the oracle"
        x.check("after batch 3", probes=probe)
        assert np.array_equal(x.states(), states_np(o.L.oracle_node_states, o.o, n)), "node tables after batch 3"
    finally:
        x.close()
        o.close()


# ---------------------------------------------------------------- 2. pile-up
def test_pile_up_on_shared_rows():
    n, m = 8, 300
    a = Arena()
    na, k = nodes_array([Node(f"n{i}", {"cpu": 64000, "memory": 256 * Gi, "pods": 110}) for i in range(n)], a)
    pa, _ = pods_array([Pod(f"p{j}", containers=[Container({"cpu": 100, "memory": 128 * Mi})]) for j in range(m)], a)
    x = W.Twin(lambda: Scheduler(n), n)
    try:
        x.upsert(na, range(n), k)
        pristine = x.states()
        b, r = x.run(pa, m, "pile-up")
        assert (r["status"] == 0).all()
        assert np.bincount(r["node_index"], minlength=n).min() >= 30  # dozens of pods per row
        x.forget(b, pa, r, list(range(m)))  # every row is hit by ~37 lanes of one launch
        x.check("all 300 forgotten", probes=[pa])
        assert np.array_equal(x.states(), pristine)
        b2, r2 = x.run(pa, m, "pile-up again")
        x.forget(b2, pa, r2, [137])
        x.check("one forgotten", probes=[pa])
        assert x.states()["pod_count"].sum() == m - 1
    finally:
        x.close()


# ----------------------------------------------------------- 3. list lengths
# the kernel's wave and block edges: one lane per pod, 256 lanes per block
@pytest.mark.parametrize("length", [1, 63, 64, 65, 255, 256, 257])
def test_list_lengths(length):
    n, m = 64, 600
    a = Arena()
    na, k = nodes_array([Node(f"n{i}", {"cpu": 8000 + 1000 * (i % 5), "memory": (16 + i % 3) * Gi, "pods": 110})
                         for i in range(n)], a)
    pa, _ = pods_array([Pod(f"p{j}", containers=[Container({"cpu": 10 + j % 7, "memory": (1 + j % 5) * Mi})])
                        for j in range(m)], a)
    x = W.Twin(lambda: Scheduler(n), n)
    try:
        x.upsert(na, range(n), k)
        b, r = x.run(pa, m, "600 pods")
        placed = [int(i) for i in np.nonzero(r["status"] == 0)[0]]
        assert len(placed) >= 257
        idx = sorted(random.Random(length).sample(placed, length))
        x.forget(b, pa, r, idx)
        ctr = x.s.forget_counters()
        assert ctr[0] == length and ctr[3] == 1, ctr
        x.check(f"{length} pods forgotten", probes=[pa])
        x.run(pa, m, "the next batch")
        x.check("after the next batch")
    finally:
        x.close()


# ------------------------------------------------------------- 4. chain pods
# "listed": the extended resources' Requested columns enter NodeResourcesFit's and BalancedAllocation's
# scores on every node, so a column the forget left wrong shows in the probes' dumps wherever a forgotten pod
# sat; under the default configuration the columns are read by the Fit filter alone
@pytest.mark.parametrize("config", ["default", "listed"])
def test_chain_pods(config):
    cfg = W.LISTED if config == "listed" else {}
    n = 200
    a = Arena()
    na, k = nodes_array(W.chain_nodes(n), a)
    pods, reps, pin = W.chain_batch(41, "a", pin="h5")
    pa, m = pods_array(pods, a)
    probes = [pods_array([p], a)[0] for p in W.chain_probes(42)]
    x = W.Twin(lambda: Scheduler(n, pods_per_round=64, **cfg), n)
    try:
        x.upsert(na, range(n), k)
        b, r = x.run(pa, m, "chain batch")
        if config == "default":  # (whether the listed configuration takes the run kernel is not this test's matter)
            assert x.s.stats().replica_pods >= 4, "no replica run"
        xres =[i for i, p in enumerate(pods) if requests_extended(p, (GPU, NIC, HUGE)) and r["status"][i] == 0]
        two = [i for i in xres if sum(requests_extended(pods[i], (nm,)) for nm in (GPU, NIC, HUGE)) >= 2]
        assert len(xres) >= 12 and len(two) >= 4  # pods with one XResDev record and with several
        assert (r["status"][reps] == 0).all() and r["status"][pin] == 0 and r["node_index"][pin] == 5
        assert W.holds_pin_port(x.s, 5)
        x.check("after the chain batch", ports=range(n), probes=probes)
        # before the forget the port is taken: the same pod again has no node
        again, _ = pods_array([W.pinned_port_pod("pin-again", "h5")], a)
        d = (_abi.KsNodeScore * n)()
        assert x.s.lib.ks_plugin_scores(x.s.ctx, again, d) == 0
        assert d[5].status == _abi.STATUS_NODE_PORTS
        placed = set(int(i) for i in np.nonzero(r["status"] == 0)[0])
        lost = set(W.seven_eighths(random.Random(43), r)) | set(reps) | {pin} | set(two)
        lost = sorted(lost & placed)
        x.forget(b, pa, r, lost)
        # the pods behind the first 20 have spread constraints, extended resources, host ports or affinity
        # terms: a one-pod program each; the 20 plain pods have none of these and no term selects them: none
        assert x.s.forget_counters()[2] == sum(1 for i in lost if i >= 20)
        assert sum(1 for i in lost if i < 20) > 0
        x.check("after forgetting chain pods", ports=range(n), probes=probes)
        assert not W.holds_pin_port(x.s, 5)
        # the next batch: another pod wanting the same port schedules on that node
        pods2, _, pin2 = W.chain_batch(44, "b", pin="h5")
        pb, m2 = pods_array(pods2, a)
        _, r2 = x.run(pb, m2, "the next chain batch")
        assert r2["status"][pin2] == 0 and r2["node_index"][pin2] == 5
        x.check("after the next chain batch", ports=range(n), probes=probes)
    finally:
        x.close()


# ---------------------------------------- 4b. extended resources at Fit's edge
def test_extended_resources_exact_fit():
    """The analogue of the pinned port for the XResDev walk: one node holds exactly what one pod requests of
    three extended resources (three records), the batch fills it, and only the forget makes room again --
    for each resource on its own, so every record's subtraction is seen, and for no more than the node
    has, so a record subtracted twice is seen too."""
    n = 6
    a = Arena()
    full = {GPU: 2, NIC: 1, HUGE: 256 * Mi}
    nodes = [Node("x0", {"cpu": 8000, "memory": 32 * Gi, "pods": 110}, {HOST: "x0"}, [], extended=dict(full))]
    nodes += [Node(f"n{i}", {"cpu": 8000, "memory": 32 * Gi, "pods": 110}, {HOST: f"n{i}"}) for i in range(1, n)]
    na, k = nodes_array(nodes, a)
    # the pod under test behind two plain pods; its sidecar and init container give the same three sums
    split = W.xres_pod("split", {GPU: 1, HUGE: 256 * Mi})
    split.init_containers = [Container({GPU: 1, NIC: 1}, restart_policy_always=True), Container({GPU: 1})]
    batches = {"one container": W.xres_pod("whole", full), "sidecar and init container": split}
    exact = {nm: pods_array([W.xres_pod(f"exact-{j}", {nm: v})], a)[0] for j, (nm, v) in enumerate(full.items())}
    over = {nm: pods_array([W.xres_pod(f"over-{j}", {nm: v + (256 * Mi if nm == HUGE else 1)})], a)[0]
            for j, (nm, v) in enumerate(full.items())}
    x = W.Twin(lambda: Scheduler(n), n)

    def fits_x0(p):
        out = []
        for t in x.both():
            d = (_abi.KsNodeScore * n)()
            assert t.lib.ks_plugin_scores(t.ctx, p, d) == 0, t.lib.ks_last_error(t.ctx)
            assert all(d[i].status != -1 for i in range(1, n))  # the other nodes have none of the resources
            out.append(d[0].status == -1)
        assert out[0] == out[1]
        return out[0]

    try:
        x.upsert(na, range(n), k)
        for what, pod in batches.items():
            pods = [W.plain_pod(random.Random(1), "q0"), W.plain_pod(random.Random(2), "q1"), pod]
            pa, m = pods_array(pods, a)
            assert all(fits_x0(p) for p in exact.values()) and not any(fits_x0(p) for p in over.values()), what
            b, r = x.run(pa, m, what)
            assert r["status"][2] == 0 and r["node_index"][2] == 0, what
            assert not any(fits_x0(p) for p in exact.values()), f"{what}: the node is full of every resource"
            x.forget(b, pa, r, [2])
            assert x.s.forget_counters()[2] == 1
            for nm in full:
                assert fits_x0(exact[nm]), f"{what}: {nm} was not given back"
                assert not fits_x0(over[nm]), f"{what}: more {nm} given back than the pod held"
            x.check(f"{what}: forgotten", probes=list(exact.values()) + list(over.values()))
        # and the same pod schedules there again
        pa, m = pods_array([W.xres_pod("again", full)], a)
        _, r = x.run(pa, m, "the same requests again")
        assert r["status"][0] == 0 and r["node_index"][0] == 0
        x.check("scheduled again")
    finally:
        x.close()


# -------------------------------------------------------------- 5. late class
def test_class_created_after_the_batch():
    n = 60
    a = Arena()
    na, k = nodes_array(W.chain_nodes(n), a)
    web = [Pod(f"w{j}", containers=[Container({"cpu": 100, "memory": 64 * Mi})], labels={"app": "web"}) for j in range(48)]
    pa, m = pods_array(web, a)
    sel = LabelSelector({"app": "web"})
    spread = lambda name: Pod(name, containers=[Container({"cpu": 100})], labels={"app": "web"},
                              topology_spread=[TSC(1, ZONE, "ScheduleAnyway", sel), TSC(1, HOST, "ScheduleAnyway", sel)])
    pb, mb = pods_array([spread(f"s{j}") for j in range(3)], a)
    probe, _ = pods_array([spread("probe")], a)
    x = W.Twin(lambda: Scheduler(n), n)

    def raws():
        out = []
        for t in x.both():
            d = (_abi.KsNodeScore * n)()
            assert t.lib.ks_plugin_scores(t.ctx, probe, d) == 0, t.lib.ks_last_error(t.ctx)
            out.append([int(d[i].spread_raw) for i in range(n)])
        return out

    try:
        x.upsert(na, range(n), k)
        ba, ra = x.run(pa, m, "batch A: no selector exists yet")
        assert (ra["status"] == 0).all()
        x.run(pb, mb, "batch B: the first selector, matching A's pods")  # its class counts A's pods
        before = raws()
        assert before[0] == before[1]
        lost = W.seven_eighths(random.Random(6), ra)
        x.forget(ba, pa, ra, lost)
        after = raws()
        assert after[0] == after[1], "spread_raw of the next spread pod"
        assert after[0] != before[0], "forgetting 42 matching pods must move the counts"
        x.check("after forgetting batch A's pods", probes=[probe])
        x.run(pb, mb, "the next spread pods")
        x.check("after the next spread pods", probes=[probe])
    finally:
        x.close()


# -------------------------------------------------------- 6. nodes that left
def test_nodes_that_left():
    n, m = 20, 120
    a = Arena()
    nodes = [Node(f"n{i}", {"cpu": 8000, "memory": 32 * Gi, "pods": 110}, {HOST: f"n{i}"}) for i in range(n)]
    na, k = nodes_array(nodes, a)
    pa, _ = pods_array([Pod(f"p{j}", containers=[Container({"cpu": 50 + j % 3, "memory": 16 * Mi})]) for j in range(m)], a)
    x = W.Twin(lambda: Scheduler(n), n)
    try:
        x.upsert(na, range(n), k)
        b, r = x.run(pa, m, "batch")
        on = lambda slot: [int(i) for i in np.nonzero((r["status"] == 0) & (r["node_index"] == slot))[0]]
        gone, refilled, upserted, kept = 3, 7, 11, 15
        assert all(len(on(s)) >= 2 for s in (gone, refilled, upserted, kept))
        x.delete([gone, refilled])
        fresh, _ = nodes_array([Node("fresh", {"cpu": 4000, "memory": 8 * Gi, "pods": 30}, {HOST: "fresh"})], a)
        x.upsert(fresh, [refilled], 1)
        bigger, _ = nodes_array([Node(f"n{upserted}", {"cpu": 9000, "memory": 48 * Gi, "pods": 110}, {HOST: f"n{upserted}"})], a)
        x.upsert(bigger, [upserted], 1)  # in place: the node keeps its pods
        idx = sorted(on(gone) + on(refilled) + on(upserted) + on(kept))
        skipped = x.forget(b, pa, r, idx, gone={gone, refilled})
        assert skipped == len(on(gone)) + len(on(refilled))
        st = x.states()
        assert st["req_cpu"][refilled] == 0 and st["nz_cpu"][refilled] == 0 and st["pod_count"][refilled] == 0
        assert st["alloc_cpu"][refilled] == 4000
        assert st["pod_count"][upserted] == 0 and st["pod_count"][kept] == 0 and st["alloc_cpu"][upserted] == 9000
        x.check("after forgetting pods of nodes that left", probes=[pa])
        # a skipped pod counts as forgotten: a second forget of it is refused
        st2, _ = W.raw_forget(x.s, b, [on(gone)[0]])
        assert st2 == _abi.KS_ERR_INVALID
        x.run(pa, m, "the next batch")
        x.check("after the next batch")
    finally:
        x.close()


# -------------------------------------------------------------- 7. refusals
def test_refusals():
    n = 4
    a = Arena()
    na, k = nodes_array([Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 110}) for i in range(n)], a)
    pods = [Pod(f"p{j}", containers=[Container({"cpu": 100 + j, "memory": 64 * Mi})]) for j in range(6)]
    pods[4] = Pod("huge", containers=[Container({"cpu": 1_000_000, "memory": 64 * Mi})])  # fits nowhere
    pa, m = pods_array(pods, a)
    x = W.Twin(lambda: Scheduler(n), n)
    try:
        x.upsert(na, range(n), k)
        b, r = x.run(pa, m, "batch")
        assert r["status"][4] != 0 and (np.delete(r["status"], 4) == 0).all()
        base = x.states()
        never = x.s.prepare(pa, m)
        x.batches.append(never)

        def refused(batch, idx, word):
            st, _ = W.raw_forget(x.s, batch, idx)
            assert st == _abi.KS_ERR_INVALID, (idx, st)
            assert word in x.s.lib.ks_last_error(x.s.ctx).decode(), x.s.lib.ks_last_error(x.s.ctx)
            assert np.array_equal(x.states(), base), f"a refused list {idx} changed the cache"

        refused(b, [0, 4], "not scheduled")          # an unscheduled pod behind a valid one: nothing applied
        refused(b, [1, 1], "strictly increasing")    # a repeat
        refused(b, [3, 2], "strictly increasing")    # descending
        refused(b, [0, 6], "6 pods")                 # an index >= n
        refused(never, [0], "not run")               # prepared, never run
        assert x.s.lib.ks_batch_forget(x.s.ctx, None, W.u32([0]), 1, None) == _abi.KS_ERR_INVALID
        assert x.s.lib.ks_batch_forget(x.s.ctx, b, None, 1, None) == _abi.KS_ERR_INVALID
        assert x.s.lib.ks_batch_forget(x.s.ctx, b, None, 0, None) == 0  # an empty list
        assert np.array_equal(x.states(), base)
        x.forget(b, pa, r, [1])
        base = x.states()
        refused(b, [0, 1], "forgotten already")      # a second forget of index 1: pod 0 stays too
        x.check("one pod forgotten", probes=[pa])
        # the batch run again places every pod anew: the same index is accepted again
        x.s.run(b)
        r2 = res_array(x.s.results(b, m), m)
        rt = res_array(x.t.schedule_raw(pa, m), m)
        assert np.array_equal(r2, rt)
        x.forget(b, pa, r2, [1])
        x.check("the batch run again, the pod forgotten again", probes=[pa])
    finally:
        x.close()


# -------------------------------------------------------------- 8. pct < 100
def test_percentage_of_nodes_to_score():
    n, m = 500, 300
    ns = synth.nodes(synth.HETERO, n, 71)
    ps = synth.pods(synth.HETERO, 2 * m, 72)
    x = W.Twin(lambda: Scheduler(n, percentage_of_nodes_to_score=30), n)
    try:
        for t in x.both():
            t.upsert_nodes_raw(ns.nodes, synth.slot_array(n), n)
        b, r = x.run(ps.pods, m, "batch 0")
        start = x.s.next_start_index()
        assert start == x.t.next_start_index()
        placed = [int(i) for i in np.nonzero(r["status"] == 0)[0]]
        half = sorted(random.Random(73).sample(placed, len(placed) // 2))
        x.forget(b, ps.pods, r, half)
        assert x.s.next_start_index() == start, "nextStartNodeIndex moved"
        x.check("half a batch forgotten", probes=[ps.pods_at(m)])
        x.run(ps.pods_at(m), m, "batch 1")
        assert x.s.next_start_index() == x.t.next_start_index()
        x.check("after batch 1")
    finally:
        x.close()


# -------------------------------------------------------------- 9. two ranks
def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "forget_multirank_main.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    # both kinds were among the forgotten: pods of the sharded rounds and pods of the replicated chain
    assert res["forgotten_plain"] > 0 and res["forgotten_solo"] > 0 and res["scheduled_after"] > 0
