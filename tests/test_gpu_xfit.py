"""NodeResourcesFit strategies that list extended resources
(ks_set_fit_strategy_resources) against the composed reference
(tests/xfit_reference.py): every result field, fail_counts, every node's state
and ks_plugin_scores, bit for bit.

Nodes are spread over the whole capacity (300 over 512 slots, 2,500 over
4,096): three workgroups of the one-pod chain with a partial last one and
empty lanes in every wave.

(a) the strategy sweep over the mixed stream of tests/xfit_workloads.py, with
    the assertion that listing the resource changes that stream's schedule;
(b) churn between batches, and a name listed before any node reports it;
(c) a strategy switch on a live context, also between prepare and run;
(d) 3 virtual shards and a two-rank world;
(e) dumps of requesting and non-requesting pods on the same nodes;
(f) refusals, the 2^44 bound from both directions.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import xfit_workloads as X
from fit_reference import LEAST, MOST, scores_np
from helpers import assert_results_equal
from ksched import Scheduler, _abi
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from rtcr_reference import RTCR, SHAPES
from test_gpu_fit_spread import FitPair
from test_xfit_reference import teeth
from xfit_reference import GPU, HUGE, NIC, XfitReference, ext_array

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
LATE = "example.com/late"  # a resource no node reports at first


class XfitPair(FitPair):
    """libksched and XfitReference fed the same cache events."""

    def __init__(self, cap, strategy, extended, **cfg):
        super().__init__(cap, (LEAST, 1, 1), **cfg)
        self.o.close()
        self.o = XfitReference(cap, strategy, extended)
        X.set_strategy(self.s, strategy, extended)

    def use(self, strategy, extended):
        X.set_strategy(self.s, strategy, extended)
        self.o.set_strategy(strategy, extended)


# ---------------------------------------------------------------- (a) sweep
@pytest.mark.parametrize("case,size,seed", [(c, "small", 71) for c in sorted(X.CASES)] +
                         [("most-1-1-gpu3", "large", 72), ("peaked-1-1-gpu2-nic1", "large", 72),
                          ("least-2-0-nic1-gpu5", "large", 72)])
def test_strategy_sweep(case, size, seed):
    # teeth first, on the reference alone: a build that accepted the list and scored cpu and memory only
    # would place these pods as the reference without the list does
    n_ask, n_moved, fit_fails = teeth(case, seed, size)
    assert 10 * n_moved >= n_ask > 0 and fit_fails > 0, (n_ask, n_moved, fit_fails)
    cap = X.SIZES[size][1]
    x = XfitPair(cap, *X.CASES[case], pods_per_round=64)
    _, res = X.sweep_stream(x, seed, size)
    r = np.concatenate(res)
    assert (r["status"] == 0).sum() > 100 and (r["fail"][:, 4] > 0).sum() > 50
    assert x.s.stats().spread_pods >= n_ask
    x.close()


# ---------------------------------------------------------------- (b) churn
def late_pod(rng, j):
    p = X.xfit_pod(rng, 10 * j + 2)
    p.containers[0].requests[LATE] = rng.choice([1, 2])
    return p


@pytest.mark.parametrize("case", ["most-1-1-gpu3", "peaked-1-1-gpu2-nic1"])
def test_churn_between_batches(case):
    strategy, extended = X.CASES[case]
    extended = dict(extended, **{LATE: 4})  # listed before any node or pod has shown it
    n, cap = X.SIZES["small"]
    rng = random.Random(81)
    slots = X.spread_slots(n, cap)
    x = XfitPair(cap, strategy, extended, pods_per_round=64)
    assert x.s.get_fit_strategy()[1][LATE] == 4
    x.upsert(X.xfit_nodes(rng, n), slots)
    live = list(zip(X.bound_pods(rng, n // 2, 60_000), [rng.choice(slots) for _ in range(n // 2)]))
    x.add([p for p, _ in live], [s for _, s in live])
    for b in range(4):
        kind = late_pod if b >= 2 else X.xfit_pod
        x.schedule([kind(rng, b * 1000 + j) for j in range(50)], f"churn {case} batch {b}")
        x.states_equal(f"churn {case} batch {b}")
        x.dump_equal(kind(rng, 97_002 + 10 * b), f"churn {case} dump {b}")
        # bound pods leave (extended requests with them); others arrive, some beyond the node's Allocatable
        rng.shuffle(live)
        gone, live = live[:20], live[20:]
        x.add([p for p, _ in gone], [s for _, s in gone], sign=-1)
        more = X.bound_pods(rng, 30, 70_000 + 100 * b)
        ms = [rng.choice(slots) for _ in more]  # (slots: the present ones)
        x.add(more, ms)
        live += list(zip(more, ms))
        # a listed resource's Allocatable changes in place; a node is deleted and re-added, another stays deleted
        pick = rng.sample(slots, 12)
        fresh = X.xfit_nodes(rng, 10, slot0=n + 20 * b)
        for nd in fresh[:5]:
            nd.extended[GPU] = rng.choice([1, 16])
        if b >= 1:  # from here on nodes report the late resource: its column appears
            for nd in fresh:
                nd.extended[LATE] = rng.choice([2, 4])
        live = [(p, s) for p, s in live if s not in pick[8:]]  # their pods leave with the deleted nodes
        x.delete(pick[8:])
        x.upsert(fresh, pick[:10])  # 8 in place, 2 re-added; pick[10:] stay deleted
        slots = [s for s in slots if s not in pick[10:]]
    assert x.s.stats().spread_pods > 150
    x.close()


# ------------------------------------------------------ (c) strategy switch
def test_strategy_switch_on_a_live_context():
    n, cap = X.SIZES["small"]
    rng = random.Random(83)
    slots = X.spread_slots(n, cap)
    x = XfitPair(cap, (MOST, 1, 1), {GPU: 3}, pods_per_round=64)
    x.upsert(X.xfit_nodes(rng, n), slots)
    pre = X.bound_pods(rng, n // 2, 60_000)
    x.add(pre, [rng.choice(slots) for _ in pre])
    batch = lambda b: pods_array([X.xfit_pod(rng, b * 1000 + j) for j in range(60)], x.a)

    def prepared(pa, m, then, what):
        """Prepared under the strategy in force, run after `then` switched it: the run's strategy counts."""
        h = x.s.prepare(pa, m)
        then()
        x.s.run(h)
        got = x.s.results(h, m)
        x.s.free(h)
        assert_results_equal(got, x.o.schedule(pa, m), m, what)
        x.states_equal(what)

    pa, m = batch(0)
    assert_results_equal(x.s.schedule_raw(pa, m), x.o.schedule(pa, m), m, "list on")
    # on -> off through the old setter, which clears the list, between prepare and run
    def off():
        x.s.set_fit_strategy(MOST, {"cpu": 1, "memory": 1})
        x.o.set_strategy((MOST, 1, 1), {})
    prepared(*batch(1), off, "prepared with the list, run without")
    assert x.s.get_fit_strategy() == (MOST, {"cpu": 1, "memory": 1})
    # off -> on with other weights and another resource, again between prepare and run
    prepared(*batch(2), lambda: x.use((LEAST, 2, 1), {GPU: 7, NIC: 2}), "prepared without the list, run with one")
    assert x.s.get_fit_strategy() == (LEAST, {"cpu": 2, "memory": 1, GPU: 7, NIC: 2})
    # one list -> another type with a shape
    prepared(*batch(3), lambda: x.use((SHAPES["peaked"], 1, 1), {NIC: 5, GPU: 1}), "run under a shape and a list")
    assert x.s.get_fit_shape() == list(SHAPES["peaked"])
    # the shape setter clears the list too
    def shape_only():
        x.s.set_fit_strategy(RTCR, {"cpu": 1, "memory": 1}, SHAPES["binpack"])
        x.o.set_strategy((SHAPES["binpack"], 1, 1), {})
    prepared(*batch(4), shape_only, "the shape setter clears the list")
    assert x.s.get_fit_strategy() == (RTCR, {"cpu": 1, "memory": 1})
    x.dump_equal(X.xfit_pod(rng, 90_002), "dump after the switches")
    x.close()


# ------------------------------------------------------------ (d) sharding
@pytest.mark.parametrize("case", ["most-1-1-gpu3", "falling-1-0-gpu1-nic3"])
def test_virtual_shards(case):
    x = XfitPair(X.SIZES["large"][1], *X.CASES[case], pods_per_round=64, virtual_shards=3)
    X.sweep_stream(x, 72, "large")
    x.close()


@pytest.mark.parametrize("case", ["most-1-1-gpu3", "binpack-1-1-gpu3"])
def test_two_ranks(case):
    # a two-rank in-process world (tests/test_gpu_multirank.py): the chain runs replicated, both ranks set the list
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "xfit", "case": case}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] > 0


# --------------------------------------------------------------- (e) dumps
@pytest.mark.parametrize("case", sorted(X.CASES))
def test_dumps_of_requesting_and_other_pods(case):
    n, cap = X.SIZES["small"]
    rng = random.Random(85)
    slots = X.spread_slots(n, cap)
    x = XfitPair(cap, *X.CASES[case])
    x.upsert(X.xfit_nodes(rng, n), slots)
    pre = X.bound_pods(rng, n, 60_000)
    x.add(pre, [rng.choice(slots) for _ in pre])
    req = {"cpu": 500, "memory": 512 * Mi}
    pods = [Pod("plain", containers=[Container(dict(req))]),
            Pod("gpu", containers=[Container(dict(req, **{GPU: 1}))]),
            Pod("both", containers=[Container(dict(req, **{GPU: 2, NIC: 1}))]),
            Pod("huge", containers=[Container(dict(req, **{HUGE: 256 * Mi}))]),  # the chain, nothing listed
            Pod("init", containers=[Container(dict(req))], init_containers=[Container({GPU: 2})])]
    fits = {}
    for p in pods:
        pa, _ = pods_array([p], x.a)
        out = (_abi.KsNodeScore * cap)()
        assert x.s.lib.ks_plugin_scores(x.s.ctx, pa, out) == 0, x.s.lib.ks_last_error(x.s.ctx)
        got, want = scores_np(out, cap), x.o.plugin_scores(pa)
        assert np.array_equal(got, want), (p.name, np.nonzero(got != want)[0][:5])
        assert (want["status"] == -1).sum() > 20
        fits[p.name] = want
    # on nodes feasible for both, the requesting pod's NodeResourcesFit score differs from the plain pod's
    both = (fits["plain"]["status"] == -1) & (fits["gpu"]["status"] == -1)
    assert (fits["plain"]["least_allocated"][both] != fits["gpu"]["least_allocated"][both]).sum() > 20
    x.close()


# ------------------------------------------------------------ (f) refusals
def set_res(s, fs, shape, extended):
    arr, n, keep = ext_array(extended) if isinstance(extended, dict) else extended
    pts = None if shape is None else (_abi.KsFitShapePoint * max(1, len(shape)))(
        *[_abi.KsFitShapePoint(u, v) for u, v in shape])
    return s.lib.ks_set_fit_strategy_resources(s.ctx, C.byref(fs), pts, 0 if shape is None else len(shape), arr, n)


def test_refusals():
    INV, UNS, RNG = _abi.KS_ERR_INVALID, _abi.KS_ERR_UNSUPPORTED, _abi.KS_ERR_RANGE
    most = _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, 1, 1, 0)
    rtcr = _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, 1, 1, 0)
    res = lambda *items: ((_abi.KsFitResource * max(1, len(items)))(*[_abi.KsFitResource(n, w, 0) for n, w in items]),
                          len(items), None)
    with Scheduler(64) as s:
        s.set_fit_strategy(MOST, {"cpu": 2, "memory": 1, GPU: 3})
        before = (MOST, {"cpu": 2, "memory": 1, GPU: 3})
        assert s.get_fit_strategy() == before
        for bad in [res((None, 1)), res((b"", 1)), res((b"cpu", 1)), res((b"memory", 1)), res((b"pods", 1)),
                    res((b"amd.com/gpu", 1), (b"amd.com/gpu", 2)),   # repeated
                    res((b"gpu", 1)), res((b"storage", 1)),          # neither scalar nor ephemeral-storage
                    res((b"amd.com/gpu", 0)), res((b"amd.com/gpu", 101)), res((b"amd.com/gpu", -1)),
                    res(*[(f"example.com/r{i}".encode(), 1) for i in range(9)])]:  # more than 8
            assert set_res(s, most, None, bad) == INV, [(bad[0][i].name, bad[0][i].weight) for i in range(bad[1])]
        assert s.lib.ks_set_fit_strategy_resources(s.ctx, C.byref(most), None, 0, None, 1) == INV
        assert s.lib.ks_set_fit_strategy_resources(s.ctx, None, None, 0, res((b"amd.com/gpu", 1))[0], 1) == INV
        # every invalid input of the sibling calls
        for w in [(101, 1), (1, 101), (-1, 1)]:
            assert set_res(s, _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, *w, 0), None, {GPU: 1}) == INV, w
        assert set_res(s, _abi.KsFitStrategy(7, 1, 1, 0), None, {GPU: 1}) == INV
        assert set_res(s, most, SHAPES["peaked"], {GPU: 1}) == INV          # a shape with another type
        assert set_res(s, rtcr, None, {GPU: 1}) == INV                      # the type without its shape
        for shape in [(), ((0, 11),), ((10, 1), (10, 2)), ((20, 1), (10, 2))]:
            assert set_res(s, rtcr, shape, {GPU: 1}) == INV, shape
        # no extended resource: the old calls, to the letter -- both weights 0 stays invalid there
        zero = _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, 0, 0, 0)
        assert set_res(s, zero, None, {}) == INV
        assert set_res(s, _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, 0, 0, 0), SHAPES["peaked"], {}) == INV
        assert set_res(s, rtcr, None, {}) == INV
        # ephemeral-storage is scored for every pod upstream: refused, not approximated
        assert set_res(s, most, None, {"ephemeral-storage": 1}) == UNS
        assert set_res(s, most, None, {GPU: 1, "ephemeral-storage": 1}) == UNS
        # refused calls change nothing
        assert s.get_fit_strategy() == before and s.get_fit_shape() == []
        n = C.c_uint32()
        out = (_abi.KsFitResource * 8)()
        assert s.lib.ks_get_fit_resources(s.ctx, out, 8, C.byref(n)) == 0 and n.value == 1
        assert (out[0].name, out[0].weight) == (GPU.encode(), 3)
        assert s.lib.ks_get_fit_resources(s.ctx, out, 0, C.byref(n)) == INV and n.value == 1  # too small
        assert s.lib.ks_get_fit_resources(s.ctx, out, 8, None) == INV
        # valid: cpu and memory both left out, every kind of scalar name
        assert set_res(s, zero, None, {GPU: 1, "hugepages-2Mi": 2, "attachable-volumes-csi-x": 3,
                                       "kubernetes.io/batteries": 100}) == 0
        assert s.get_fit_strategy() == (MOST, {"cpu": 0, "memory": 0, GPU: 1, "hugepages-2Mi": 2,
                                               "attachable-volumes-csi-x": 3, "kubernetes.io/batteries": 100})
        # n_extended == 0 is the old call: it clears the list
        assert set_res(s, most, None, {}) == 0
        assert s.get_fit_strategy() == (MOST, {"cpu": 1, "memory": 1})
        assert s.lib.ks_get_fit_resources(s.ctx, out, 8, C.byref(n)) == 0 and n.value == 0

        # ---- the 2^44 bound on a listed resource's Allocatable
        big, ok = 1 << 44, (1 << 44) - 1
        node = lambda name, v: Node(name, {"cpu": 4000, "memory": 8 * Gi, "pods": 10},
                                    extended={GPU: v, "ephemeral-storage": 20 * 1024 * Gi})
        s.upsert_nodes([node("n0", big)], [0])  # unlisted: the whole int64 range
        assert set_res(s, most, None, {GPU: 3}) == RNG  # from the setter: a present node holds such a value
        assert s.get_fit_strategy() == (MOST, {"cpu": 1, "memory": 1})
        s.upsert_nodes([node("n0", ok)], [0])
        assert set_res(s, most, None, {GPU: 3}) == 0
        state = lambda: [(t.alloc_milli_cpu, t.alloc_memory, t.alloc_pods) for t in s.node_states([1, 2])]
        empty = state()
        with pytest.raises(_abi.KschedError):  # from the node side: refused before anything is applied
            s.upsert_nodes([node("n1", 8), node("n2", big)], [1, 2])
        assert state() == empty, "a refused upsert applied a node"
        ev = (_abi.KsEvent * 1)()
        a = Arena()
        na, _ = nodes_array([node("n2", big)], a)
        ev[0].kind, ev[0].slot, ev[0].node = _abi.KS_EV_NODE_UPSERT, 2, na
        assert s.lib.ks_events_apply(s.ctx, ev, 1) == RNG
        s.upsert_nodes([node("n1", 8)], [1])
        # and a pod is scored with the largest value in range
        r = s.schedule_pods([Pod("p", containers=[Container({"cpu": 100, GPU: 4})])])
        assert r[0].suggested_host in ("n0", "n1")
        s.set_fit_strategy(MOST)  # the list is gone: the node is accepted again
        s.upsert_nodes([node("n2", big)], [2])
    with Scheduler(64, percentage_of_nodes_to_score=5) as s:
        assert set_res(s, _abi.KsFitStrategy(_abi.FIT_LEAST_ALLOCATED, 1, 1, 0), None, {GPU: 1}) == UNS
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1})
    with Scheduler(64, fit_strategy=RTCR, fit_resource_weights={"cpu": 1, "memory": 1, GPU: 3},
                   fit_shape=[(0, 0), (100, 10)]) as s:  # the bin-packing guide's profile
        assert s.get_fit_strategy() == (RTCR, {"cpu": 1, "memory": 1, GPU: 3}) and s.get_fit_shape() == [(0, 0), (100, 10)]
