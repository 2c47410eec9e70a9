"""NodeResourcesBalancedAllocation over a list of resources
(ks_set_balanced_resources) against the composed reference
(tests/ba_reference.py): ks_plugin_scores on every node, every result field,
fail_counts and every node's state, bit for bit.

(1) the grid dump: 12,100 nodes in 16,384 slots whose fractions cover
    {0..10}^2 x {1..10}^2 tenths, and the extra nodes (memory Allocatable 0,
    cpu Requested beyond Allocatable), under every list order of
    ba_workloads.GRID_LISTS -- the device's float64 sequence and its square
    root against numpy's, where one ulp of std or another summation order
    changes a score;
(2) scheduling parity over the mixed stream of tests/xfit_workloads.py with
    churn, under every NodeResourcesFit variant of the filter pass, each case
    first asserting that the list moves the requesting pods;
(3) a name listed before its column exists, a list switched between prepare and
    run in both directions, 3 virtual shards, two ranks, the refusals.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ba_workloads as W
import xfit_workloads as X
from ba_reference import BaReference
from fit_reference import LEAST, MOST, scores_np
from helpers import assert_results_equal
from ksched import Scheduler, _abi
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from test_ba_reference import grid_scores, teeth
from test_gpu_fit_spread import FitPair
from xfit_reference import GPU, HUGE, NIC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
LATE = "example.com/late"  # a resource no node reports at first


class BaPair(FitPair):
    """libksched and BaReference fed the same cache events."""

    def __init__(self, cap, case, **cfg):
        super().__init__(cap, (LEAST, 1, 1), **cfg)
        self.o.close()
        self.o = BaReference(cap, *W.CASES[case])
        W.configure(self.s, case)

    def use(self, balanced):
        self.s.set_balanced_resources(balanced)
        self.o.set_balanced(balanced)


# ------------------------------------------------------------ (1) the grid
@pytest.fixture(scope="module")
def grid_scheduler():
    nodes, slots, pods, pslots, _ = W.grid()
    a = Arena()
    s = Scheduler(W.GRID_CAP)
    s.upsert_nodes(nodes, slots)
    pa, m = pods_array(pods, a)
    assert s.lib.ks_pods_add(s.ctx, pa, (C.c_uint32 * m)(*pslots), m) == 0, s.lib.ks_last_error(s.ctx)
    ask, _ = pods_array([W.grid_pod()], a)
    yield s, ask
    s.close()


@pytest.mark.parametrize("name", list(W.GRID_LISTS))
def test_grid_dump(grid_scheduler, name):
    s, ask = grid_scheduler
    # teeth, on the reference alone: the order and the list change scores on this grid
    slots = np.array(W.grid()[1])
    ref = {k: grid_scores(k)["balanced_allocation"][slots] for k in ("cpu-mem-a-b", "a-b-cpu-mem", "default")}
    assert (ref["cpu-mem-a-b"] != ref["a-b-cpu-mem"]).any()
    assert 2 * (ref["cpu-mem-a-b"] != ref["default"]).sum() > len(slots)
    s.set_balanced_resources(W.GRID_LISTS[name])
    assert s.get_balanced_resources() == (W.GRID_LISTS[name] or ["cpu", "memory"])
    out = (_abi.KsNodeScore * W.GRID_CAP)()
    assert s.lib.ks_plugin_scores(s.ctx, ask, out) == 0, s.lib.ks_last_error(s.ctx)
    got, want = scores_np(out, W.GRID_CAP), grid_scores(name)
    assert (want["status"][slots] == -1).all()
    bad = np.nonzero(got["balanced_allocation"] != want["balanced_allocation"])[0]
    assert len(bad) == 0, (name, len(bad), [(int(i), int(got["balanced_allocation"][i]),
                                             int(want["balanced_allocation"][i])) for i in bad[:5]])
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:5])


# ------------------------------------------------- (2) scheduling parity
@pytest.mark.parametrize("case,size,seed", [(c, "small", 71) for c in sorted(W.CASES)] + [("default-gpu", "large", 72)])
def test_scheduling_parity(case, size, seed):
    # teeth first, on the reference alone: a build that accepted the list and scored cpu and memory only
    # would place these pods as the reference without the list does
    n_ask, n_moved = teeth(case, seed, size)
    assert 10 * n_moved >= n_ask > 0, (n_ask, n_moved)
    x = BaPair(X.SIZES[size][1], case, pods_per_round=64)
    _, res = X.sweep_stream(x, seed, size)
    r = np.concatenate(res)
    assert (r["status"] == 0).sum() > 100
    assert x.s.stats().spread_pods >= n_ask
    x.close()


@pytest.mark.parametrize("case", ["default-three", "binpack-gpu3-three"])
def test_three_listed_records(case):
    """Pods whose three records are all listed: the filter pass keeps the
    fractions of the first two from its fit check and computes the third from
    a second read of its columns."""
    n, cap = X.SIZES["small"]
    rng = random.Random(87)
    slots = X.spread_slots(n, cap)
    x = BaPair(cap, case, pods_per_round=64)
    nodes = X.xfit_nodes(rng, n)
    for nd in nodes[::2]:  # enough nodes that hold all three
        nd.extended.update({GPU: rng.choice([4, 8]), NIC: rng.randint(2, 4), HUGE: rng.choice([512, 1024]) * Mi})
    x.upsert(nodes, slots)
    pre = X.bound_pods(rng, n // 2, 60_000)
    x.add(pre, [rng.choice(slots) for _ in pre])

    def pod(j):
        return Pod(f"t{j}", containers=[Container({"cpu": rng.randrange(1, 10) * 100, "memory": rng.randrange(1, 8) * 128 * Mi,
                                                   GPU: rng.choice([1, 2]), NIC: 1, HUGE: rng.choice([128, 256]) * Mi})])

    # teeth, on the reference alone: the three fractions change such a pod's score on most nodes
    pa, _ = pods_array([pod(98)], x.a)
    with_list = x.o.ba(pa)
    x.o.set_balanced(None)
    without = x.o.ba(pa)
    x.o.set_balanced(W.CASES[case][2])
    assert (with_list != without).sum() > n // 4
    r = x.schedule([pod(j) for j in range(60)], f"three records {case}")
    assert (r["status"] == 0).sum() > 30
    x.states_equal(f"three records {case}")
    x.dump_equal(pod(99), f"three records {case}: dump")
    x.close()


def late_pod(rng, j):
    p = X.xfit_pod(rng, 10 * j + 2)
    p.containers[0].requests[LATE] = rng.choice([1, 2])
    return p


@pytest.mark.parametrize("case", ["default-gpu", "most-gpu3-gpu"])
def test_churn_and_a_name_listed_before_its_column(case):
    n, cap = X.SIZES["small"]
    rng = random.Random(81)
    slots = X.spread_slots(n, cap)
    x = BaPair(cap, case, pods_per_round=64)
    x.use([LATE] + W.CASES[case][2])  # listed before any node or pod has shown it
    assert x.s.get_balanced_resources()[0] == LATE
    x.upsert(X.xfit_nodes(rng, n), slots)
    live = list(zip(X.bound_pods(rng, n // 2, 60_000), [rng.choice(slots) for _ in range(n // 2)]))
    x.add([p for p, _ in live], [s for _, s in live])
    for b in range(4):
        kind = late_pod if b >= 2 else X.xfit_pod
        x.schedule([kind(rng, b * 1000 + j) for j in range(50)], f"churn {case} batch {b}")
        x.states_equal(f"churn {case} batch {b}")
        x.dump_equal(kind(rng, 97_002 + 10 * b), f"churn {case} dump {b}")
        rng.shuffle(live)
        gone, live = live[:20], live[20:]
        x.add([p for p, _ in gone], [s for _, s in gone], sign=-1)
        more = X.bound_pods(rng, 30, 70_000 + 100 * b)
        ms = [rng.choice(slots) for _ in more]
        x.add(more, ms)
        live += list(zip(more, ms))
        pick = rng.sample(slots, 12)
        fresh = X.xfit_nodes(rng, 10, slot0=n + 20 * b)
        for nd in fresh[:5]:
            nd.extended[GPU] = rng.choice([1, 16])
        if b >= 1:  # from here on nodes report the late resource: its column appears
            for nd in fresh:
                nd.extended[LATE] = rng.choice([2, 4])
        live = [(p, s) for p, s in live if s not in pick[8:]]
        x.delete(pick[8:])
        x.upsert(fresh, pick[:10])
        slots = [s for s in slots if s not in pick[10:]]
    assert x.s.stats().spread_pods > 150
    x.close()


# ------------------------------------------------------------ (3) variants
def test_list_switched_between_prepare_and_run():
    n, cap = X.SIZES["small"]
    rng = random.Random(83)
    slots = X.spread_slots(n, cap)
    x = BaPair(cap, "default-gpu", pods_per_round=64)
    x.upsert(X.xfit_nodes(rng, n), slots)
    pre = X.bound_pods(rng, n // 2, 60_000)
    x.add(pre, [rng.choice(slots) for _ in pre])
    batch = lambda b: pods_array([X.xfit_pod(rng, b * 1000 + j) for j in range(60)], x.a)

    def prepared(pa, m, then, what):
        """Prepared under the list in force, run after `then` switched it: the run's list counts."""
        h = x.s.prepare(pa, m)
        then()
        x.s.run(h)
        got = x.s.results(h, m)
        x.s.free(h)
        assert_results_equal(got, x.o.schedule(pa, m), m, what)
        x.states_equal(what)

    pa, m = batch(0)
    assert_results_equal(x.s.schedule_raw(pa, m), x.o.schedule(pa, m), m, "list on")
    prepared(*batch(1), lambda: x.use(None), "prepared with the list, run without")
    assert x.s.get_balanced_resources() == ["cpu", "memory"]
    prepared(*batch(2), lambda: x.use(W.THREE), "prepared without the list, run with one")
    assert x.s.get_balanced_resources() == W.THREE
    prepared(*batch(3), lambda: x.use([NIC, "memory", "cpu", GPU]), "one list to another order and set")
    x.dump_equal(X.xfit_pod(rng, 90_002), "dump after the switches")
    x.close()


@pytest.mark.parametrize("case", ["default-three", "most-gpu3-gpu"])
def test_virtual_shards(case):
    x = BaPair(X.SIZES["large"][1], case, pods_per_round=64, virtual_shards=3)
    X.sweep_stream(x, 72, "large")
    x.close()


@pytest.mark.parametrize("case", ["default-gpu", "binpack-gpu3-three"])
def test_two_ranks(case):
    # a two-rank in-process world (tests/test_gpu_multirank.py): the chain runs replicated, both ranks set the list
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "ba", "case": case}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] > 0


def set_list(s, names):
    arr = (C.c_char_p * max(1, len(names)))(*names)
    return s.lib.ks_set_balanced_resources(s.ctx, arr, len(names))


def test_refusals():
    INV, UNS, RNG = _abi.KS_ERR_INVALID, _abi.KS_ERR_UNSUPPORTED, _abi.KS_ERR_RANGE
    g = GPU.encode()
    with Scheduler(64, balanced_resources=["cpu", "memory", GPU]) as s:
        before = ["cpu", "memory", GPU]
        assert s.get_balanced_resources() == before
        for bad in [[b"cpu", None, b"memory"], [b"cpu", b"memory", b""], [b"cpu", b"memory", g, g], [b"cpu", b"cpu", b"memory"],
                    [b"cpu", b"memory", b"pods"], [b"cpu", b"memory", b"gpu"], [b"cpu", b"memory", b"storage"],
                    [b"cpu", b"memory"] + [f"example.com/r{i}".encode() for i in range(9)]]:  # more than 8 scalar names
            assert set_list(s, bad) == INV, bad
        assert s.lib.ks_set_balanced_resources(s.ctx, None, 3) == INV
        # ephemeral-storage is scored for every pod upstream; a list without cpu or memory changes every pod's score
        assert set_list(s, [b"cpu", b"memory", b"ephemeral-storage"]) == UNS
        for short in [[g], [b"cpu", g], [b"memory", g], [b"cpu"]]:
            assert set_list(s, short) == UNS, short
        assert s.get_balanced_resources() == before  # refused calls change nothing
        n = C.c_uint32()
        out = (C.c_char_p * 10)()
        assert s.lib.ks_get_balanced_resources(s.ctx, out, 10, C.byref(n)) == 0 and n.value == 3
        assert [out[i] for i in range(3)] == [b"cpu", b"memory", g]
        assert s.lib.ks_get_balanced_resources(s.ctx, out, 2, C.byref(n)) == INV and n.value == 3  # too small
        assert s.lib.ks_get_balanced_resources(s.ctx, out, 10, None) == INV
        # valid: every kind of scalar name, eight of them, cpu and memory anywhere
        full = ["hugepages-2Mi", "cpu", "attachable-volumes-csi-x", "kubernetes.io/batteries", GPU, "memory"] + [
            f"example.com/r{i}" for i in range(4)]
        s.set_balanced_resources(full)
        assert s.get_balanced_resources() == full
        s.set_balanced_resources([])  # n == 0 restores the default
        assert s.get_balanced_resources() == ["cpu", "memory"]
        assert s.lib.ks_get_balanced_resources(s.ctx, out, 10, C.byref(n)) == 0 and n.value == 2

        # ---- the 2^44 bound on a listed resource's Allocatable
        big, ok = 1 << 44, (1 << 44) - 1
        node = lambda name, v: Node(name, {"cpu": 4000, "memory": 8 * Gi, "pods": 10}, extended={GPU: v})
        s.upsert_nodes([node("n0", big)], [0])  # unlisted: the whole int64 range
        assert set_list(s, [b"cpu", b"memory", g]) == RNG  # from the setter: a present node holds such a value
        assert s.get_balanced_resources() == ["cpu", "memory"]
        s.upsert_nodes([node("n0", ok)], [0])
        assert set_list(s, [b"cpu", b"memory", g]) == 0
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
        # a pod is scored with the largest value in range: fractions 0.025, ~0, ~2^-42 -> 98
        r = s.schedule_pods([Pod("p", containers=[Container({"cpu": 100, GPU: 4})])])
        assert r[0].suggested_host in ("n0", "n1")
        s.set_balanced_resources(None)  # the list is gone: the node is accepted again
        s.upsert_nodes([node("n2", big)], [2])
    with Scheduler(64, percentage_of_nodes_to_score=5) as s:
        assert set_list(s, [b"cpu", b"memory", g]) == UNS
        assert set_list(s, [b"memory", b"cpu"]) == UNS  # any list other than the default
        assert set_list(s, [b"cpu", b"memory"]) == 0 and set_list(s, []) == 0
        assert s.get_balanced_resources() == ["cpu", "memory"]
