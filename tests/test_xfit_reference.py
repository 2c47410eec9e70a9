"""The reference for strategies that list extended resources, on the CPU
(tests/xfit_reference.py): hand-derived answers, the
pod-request restatement, equality with FitReference / RtcrReference when
nothing is listed, and the teeth of the GPU tests' streams -- listing the
resource must change the schedule, so a kernel that ignored the records
could not pass tests/test_gpu_xfit.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import xfit_workloads as X
from fit_reference import LEAST, MOST, FitReference
from helpers import assert_results_equal, res_array
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from rtcr_reference import SHAPES, RtcrReference
from xfit_reference import GPU, NIC, XfitReference, combine, pod_xrequests

Gi = 1 << 30


def one(kind, resources):
    """Node score of one node from [(weight, capacity, requested)]."""
    return int(combine(kind, [(w, [c], [r]) for w, c, r in resources])[0])


# ------------------------------------------------------ hand-derived answers
def test_most_allocated_with_an_extended_resource():
    # cpu 25 %, memory 75 %, gpu 8 allocatable with 2 requested, the pod asks 2: gpu 4 * 100 / 8 = 50
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6), (3, 8, 4)]) == (25 + 75 + 150) // 5 == 50
    # the same node for a pod that asks no gpu: the resource is bypassed, d = 2
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6)]) == (25 + 75) // 2 == 50
    # gpu 8 with 6 requested, the pod asks 2: gpu 100 -> (25 + 75 + 300) / 5 = 80, against 50 without it
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6), (3, 8, 8)]) == 80
    # truncation of the weighted mean: (25 + 75 + 3 * 37) / 5 = 42.2 -> 42 (gpu 3 of 8 = 37.5 -> 37)
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6), (3, 8, 3)]) == 42
    # requested beyond capacity clamps to 100 (Requested can pass Allocatable after pods are added)
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6), (3, 8, 11)]) == 80
    # a node without the resource: Allocatable 0 leaves it out (such a node fails the filter; the score is still defined)
    assert one(MOST, [(1, 4000, 1000), (1, 8, 6), (3, 0, 2)]) == 50


def test_least_allocated_extended_resource_alone():
    # {gpu 1} alone: 3 of 8 after the pod -> 5 * 100 / 8 = 62.5 -> 62
    assert one(LEAST, [(0, 4000, 1000), (0, 8, 6), (1, 8, 3)]) == 62
    assert one(LEAST, [(0, 4000, 1000), (0, 8, 6), (1, 8, 9)]) == 0     # requested > capacity
    assert one(LEAST, [(0, 4000, 1000), (0, 8, 6)]) == 0                # a pod asking no gpu: nothing is scored
    # {cpu 2, nic 1, gpu 5}: cpu 75 free, nic 1 of 4 -> 75, gpu 6 of 8 -> 25: (150 + 75 + 125) / 8 = 43.75 -> 43
    assert one(LEAST, [(2, 4000, 1000), (0, 8, 6), (1, 4, 1), (5, 8, 6)]) == 43
    # the same pod without nic: (150 + 125) / 7 = 39.28 -> 39
    assert one(LEAST, [(2, 4000, 1000), (0, 8, 6), (5, 8, 6)]) == 39


def test_requested_to_capacity_ratio_with_an_extended_resource():
    b = SHAPES["binpack"]  # raw(p) = p
    # {cpu 1, memory 1, gpu 3}: gpu 1 of 200 is utilisation 0, table score 0, and leaves d:
    # (25 + 75) / 2 = 50 (kept in d it would be 100 / 5 = 20)
    assert one(b, [(1, 4000, 1000), (1, 8, 6), (3, 200, 1)]) == 50
    # and a half: cpu 30, memory 45, gpu 0 -> 75 / 2 = 37.5 -> 38
    assert one(b, [(1, 100, 30), (1, 100, 45), (3, 200, 1)]) == 38
    # all three positive: (25 + 75 + 3 * 50) / 5 = 50
    assert one(b, [(1, 4000, 1000), (1, 8, 6), (3, 8, 4)]) == 50
    # cpu's score 0 leaves d = 4: (45 + 3 * 75) / 4 = 67.5 -> 68
    assert one(b, [(1, 1000, 5), (1, 100, 45), (3, 8, 6)]) == 68
    # (30 + 45 + 3 * 12) / 5 = 22.2 -> 22; gpu 1 of 8 = 12.5 -> 12
    assert one(b, [(1, 100, 30), (1, 100, 45), (3, 8, 1)]) == 22
    p = SHAPES["peaked"]  # {0:0, 50:100, 100:0}: a full gpu scores 0 and leaves d
    assert one(p, [(1, 100, 25), (1, 100, 75), (2, 8, 8)]) == 50
    assert one(p, [(1, 100, 25), (1, 100, 75), (2, 8, 4)]) == (50 + 50 + 200 + 2) // 4 == 75  # 300 / 4
    assert one(p, [(0, 100, 25), (0, 100, 75), (2, 8, 8)]) == 0  # no positive score at all
    f = SHAPES["falling"]  # {0:100, 30:0}: raw(12) = 100 - 100 * 12 / 30 = 60
    assert one(f, [(1, 100, 15), (0, 100, 75), (1, 8, 1), (3, 4, 4)]) == (50 + 60 + 1) // 2 == 55  # nic full: 0


def pod_ptr(pod):
    a = Arena()
    pa, _ = pods_array([pod], a)
    return pa, a


def test_pod_requests_restated():
    # containers 1 + 2; a sidecar of 1 counts with them (4) and under the init container after it (4 + 1)
    p = Pod("p", containers=[Container({GPU: 1, "cpu": 100}), Container({GPU: 2, NIC: 1})],
            init_containers=[Container({GPU: 1}, restart_policy_always=True), Container({GPU: 4})])
    pa, keep = pod_ptr(p)
    assert pod_xrequests(pa) == {GPU: 5, NIC: 1}
    # an init container before the sidecar does not run beside it
    p.init_containers = [Container({GPU: 4}), Container({GPU: 1}, restart_policy_always=True)]
    pa, keep = pod_ptr(p)
    assert pod_xrequests(pa) == {GPU: 4, NIC: 1}
    p = Pod("q", containers=[Container({GPU: 0, "cpu": 100})])  # a zero request is no request: bypassed
    pa, keep = pod_ptr(p)
    assert pod_xrequests(pa) == {}


def test_mirror_and_end_to_end_example():
    """The issue's MostAllocated example through the reference itself: the
    mirror of extended Allocatable / Requested, the bypass and the commit."""
    a = Arena()
    nodes = [Node("n0", {"cpu": 4000, "memory": 8 * Gi, "pods": 10}, extended={GPU: 8}),
             Node("n1", {"cpu": 4000, "memory": 8 * Gi, "pods": 10}, extended={GPU: 8})]
    na, k = nodes_array(nodes, a)
    bound = [Pod("b0", containers=[Container({"cpu": 500, "memory": 5 * Gi, GPU: 2})]),
             Pod("b1", containers=[Container({"cpu": 500, "memory": 5 * Gi, GPU: 6})])]
    ba, m = pods_array(bound, a)
    slots = (C.c_uint32 * 2)(0, 1)
    r = XfitReference(2, (MOST, 1, 1), {GPU: 3})
    r.upsert(na, slots, k)
    r.add_pods(ba, slots, m)
    ask, keep = pod_ptr(Pod("p", containers=[Container({"cpu": 500, "memory": Gi, GPU: 2})]))
    assert r.fit(ask).tolist() == [50, 80]
    plain, keep2 = pod_ptr(Pod("q", containers=[Container({"cpu": 500, "memory": Gi})]))
    assert r.fit(plain).tolist() == [50, 50]
    res = r.schedule_one(ask)
    assert (res.status, res.node_index) == (0, 1) and r.xreq[GPU].tolist() == [2, 8]
    assert r.plugin_scores(ask)["status"].tolist() == [-1, 4]  # n1 is full: NodeResourcesFit
    r.remove_pods(ba, slots, m)
    assert r.xreq[GPU].tolist() == [0, 2]
    r.delete(slots, 1)
    r.upsert(na, slots, k)  # n0 re-added, n1 replaced in place: its Requested stays
    assert r.xreq[GPU].tolist() == [0, 2] and r.xalloc[GPU].tolist() == [8, 8]
    r.close()


# ------------------------------------------- nothing listed: the older references
class Solo:
    """A stream driven through one reference, nothing compared."""

    def __init__(self, ref):
        self.o, self.a = ref, Arena()

    @staticmethod
    def _u32(xs):
        return (C.c_uint32 * max(1, len(xs)))(*xs)

    def upsert(self, nodes, slots):
        na, k = nodes_array(nodes, self.a)
        self.o.upsert(na, self._u32(slots), k)

    def delete(self, slots):
        self.o.delete(self._u32(slots), len(slots))

    def add(self, pods, slots, sign=1):
        if pods:
            pa, k = pods_array(pods, self.a)
            (self.o.add_pods if sign > 0 else self.o.remove_pods)(pa, self._u32(slots), k)

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        return res_array(self.o.schedule(pa, m), m)

    def dump_equal(self, pod, what=""):
        pass

    def states_equal(self, what=""):
        pass


class Both(Solo):
    """Two references fed the same events and compared field for field."""

    def __init__(self, ref, other):
        super().__init__(ref)
        self.s = other

    def upsert(self, nodes, slots):
        na, k = nodes_array(nodes, self.a)
        for t in (self.s, self.o):
            t.upsert(na, self._u32(slots), k)

    def add(self, pods, slots, sign=1):
        if pods:
            pa, k = pods_array(pods, self.a)
            for t in (self.s, self.o):
                (t.add_pods if sign > 0 else t.remove_pods)(pa, self._u32(slots), k)

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        want, got = self.o.schedule(pa, m), self.s.schedule(pa, m)
        assert_results_equal(got, want, m, what)
        return res_array(got, m)

    def dump_equal(self, pod, what=""):
        pa, _ = pods_array([pod], self.a)
        g, w = self.s.plugin_scores(pa), self.o.plugin_scores(pa)
        assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])

    def states_equal(self, what=""):
        assert np.array_equal(self.s.states(), self.o.states()), what


@pytest.mark.parametrize("strategy", [(MOST, 3, 1), (LEAST, 1, 1), (SHAPES["peaked"], 1, 1), (SHAPES["falling"], 1, 0)],
                         ids=["most-3-1", "default", "peaked-1-1", "falling-1-0"])
def test_nothing_listed_is_the_older_reference(strategy):
    cap = X.SIZES["small"][1]
    older = FitReference(cap, strategy) if isinstance(strategy[0], str) else RtcrReference(cap, strategy)
    x = Both(XfitReference(cap, strategy, {}), older)
    _, res = X.sweep_stream(x, 61, "small")
    assert sum(int((r["status"] == 0).sum()) for r in res) > 100
    x.o.close()
    x.s.close()


# --------------------------------------------------------------------- teeth
@functools.lru_cache(maxsize=None)
def placements(case, seed, size, listed):
    strategy, extended = X.CASES[case]
    if not listed and strategy[1] == 0 and strategy[2] == 0:
        strategy = (strategy[0], 1, 1)  # nothing at all would be listed: the default weights
    r = XfitReference(X.SIZES[size][1], strategy, extended if listed else {})
    pods, res = X.sweep_stream(Solo(r), seed, size, dumps=False)
    r.close()
    return pods, np.concatenate(res)


def teeth(case, seed, size):
    """(pods requesting a listed resource, how many of them the listing moves,
    NodeResourcesFit failures seen by those pods)."""
    pods, with_list = placements(case, seed, size, True)
    _, without = placements(case, seed, size, False)
    ask = np.array([X.requests_extended(p, X.CASES[case][1]) for p in pods])
    moved = ask & (with_list["node_index"] != without["node_index"])
    return int(ask.sum()), int(moved.sum()), int(with_list["fail"][ask, 4].sum())


@pytest.mark.parametrize("case", sorted(X.CASES))
def test_listing_the_resource_changes_the_schedule(case):
    n_ask, n_moved, fit_fails = teeth(case, 71, "small")
    assert n_ask >= 100 and fit_fails > 0
    assert 10 * n_moved >= n_ask, f"{case}: only {n_moved} of {n_ask} requesting pods move"
