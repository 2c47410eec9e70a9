"""The reference for NodeResourcesBalancedAllocation over a list of resources,
on the CPU (tests/ba_reference.py): the known answers,
equality with the oracle's own schedule under the default list and under a
list no pod requests from, and the counts the GPU tests' teeth rest on
(tests/test_gpu_ba.py): the list and its order change the grid's scores and
the streams' schedules, so a build that ignored either could not pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import ba_workloads as W
import pyoracle
import xfit_workloads as X
from ba_reference import BaReference, ba_scores
from fit_reference import scores_np
from ksched.objects import Arena, nodes_array, pods_array
from test_xfit_reference import Both, Solo


def one(fractions, den=1000):
    """Score of one node from fractions given as exact multiples of 1 / den."""
    return int(ba_scores([([den], [round(f * den)]) for f in fractions])[0])


# ------------------------------------------------------------ known answers
def test_known_answers():
    assert one((0.25, 0.75, 0.5)) == 79
    assert one((0, 0, 1)) == 52
    # the variance is an exact square: a square root one ulp high gives 74
    assert one((0.25, 0.25, 0.75, 0.75)) == 75
    for k in range(11):  # the rounded mean differs from the fractions at 0.7 and 0.8
        assert one((k / 10,) * 3, den=10) == (99 if k in (7, 8) else 100), k
    # the list's order decides
    assert one((0, 0.1, 0.4, 0.9), den=10) == 65
    assert one((0.4, 0.9, 0, 0.1), den=10) == 64
    # two fractions keep the shortcut, which the general formula does not reproduce here
    shortcut = int((1.0 - abs((0.1 - 0.8) / 2)) * 100.0)
    mean = (0.1 + 0.8) / 2.0
    general = int((1.0 - np.sqrt(((0.1 - mean) * (0.1 - mean) + (0.8 - mean) * (0.8 - mean)) / 2.0)) * 100.0)
    assert one((0.1, 0.8), den=10) == shortcut != general
    assert one((0.3,), den=10) == 100 and int(ba_scores([])[0]) == 100


def test_zero_allocatable_and_the_clamp():
    # a zero Allocatable leaves the resource out: two fractions remain, the shortcut
    assert int(ba_scores([([10], [1]), ([0], [5]), ([10], [8])])[0]) == one((0.1, 0.8), den=10)
    # requested beyond Allocatable clamps to 1
    assert int(ba_scores([([10], [25]), ([10], [10]), ([10], [10])])[0]) == 100
    assert int(ba_scores([([10], [25]), ([10], [0]), ([10], [0])])[0]) == one((0, 0, 1))


# ------------------------------------------------- the default list: the oracle
class OracleSide:
    """pyoracle.Oracle behind the methods Both compares."""

    def __init__(self, cap):
        self.o, self.cap = pyoracle.Oracle(cap), cap
        for name in ("upsert", "delete", "add_pods", "remove_pods", "schedule", "close"):
            setattr(self, name, getattr(self.o, name))

    def plugin_scores(self, pa):
        return scores_np(self.o.plugin_scores(pa), self.cap)


class BothNoStates(Both):
    def states_equal(self, what=""):
        pass


@pytest.mark.parametrize("balanced", [None, ["memory", "cpu"], ["cpu", "memory", "example.com/none"]],
                         ids=["default", "memory-cpu", "nobody-requests"])
def test_default_list_reproduces_the_oracle(balanced):
    """oracle.schedule field for field, and every dump, with the default list;
    and a list whose scalar name no pod requests is the default."""
    cap = X.SIZES["small"][1]
    x = BothNoStates(BaReference(cap, balanced=balanced), OracleSide(cap))
    _, res = X.sweep_stream(x, 61, "small")
    assert sum(int((r["status"] == 0).sum()) for r in res) > 100
    x.o.close()
    x.s.close()


# --------------------------------------------------------------------- teeth
@functools.lru_cache(maxsize=None)
def placements(case, seed, size, listed):
    strategy, extended, balanced = W.CASES[case]
    r = BaReference(X.SIZES[size][1], strategy, extended, balanced if listed else None)
    pods, res = X.sweep_stream(Solo(r), seed, size, dumps=False)
    r.close()
    return pods, np.concatenate(res)


def teeth(case, seed, size):
    """(pods requesting a listed scalar resource, how many of them the list moves)."""
    pods, with_list = placements(case, seed, size, True)
    _, without = placements(case, seed, size, False)
    ask = np.array([X.requests_extended(p, [n for n in W.CASES[case][2] if n not in ("cpu", "memory")]) for p in pods])
    moved = ask & (with_list["node_index"] != without["node_index"])
    return int(ask.sum()), int(moved.sum())


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_the_list_changes_the_schedule(case):
    n_ask, n_moved = teeth(case, 71, "small")
    print(f"{case}: {n_moved} of {n_ask} requesting pods move")
    assert n_ask >= 100
    assert 10 * n_moved >= n_ask, f"{case}: only {n_moved} of {n_ask} requesting pods move"


@functools.lru_cache(maxsize=None)
def grid_reference():
    """The grid cluster in a BaReference, and the asking pod."""
    nodes, slots, pods, pslots, units = W.grid()
    a = Arena()
    r = BaReference(W.GRID_CAP)
    u32 = lambda xs: (C.c_uint32 * len(xs))(*xs)
    na, k = nodes_array(nodes, a)
    r.upsert(na, u32(slots), k)
    pa, m = pods_array(pods, a)
    r.add_pods(pa, u32(pslots), m)
    ask, _ = pods_array([W.grid_pod()], a)
    return r, ask, a


@functools.lru_cache(maxsize=None)
def grid_scores(name):
    r, ask, _ = grid_reference()
    r.set_balanced(W.GRID_LISTS[name])
    return r.plugin_scores(ask)


def test_grid_has_teeth():
    _, slots, _, _, units = W.grid()
    slots = np.array(slots)
    sc = {name: grid_scores(name) for name in W.GRID_LISTS}
    feas = sc["default"]["status"][slots] == -1
    assert feas.all()
    ba = {name: s["balanced_allocation"][slots] for name, s in sc.items()}
    order = int((ba["cpu-mem-a-b"] != ba["a-b-cpu-mem"]).sum())
    listed = int((ba["cpu-mem-a-b"] != ba["default"]).sum())
    print(f"grid: {order} nodes depend on the order, {listed} of {len(slots)} on the list")
    assert order >= 1 and (ba["a-cpu-b-mem"] != ba["cpu-mem-a-b"]).any()
    assert 2 * listed > len(slots)
    assert (sc["cpu-mem-a-b"]["total_score"][slots] != sc["default"]["total_score"][slots]).sum() == listed
    # three equal fractions k/10 under [cpu, memory, a]: 99 at k = 7 and 8
    for k in range(1, 11):
        eq = (units[:, 0] == k) & (units[:, 1] == k) & (units[:, 2] == k - 1) & (np.arange(len(units)) < 12100)
        assert eq.sum() == 10 and (ba["cpu-mem-a"][eq] == (99 if k in (7, 8) else 100)).all(), k
    # memory Allocatable 0: the shortcut's value at (0.1, 0.8)
    z = 12100
    assert tuple(units[z]) == (1, 0, 7, 3) and ba["cpu-mem-a"][z] == int((1.0 - abs((0.1 - 0.8) / 2)) * 100.0)
    # cpu Requested beyond Allocatable: the fraction is 1
    c = 12105
    assert units[c][0] == 15 and ba["cpu-mem-a"][c] == int(ba_scores([([10], [10]), ([10], [5]), ([10], [3])])[0])
