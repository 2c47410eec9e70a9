"""Workloads of the tests of NodeResourcesBalancedAllocation over a list of
resources: shared by the CPU test of the reference (tests/test_ba_reference.py,
which also counts what the GPU tests' teeth rest on) and the GPU tests
(tests/test_gpu_ba.py).  The streams are tests/xfit_workloads.py's, driven
through a pair object with the same interface.
"""
import functools

import numpy as np

import xfit_workloads as X
from ba_reference import BaReference
from fit_reference import LEAST, MOST
from ksched.objects import Container, Node, Pod
from rtcr_reference import SHAPES
from xfit_reference import GPU, HUGE, NIC

Gi = 1 << 30
ONE = ["cpu", "memory", GPU]
THREE = [GPU, "cpu", NIC, "memory", HUGE]  # cpu and memory inside the list, not at its head

# (NodeResourcesFit strategy, its extended {name: weight}, the balanced list):
# every fit variant of the filter pass under a list
CASES = {
    "default-gpu": ((LEAST, 1, 1), {}, ONE),
    "default-three": ((LEAST, 1, 1), {}, THREE),
    "most-gpu3-gpu": ((MOST, 1, 1), {GPU: 3}, ONE),          # the strategy lists the same resource
    "most-3-1-three": ((MOST, 3, 1), {}, THREE),
    "peaked-gpu": ((SHAPES["peaked"], 1, 1), {}, [GPU, "memory", "cpu"]),
    "binpack-gpu3-three": ((SHAPES["binpack"], 1, 1), {GPU: 3}, THREE),
}


def configure(s, case):
    """A case on a ksched.Scheduler."""
    strategy, extended, balanced = CASES[case]
    X.set_strategy(s, strategy, extended)
    s.set_balanced_resources(balanced)


def two_rank_case(cfg):
    return X.replicated_case(93, lambda cap: BaReference(cap, *CASES[cfg["case"]]), lambda s: configure(s, cfg["case"]))


# ---------------------------------------------------------------- the grid
A, B = "example.com/a", "example.com/b"
GRID_CAP = 16384
UNITS = {"cpu": 1000, "memory": Gi, A: 1, B: 1}  # Allocatable is 10 units of each


def _node(name, memory=10):
    return Node(name, {"cpu": 10 * UNITS["cpu"], "memory": memory * UNITS["memory"], "pods": 8},
                extended={A: 10, B: 10})


def _bound(name, cpu, mem, a, b):
    req = {k: v * UNITS[k] for k, v in (("cpu", cpu), ("memory", mem), (A, a), (B, b)) if v}
    return Pod(name, containers=[Container(req)])


@functools.lru_cache(maxsize=None)
def grid():
    """(nodes, slots, bound pods, their slots, units): 12,100 nodes whose
    Requested, in units of a tenth of the Allocatable, covers {0..10}^2 for cpu
    and memory and {0..9}^2 for the two extended resources -- the asking pod
    (grid_pod) adds one unit of each of those, and no cpu or memory.  Then the
    extra nodes: memory Allocatable 0 (two fractions under [cpu, memory, a]:
    the shortcut, at (0.1, 0.8) among others), and cpu Requested beyond
    Allocatable (the clamp; the pod asks no cpu, so they stay feasible)."""
    units = [(c, m, a, b) for c in range(11) for m in range(11) for a in range(10) for b in range(10)]
    nodes = [_node(f"g{i}") for i in range(len(units))]
    nomem = [(1, 0, 7, 3), (5, 0, 0, 0), (10, 0, 9, 9), (0, 0, 4, 6), (3, 0, 2, 8)]
    clamp = [(15, 5, 2, 7), (11, 0, 0, 0), (40, 10, 9, 9), (12, 3, 4, 1)]
    nodes += [_node(f"z{i}", memory=0) for i in range(len(nomem))] + [_node(f"c{i}") for i in range(len(clamp))]
    units += nomem + clamp
    slots = X.spread_slots(len(nodes), GRID_CAP)
    pods, pslots = [], []
    for i, (u, s) in enumerate(zip(units, slots)):
        if any(u):
            pods.append(_bound(f"b{i}", *u))
            pslots.append(s)
    return nodes, slots, pods, pslots, np.array(units, dtype=np.int64)


def grid_pod():
    return Pod("ask", containers=[Container({A: 1, B: 1})])


GRID_LISTS = {"cpu-mem-a-b": ["cpu", "memory", A, B], "a-b-cpu-mem": [A, B, "cpu", "memory"],
              "a-cpu-b-mem": [A, "cpu", B, "memory"], "cpu-mem-a": ["cpu", "memory", A], "default": None}
