"""The identity behind ks_capacity, on the CPU: on random pre-filled clusters
the reference scheduler places replica after replica of one pod until the first
unschedulable result, and the number placed and every node's pod-count delta
equal the closed form of tests/capacity_reference.py.  These tests run no
product kernel: they pin the reference the GPU tests compare against."""
import random

import numpy as np
import pytest

import capacity_reference as CR
import diag_reference as R

XORDER = [CR.GPU, CR.DISK]


def cluster(seed, n, extended):
    rng = random.Random(seed)
    ref = R.DiagReference(n)
    ref.upsert(CR.rand_cluster(rng, n, extended=extended), list(range(n)))
    pods, slots = CR.rand_prefill(rng, n, extended=extended)
    ref.add(pods, slots)
    return ref


def fill(ref, pod, limit):
    """Replicas of `pod` scheduled until the first unschedulable result: (placed, pod-count delta per slot)."""
    before = ref.o.states()["pod_count"].astype(np.int64)
    placed, done = 0, False
    while not done:
        assert placed <= limit, "the fill does not end"
        res = ref.schedule([pod] * 64)
        status = [int(res[i].status) for i in range(64)]
        k = status.index(1) if 1 in status else 64
        assert all(s == 0 for s in status[:k]) and all(s == 1 for s in status[k:]), status
        placed += k
        done = k < 64
    return placed, ref.o.states()["pod_count"].astype(np.int64) - before


@pytest.mark.parametrize("seed,n", [(1, 50), (2, 137), (3, 300)])
@pytest.mark.parametrize("shape", ["resources", "selector", "besteffort"])
def test_fill_equals_the_closed_form(seed, n, shape):
    ref = cluster(seed, n, extended=False)
    pod = CR.shapes()[shape]
    want = CR.capacity(ref, pod)
    assert want["eligible_nodes"] > 0 and want["replicas"] > want["nodes_with_room"] > 0, want
    assert sum(want["bound_by"].values()) == want["eligible_nodes"]
    if shape == "besteffort":
        assert set(want["bound_by"]) == {"pods"}
    placed, delta = fill(ref, pod, want["replicas"])
    assert placed == want["replicas"]
    assert np.array_equal(delta, want["per_node"].astype(np.int64))
    after = CR.capacity(ref, pod)
    assert after["replicas"] == 0 and after["nodes_with_room"] == 0 and after["eligible_nodes"] == want["eligible_nodes"]
    ref.close()


def test_fill_equals_the_closed_form_extended():
    ref = cluster(4, 120, extended=True)
    pod = CR.shapes()["extended"]
    want = CR.capacity(ref, pod, XORDER)
    assert want["replicas"] > 0 and any(k in want["bound_by"] for k in XORDER), want
    placed, delta = fill(ref, pod, want["replicas"])
    assert placed == want["replicas"]
    assert np.array_equal(delta, want["per_node"].astype(np.int64))
    ref.close()


def test_node_capacity_ties_and_edges():
    f = CR.node_capacity
    assert f(5, [("cpu", 1000)], [("cpu", 200)], False) == (5, "pods")           # a tie goes to the first term
    assert f(6, [("cpu", 1000), ("memory", 10)], [("cpu", 200), ("memory", 2)], False) == (5, "cpu")
    assert f(6, [("cpu", 1001), ("memory", 9)], [("cpu", 200), ("memory", 2)], False) == (4, "memory")
    assert f(0, [("cpu", -5)], [("cpu", 1)], False) == (0, "pods")              # the zero minimum included
    assert f(-3, [("cpu", 7)], [("cpu", 1)], True) == (0, "pods")
    assert f(4, [("cpu", -5)], [("cpu", 1)], True) == (0, "cpu")
    assert f(9, [("cpu", 900)], [("cpu", 100)], True) == (1, "ports")           # ports bind only above 1
    assert f(9, [("cpu", 100)], [("cpu", 100)], True) == (1, "cpu")
    assert f(1, [], [], True) == (1, "pods")
    assert f(2 ** 31 - 1, [("x", 2 ** 62 + 1)], [("x", 2 ** 31)], False) == (2 ** 31 - 1, "pods")
    assert f(2 ** 31 - 1, [("x", 2 ** 62 - 2 ** 31 - 1)], [("x", 2 ** 31)], False) == (2 ** 31 - 2, "x")


def test_the_float_shortcut_is_wrong_somewhere():
    wrong = 0
    for req in (3, 7, 100, 2 ** 20 + 1, 2 ** 43 - 1):
        for q in (1, 2, 109, 2 ** 20, 2 ** 30):
            for base in (2 ** 53, 2 ** 62):
                free = (base // req + q) * req - 1
                wrong += CR.float_divide_truncate(free, req) != free // req
    assert wrong > 0
