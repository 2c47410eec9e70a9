"""The resource-only sweep's fetch-ahead at small shapes.

The sweep loads a pod group's list entries with one vector load (lane l the
entry of the group's pod l), takes a pod's entry by v_readlane, and requests
pod q + 1's descriptor before pod q's arithmetic; the default strategy's body
clamps a BalancedAllocation fraction to 1 only for a zero request.  Every pod
of a case has its own cpu and its own memory request, in a window order that
is not the sorted one, so a descriptor used one pod early or late changes a
score or a placement.  Every case compares every result field and every
node's state with the oracle and reads back the geometry it ran:

(a) pod groups of 1, 2, 8, 9 and 16 pods (a batch without a next pod, a full
    batch, a second batch of one), a last group of one pod, a batch whose last
    pod is the last element of the pods array;
(b) a round whose list is shorter than the window (identical pods), its tail
    left over from a longer round of the same context; dedup switched off;
(c) second and third rounds of a batch (the window starts past 0);
(d) zero-request pods among pods with requests on a cluster with a node whose
    Requested memory exceeds its Allocatable and one with the same for cpu:
    with BalancedAllocation alone weighted, the clamp decides where they go;
(e) 2 and 8 nodes per lane; MostAllocated and RequestedToCapacityRatio.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
import test_gpu_fit
import test_gpu_rtcr
from helpers import assert_results_equal, oracle_weights, res_array
from ksched import Scheduler, synth
from ksched.objects import Arena, nodes_array, pods_array
from scenarios import node, pod
from test_gpu_geometry import CAP_A, GROUPS, KNPL, LAUNCHES, PG, SUB, all_states, counters, geometry, spread
from test_gpu_sweep_share import DUPS, ROUNDS, Cluster, build, cluster, one

pytestmark = pytest.mark.gpu

Gi, Mi = 1 << 30, 1 << 20
BLOCKS = 2  # the clusters here: 2,048 slots at 4 nodes per lane


def distinct(m, seed=0):
    """m pods, each with its own cpu and its own memory request; window order
    is a permutation of the cpu order the sweep walks, and neighbours in that
    order are far apart in memory (small and large in turn), so a pod scored
    with its neighbour's descriptor lands elsewhere."""
    step = next(s for s in (37, 41, 43, 47, 53) if m % s)
    return [one(100 + 10 * j, (1 + (j + seed) % 2 * 150 + j) * 8 * Mi) for j in ((i * step + seed) % m for i in range(m))]


def run_batches(cl, batches, P, pairs, geom, K=0, npl=4, options=None, weights=None, bound=None, what=""):
    """Schedule the batches in turn on one context and on the oracle; every
    result field of every batch and every node's state agree, and the
    geometry read back is `geom` = (kernel nodes per lane, sub, groups, pods
    per group).  bound: pods bound to nodes before (pods array, slots, count).
    Returns the counters and the oracle's results per batch."""
    a = Arena()
    arrays = [pods_array(build(specs, cl.kwok), a) for specs in batches]
    o = pyoracle.Oracle(cl.cap, weights=oracle_weights(weights)) if weights else pyoracle.Oracle(cl.cap)
    o.upsert(cl.nodes, cl.slots, cl.n)
    if cl.pf is not None:
        o.add_pods(cl.pf.pods, cl.pf_slots, cl.pf.n_pods)
    if bound:
        o.add_pods(*bound)
    wants = [o.schedule(pa, m) for pa, m in arrays]
    states = all_states(o, cl.cap)
    o.close()
    kw = dict(weights=weights) if weights else {}
    with Scheduler(cl.cap, pods_per_round=P, topk=K, nodes_per_lane=npl,
                   options=dict(options or {}, sweep_pairs=pairs), **kw) as s:
        s.upsert_nodes_raw(cl.nodes, cl.slots, cl.n)
        if cl.pf is not None:
            assert s.lib.ks_pods_add(s.ctx, cl.pf.pods, cl.pf_slots, cl.pf.n_pods) == 0
        if bound:
            assert s.lib.ks_pods_add(s.ctx, *bound) == 0, s.lib.ks_last_error(s.ctx)
        for i, ((pa, m), want) in enumerate(zip(arrays, wants)):
            b = s.prepare(pa, m)  # exactly m pods: the batch's last pod ends the pods array
            s.run(b)
            got = s.results(b, m)
            s.free(b)
            assert_results_equal(got, want, m, f"{what}, batch {i}")
        assert np.array_equal(all_states(s, cl.cap), states), f"{what}: node state differs"
        g = geometry(s, False)
        assert g[LAUNCHES] > 0 and geometry(s, True)[LAUNCHES] == 0, g
        assert (g[KNPL], g[SUB], g[GROUPS], g[PG]) == geom, (what, g)
        k = counters(s)
    return k, [res_array(w, m) for w, (_, m) in zip(wants, arrays)]


def shape(P, groups):
    """sweep_pairs and the geometry of `groups` pod groups over a window of P."""
    pg = -(-P // groups)
    assert -(-P // pg) == groups
    return groups * BLOCKS, (4, 1, groups, pg)


# ------------------------------------------------- (a) group and batch sizes
# pods per round, pod groups -> pods per group, pods of the last group
@pytest.mark.parametrize("P,groups,pg,last", [(5, 5, 1, 1), (5, 3, 2, 1), (16, 2, 8, 8), (57, 8, 8, 1),
                                              (18, 2, 9, 9), (73, 9, 9, 1), (32, 2, 16, 16), (33, 3, 11, 11)],
                         ids=["5x1", "2+2+1", "2x8", "7x8+1", "2x9", "8x9+1", "2x16", "3x11"])
def test_group_sizes(P, groups, pg, last):
    pairs, geom = shape(P, groups)
    assert geom[3] == pg and P - (groups - 1) * pg == last
    # one window exactly: the last group's last pod is the last element of the pods array
    k, (wr,) = run_batches(cluster(synth.HETERO), [distinct(P)], P, pairs, geom, what=f"{groups} groups of {pg}")
    assert k[DUPS] == 0 and (wr["status"] == 0).any(), k


# --------------------------------------- (b) a list shorter than the window
def short_list_batches(P):
    long = distinct(2 * P + 3)  # rounds with full lists (both list buffers)
    same = one(300, 40 * Mi)
    # identical pods spread over the window: P // 3 representatives and change
    short = [same if i % 3 else s for i, s in enumerate(distinct(P - 5, seed=5))]
    return [long, short]


@pytest.mark.parametrize("groups", [8, 3], ids=["8x8", "3x19"])
def test_list_shorter_than_the_window_after_a_longer_round(groups):
    P = 57
    pairs, geom = shape(P, groups)
    batches = short_list_batches(P)
    k, _ = run_batches(cluster(synth.HETERO), batches, P, pairs, geom, what="short list")
    assert k[DUPS] >= sum(1 for i in range(len(batches[1])) if i % 3) - 1, k


def test_dedup_switched_off():
    P = 57
    pairs, geom = shape(P, 8)
    k, _ = run_batches(cluster(synth.HETERO), short_list_batches(P), P, pairs, geom,
                       options=dict(dedup_identical_pods=0), what="dedup off")
    assert k[DUPS] == 0, k


# ------------------------------------------ (c) windows that start past zero
@pytest.mark.parametrize("groups", [8, 3], ids=["8x8", "3x19"])
def test_later_rounds_of_a_batch(groups):
    P = 57
    pairs, geom = shape(P, groups)
    m = 3 * P + 1  # a fourth window of one pod: a last group of one, a batch of one
    k, _ = run_batches(cluster(synth.HETERO), [distinct(m)], P, pairs, geom, K=4, what="later rounds")
    assert k[ROUNDS] > 4, f"{k[ROUNDS]} rounds for {m} pods: no round ended early"


# --------------------------------------------- (d) the clamp and zero requests
@functools.lru_cache(maxsize=None)
def overcommitted():
    """1,500 nodes, half of them part filled, and two at the lowest slots
    whose bound pods ask for more than the node has: slot 0 twice its memory
    (and all of its cpu), slot 1 one and a half times its cpu (and all of its
    memory).  Slot 0 has room for one pod more, slot 1 for many."""
    n = 1500
    sl = [int(x) for x in spread(n, CAP_A)]
    assert sl[0] == 0 and sl[1] == 1
    nodes = [node("over-mem", cpu=4000, mem=8 * Gi, pods=2), node("over-cpu", cpu=4000, mem=8 * Gi, pods=110)]
    nodes += [node(f"s{i}", cpu=2000 + 500 * (i % 5), mem=(4 + 2 * (i % 7)) * Gi, pods=110) for i in range(2, n)]
    bound = [pod("b0", cpu=4000, mem=16 * Gi), pod("b1", cpu=6000, mem=8 * Gi)]
    where = [0, 1]
    for i in range(2, n, 2):  # every ordinary node holds something or nothing, none is balanced at 1
        bound.append(pod(f"b{i}", cpu=100 + 50 * (i % 9), mem=(1 + i % 5) * 256 * Mi))
        where.append(sl[i])
    a = Arena()
    na, nn = nodes_array(nodes, a)
    ba, nb = pods_array(bound, a)
    cl = Cluster(CAP_A, na, (C.c_uint32 * n)(*sl), nn, None, None, False, a)
    return cl, (ba, (C.c_uint32 * nb)(*where), nb)


def test_zero_request_pods_meet_overcommitted_nodes():
    cl, bound = overcommitted()
    P = 16
    pairs, geom = shape(P, 2)
    specs = distinct(P)
    be, zero = 3, 12  # a best-effort pod (no requests at all) and one that requests "0" of both
    specs[be] = ((None, None),)
    specs[zero] = one(0, 0)
    # BalancedAllocation alone decides: both fractions of the two nodes clamp
    # to 1, a score of 100, and the lowest slot wins the tie with empty nodes
    w = {"NodeResourcesFit": 0, "NodeResourcesBalancedAllocation": 1}
    k, (wr,) = run_batches(cl, [specs], P, pairs, geom, weights=w, bound=bound, what="overcommitted nodes")
    first, second = sorted((be, zero))
    # what the cluster was built for, from the oracle (the results above equal it)
    assert wr["node_index"][first] == 0 and wr["node_index"][second] == 1, (wr[be], wr[zero])
    assert wr["feasible"][be] == cl.n and wr["feasible"][zero] == cl.n - 1
    others = [j for j in range(P) if j not in (be, zero)]
    assert (wr["status"][others] == 0).all() and not np.isin(wr["node_index"][others], (0, 1)).any()
    assert (wr["feasible"][others] <= cl.n - 2).all()  # Fit fails on both nodes for every pod with a request


# ------------------------------------------- (e) lanes and the other strategies
@pytest.mark.parametrize("npl", [2, 8])
def test_nodes_per_lane(npl):
    P = 57
    k, _ = run_batches(cluster(synth.HETERO), [distinct(P + 9)], P, 1, (npl, 1, 1, P), npl=npl, what=f"npl {npl}")
    assert k[DUPS] == 0, k


def test_most_allocated():
    test_gpu_fit.run_groups("hetero-2x64", "most-3-1", 0, {})


def test_requested_to_capacity_ratio():
    test_gpu_rtcr.run_groups("hetero-2x64", "peaked-1-1", 0)
