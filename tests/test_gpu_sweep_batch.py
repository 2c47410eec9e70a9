"""The resource-only sweep's batched wave lists at small shapes.

The sweep sets the lanes' two best keys of a pod aside and reduces the wave
lists of WL_T = 8 pods together, a lane folding one pod's keys of 8 lanes.
Clusters of 1,500 to 2,100 nodes spread over a capacity of whole blocks force
the shapes with sweep_pairs, every case reads back what it ran
(ks_debug_sweep_geometry) and compares every result field and every node's
state with the oracle:

(a) pods per group of 1, T - 1, T, T + 1 and 2T + 3 and last groups of 1: a
    partial batch, an exact one, a batch step that runs once, twice or three
    times; each stream's first round holds a run of identical request-less
    pods, so the dedup list ends inside a batch, and topk = 4 starts rounds
    mid-batch;
(b) a hand-built cluster where most nodes are too small for the large pods:
    waves with 0, 1 and 2 feasible nodes for some pods of a batch and plenty
    for the others, the two best nodes of the large pods in one lane (slots
    l and l + 64 x layout waves) and the third elsewhere in the wave; a
    large pod's round record lists exactly the highest keys with a covering
    bound;
(c) identical kwok nodes: every score ties and only positions order the keys;
(d) 2 and 8 nodes per lane;
(e) the general NodeResourcesFit variants (MostAllocated, RequestedToCapacityRatio).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
import test_gpu_fit
import test_gpu_rtcr
from helpers import assert_results_equal, assert_round_records, oracle_keys, res_array
from ksched import Scheduler, synth
from ksched.objects import Arena, nodes_array, pods_array
from scenarios import FIT, node, pod
from test_gpu_geometry import (BLOCKS, CAP_A, GROUPS, KNPL, LAUNCHES, N_A, PG, SUB, all_states, counters, geometry,
                               group_workload, pods_at, run_groups, spread)

pytestmark = pytest.mark.gpu

Gi = 1 << 30
T = 8  # WL_T (ksched_dev.hpp)

# ---------------------------------------------------- (a) pods per group vs T
# pods per round, pod groups, pods per group, pods of the last group
SHAPES = [(57, 57, 1, 1), (43, 7, T - 1, 1), (57, 8, T, 1), (73, 9, T + 1, 1), (57, 3, 2 * T + 3, 2 * T + 3)]


@pytest.mark.parametrize("K", ["P", 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: f"P{t[0]}-{t[1]}x{t[2]}")
def test_pods_per_group_around_a_batch(shape, K):
    P = shape[0]
    k, m = run_groups("hetero", shape, P if K == "P" else K, {})
    assert k[7] > 0, f"no identical pod was skipped: the dedup list ended in no batch {k}"
    if K == 4:
        assert k[0] > -(-m // P), f"{k[0]} rounds for {m} pods: no round ended early"


# ------------------------------- (b) few feasible nodes, two best in one lane
CAP_B, WAVES_B = 2048, 8  # 4 nodes per lane: 8 layout waves, 2 blocks
N_SMALL = 1600
LANE_B = 5  # the lane that holds both best nodes of layout wave 3
LARGE = (0, 6, 9)  # the pods that fit the BIG nodes only


def slot_of(wave, lane, step):
    return step * 64 * WAVES_B + lane * WAVES_B + wave


# the nodes the large pods fit on: (layout wave, lane, step, cpu); wave 0 none,
# wave 1 one, wave 2 two; wave 3 its two largest in one lane and a third
# elsewhere; waves 4..7 (the other block) one each in wave 4 and 6
BIG = [(1, 9, 2, 48000), (2, 3, 0, 40000), (2, 40, 3, 44000),
       (3, LANE_B, 0, 64000), (3, LANE_B, 1, 60000), (3, 33, 2, 56000), (3, 12, 3, 36000),
       (4, 63, 1, 52000), (6, 0, 3, 34000)]


@functools.lru_cache(maxsize=None)
def sparse_cluster():
    big = {slot_of(w, l, st): cpu for w, l, st, cpu in BIG}
    assert len(big) == len(BIG)
    small = [sl for sl in (int(x) for x in spread(N_SMALL, CAP_B)) if sl not in big]
    nodes, slots = [], []
    for i, sl in enumerate(small):
        nodes.append(node(f"s{i}", cpu=2000 + 500 * (i % 3), mem=(8 + 4 * (i % 4)) * Gi, pods=110))
        slots.append(sl)
    for sl, cpu in sorted(big.items()):
        nodes.append(node(f"b{sl}", cpu=cpu, mem=cpu // 1000 * 4 * Gi, pods=110))
        slots.append(sl)
    # a batch and a half: large pods (the BIG nodes only), small ones (every
    # node), a very large one (five of the BIG nodes) and one that fits
    # nowhere, in one batch
    pods = []
    for j in range(T + T // 2):
        cpu, mem = (5000 + 100 * j, 9 * Gi) if j in LARGE else (100 + 10 * j, Gi // 4)
        if j == 3:
            cpu, mem = 47000, 30 * Gi
        if j == 7:
            cpu = 10 ** 6
        pods.append(pod(f"p{j}", cpu=cpu, mem=mem))
    a = Arena()
    na, n = nodes_array(nodes, a)
    pa, m = pods_array(pods, a)
    return dict(arena=a, na=na, n=n, slots=(C.c_uint32 * n)(*slots), pa=pa, m=m, big=big)


def test_few_feasible_nodes_and_two_best_in_one_lane():
    w = sparse_cluster()
    n, m, K = w["n"], w["m"], 64
    o = pyoracle.Oracle(CAP_B)
    o.upsert(w["na"], w["slots"], n)
    keys = [oracle_keys(o, pods_at(w["pa"].contents, i)) for i in range(m)]  # round-start state
    want = o.schedule(w["pa"], m)
    wr = res_array(want, m)
    # what the cluster was built for, from the oracle: the large pods' feasible
    # nodes are the BIG ones (1 and 2 in layout waves 1 and 2, none in 0), and
    # their two highest keys are the two nodes of one lane, the third in the
    # same wave elsewhere
    top_slots = lambda i, c: [0xFFFFFFFF - (int(x) & 0xFFFFFFFF) for x in keys[i][0][:c]]  # noqa: E731
    for i in LARGE:
        assert keys[i][1] == len(BIG) and wr["fail"][i][FIT] == n - len(BIG), (i, keys[i][1])
        assert sorted(top_slots(i, len(BIG))) == sorted(w["big"])
        wave3 = [sl for sl in top_slots(i, len(BIG)) if sl % WAVES_B == 3]
        assert wave3[:3] == [slot_of(3, LANE_B, 0), slot_of(3, LANE_B, 1), slot_of(3, 33, 2)], wave3
        assert top_slots(i, 2) == wave3[:2]  # the pod's two best nodes overall
    assert keys[1][1] == n and keys[7][1] == 0 and wr["status"][7] == 1
    assert keys[3][1] == 5
    with Scheduler(CAP_B, pods_per_round=16, topk=K, options={"sweep_pairs": 1}) as s:
        s.upsert_nodes_raw(w["na"], w["slots"], n)
        got = s.schedule_raw(w["pa"], m)
        assert_results_equal(got, want, m, "sparse cluster")  # feasible and Fit-failure counts per pod among them
        assert np.array_equal(all_states(s, CAP_B), all_states(o, CAP_B)), "node state differs"
        g = geometry(s, False)
        assert g[LAUNCHES] > 0 and (g[KNPL], g[SUB], g[BLOCKS], g[GROUPS], g[PG]) == (4, 1, 2, 1, 16), g
    # the round record of a large pod (the records read back are the last
    # round's, so a batch that one round resolves: the pod alone): exactly the
    # highest keys and a bound at least every unlisted key
    with Scheduler(CAP_B, pods_per_round=16, topk=K, options={"sweep_pairs": 1}) as s:
        s.upsert_nodes_raw(w["na"], w["slots"], n)
        got = s.schedule_raw(w["pa"], 1)
        r = res_array(got, 1)
        assert np.array_equal(r, wr[:1]), (r, wr[:1])
        assert counters(s)[0] == 1 and geometry(s, False)[LAUNCHES] == 1
        # (the lane's second best is the wave's largest second, so the wave
        # lists its best key alone and bounds the rest by the second)
        listed = assert_round_records(s, keys, r, 1, K)
        assert listed >= 1, listed
    o.close()


# ---------------------------------------------------- (c) identical kwok nodes
def test_identical_nodes_tie_everywhere():
    P, groups, pg = 57, 8, T
    ns = synth.nodes(synth.KWOK, N_A, 91)
    ps = synth.pods(synth.KWOK, 2 * P + 5, 92)
    slots = spread(N_A, CAP_A)
    o = pyoracle.Oracle(CAP_A)
    o.upsert(ns.nodes, slots, N_A)
    want = o.schedule(ps.pods, ps.n_pods)
    with Scheduler(CAP_A, pods_per_round=P, options={"sweep_pairs": groups * 2}) as s:
        s.upsert_nodes_raw(ns.nodes, slots, N_A)
        got = s.schedule_raw(ps.pods, ps.n_pods)
        assert_results_equal(got, want, ps.n_pods, "kwok")
        assert np.array_equal(all_states(s, CAP_A), all_states(o, CAP_A)), "node state differs"
        g = geometry(s, False)
        assert g[LAUNCHES] > 0 and (g[KNPL], g[BLOCKS], g[GROUPS], g[PG]) == (4, 2, groups, pg), g
    o.close()


# ------------------------------------------------------- (d) nodes per lane
@pytest.mark.parametrize("npl", [2, 8])
def test_resource_only_lanes(npl):
    P = 57
    w = group_workload("hetero", P)
    with Scheduler(CAP_A, pods_per_round=P, nodes_per_lane=npl, options={"sweep_pairs": 1}) as s:
        s.upsert_nodes_raw(w["ns"].nodes, w["slots"], N_A)
        assert s.lib.ks_pods_add(s.ctx, w["pf"].pods, w["pf_slots"], w["pf"].n_pods) == 0
        m, m1 = w["m"], w["m1"]
        for call, (lo, cnt) in enumerate([(0, m1), (m1, m - m1)]):
            got = s.schedule_raw(pods_at(w["arr"], lo), cnt)
            assert_results_equal(got, w["want"][call], cnt, f"npl {npl} call {call}")
            assert np.array_equal(all_states(s, CAP_A), w["states"][call]), f"npl {npl} call {call}: node state differs"
            g = geometry(s, False)
            assert g[LAUNCHES] > 0 and (g[KNPL], g[SUB], g[GROUPS], g[PG]) == (npl, 1, 1, P), g


# ------------------------------------------- (e) the general Fit variants
def test_most_allocated_groups():
    # 64 pods per group (8 whole batches) and a last group of one pod
    k, _ = test_gpu_fit.run_groups("hetero-2x64", "most-3-1", 0, {})
    assert k[7] > 0, k


def test_requested_to_capacity_ratio_groups():
    k, _ = test_gpu_rtcr.run_groups("hetero-2x64", "peaked-1-1", 0)
    assert k[7] > 0, k
