"""The resource-only sweep's shared cpu terms at small shapes.

A resource-only round's sweep list is the round's representatives sorted by
cpu key (req_cpu, nz_cpu), then window index, and the default strategy's
kernels keep a node's cpu terms (BalancedAllocation fraction, LeastAllocated
term, pod-count and cpu fit mask) while the key stays.  ks_debug_counters [9]
counts the list entries whose key equals their predecessor's in the same pod
group: the evaluations that kept them.  Clusters of 1,500 to 2,100 nodes
spread over whole blocks force the shapes with sweep_pairs; every case
compares every result field and every node's state with the oracle, reads
back the geometry it ran and reads the counter:

(a) one cpu key over a whole round, all keys distinct, keys alternating in
    window order: the counter is what the sorted list gives, computed here;
(b) runs of one key across a WL_T = 8 batch boundary and across a pod-group
    boundary (the next group's first pod has the previous group's last key);
(c) keys that differ in one half only: best-effort (0, 100) against 100 m
    (100, 100), a container without a cpu request (200, 300) between
    (200, 200) and (300, 300), memory-only pods (cpu check masked off)
    against cpu-only pods; requests too large for the one-word sort key;
(d) feasibility through the kept mask on the sparse hand-built cluster: pods
    of one cpu key that fail on memory on some nodes, on all nodes, or nowhere,
    with small pods of another key between them in window order;
(e) identical pods inside a run of one key; a batch without identical pods;
    dedup_identical_pods = 0;
(f) topk = 4 (rounds end early, the next list starts where the round stopped),
    2 and 8 nodes per lane, identical kwok nodes;
(g) the general NodeResourcesFit variants on the sorted order.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest

import pyoracle
import test_gpu_fit
import test_gpu_rtcr
from helpers import assert_results_equal, res_array
from ksched import Scheduler, synth
from ksched.objects import Arena, Container, Pod, Toleration, pods_array
from scenarios import FIT
from test_gpu_geometry import (CAP_A, GROUPS, KNPL, LAUNCHES, N_A, PG, SUB, all_states, counters, geometry,
                               spread)
from test_gpu_sweep_batch import BIG, CAP_B, sparse_cluster

pytestmark = pytest.mark.gpu

Gi, Mi = 1 << 30, 1 << 20
T = 8            # WL_T (ksched_dev.hpp)
CPU_SHARED = 9   # ks_debug_counters: list entries that kept their predecessor's cpu terms
DUPS = 7         # identical pods not swept
ROUNDS = 0
MARK_ROUND_START = 2  # ks_batch_marks (include/ksched.h)
NZ_CPU, NZ_MEM = 100, 200 * Mi  # the non-zero defaults of a container without the request

Cluster = namedtuple("Cluster", "cap nodes slots n pf pf_slots kwok keep")


@functools.lru_cache(maxsize=None)
def cluster(kind):
    ns = synth.nodes(kind, N_A, 71)
    slots = spread(N_A, CAP_A)
    pf = synth.prefill(kind, N_A, 71, 72, 0.5)  # names nodes by their index
    pf_slots = (C.c_uint32 * pf.n_pods)(*[slots[pf.slot_ptr[j]] for j in range(pf.n_pods)])
    return Cluster(CAP_A, ns.nodes, slots, N_A, pf, pf_slots, True, ns)


def sparse():
    w = sparse_cluster()
    return Cluster(CAP_B, w["na"], w["slots"], w["n"], None, None, False, w)


# A pod is its containers' (cpu, memory) requests, None for a missing one.
def one(cpu, mem):
    return ((cpu, mem),)


def pod_key(spec):
    """(req_cpu, nz_cpu, req_mem, nz_mem) of a pod: identical pods agree in all
    four, the sweep's cpu key is the first two."""
    return (sum(c or 0 for c, _ in spec), sum(NZ_CPU if c is None else c for c, _ in spec),
            sum(m or 0 for _, m in spec), sum(NZ_MEM if m is None else m for _, m in spec))


def build(specs, kwok):
    # the synthetic clusters' nodes carry kwok's taint, which their pods
    # tolerate (the batch stays resource-only: it tolerates every hard taint)
    tol = [Toleration("kwok.x-k8s.io/node", "Exists", "", "NoSchedule")] if kwok else []
    pods = []
    for i, spec in enumerate(specs):
        cs = [Container({k: v for k, v in (("cpu", c), ("memory", m)) if v is not None}) for c, m in spec]
        pods.append(Pod(f"p{i}", containers=cs, tolerations=list(tol)))
    return pods


def shared_entries(specs, pg, dedup=True, order="sorted"):
    """The counter after one round over `specs`: representatives (the first of
    each class of identical pods) by (cpu key, window index), entries equal to
    their predecessor within a pod group of pg list entries."""
    keys = [pod_key(s) for s in specs]
    reps = [i for i in range(len(keys)) if not dedup or keys.index(keys[i]) == i]
    if order == "sorted":
        reps.sort(key=lambda i: (keys[i][:2], i))
    return sum(1 for k in range(1, len(reps)) if k % pg and keys[reps[k]][:2] == keys[reps[k - 1]][:2]), len(reps)


def run(cl, specs, P, pairs, geom, K=0, npl=4, options=None, what=""):
    """Schedule the pods on the cluster and on the oracle; every result field
    and every node's state agree; the geometry read back is `geom` = (kernel
    nodes per lane, sub, groups, pods per group).  Returns the counters, the
    oracle's results and the first pod of every resolved round."""
    a = Arena()
    pa, m = pods_array(build(specs, cl.kwok), a)
    o = pyoracle.Oracle(cl.cap)
    o.upsert(cl.nodes, cl.slots, cl.n)
    if cl.pf is not None:
        o.add_pods(cl.pf.pods, cl.pf_slots, cl.pf.n_pods)
    want = o.schedule(pa, m)
    states = all_states(o, cl.cap)
    o.close()
    with Scheduler(cl.cap, pods_per_round=P, topk=K, nodes_per_lane=npl,
                   options=dict(options or {}, sweep_pairs=pairs)) as s:
        s.upsert_nodes_raw(cl.nodes, cl.slots, cl.n)
        if cl.pf is not None:
            assert s.lib.ks_pods_add(s.ctx, cl.pf.pods, cl.pf_slots, cl.pf.n_pods) == 0
        b = s.prepare(pa, m)
        s.run(b)
        got = s.results(b, m)
        marks = s.marks(b, m)
        s.free(b)
        assert_results_equal(got, want, m, what)
        assert np.array_equal(all_states(s, cl.cap), states), f"{what}: node state differs"
        g = geometry(s, False)
        assert g[LAUNCHES] > 0 and geometry(s, True)[LAUNCHES] == 0, g
        assert (g[KNPL], g[SUB], g[GROUPS], g[PG]) == geom, (what, g)
        k = counters(s)
    return k, res_array(want, m), [i for i in range(m) if marks[i] & MARK_ROUND_START]


# pods per round, pod groups, pods per group, pods of the last group (test_gpu_sweep_batch.SHAPES)
BY_BATCH = (57, 8, T, 1)             # a group is one batch
BY_GROUP = (57, 3, 2 * T + 3, 19)    # a group is two batches and a part


def run_shape(specs, shape, dedup=True, **kw):
    """One window of pods at a (pods per round, groups, pods per group) shape.
    A round that ends early is followed by one that sweeps the rest of the
    window from where it stopped (a speculated round in between starts past
    the batch and lists nothing), so the counter is the sum of
    shared_entries over the windows the resolved rounds started at; the pods
    swept and skipped confirm the windows.  Returns the counters and the
    first window's count."""
    P, groups, pg, _ = shape
    m = len(specs)
    assert m <= P
    if not dedup:
        kw["options"] = dict(kw.get("options") or {}, dedup_identical_pods=0)
    k, _, starts = run(cluster(synth.HETERO), specs, P, groups * 2, (4, 1, groups, pg), **kw)
    assert starts and starts[0] == 0, starts
    assert k[2] + k[DUPS] == sum(m - s for s in starts), (k, starts)
    want = [shared_entries(specs[s:], pg, dedup)[0] for s in starts]
    assert k[CPU_SHARED] == sum(want), (k, starts, want)
    return k, want[0]


def mems(i):
    return (1 + i) * 16 * Mi


# ---------------------------------------------------------- (a) the counter
@pytest.mark.parametrize("shape", [BY_BATCH, BY_GROUP], ids=["8x8", "3x19"])
def test_one_cpu_key(shape):
    P, groups, pg, _ = shape
    specs = [one(500, mems(i)) for i in range(P)]
    k, first = run_shape(specs, shape, what="one key")
    # the whole window: every entry but the first of each group
    assert first == P - groups and k[CPU_SHARED] >= first and k[DUPS] == 0, k


def test_all_keys_distinct():
    specs = [one(100 + 10 * i, mems(i % 5)) for i in range(57)]
    k, first = run_shape(specs, BY_BATCH, what="distinct keys")
    assert first == 0 and k[CPU_SHARED] == 0 and k[DUPS] == 0, k


def test_keys_alternating_in_window_order():
    specs = [one(250 if i % 2 else 1000, mems(i)) for i in range(57)]
    pg = BY_GROUP[2]
    assert shared_entries(specs, pg, order="window")[0] == 0  # a b a b ...: nothing to keep without the sort
    want, _ = shared_entries(specs, pg)
    assert want == 57 - 3 - 1  # two runs; the change of key falls inside a group
    k, first = run_shape(specs, BY_GROUP, what="alternating keys")
    assert first == want and k[CPU_SHARED] >= want, k


# ------------------------------------- (b) runs across batches and groups
@pytest.mark.parametrize("shape", [BY_BATCH, BY_GROUP], ids=["8x8", "3x19"])
def test_run_crosses_batch_and_group_boundaries(shape):
    P, _, pg, _ = shape
    # sorted: 5 small keys, a run of 12 at list entries 5..16 (across entry 8:
    # the next batch, or with 8 per group the next group; and across 16), then
    # distinct keys up to entry 36, and a run to the end (across 38 = 2 x 19)
    keys = [100 + 10 * i for i in range(5)] + [500] * 12 + [600 + 10 * i for i in range(20)] + [900] * 20
    assert len(keys) == P
    order = [(i * 37) % P for i in range(P)]  # window order: a permutation of the sorted one
    specs = [one(keys[j], mems(j)) for j in order]
    want, n = shared_entries(specs, pg)
    assert n == P and want == sum(1 for e in range(1, P) if e % pg and keys[e] == keys[e - 1])
    k, first = run_shape(specs, shape, what="runs across boundaries")
    assert first == want and k[CPU_SHARED] >= want, k


# ------------------------------------------------------ (c) the key is a pair
def pair_specs():
    specs = []
    for i in range(8):
        m = mems(3 * i)
        specs += [((None, None),) if i == 0 else one(None, m),       # (0, 100): best effort, then memory only
                  one(100, None) if i % 2 else one(100, m),          # (100, 100): cpu only / both
                  ((200, m), (None, m)),                             # (200, 300): a container without a cpu request
                  one(200, m), one(300, m),                          # (200, 200), (300, 300)
                  ((100, None), (None, 2 * m)),                      # (100, 200)
                  one(0, m)]                                         # (0, 0): cpu: "0" is a request
    return specs


@pytest.mark.parametrize("shape", [BY_BATCH, BY_GROUP], ids=["8x8", "3x19"])
def test_key_pairs(shape):
    specs = pair_specs()
    assert len(specs) == 56
    cpu_keys = sorted({pod_key(s)[:2] for s in specs})
    assert cpu_keys == [(0, 0), (0, 100), (100, 100), (100, 200), (200, 200), (200, 300), (300, 300)]
    want, n = shared_entries(specs, shape[2])
    assert n == len(specs) - 3 and want > 0  # (the cpu-only pods of 100 m are one class)
    k, first = run_shape(specs, shape, what="key pairs")
    assert first == want and k[CPU_SHARED] >= want, k


def test_cpu_keys_beyond_one_word():
    # a request of 2^28 millicores or more: the list is ranked by the two key
    # halves instead of one packed word; such pods fit nowhere
    big = 1 << 28
    specs = [one((250, big, 500, big + 1, 250, 1 << 40)[i % 6], mems(i)) for i in range(57)]
    want, n = shared_entries(specs, T)
    assert n == 57 and want > 0
    k, first = run_shape(specs, BY_BATCH, what="wide keys")
    assert first == want and k[CPU_SHARED] >= want, k


# -------------------------------------- (d) feasibility through the kept mask
def test_feasibility_through_the_kept_mask():
    cl = sparse()
    nbig = len(BIG)
    mem_of = sorted(cpu // 1000 * 4 * Gi for _, _, _, cpu in BIG)  # the BIG nodes' memory
    # window order: large pods of one cpu key (they pass cpu on the BIG nodes
    # only) with memory that every, some, one and no BIG node holds, small pods
    # of another key between them
    large = {0: 9 * Gi, 2: mem_of[4], 5: mem_of[-1], 6: mem_of[-1] + Gi, 9: 20 * Gi, 11: mem_of[2] + 1}
    specs = [one(5000, large[j]) if j in large else one(100, Gi // 4 + mems(j)) for j in range(T + T // 2)]
    want, n = shared_entries(specs, 16)
    assert n == len(specs) and want == len(specs) - 2
    k, wr, starts = run(cl, specs, 16, 1, (4, 1, 1, 16), K=64, what="kept mask")
    assert k[CPU_SHARED] == sum(shared_entries(specs[s:], 16)[0] for s in starts) >= want, (k, starts)
    # what the cluster was built for, from the oracle (the results above equal
    # it field by field, feasible and the Fit failure counts among them)
    for j, mem in large.items():
        # at most the BIG nodes that hold the memory when empty (earlier pods of the round took some)
        assert wr["feasible"][j] <= sum(1 for x in mem_of if x >= mem), (j, wr[j])
        assert wr["fail"][j][FIT] == cl.n - wr["feasible"][j], (j, wr[j])
    assert wr["status"][6] == 1 and wr["feasible"][6] == 0 and wr["fail"][6][FIT] == cl.n
    assert wr["feasible"][0] == nbig and wr["feasible"][1] == cl.n
    assert 0 < wr["feasible"][2] < wr["feasible"][9] <= nbig  # memory alone fails some of the nodes cpu passes


# ------------------------------------------ (e) identical pods and no dedup
def dup_specs():
    # a run of one cpu key; a run of identical pods inside it
    specs = [one(100 + 10 * i, mems(i)) for i in range(10)]
    specs += [one(500, mems(i)) for i in range(10)] + [one(500, 24 * Mi)] * 12 + [one(500, mems(20 + i)) for i in range(10)]
    specs += [one(700 + 10 * i, mems(i)) for i in range(15)]
    return specs


def test_identical_pods_inside_a_run():
    specs = dup_specs()
    want, n = shared_entries(specs, T)
    k, first = run_shape(specs, BY_BATCH, what="identical pods in a run")
    assert n == len(specs) - 11 and k[DUPS] >= 11, k
    assert first == want > 0 and k[CPU_SHARED] >= want, k


def test_no_identical_pod():
    specs = [one(100 * (1 + i % 4), mems(i)) for i in range(57)]
    want, n = shared_entries(specs, T)
    assert n == 57
    k, first = run_shape(specs, BY_BATCH, what="no identical pod")
    assert k[DUPS] == 0 and first == want > 0 and k[CPU_SHARED] >= want, k


def test_dedup_switched_off():
    specs = dup_specs()
    want, n = shared_entries(specs, T, dedup=False)
    assert n == len(specs)
    k, first = run_shape(specs, BY_BATCH, dedup=False, what="dedup off")
    assert k[DUPS] == 0 and first == want > 0 and k[CPU_SHARED] >= want, k


# ----------------------------- (f) early round ends, lanes, identical nodes
def stream_specs(m):
    # quantised cpu as pod specs are, memory finer; every seventh pod repeats one
    return [one(500, 64 * Mi) if i % 7 == 3 else one((100, 250, 500, 1000, 2000)[(i * 3) % 5], mems(i % 23)) for i in range(m)]


def test_rounds_end_early():
    P, groups, pg, _ = BY_GROUP
    specs = stream_specs(2 * P + 11)
    k, _, _ = run(cluster(synth.HETERO), specs, P, groups * 2, (4, 1, groups, pg), K=4, what="topk 4")
    assert k[ROUNDS] > -(-len(specs) // P), f"{k[ROUNDS]} rounds for {len(specs)} pods: no round ended early"
    assert k[CPU_SHARED] > 0 and k[DUPS] > 0, k


@pytest.mark.parametrize("npl", [2, 8])
def test_nodes_per_lane(npl):
    P = 57
    specs = stream_specs(P + 20)
    k, _, _ = run(cluster(synth.HETERO), specs, P, 1, (npl, 1, 1, P), npl=npl, what=f"npl {npl}")
    assert k[CPU_SHARED] > 0 and k[DUPS] > 0, k


def test_identical_nodes_tie_everywhere():
    P, groups, pg, _ = BY_BATCH
    specs = stream_specs(2 * P + 5)
    k, _, _ = run(cluster(synth.KWOK), specs, P, groups * 2, (4, 1, groups, pg), what="kwok")
    assert k[CPU_SHARED] > 0 and k[DUPS] > 0, k


# ------------------------------------------- (g) the general Fit variants
def test_most_allocated_on_the_sorted_order():
    k, _ = test_gpu_fit.run_groups("hetero-2x64", "most-3-1", 0, {})
    assert k[CPU_SHARED] > 0 and k[DUPS] > 0, k


def test_requested_to_capacity_ratio_on_the_sorted_order():
    k, _ = test_gpu_rtcr.run_groups("hetero-2x64", "peaked-1-1", 0)
    assert k[CPU_SHARED] > 0 and k[DUPS] > 0, k
