"""Workloads of the NodeResourcesFit strategy tests, shared by the CPU test
that validates the composed reference (tests/test_fit_reference.py: with the
default strategy it must reproduce oracle.schedule on exactly these streams)
and the GPU tests that trust it (tests/test_gpu_fit*.py).  Every reference is
computed once per (workload, strategy) and left unchanged."""
import ctypes as C
import functools
import random

import numpy as np

from fit_reference import DEFAULT, STRATEGIES, FitReference, scores_np
from helpers import assert_results_equal, res_array, states_np
from ksched import _abi, synth
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array

Gi, Mi = 1 << 30, 1 << 20
ALL = dict(STRATEGIES, default=DEFAULT)


def pods_at(arr, start):
    return C.cast(C.cast(arr, C.c_void_p).value + start * C.sizeof(_abi.KsPod), C.POINTER(_abi.KsPod))


def spread(n, cap):
    """n distinct slots spread evenly over cap (tests/test_gpu_geometry.py
    spread: every lane step populated, every wave with holes)."""
    assert cap >= n
    return (C.c_uint32 * n)(*[i * cap // n for i in range(n)])


# ------------------------------------------------------- sweep geometry streams
N_A, CAP_A = 1500, 2048
KINDS = {"hetero": (synth.HETERO, False), "labeled": (synth.LABELED, True)}


@functools.lru_cache(maxsize=None)
def group_stream(kind_name, P):
    """1,500 nodes spread over a capacity of 2,048, a prefill, and a stream of
    2P + P/3 pods (plus a run of identical request-less pods in the first
    round) split mid-round over two calls."""
    kind = KINDS[kind_name][0]
    ns = synth.nodes(kind, N_A, 171)
    slots = spread(N_A, CAP_A)
    pf = synth.prefill(kind, N_A, 171, 172, 0.5)
    pf_slots = (C.c_uint32 * pf.n_pods)(*[slots[pf.slot_ptr[j]] for j in range(pf.n_pods)])
    run = max(3, P // 3)
    head = P // 2 + 1
    m = 2 * P + P // 3 + run
    src = synth.pods(kind, m - run, 173)
    be = synth.besteffort_pods(run)
    arr = (_abi.KsPod * m)()
    for j in range(m):
        arr[j] = src.pods[j] if j < head else be.pods[j - head] if j < head + run else src.pods[j - run]
    return dict(ns=ns, slots=slots, pf=pf, pf_slots=pf_slots, arr=arr, m=m, m1=P + P // 2 + 1, keep=(src, be))


def group_setup(t, w):
    """Load a group_stream's nodes and prefill into a Scheduler or a FitReference."""
    if isinstance(t, FitReference):
        t.upsert(w["ns"].nodes, w["slots"], N_A)
        t.add_pods(w["pf"].pods, w["pf_slots"], w["pf"].n_pods)
    else:
        t.upsert_nodes_raw(w["ns"].nodes, w["slots"], N_A)
        assert t.lib.ks_pods_add(t.ctx, w["pf"].pods, w["pf_slots"], w["pf"].n_pods) == 0


@functools.lru_cache(maxsize=None)
def group_reference(kind_name, P, strategy_name):
    """Results and node states after each of the stream's two calls."""
    w = group_stream(kind_name, P)
    r = FitReference(CAP_A, ALL[strategy_name])
    group_setup(r, w)
    out = []
    for lo, cnt in ((0, w["m1"]), (w["m1"], w["m"] - w["m1"])):
        out.append((r.schedule(pods_at(w["arr"], lo), cnt), r.states()))
    r.close()
    return out


# -------------------------------------------------------------- pile-up stream
N_PILE = 400


@functools.lru_cache(maxsize=None)
def pile_stream():
    """400 nodes whose pod capacity is 1-3 (they fill mid-round), 700 identical
    request-less pods, then 300 identical pods with requests."""
    a = Arena()
    nodes = [Node(f"n{i}", {"cpu": (2 + i % 7) * 1000, "memory": (4 + i % 5) * Gi, "pods": 1 + i % 3})
             for i in range(N_PILE)]
    na, n = nodes_array(nodes, a)
    bare = [Pod(f"be{j}", containers=[Container({})]) for j in range(700)]
    req = [Pod(f"rq{j}", containers=[Container({"cpu": 300, "memory": 512 * Mi})]) for j in range(300)]
    pa, m = pods_array(bare + req, a)
    return dict(arena=a, nodes=na, n=n, slots=synth.slot_array(n), pods=pa, m=m, m1=700)


@functools.lru_cache(maxsize=None)
def pile_reference(strategy_name):
    w = pile_stream()
    r = FitReference(N_PILE, ALL[strategy_name])
    r.upsert(w["nodes"], w["slots"], w["n"])
    out = []
    for lo, cnt in ((0, w["m1"]), (w["m1"], w["m"] - w["m1"])):
        out.append((r.schedule(pods_at(w["pods"], lo), cnt), r.states()))
    r.close()
    return out


# ------------------------------------------------------- heterogeneous stream
N_H, P_H = 2000, 128


@functools.lru_cache(maxsize=None)
def hetero_stream(kind_name="hetero"):
    kind = KINDS[kind_name][0]
    return dict(ns=synth.nodes(kind, N_H, 181), ps=synth.pods(kind, 3 * P_H, 182),
                pf=synth.prefill(kind, N_H, 181, 183, 0.5), m=3 * P_H)


def hetero_setup(t, w):
    if isinstance(t, FitReference):
        t.upsert(w["ns"].nodes, synth.slot_array(N_H), N_H)
        t.add_pods(w["pf"].pods, w["pf"].slot_ptr, w["pf"].n_pods)
    else:
        t.upsert_nodes_raw(w["ns"].nodes, synth.slot_array(N_H), N_H)
        assert t.lib.ks_pods_add(t.ctx, w["pf"].pods, w["pf"].slot_ptr, w["pf"].n_pods) == 0


@functools.lru_cache(maxsize=None)
def hetero_reference(kind_name, strategy_name):
    w = hetero_stream(kind_name)
    r = FitReference(N_H, ALL[strategy_name])
    hetero_setup(r, w)
    out = (r.schedule(w["ps"].pods, w["m"]), r.states())
    r.close()
    return out


def hetero_case(w, want, states, configure):
    """The stream `w` as a two-rank case (tests/chain_multirank_main.py): two calls, each rank configured alike."""
    m = w["m"]

    def setup(s):
        configure(s)
        hetero_setup(s, w)

    return dict(capacity=N_H, pods_per_round=P_H, setup=setup, want=res_array(want, m), states=states,
                batches=[(pods_at(w["ps"].pods, a), b - a) for a, b in ((0, m // 2), (m // 2, m))])


def two_rank_case(cfg):
    kind, wc, wm = STRATEGIES[cfg["strategy_name"]]
    return hetero_case(hetero_stream(cfg["kind_name"]), *hetero_reference(cfg["kind_name"], cfg["strategy_name"]),
                       lambda s: s.set_fit_strategy(kind, {"cpu": wc, "memory": wm}))


# --------------------------------------- the widening label-dictionary batches
@functools.lru_cache(maxsize=None)
def wide_reference(strategy_name):
    """The batches of tests/test_gpu_geometry.py wide_workload (2,100 labelled
    and tainted nodes over a capacity of 4,096; the pods' label programs widen
    the dictionary to 1, 2 and 4 label words) under a strategy: results and
    node states after each batch."""
    from test_gpu_geometry import CAP_B, wide_workload
    w = wide_workload()
    r = FitReference(CAP_B, ALL[strategy_name])
    r.upsert(w["nodes"], w["slots"], w["n"])
    out = [(r.schedule(pa, m), r.states()) for pa, m, _, _ in w["batches"]]
    r.close()
    return out


def states_matrix(rec):
    """helpers.state_array's int64 matrix from a STATE_DT record array."""
    return np.stack([rec[f].astype(np.int64) for f in rec.dtype.names], axis=1)


# --------------------------------------------- one-pod chain and replica runs
class RefPair:
    """The oracle and the composed reference fed the same cache events (the
    interface of tests/test_gpu_spread.py Pair, whose `s` is libksched): what
    the CPU test drives the chain streams through."""

    def __init__(self, n, strategy=DEFAULT):
        import pyoracle
        self.n = n
        self.a = Arena()
        self.s = pyoracle.Oracle(n)
        self.o = FitReference(n, strategy)

    @staticmethod
    def _u32(xs):
        return (C.c_uint32 * max(1, len(xs)))(*xs)

    def upsert(self, nodes, slots):
        na, k = nodes_array(nodes, self.a)
        self.s.upsert(na, self._u32(slots), k)
        self.o.upsert(na, self._u32(slots), k)

    def delete(self, slots):
        self.s.delete(self._u32(slots), len(slots))
        self.o.delete(self._u32(slots), len(slots))

    def add(self, pods, slots, sign=1):
        if not pods:
            return
        pa, k = pods_array(pods, self.a)
        for t in (self.s, self.o):
            (t.add_pods if sign > 0 else t.remove_pods)(pa, self._u32(slots), k)

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        want = self.o.schedule(pa, m)
        got = self.s.schedule(pa, m)
        assert_results_equal(got, want, m, what)
        return res_array(got, m)

    def dump_equal(self, pod, what=""):
        pa, _ = pods_array([pod], self.a)
        g, w = scores_np(self.s.plugin_scores(pa), self.n), self.o.plugin_scores(pa)
        assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])

    def states_equal(self, what=""):
        g = states_np(self.s.L.oracle_node_states, self.s.o, self.n)
        assert np.array_equal(g, self.o.states()), what

    def close(self):
        self.s.close()
        self.o.close()


def chain_stream(x, seed, n):
    """Four batches of 90 pods of the one-pod chain's kinds (topology spread,
    inter-pod affinity, extended resources and images; the generators of
    tests/test_gpu_spread.py) between plain pods, with bound pods removed and
    nodes deleted and re-added between batches, and a score dump per batch."""
    from test_gpu_spread import rand_ipa_pod, rand_pod, rand_res_nodes, rand_res_pod
    rng = random.Random(seed)
    x.upsert(rand_res_nodes(rng, n), list(range(n)))
    pre = [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n // 3)]
    live = [(p, rng.randrange(n)) for p in pre]
    x.add([p for p, _ in live], [s for _, s in live])
    for b in range(4):
        pods = []
        for j in range(30):
            pods += [rand_pod(rng, b * 1000 + 3 * j), rand_ipa_pod(rng, b * 1000 + 3 * j + 1, frac=0.5),
                     rand_res_pod(rng, b * 1000 + 3 * j + 2)]
        x.schedule(pods, f"chain seed {seed} batch {b}")
        x.states_equal(f"chain seed {seed} batch {b}")
        rng.shuffle(live)
        gone, live = live[:5], live[5:]
        x.add([p for p, _ in gone], [s for _, s in gone], sign=-1)
        slots = rng.sample(range(n), 3)
        live = [(p, s) for p, s in live if s not in slots[:2]]  # their pods leave with the deleted nodes
        x.delete(slots[:2])
        x.upsert(rand_res_nodes(rng, 1, slot0=n + 10 * b), [slots[0]])  # one re-added, one stays deleted
        x.upsert(rand_res_nodes(rng, 1, slot0=n + 10 * b + 5), [slots[2]])  # one replaced in place
        live = [(p, s) for p, s in live if s != slots[2]]
        x.dump_equal(rand_pod(rng, 99_000 + b, spread_frac=1.0), f"chain seed {seed} spread dump {b}")
        x.dump_equal(rand_pod(rng, 98_000 + b, spread_frac=0.0), f"chain seed {seed} plain dump {b}")


N_DEP = 600


def deployment_stream(x, variant):
    """300 identical replicas of one deployment under the system-default
    constraints ("defaults") or zone DoNotSchedule ("dns"), over prefilled nodes."""
    from test_gpu_replica import replicas
    from test_gpu_spread import rand_nodes
    rng = random.Random(91)
    x.upsert(rand_nodes(rng, N_DEP, 5), list(range(N_DEP)))
    bound = [Pod(f"b{j}", containers=[Container({"cpu": 100, "memory": 128 * Mi})],
                 labels={"app": rng.choice(["web", "api"])}) for j in range(N_DEP)]
    x.add(bound, [rng.randrange(N_DEP) for _ in bound])
    x.schedule(replicas("web", 300, {"cpu": 250, "memory": 256 * Mi}, variant), f"deployment {variant}")
    x.states_equal(f"deployment {variant}")
