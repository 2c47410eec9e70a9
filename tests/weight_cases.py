"""Score plugin weights other than the default profile's: the weight vectors
and the workloads of tests/test_weight_cases.py (CPU: the inputs can tell a
wrong weight from a right one) and tests/test_gpu_weights.py (every kernel
family against the oracle under the same weights).  DESIGN.md §8j.

A vector is (fit, balanced, taint, affinity, image, spread, ipa, hard):
ks_config's weight_* fields in their order, then hard_pod_affinity_weight.
helpers.weight_forms turns one into Scheduler's keyword arguments and
pyoracle.Oracle's tuple.

Every workload is a function of a vector that returns the reference's results
(computed once per (workload, vector) and left unchanged).  The chain
workloads are drivers over the interface of tests/test_gpu_spread.py Pair, so
the same driver feeds libksched beside the reference (GPU) or the reference
alone (OraclePair here)."""
import ctypes as C
import functools
import random

import numpy as np

import pyoracle
from helpers import DEFAULT_VECTOR, res_array, states_np
from ksched import synth
from ksched.objects import (Arena, Container, LabelSelector, Node, NodeSelectorRequirement as Req,
                            NodeSelectorTerm as Term, Pod, PodAffinityTerm, PreferredSchedulingTerm as Pref, Taint,
                            nodes_array, pods_array)

Gi, Mi = 1 << 30, 1 << 20
FIT, BALANCED, TAINT, AFFINITY, IMAGE, SPREAD, IPA, HARD = range(8)

# ------------------------------------------------------------------ vectors
DEFAULT = DEFAULT_VECTOR
PRIME = (3, 7, 2, 5, 11, 13, 17, 4)                  # all distinct: two swapped or defaulted weights change totals
CAP = (10000, 2500, 10000, 5000, 10000, 10000, 10000, 100)  # the cap on operands and key, asymmetric
CAP_ALL = (10000,) * 8                               # the largest key; decisions equal the all-ones profile's
SKEW = (5, 0, 1, 10000, 2, 9, 0, 0)                  # zeros beside the cap; hard 0: no record for required terms
ZERO = (0, 0, 0, 0, 0, 0, 0, 1)                      # every feasible node ties at 0: the lowest slot wins


def one_hot(k):
    return tuple(1 if i == k else 0 for i in range(7)) + (1,)


def scaled(c):
    return tuple(c * v for v in DEFAULT[:7]) + (1,)


VECTORS = {"DEFAULT": DEFAULT, "PRIME": PRIME, "CAP": CAP, "CAP_ALL": CAP_ALL, "SKEW": SKEW, "ZERO": ZERO,
           "SCALED7": scaled(7), "SCALED3333": scaled(3333)}
VECTORS.update({f"ONE_HOT{k}": one_hot(k) for k in range(7)})
SCALES = {"SCALED7": 7, "SCALED3333": 3333}
# the vectors whose (workload, vector) pairs must move a tenth of the placements
DISCRIMINATING = {"PRIME", "CAP", "SKEW"} | {f"ONE_HOT{k}" for k in range(7)}


def replica_vector(fit, balanced, taint, affinity):
    """Replica-run cases: the four static weights, the others at their defaults."""
    return (fit, balanced, taint, affinity) + DEFAULT[4:]


def s_bits(vec):
    """Bit length of the largest static score of a replica run's sort key."""
    return max(1, (100 * sum(vec[:4])).bit_length())


# (fit, balanced, taint, affinity) -> s_bits, as DESIGN.md §8j tabulates them
REPLICA_CASES = {"static0": (replica_vector(0, 0, 0, 0), 1), "static1": (replica_vector(1, 0, 0, 0), 7),
                 "static5": (replica_vector(2, 1, 1, 1), 9), "static6": (replica_vector(2, 2, 1, 1), 10),
                 "PRIME": (PRIME, 11), "CAP_ALL": (CAP_ALL, 22)}
VECTORS.update({k: v for k, (v, _) in REPLICA_CASES.items() if k not in VECTORS})


# ------------------------------------------------ the reference alone as a Pair
def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


class OraclePair:
    """A reference (pyoracle.Oracle, or a composed one of tests/*_reference.py)
    behind the interface of tests/test_gpu_spread.py Pair; the results of every
    schedule call are kept in `res`."""

    def __init__(self, n, ref):
        self.n, self.a, self.o, self.res = n, Arena(), ref, []

    def upsert(self, nodes, slots):
        na, k = nodes_array(nodes, self.a)
        self.o.upsert(na, u32(slots), k)

    def delete(self, slots):
        self.o.delete(u32(slots), len(slots))

    def add(self, pods, slots, sign=1):
        if pods:
            pa, k = pods_array(pods, self.a)
            (self.o.add_pods if sign > 0 else self.o.remove_pods)(pa, u32(slots), k)

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        r = res_array(self.o.schedule(pa, m), m)
        self.res.append(r)
        return r

    def dump_equal(self, pod, what=""):
        pass

    def states_equal(self, what=""):
        pass

    def close(self):
        self.o.close()


def record(x, r):
    """Keep a driver's results on a Pair that has no `res` of its own."""
    if not hasattr(x, "res"):
        x.res = []
    if not isinstance(x, OraclePair):
        x.res.append(r)
    return r


# ------------------------------------------------------------ synth streams
N_S, CAP_S, M_S = 1500, 2048, 600
KINDS = {"hetero": synth.HETERO, "labeled": synth.LABELED, "kwok": synth.KWOK}


def spread(n, cap):
    return (C.c_uint32 * n)(*[i * cap // n for i in range(n)])


@functools.lru_cache(maxsize=None)
def synth_stream(kind_name):
    """1,500 nodes spread over 2,048 slots, a prefill to one half, 600 pods."""
    kind = KINDS[kind_name]
    ns = synth.nodes(kind, N_S, 71)
    slots = spread(N_S, CAP_S)
    ps = synth.pods(kind, M_S, 72)
    pf = synth.prefill(kind, N_S, 71, 73, 0.5)  # names nodes by their index
    pf_slots = (C.c_uint32 * pf.n_pods)(*[slots[pf.slot_ptr[j]] for j in range(pf.n_pods)])
    return dict(cap=CAP_S, n=N_S, nodes=ns.nodes, slots=slots, pods=ps.pods, m=M_S, pf=pf.pods, pf_slots=pf_slots,
                n_pf=pf.n_pods, keep=(ns, ps, pf))


def load(t, w):
    """A stream's nodes and prefill into a Scheduler, an Oracle or a composed reference."""
    if hasattr(t, "upsert_nodes_raw"):
        t.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        if w.get("n_pf"):
            assert t.lib.ks_pods_add(t.ctx, w["pf"], w["pf_slots"], w["n_pf"]) == 0, t.lib.ks_last_error(t.ctx)
    else:
        t.upsert(w["nodes"], w["slots"], w["n"])
        if w.get("n_pf"):
            t.add_pods(w["pf"], w["pf_slots"], w["n_pf"])


def oracle_states(o, cap):
    return states_np(o.L.oracle_node_states, o.o, cap)


def run_reference(w, ref, m=None):
    """(results, node states) of the stream's first m pods on a reference."""
    m = w["m"] if m is None else m
    load(ref, w)
    r = res_array(ref.schedule(w["pods"], m), m)
    st = oracle_states(ref, w["cap"])
    ref.close()
    return r, st


@functools.lru_cache(maxsize=None)
def synth_reference(kind_name, vec):
    w = synth_stream(kind_name)
    return run_reference(w, pyoracle.Oracle(w["cap"], vec))


# ------------------------------------------- the general NodeResourcesFit variants
M_GF = 300  # the composed references score in numpy, pod by pod
GF_CASES = {"most-3-1": 1, "binpack-1-1": 2}  # strategy -> the sweep's GF


def gf_reference_object(name, cap, vec):
    from fit_reference import STRATEGIES, FitReference
    from rtcr_reference import RtcrReference
    from rtcr_workloads import case
    return FitReference(cap, STRATEGIES[name], vec) if name in STRATEGIES else RtcrReference(cap, case(name), vec)


def gf_use(s, name):
    from fit_reference import STRATEGIES
    if name in STRATEGIES:
        kind, wc, wm = STRATEGIES[name]
        s.set_fit_strategy(kind, {"cpu": wc, "memory": wm})
    else:
        import rtcr_workloads
        rtcr_workloads.use(s, name)


@functools.lru_cache(maxsize=None)
def gf_reference(name, vec):
    w = synth_stream("hetero")
    return run_reference(w, gf_reference_object(name, w["cap"], vec), M_GF)


# ------------------------------------------------- the 300-node normaliser cluster
@functools.lru_cache(maxsize=None)
def normaliser_stream():
    """tests/test_gpu_semantics.py test_fix_list_spans_several_groups' cluster:
    a PreferNoSchedule taint on every seventh node; four pods of five carry a
    preferred term no node matches (their guessed NodeAffinity maximum is
    wrong), the fifth one that a quarter of the nodes match."""
    from scenarios import node, pod
    nodes = [node(f"n{i}", cpu=(8 + 8 * (i % 5)) * 1000, mem=(32 << (i % 4)) * Gi,
                  labels={"zone": f"z{i % 3}", "disk": "ssd" if i % 4 == 0 else "hdd"},
                  taints=[Taint("spot", "true", "PreferNoSchedule")] if i % 7 == 0 else [])
             for i in range(300)]
    pods = []
    for j in range(600):
        if j % 5 != 0:
            pref = [Pref(1 + j % 90, Term([Req("gpu", "Exists")]))]
        else:
            pref = [Pref(10, Term([Req("disk", "In", ["ssd"])]))]
        pods.append(pod(f"p{j}", cpu=100 + 37 * (j % 23), mem=(1 + j % 7) * Gi // 4, preferred=pref))
    a = Arena()
    na, n = nodes_array(nodes, a)
    pa, m = pods_array(pods, a)
    return dict(cap=n, n=n, nodes=na, slots=(C.c_uint32 * n)(*range(n)), pods=pa, m=m, flagged=480, keep=a,
                pypods=pods)


@functools.lru_cache(maxsize=None)
def normaliser_reference(vec):
    w = normaliser_stream()
    return run_reference(w, pyoracle.Oracle(w["cap"], vec))


# ------------------------------------------------------- one-pod chain drivers
def soft_taints(rng, nodes, frac=0.3):
    for nd in nodes:
        if rng.random() < frac:
            nd.taints = nd.taints + [Taint("soft", "1", "PreferNoSchedule")]
    return nodes


def spread_stream(x):
    """Non-replica pods with DoNotSchedule and ScheduleAnyway constraints over prefilled nodes."""
    from test_gpu_spread import rand_nodes, rand_pod
    rng = random.Random(101)
    n = x.n
    x.upsert(soft_taints(rng, rand_nodes(rng, n, 5)), list(range(n)))
    pre = [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n // 2)]
    x.add(pre, [rng.randrange(n) for _ in pre])
    for b in range(2):
        record(x, x.schedule([rand_pod(rng, b * 1000 + j, spread_frac=1.0) for j in range(100)], f"spread batch {b}"))
        x.states_equal(f"spread batch {b}")
        x.dump_equal(rand_pod(rng, 99_000 + b, spread_frac=1.0), f"spread dump {b}")


def ipa_stream(x):
    """Preferred affinity / anti-affinity of the incoming pods, and bound pods
    whose required affinity terms match them (hardPodAffinityWeight)."""
    from spread_cases import HOST, ZONE
    from test_gpu_spread import APPS, rand_ipa_pod, rand_nodes
    rng = random.Random(102)
    n = x.n
    x.upsert(rand_nodes(rng, n, 4), list(range(n)))
    pre = []
    for j in range(n // 3):
        p = rand_ipa_pod(rng, 10_000 + j, frac=0.0, spread_frac=0.0)
        if j % 2 == 0:  # an existing pod that requires pods of an app beside it
            p.affinity_terms = [PodAffinityTerm(rng.choice([ZONE, HOST, "rack"]), LabelSelector({"app": rng.choice(APPS)}),
                                                kind="affinity")]
        pre.append(p)
    x.add(pre, [rng.randrange(n) for _ in pre])
    for b in range(2):
        pods = []
        for j in range(80):
            p = rand_ipa_pod(rng, b * 1000 + j, frac=0.0, spread_frac=0.0)
            if j % 4:
                p.affinity_terms = [PodAffinityTerm(rng.choice([ZONE, "rack"]), LabelSelector({"app": rng.choice(APPS)}),
                                                    kind=rng.choice(["preferred-affinity", "preferred-anti-affinity"]),
                                                    weight=rng.randint(1, 100)) for _ in range(rng.randint(1, 2))]
            pods.append(p)
        record(x, x.schedule(pods, f"ipa batch {b}"))
        x.states_equal(f"ipa batch {b}")
        x.dump_equal(rand_ipa_pod(rng, 99_000 + b, frac=1.0, spread_frac=0.0), f"ipa dump {b}")


def image_stream(x):
    """Pods whose images some nodes hold."""
    from test_gpu_spread import IMAGES, rand_res_nodes, rand_res_pod
    rng = random.Random(103)
    n = x.n
    x.upsert(rand_res_nodes(rng, n), list(range(n)))
    pods = []
    for j in range(150):
        p = rand_res_pod(rng, j)
        p.topology_spread = []
        p.containers[0].image = rng.choice(IMAGES)[0]
        pods.append(p)
    record(x, x.schedule(pods, "images"))
    x.states_equal("images")
    x.dump_equal(pods[0], "image dump")


def xfit_stream(x):
    import xfit_workloads
    _, res = xfit_workloads.sweep_stream(x, 71, "small", dumps=False)
    for r in res:
        record(x, r)


def pct_stream(x):
    """percentageOfNodesToScore 30: every pod takes the one-pod chain's window."""
    from test_gpu_spread import rand_nodes, rand_pod
    rng = random.Random(104)
    n = x.n
    x.upsert(rand_nodes(rng, n, 6), list(range(n)))
    pre = [rand_pod(rng, 10_000 + j, spread_frac=0.0) for j in range(n // 2)]
    x.add(pre, [rng.randrange(n) for _ in pre])
    record(x, x.schedule([rand_pod(rng, j, spread_frac=0.3) for j in range(200)], "pct 30"))
    x.states_equal("pct 30")


N_REP = 600


def replica_stream(x):
    """Replicas of two deployments, under the system defaults and under zone
    DoNotSchedule + hostname ScheduleAnyway, on 600 nodes in 4 zones; soft
    taints and a preferred term, so all four static weights count."""
    from test_gpu_replica import replicas
    from test_gpu_spread import rand_nodes
    rng = random.Random(105)
    n = x.n
    x.upsert(soft_taints(rng, rand_nodes(rng, n, 4)), list(range(n)))
    bound = [Pod(f"b{j}", containers=[Container({"cpu": 100 * rng.randrange(1, 20), "memory": 128 * Mi * rng.randrange(1, 16)})],
                 labels={"app": rng.choice(["web", "api", "db"])}) for j in range(n)]
    x.add(bound, [rng.randrange(n) for _ in bound])
    pref = [Pref(20, Term([Req("disk", "In", ["ssd"])]))]
    pods = replicas("web", 250, {"cpu": 250, "memory": 256 * Mi}, "defaults", preferred=pref) + \
        replicas("api", 250, {"cpu": 150, "memory": 512 * Mi}, "dns-host", preferred=pref)
    record(x, x.schedule(pods, "replicas"))
    x.states_equal("replicas")


def fill_stream(x):
    """Nodes fill after 2 to 5 pods: runs end at Fit losses, taken nodes are
    re-scored, the last replicas find no node."""
    from spread_cases import HOST, ZONE
    from test_gpu_replica import replicas
    rng = random.Random(106)
    n = x.n
    nodes = [Node(f"h{i}", {"cpu": rng.choice([2000, 4000, 8000]), "memory": rng.choice([4, 8, 16]) * Gi,
                            "pods": rng.choice([2, 3, 5])}, {HOST: f"h{i}", ZONE: f"z{i % 3}"}) for i in range(n)]
    x.upsert(nodes, list(range(n)))
    r = record(x, x.schedule(replicas("web", 600, {"cpu": 300, "memory": 256 * Mi}), "fill"))
    assert (r["status"] == 0).any() and (r["status"] == 1).any()
    x.states_equal("fill")


# name -> (driver, slots, reference factory (capacity, vector) or None for the oracle, percentage)
def _xfit_ref(cap, vec):
    import xfit_workloads
    from xfit_reference import XfitReference
    return XfitReference(cap, *xfit_workloads.CASES[XFIT_CASE], weights=vec)


def _ba_ref(cap, vec):
    import ba_workloads
    from ba_reference import BaReference
    return BaReference(cap, *ba_workloads.CASES[BA_CASE], weights=vec)


XFIT_CASE, BA_CASE = "most-1-1-gpu3", "default-three"
CHAIN = {"spread": (spread_stream, 300, None, 100), "ipa": (ipa_stream, 300, None, 100),
         "image": (image_stream, 400, None, 100), "xfit": (xfit_stream, 512, _xfit_ref, 100),
         "ba": (xfit_stream, 512, _ba_ref, 100), "pct30": (pct_stream, 1000, None, 30),
         "replica": (replica_stream, N_REP, None, 100), "fill": (fill_stream, 150, None, 100)}


def chain_reference_object(name, vec):
    _, n, make, pct = CHAIN[name]
    return make(n, vec) if make else pyoracle.Oracle(n, vec, percentage=pct)


@functools.lru_cache(maxsize=None)
def chain_reference(name, vec):
    """The reference's results of a chain driver, concatenated."""
    x = OraclePair(CHAIN[name][1], chain_reference_object(name, vec))
    CHAIN[name][0](x)
    x.close()
    return np.concatenate(x.res)


# ------------------------------------------------------------- the registry
def reference(workload, vec):
    """A workload's reference results under a vector, by the workload's name."""
    if workload in KINDS:
        return synth_reference(workload, vec)[0]
    if workload in GF_CASES:
        return gf_reference(workload, vec)[0]
    if workload == "normaliser":
        return normaliser_reference(vec)[0]
    return chain_reference(workload, vec)


WORKLOADS = sorted(KINDS) + sorted(GF_CASES) + ["normaliser"] + sorted(CHAIN)

# the (workload, vector) pairs tests/test_gpu_weights.py runs with a
# discriminating vector: each must move a tenth of the oracle's placements
# (tests/test_weight_cases.py)
PAIRS = [(k, v) for k in ("hetero", "kwok") for v in ("PRIME", "CAP", "SKEW")] + \
    [(g, v) for g in sorted(GF_CASES) for v in ("PRIME", "CAP")] + \
    [(k, v) for k in ("labeled", "normaliser") for v in ("PRIME", "CAP", "SKEW", f"ONE_HOT{TAINT}", f"ONE_HOT{AFFINITY}")] + \
    [("spread", v) for v in ("PRIME", "SKEW", f"ONE_HOT{SPREAD}")] + \
    [("image", v) for v in (f"ONE_HOT{IMAGE}", "PRIME")] + \
    [("xfit", "PRIME"), ("ba", "PRIME"), ("pct30", "PRIME"), ("replica", "PRIME"), ("fill", "PRIME")]


def moved(workload, vec_name):
    """(pods placed elsewhere than under the default weights, pods)."""
    a, b = reference(workload, VECTORS[vec_name]), reference(workload, DEFAULT)
    return int(((a["node_index"] != b["node_index"]) | (a["status"] != b["status"])).sum()), len(a)
