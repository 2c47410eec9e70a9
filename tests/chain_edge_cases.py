"""Workloads that enter the one-pod chain's domain-table, prefetch and
renumbering edges, with answers known by construction.  Plain
Python over Node / Pod objects: tests/test_oracle_chain_edges.py runs them on
the CPU oracle, tests/test_gpu_chain_edges.py on the device next to it.

The constants restate ksched_spread_dev.hpp, ksched_kernels.hpp and
ksched_host.cpp (spread_scratch, spread_nodes_changed).  A topology key's id
count is its distinct non-empty values issued since its column was built,
plus 1 (id 0 is the value ""); ids are issued in slot order when the column is
built and in upsert order after it.

A case is a dict: nodes, bound [(pod, slot)], pods (one batch), exp (as
scenarios.check) and dumps {pod index: {ks_node_score field: [per node]}} of
that pod against the cache before the batch.  The streams drive a target `x`
with upsert(nodes, slots), add(pods, slots), schedule(pods, what) -> results
and dump_equal(pod, what) -> per-node scores (test_gpu_spread.Pair, or the
oracle alone)."""
import math

from ksched.objects import (Container, LabelSelector, Node, Pod, PodAffinityTerm as T,
                            TopologySpreadConstraint as TSC)
from scenarios import POD_AFFINITY, SPREAD, check

Gi, Mi = 1 << 30, 1 << 20
ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"
WEB = LabelSelector({"app": "web"})
DNS, ANYWAY = "DoNotSchedule", "ScheduleAnyway"

SP_LDS = 4096       # LDS domain-histogram entries per block, first fit in record order
SP_LDS_DOM = 1024   # a key with more ids than this aggregates by global atomics
SP_PF = AF_PF = 4   # constraints / records whose loads are prefetched
SCRATCH_MIN = 1024  # entries per constraint of the domain scratch at first
RK_DZ_NONE = 2047   # a replica run takes a non-hostname key of at most this many ids
RUN_GROUPS = 512    # ... and at most this many (domain, hostname count) groups of candidates


def renumber_above(cap):
    """spread_nodes_changed rebuilds a key's column once its id count passes this."""
    return 2 * cap + 1024


def node(i, labels, name=None):
    lab = {HOST: name or f"n{i}"}
    lab.update(labels)
    return Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 110}, lab)


def pod(name, labels=None, spread=None, terms=None, **kw):
    return Pod(name, containers=[Container({"cpu": 100, "memory": 100 * Mi})],
               labels=dict(labels if labels is not None else {"app": "web"}), topology_spread=list(spread or []),
               affinity_terms=list(terms or []), **kw)


def run_case(x, case, what="", before=None):
    """Feed a case to the target; check its dumps and expectations; the results.
    before(x): what else to ask about the cache the batch meets."""
    n = len(case["nodes"])
    x.upsert(case["nodes"], list(range(n)))
    x.add([p for p, _ in case["bound"]], [s for _, s in case["bound"]])
    for j, fields in case["dumps"].items():
        out = x.dump_equal(case["pods"][j], f"{what} dump {j}")
        for f, want in fields.items():
            got = [getattr(out[i], f) for i in range(n)]
            assert got == want, (what, j, f, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
    if before:
        before(x)
    r = x.schedule(case["pods"], what)
    check(r, case["exp"])
    return r


# ------------------------------------------------------------ 1. wide key, last domain

WIDE_D = [1022, 1023, 1024, 1025]  # id counts 1023 .. 1026: LDS up to 1024, then global atomics and a grown scratch
WIDE_VARIANTS = ["dns", "anyway", "anti"]
WIDE_REASON = "node(s) didn't match pod topology spread constraints"


def wide_key(D, variant):
    """D cells on D + 37 nodes (cells 0-36 hold two); one web pod on each of
    slots 0 .. D-2, so cell D-1 -- the last id issued, the table's last entry
    -- is the only one without."""
    n = D + 37
    nodes = [node(i, {"cell": f"c{i % D}"}) for i in range(n)]
    bound = [(pod(f"b{i}"), i) for i in range(D - 1)]
    last = [i for i in range(n) if i % D == D - 1]
    assert last == [D - 1]
    if variant == "dns":
        c = [TSC(1, "cell", DNS, WEB)]
        pods = [pod("p0", spread=c), pod("p1", spread=c)]
        # p0: global minimum 0 (cell D-1), every other cell 1 + 1 - 0 > 1; p1: every cell 1, minimum 1: all
        # feasible, no spread score; slots D .. D+36 hold no pod, the lowest of them wins
        exp = [dict(node=D - 1, feasible=1, fails={SPREAD: n - 1}), dict(node=D, feasible=n)]
        dumps = {}
    elif variant == "anyway":
        c = [TSC(1, "cell", ANYWAY, WEB)]
        pods = [pod("p0", spread=c), pod("p1", spread=c)]
        w = math.log(D + 2)  # D cells among the filtered nodes; maxSkew - 1 = 0
        raw = [0 if i % D == D - 1 else round(1 * w + 0) for i in range(n)]
        assert max(raw) == 7
        score = [100 * (7 + 0 - r) // 7 for r in raw]  # 100 on slot D-1, else 0
        exp = [dict(node=D - 1, feasible=n), dict(node=D, feasible=n)]  # p1: every cell 1, equal spread scores
        dumps = {0: {"spread_raw": raw, "spread_score": score}}
    else:
        t = [T("cell", WEB, kind="preferred-anti-affinity", weight=10)]
        pods = [pod("p0", terms=t), pod("p1", terms=t)]
        raw = [0 if i % D == D - 1 else -10 for i in range(n)]
        score = [100 * (r + 10) // 10 for r in raw]
        # p1: its term counts -10 in every cell, p0's term (it selects p1) another -10 in cell D-1
        exp = [dict(node=D - 1, feasible=n), dict(node=D, feasible=n)]
        dumps = {0: {"affinity_pod_raw": raw, "affinity_pod_score": score}}
    return dict(nodes=nodes, bound=bound, pods=pods, exp=exp, dumps=dumps, ids={"cell": D + 1})


# ------------------------------------------------------------ 2. the LDS budget

BUDGET_N = 1100
BUDGET_MUL = [(1, 0), (3, 17), (7, 29), (9, 41), (11, 53)]  # k0 .. k4: (a i + b) % 1000, a coprime to 1000
BUDGET_IDS = {"k0": 1001, "k1": 1001, "k2": 1001, "k3": 1001, "k4": 1001, "k5": 92, "k5b": 93, ZONE: 9}
GROUPS = 8
ALL_G = {f"g{j}": "y" for j in range(GROUPS)}


def G(j):
    return LabelSelector({f"g{j}": "y"})


def budget_cluster():
    nodes = []
    for i in range(BUDGET_N):
        lab = {f"k{j}": f"v{(a * i + b) % 1000}" for j, (a, b) in enumerate(BUDGET_MUL)}
        lab.update({"k5": f"v{i % 91}", "k5b": f"v{i % 92}", ZONE: f"z{i % 8}"})
        nodes.append(node(i, lab))
    # a dozen pods per selector at fixed slots; three carry a required anti-affinity term that selects role=edge
    bound = [(pod(f"b{j}-{q}", {f"g{j}": "y"}), (89 * q + 131 * j + 5) % BUDGET_N) for j in range(GROUPS)
             for q in range(12)]
    edge = LabelSelector({"role": "edge"})
    bound += [(pod(f"guard{q}", {"app": "guard"}, terms=[T("k5", edge, kind="anti-affinity")]), 300 * q + 7)
              for q in range(3)]
    return nodes, bound


def budget_pods():
    """Four keys of 1001 ids fill 4004 LDS entries; the fifth spills to global
    atomics; then 92 ids fit exactly (4096) and 93 do not."""
    five = [TSC(1, f"k{j}", DNS, G(j)) for j in range(5)]
    a = five + [TSC(1, "k5", DNS, G(5))]
    b = five + [TSC(1, "k5b", DNS, G(5))]
    c = list(reversed(a))
    d = five[:4] + [TSC(1, "k4", ANYWAY, G(4)), TSC(1, "k5", ANYWAY, G(5))]
    e_terms = [T("k3", G(3), kind="anti-affinity"), T("k4", G(4), kind="preferred-anti-affinity", weight=5),
               T("k5", G(5), kind="preferred-affinity", weight=7), T(ZONE, G(0), kind="affinity"),
               T(HOST, G(1), kind="anti-affinity"), T("k4", G(2), kind="preferred-affinity", weight=3)]
    f = a + [TSC(2, ZONE, DNS, G(6)), TSC(1, ZONE, ANYWAY, G(7))]
    assert len(f) == 8  # MAX_SPREAD
    lab = dict(ALL_G, role="edge")
    return {"a": pod("pa", lab, a), "b": pod("pb", lab, b), "c": pod("pc", lab, c), "d": pod("pd", lab, d),
            "e": pod("pe", lab, five[:3], e_terms), "f": pod("pf", lab, f)}


def lds_split(ids):
    """lds_segments over the id counts of a pod's records in order: which take LDS."""
    o, out = 0, []
    for nd in ids:
        small = nd <= SP_LDS_DOM and o + nd <= SP_LDS
        out.append(small)
        o += nd if small else 0
    return out


# what the issue's packing rests on
assert lds_split([1001] * 5 + [92]) == [True] * 4 + [False, True]
assert lds_split([1001] * 5 + [93]) == [True] * 4 + [False, False]
assert lds_split([92] + [1001] * 5) == [True] * 5 + [False]  # reversed: 92 + 4 x 1001 = 4096, k0 spills instead


# ------------------------------------------------------------ 3. beyond the prefetch width

PF_N = 130  # crosses the 64- and 128-thread wave edges
PF_UNIFORM = [("q2", 2), (ZONE, 3), ("q4", 4), ("q6", 6), ("q12", 12)]  # 12 consecutive slots: equal counts per domain
PF_OTHER = [("q5", 5), ("q7", 7), ("q11", 11)]
PF_FREE = [i for i in range(PF_N) if i % 13 == 12]  # the nodes of q13's one domain without a web pod


def pf_cluster(bound_terms=None):
    keys = PF_UNIFORM + PF_OTHER + [("q13", 13)]
    nodes = [node(i, {k: f"{k}-{i % m}" for k, m in keys}) for i in range(PF_N)]
    # web pods on slots 13 .. 24: q13's domains 0 .. 11 hold one each, domain 12 none
    bound = [(pod(f"b{i}", terms=bound_terms), i) for i in range(13, 25)]
    return nodes, bound


def pf_exp(decided_by):
    # the deciding record leaves PF_FREE; slot 12 is the lowest of them and, as most, holds no pod
    return [dict(node=12, feasible=len(PF_FREE), fails={decided_by: PF_N - len(PF_FREE)})]


def pf_spread(ncons, mode):
    """ncons constraints; the last one (index >= SP_PF) is the only one that
    rejects (mode dns) or the only one that scores (mode anyway).  The others
    count db pods -- one in every q13 domain, slots 26 .. 38 -- on other keys
    under a maxSkew that never binds: read for the last constraint, their
    selector's counts or their keys' domains give another answer."""
    assert ncons > SP_PF
    nodes, bound = pf_cluster()
    bound += [(pod(f"d{i}", {"app": "db"}), i) for i in range(26, 39)]
    keys = ["q2", ZONE, "q4", "q6", HOST, "q5", "q7"][:ncons - 1]  # from six constraints on, the hostname too
    idle = [TSC(100, k, DNS, LabelSelector({"app": "db"})) for k in keys]
    assert len(idle) == ncons - 1
    last = TSC(1, "q13", DNS if mode == "dns" else ANYWAY, WEB)
    pods = [pod("p0", spread=idle + [last])]
    control = [pod("p0", spread=idle)]  # without the deciding constraint: slot 0, the lowest without a pod
    if mode == "dns":
        return dict(nodes=nodes, bound=bound, pods=pods, exp=pf_exp(SPREAD), dumps={}, control=control)
    w = math.log(13 + 2)
    raw = [0 if i % 13 == 12 else round(w) for i in range(PF_N)]  # 3 = round(2.708)
    score = [100 * (3 + 0 - r) // 3 for r in raw]
    return dict(nodes=nodes, bound=bound, pods=pods, exp=[dict(node=12, feasible=PF_N)],
                dumps={0: {"spread_raw": raw, "spread_score": score}}, control=control)


def pf_affinity(nrec, whose):
    """nrec summed InterPodAffinity records; the last is a required
    anti-affinity term on q13: the pod's own (whose = own) or one that the
    bound web pods carry and that selects the pod (whose = bound).  The nrec - 1
    before it are preferred terms on keys whose domains hold equal counts (and,
    from the fifth on, the hostname): they move every node's score alike,
    except that the hostname term lowers slots 13 .. 24."""
    assert nrec > AF_PF
    edge = LabelSelector({"role": "edge"})
    nodes, bound = pf_cluster([T("q13", edge, kind="anti-affinity")] if whose == "bound" else None)
    pref = [T(k, WEB, kind="preferred-affinity", weight=3 + j) for j, (k, _) in enumerate(PF_UNIFORM[:4])]
    pref += [T(HOST, WEB, kind="preferred-anti-affinity", weight=2), T("q12", WEB, kind="preferred-affinity", weight=9),
             T("q2", WEB, kind="preferred-anti-affinity", weight=1),
             T(ZONE, WEB, kind="preferred-anti-affinity", weight=4)]
    pref = pref[:nrec - 1]
    if whose == "own":
        labels = {"app": "api"}
        pods = [pod("p0", labels, terms=pref + [T("q13", WEB, kind="anti-affinity")])]
        control = [pod("p0", labels, terms=pref)]
    else:
        pods = [pod("p0", {"app": "api", "role": "edge"}, terms=pref)]
        control = [pod("p0", {"app": "api"}, terms=pref)]  # not selected by the bound pods' term
    return dict(nodes=nodes, bound=bound, pods=pods, exp=pf_exp(POD_AFFINITY), dumps={}, control=control)


PF_CASES = {f"spread-{mode}-{k}": (lambda k=k, mode=mode: pf_spread(k, mode)) for mode in ("dns", "anyway")
            for k in (5, 6, 8)}
PF_CASES.update({f"affinity-own-{k}": (lambda k=k: pf_affinity(k, "own")) for k in (5, 6, 7, 8, 9)})
PF_CASES.update({f"affinity-bound-{k}": (lambda k=k: pf_affinity(k, "bound")) for k in (5, 9)})


# ------------------------------------------------------------ 4. churn

CHURN_CAP, CHURN_NODES, CHURN_STEPS = 64, 60, 24
CHURN_PHASES = [0, 2]  # the two nodes share a value at the renumbering step, or no two do


class KeyModel:
    """ksched_host.cpp's TopoKey as far as ks_debug_topology shows it."""

    def __init__(self, present):
        self.at = dict(present)  # slot -> value
        self.issued = set(self.at.values())
        self.rebuilds = 0

    def upsert(self, vals, cap):
        self.at.update(vals)
        self.issued |= set(vals.values())
        peak = self.ids
        if peak > renumber_above(cap):
            self.issued = set(self.at.values())
            self.rebuilds += 1
        return peak

    @property
    def ids(self):
        return len(self.issued) + 1

    @property
    def shared(self):
        vs = list(self.at.values())
        return sum(1 for v in set(vs) if vs.count(v) > 1)


def churn_labels(step, phase):
    """Labels of the 60 nodes after `step`: a fresh rack value each step, a
    fresh hostname every third; during two steps of every four, node 11 takes
    node 10's rack and hostname."""
    hs = step - step % 3
    out = []
    for i in range(CHURN_NODES):
        src = 10 if i == 11 and step and (step + phase) % 4 < 2 else i
        out.append({HOST: f"h{hs}-{src}", "rack": f"r{step}-{src}", ZONE: f"z{i % 4}"})
    return out


def churn_pods(step):
    anti = LabelSelector({"anti": "y"})
    return [pod(f"s{step}-rack", spread=[TSC(1, "rack", DNS, WEB)]),
            pod(f"s{step}-host", spread=[TSC(1, HOST, ANYWAY, WEB)]),
            pod(f"s{step}-anti", {"app": "web", "anti": "y"}, terms=[T(HOST, anti, kind="anti-affinity")]),
            pod(f"s{step}-zone", terms=[T(ZONE, WEB, kind="preferred-affinity", weight=10)])]


def churn_stream(x, phase, probe=None):
    """Step 0 fills the cache and schedules the four pods (the columns are
    built); steps 1 .. 24 upsert all nodes with new labels and schedule four
    more.  probe(step, models, scratch): after each step's pods, the KeyModel
    of rack and hostname and the modelled scratch capacity.  Returns the
    results of every step and the steps at which the rack key left LDS and was
    renumbered."""
    slots = list(range(CHURN_NODES))
    mk = lambda step: [Node(f"n{i}", {"cpu": 4000, "memory": 8 * Gi, "pods": 110}, lab)  # noqa: E731
                       for i, lab in enumerate(churn_labels(step, phase))]
    x.upsert(mk(0), slots)
    x.add([pod(f"b{i}") for i in range(0, CHURN_NODES, 2)], list(range(0, CHURN_NODES, 2)))
    res = [x.schedule(churn_pods(0), "churn step 0")]
    labs = churn_labels(0, phase)
    models = {k: KeyModel({i: lab[k] for i, lab in enumerate(labs)}) for k in ("rack", HOST)}
    scratch, left_lds, renumbered, shared_then = SCRATCH_MIN, None, None, None
    if probe:
        probe(0, models, scratch)
    for step in range(1, CHURN_STEPS + 1):
        labs = churn_labels(step, phase)
        x.upsert(mk(step), slots)
        before = models["rack"].rebuilds
        need = max(m.upsert({i: lab[k] for i, lab in enumerate(labs)}, CHURN_CAP) for k, m in models.items())
        if need > scratch:
            scratch = max(need, 2 * scratch)
        if left_lds is None and need > SP_LDS_DOM:
            left_lds = step
        if models["rack"].rebuilds > before:
            renumbered, shared_then = step, models["rack"].shared
        res.append(x.schedule(churn_pods(step), f"churn step {step}"))
        x.dump_equal(churn_pods(1000 + step)[step % 4], f"churn dump {step}")
        if probe:
            probe(step, models, scratch)
    return res, dict(left_lds=left_lds, renumbered=renumbered, shared_then=shared_then, scratch=scratch,
                     rack_ids=models["rack"].ids)


# ------------------------------------------------------------ 5. replica-run width

RUN_D = [1030, 2045, 2046, 2047]  # id counts 1031 .. 2048: the run takes up to 2047
RUN_VARIANTS = ["defaults", "dns"]
RUN_REPLICAS = 40


def run_width(D, variant):
    """D cells on D + 50 nodes.  The deployment's node selector leaves the 10
    first and the 32 last cells (52 nodes, at most 42 x 2 groups: a run holds
    RUN_GROUPS), so its candidates carry the lowest and the highest domain ids
    of the run kernel's LDS tables, while the cell constraint counts the web
    pods of every cell (nodeAffinityPolicy Ignore): one on every 9th between
    the two ends, one on cell 3 and one on cell D-3.  That leaves 40 of the
    deployment's cells without a web pod, one per replica."""
    n = D + 50
    pool = lambda i: i % D < 10 or i % D >= D - 32  # noqa: E731
    nodes = [node(i, dict({"cell": f"c{i % D}"}, **({"pool": "run"} if pool(i) else {}))) for i in range(n)]
    assert sum(pool(i) for i in range(n)) == 52 and pool(D - 1) and 2 * 42 <= RUN_GROUPS
    bound = [(pod(f"b{i}"), i) for i in [3, D - 3] + list(range(40, D - 40, 9))]
    assert sum(pool(i) for _, i in bound) == 2 and RUN_REPLICAS == 42 - 2
    if variant == "defaults":  # the system defaults' shape, `cell` in the zone's place
        spread = [TSC(3, HOST, ANYWAY, WEB), TSC(5, "cell", ANYWAY, WEB, node_affinity_policy="Ignore")]
    else:
        spread = [TSC(1, "cell", DNS, WEB, node_affinity_policy="Ignore")]
    pods = [Pod(f"web-{j}", containers=[Container({"cpu": 100, "memory": 100 * Mi})], labels={"app": "web"},
                topology_spread=spread, spread_defaulted=variant == "defaults", node_selector={"pool": "run"})
            for j in range(RUN_REPLICAS)]
    return dict(nodes=nodes, bound=bound, pods=pods, exp=[], dumps={},
                ids={"cell": D + 1}, runs=D + 1 <= RK_DZ_NONE)


# ------------------------------------------------------------ two ranks (tests/chain_multirank_main.py)

def two_rank_case(cfg):
    """wide_key(D, variant) on two in-process ranks: the chain runs replicated."""
    import ctypes as C

    import numpy as np

    import pyoracle
    from helpers import res_array, states_np
    from ksched.objects import Arena, nodes_array, pods_array
    case = wide_key(cfg["D"], cfg["variant"])
    n = len(case["nodes"])
    a = Arena()
    na, k = nodes_array(case["nodes"], a)
    sl = (C.c_uint32 * k)(*range(k))
    ba, nb = pods_array([p for p, _ in case["bound"]], a)
    bs = (C.c_uint32 * nb)(*[s for _, s in case["bound"]])
    batches = [pods_array([p], a) for p in case["pods"]]
    o = pyoracle.Oracle(n)
    o.upsert(na, sl, k)
    o.add_pods(ba, bs, nb)
    want = np.concatenate([res_array(o.schedule(pa, m), m) for pa, m in batches])
    check(want, case["exp"])
    states = states_np(o.L.oracle_node_states, o.o, n)
    o.close()

    def setup(s):
        s.upsert_nodes_raw(na, sl, k)
        assert s.lib.ks_pods_add(s.ctx, ba, bs, nb) == 0, s.lib.ks_last_error(s.ctx)

    def also(s):
        ids = s.debug_topology("cell")[0]
        if ids != case["ids"]["cell"]:
            return f"cell has {ids} ids, not {case['ids']['cell']}"

    return dict(capacity=n, pods_per_round=64, setup=setup, arena=a, batches=batches, want=want, states=states,
                check=also, report={"ids": case["ids"]["cell"]})
