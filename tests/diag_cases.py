"""ks_diagnose cases with answers derived by hand from upstream v1.31.3's
status reasons (the table of DESIGN.md §5.15): small clusters in the style of
tests/spread_cases.py / ipa_cases.py.

Every case is (nodes, bound, pod, want): bound [(pod, slot)] are bound before
the diagnosis; want holds `reasons` {reason: nodes}, `plugin_nodes` (eight
first-failure counts), `feasible_nodes`, and, where it matters,
`node_ports_nodes` / `prefilter_msg` / `message`.  Used by
test_diag_reference.py (the reference alone, CPU) and test_gpu_diag.py
(libksched against these answers and the reference).
"""
from ksched.objects import (Container, LabelSelector, Node, NodeSelectorRequirement as Req, NodeSelectorTerm as Term,
                            Pod, PodAffinityTerm as T, Taint, Toleration, TopologySpreadConstraint as TSC)
from spread_cases import HOST, ZONE, node, pod

Gi, Mi = 1 << 30, 1 << 20
WEB, DB = LabelSelector({"app": "web"}), LabelSelector({"app": "db"})
PORT_PAIRS, PORT_IPS = [("TCP", 80)], ["10.0.0.1"]  # the NodePorts case's universe (PortsReference)

TAINT = "node(s) had untolerated taint {%s: %s}"
SPREAD_LABEL = "node(s) didn't match pod topology spread constraints (missing required label)"
SPREAD_SKEW = "node(s) didn't match pod topology spread constraints"
IPA_AFF = "node(s) didn't match pod affinity rules"
IPA_ANTI = "node(s) didn't match pod anti-affinity rules"
IPA_EXIST = "node(s) didn't satisfy existing pods anti-affinity rules"

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def pn(**kw):
    """plugin_nodes from plugin numbers: pn(p2=3, p4=1)."""
    out = [0] * 8
    for k, v in kw.items():
        out[int(k[1:])] = v
    return out


# ------------------------------------------------------- one per table row
@case
def node_unschedulable():
    # an unschedulable node that also has taints: NodeUnschedulable comes first
    nodes = [node("n0"), node("n1", taints=[Taint("a", "1")]), node("n2")]
    nodes[1].unschedulable = nodes[2].unschedulable = True
    p = pod("p", node_name="n9")  # n0 fails NodeName
    return nodes, [], p, dict(reasons={"node(s) were unschedulable": 2,
                                       "node(s) didn't match the requested node name": 1},
                              plugin_nodes=pn(p0=2, p1=1), feasible_nodes=0,
                              message="0/3 nodes are available: 1 node(s) didn't match the requested node name, "
                                      "2 node(s) were unschedulable.")


@case
def node_name():
    nodes = [node("n0"), node("n1"), node("n2")]
    return nodes, [], pod("p", node_name="n1"), dict(
        reasons={"node(s) didn't match the requested node name": 2}, plugin_nodes=pn(p1=2), feasible_nodes=1)


@case
def taint_first_in_node_order():
    t1, t2, t3 = Taint("k1", "v1"), Taint("k2", "v2", "NoExecute"), Taint("k3", "")
    soft = Taint("soft", "x", "PreferNoSchedule")  # never a reason
    nodes = [node("n0", taints=[t1, t2]), node("n1", taints=[t2, t1]), node("n2", taints=[soft, t3, t1, t2]),
             node("n3", taints=[t1]), node("n4", taints=[soft]),
             # one key and value under both effects: one string
             node("n5", taints=[Taint("k4", "v"), Taint("k4", "v", "NoExecute")]),
             node("n6", taints=[Taint("k4", "v", "NoExecute")])]
    p = pod("p", tolerations=[Toleration("k3", "Exists")])  # n2's first untolerated is then k1
    return nodes, [], p, dict(
        reasons={TAINT % ("k1", "v1"): 3, TAINT % ("k2", "v2"): 1, TAINT % ("k4", "v"): 2},
        plugin_nodes=pn(p2=6), feasible_nodes=1)


@case
def taint_tolerate_all():
    nodes = [node("n0", taints=[Taint("k1", "v1"), Taint("k2", "v2", "NoExecute")]), node("n1", taints=[Taint("k1", "v1")])]
    p = pod("p", tolerations=[Toleration("", "Exists")])  # an empty key with Exists tolerates everything
    return nodes, [], p, dict(reasons={}, plugin_nodes=pn(), feasible_nodes=2, message="0/2 nodes are available:")


@case
def node_affinity():
    nodes = [node("n0", labels={"disk": "ssd"}), node("n1"), node("n2", labels={"disk": "hdd"})]
    return nodes, [], pod("p", node_selector={"disk": "ssd"}), dict(
        reasons={"node(s) didn't match Pod's node affinity/selector": 2}, plugin_nodes=pn(p3=2), feasible_nodes=1)


@case
def node_affinity_conflict():
    nodes = [node("n0"), node("n1"), node("n2", taints=[Taint("a", "1")])]
    nodes[1].unschedulable = True  # PreFilter rejects the pod: no Filter runs, every node carries the conflict
    name_is = lambda v: Req("metadata.name", "In", [v])
    p = pod("p", required_terms=[Term(match_fields=[name_is("n0"), name_is("n1")])])
    return nodes, [], p, dict(reasons={"pod affinity terms conflict": 3}, plugin_nodes=pn(p3=3), feasible_nodes=0,
                              prefilter_msg="pod affinity terms conflict",
                              message="0/3 nodes are available: pod affinity terms conflict.")


@case
def prefilter_result():
    nodes = [node("n0"), node("n1"), node("n2"), node("n3", taints=[Taint("a", "1")])]
    p = pod("p", required_terms=[Term(match_fields=[Req("metadata.name", "In", [nm])]) for nm in ("n1", "n3", "gone")])
    return nodes, [], p, dict(
        reasons={"node is filtered out by the prefilter result": 2, TAINT % ("a", "1"): 1},
        plugin_nodes=pn(p7=2, p2=1), feasible_nodes=1)


@case
def node_ports():
    small = Node("n1", {"cpu": 50, "memory": 8 * Gi, "pods": 110}, {HOST: "n1"})
    nodes = [node("n0"), small, node("n2")]
    holder = lambda nm: Pod(nm, containers=[Container({"cpu": 10})], host_ports=[(None, "TCP", 80)])
    bound = [(holder("h0"), 0), (holder("h1"), 1)]
    # n0 fails NodePorts alone, n1 NodePorts and NodeResourcesFit (reported as NodePorts), n2 passes
    p = Pod("p", containers=[Container({"cpu": 100, "memory": 100 * Mi})], host_ports=[("10.0.0.1", "TCP", 80)])
    return nodes, bound, p, dict(
        reasons={"node(s) didn't have free ports for the requested pod ports": 2}, plugin_nodes=pn(),
        node_ports_nodes=2, feasible_nodes=1)


def sized(name, cpu, mem, pods, ext=None):
    return Node(name, {"cpu": cpu, "memory": mem, "pods": pods}, {HOST: name}, extended=dict(ext or {}))


@case
def fit_every_reason_at_once():
    gpu, eph = "amd.com/gpu", "ephemeral-storage"
    nodes = [sized("n0", 100, 1 * Gi, 1, {gpu: 1, eph: 10 * Gi}),   # pods, cpu, memory and gpu at once
             sized("n1", 4000, 8 * Gi, 110, {eph: 100 * Gi}),        # amd.com/gpu absent on the node
             sized("n2", 4000, 8 * Gi, 110, {gpu: 8, eph: 1 * Gi}),  # ephemeral-storage
             sized("n3", 4000, 1 * Gi, 110, {gpu: 8, eph: 100 * Gi}),  # memory only
             sized("n4", 4000, 8 * Gi, 110, {gpu: 8, eph: 100 * Gi})]  # fits
    bound = [(Pod("b", containers=[Container({"cpu": 50})]), 0)]
    p = Pod("p", containers=[Container({"cpu": 200, "memory": 2 * Gi, gpu: 2, eph: 5 * Gi})])
    return nodes, bound, p, dict(
        reasons={"Too many pods": 1, "Insufficient cpu": 1, "Insufficient memory": 2, "Insufficient amd.com/gpu": 2,
                 "Insufficient ephemeral-storage": 1},
        plugin_nodes=pn(p4=4), feasible_nodes=1,
        message="0/5 nodes are available: 1 Insufficient cpu, 1 Insufficient ephemeral-storage, 1 Too many pods, "
                "2 Insufficient amd.com/gpu, 2 Insufficient memory.")


@case
def fit_requestless_pod():
    nodes = [sized("n0", 0, 0, 1), sized("n1", 0, 0, 2)]
    bound = [(Pod("b0", containers=[Container({"cpu": 50})]), 0), (Pod("b1", containers=[Container({"cpu": 50})]), 1)]
    # Requested is above Allocatable on both; a pod that requests nothing is asked about the pod count alone
    return nodes, bound, Pod("p"), dict(reasons={"Too many pods": 1}, plugin_nodes=pn(p4=1), feasible_nodes=1)


@case
def fit_cpu_only_and_requested_above_allocatable():
    nodes = [sized("n0", 1000, 0, 110), sized("n1", 1000, 0, 110), sized("n2", 1000, 4 * Gi, 110)]
    bound = [(Pod("b0", containers=[Container({"cpu": 1500})]), 0),   # Requested above Allocatable after the add
             (Pod("b1", containers=[Container({"cpu": 950})]), 1)]
    p = Pod("p", containers=[Container({"cpu": 100})])  # no memory request: zero-memory nodes do not matter
    return nodes, bound, p, dict(reasons={"Insufficient cpu": 2}, plugin_nodes=pn(p4=2), feasible_nodes=1)


@case
def fit_memory_only():
    nodes = [sized("n0", 0, 1 * Gi, 110), sized("n1", 0, 4 * Gi, 110)]
    p = Pod("p", containers=[Container({"memory": 2 * Gi})])
    return nodes, [], p, dict(reasons={"Insufficient memory": 1}, plugin_nodes=pn(p4=1), feasible_nodes=1)


# ------------------------------------------------------- PodTopologySpread
@case
def spread_missing_label_against_skew():
    # zones a, a, b and a node without the zone label; web pods: 2 in a, 0 in b
    nodes = [node("n0", "a"), node("n1", "a"), node("n2", "b"), node("n3")]
    bound = [(pod("b0"), 0), (pod("b1"), 1)]
    p = pod("p", spread=[TSC(1, ZONE, "DoNotSchedule", WEB)])
    # min 0 (zone b); zone a: 2 + 1 - 0 > 1 fails by skew, b: 0 + 1 - 0 fits, n3 lacks the label
    return nodes, bound, p, dict(reasons={SPREAD_SKEW: 2, SPREAD_LABEL: 1}, plugin_nodes=pn(p5=3), feasible_nodes=1)


@case
def spread_two_constraints_first_decides():
    rack = lambda nm, z, r: node(nm, z, labels={"rack": r} if r else None)
    # n0 (zone a, no rack): a node lacking ANY key is not counted, and fails at its first failing constraint
    nodes = [rack("n0", "a", None), rack("n1", "a", "r1"), rack("n2", "b", "r2"), rack("n3", None, "r1")]
    bound = [(pod("b0"), 1), (pod("b1"), 1), (pod("b2"), 1)]
    p = pod("p", spread=[TSC(1, ZONE, "DoNotSchedule", WEB), TSC(1, "rack", "DoNotSchedule", WEB)])
    # eligible: n1, n2.  zone: a 3, b 0, min 0; rack: r1 3, r2 0, min 0.
    # n0: zone a 3 + 1 > 1 -> skew (before its missing rack label is looked at)
    # n1: skew; n2: fits both; n3: zone label missing -> missing label (its rack r1 would fail by skew)
    return nodes, bound, p, dict(reasons={SPREAD_SKEW: 2, SPREAD_LABEL: 1}, plugin_nodes=pn(p5=3), feasible_nodes=1)


@case
def spread_second_constraint_missing_label():
    nodes = [node("n0", "a", labels={"rack": "r1"}), node("n1", "a"), node("n2", "b", labels={"rack": "r2"})]
    p = pod("p", spread=[TSC(1, ZONE, "DoNotSchedule", WEB), TSC(1, "rack", "DoNotSchedule", WEB)])
    # no web pod anywhere: every skew is 1; n1 passes the zone constraint and lacks the rack label
    return nodes, [], p, dict(reasons={SPREAD_LABEL: 1}, plugin_nodes=pn(p5=1), feasible_nodes=2)


@case
def spread_min_domains():
    nodes = [node("n0", "a"), node("n1", "b")]
    bound = [(pod("b0"), 0), (pod("b1"), 0), (pod("b2"), 1)]
    # two domains < minDomains 3: the global minimum counts as 0; a: 2 + 1 > 2, b: 1 + 1 <= 2
    p = pod("p", spread=[TSC(2, ZONE, "DoNotSchedule", WEB, min_domains=3)])
    return nodes, bound, p, dict(reasons={SPREAD_SKEW: 1}, plugin_nodes=pn(p5=1), feasible_nodes=1)


# -------------------------------------------------------- InterPodAffinity
def ipa_cluster():
    # zones a, a, b, c; web pods: 2 on n0, 1 on n2
    nodes = [node("n0", "a"), node("n1", "a"), node("n2", "b"), node("n3", "c")]
    return nodes, [(pod("w0"), 0), (pod("w1"), 0), (pod("w2"), 2)]


@case
def ipa_affinity_rules():
    nodes, bound = ipa_cluster()
    nodes.append(node("n4"))  # no zone label: all topology labels must exist
    bound.append((pod("db", {"app": "db"}), 2))
    p = pod("front", {"app": "front"}, affinity_terms=[T(ZONE, DB)])
    return nodes, bound, p, dict(reasons={IPA_AFF: 4}, plugin_nodes=pn(p6=4), feasible_nodes=1)


@case
def ipa_anti_affinity_rules():
    nodes, bound = ipa_cluster()
    p = pod("p", {"app": "api"}, affinity_terms=[T(ZONE, WEB, kind="anti-affinity")])
    return nodes, bound, p, dict(reasons={IPA_ANTI: 3}, plugin_nodes=pn(p6=3), feasible_nodes=1)


@case
def ipa_existing_pods_anti_affinity():
    nodes, bound = ipa_cluster()
    bound += [(pod("db0", {"app": "db"}, affinity_terms=[T(HOST, WEB, kind="anti-affinity")]), 1),
              (pod("db1", {"app": "db"}, affinity_terms=[T(ZONE, WEB, kind="anti-affinity")]), 2)]
    return nodes, bound, pod("web"), dict(reasons={IPA_EXIST: 2}, plugin_nodes=pn(p6=2), feasible_nodes=2)


@case
def ipa_first_failing_check_is_reported():
    nodes, bound = ipa_cluster()
    bound += [(pod("db0", {"app": "db"}, affinity_terms=[T(ZONE, LabelSelector({"app": "api"}), kind="anti-affinity")]), 3),
              (pod("db1", {"app": "db"}), 0)]
    # the pod wants a db pod in its zone (a, c hold one) and no web pod on its host (n0, n2 hold one);
    # db0 in zone c refuses api pods zone-wide
    p = pod("p", {"app": "api"}, affinity_terms=[T(ZONE, DB), T(HOST, WEB, kind="anti-affinity")])
    # n0: affinity ok (zone a), anti-affinity fails            -> anti-affinity
    # n1: passes all three
    # n2: affinity fails (zone b holds no db) and anti fails   -> affinity, the first check
    # n3: affinity ok (zone c), anti ok, existing fails        -> existing
    return nodes, bound, p, dict(reasons={IPA_AFF: 1, IPA_ANTI: 1, IPA_EXIST: 1}, plugin_nodes=pn(p6=3), feasible_nodes=1)
