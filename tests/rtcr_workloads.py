"""References of the RequestedToCapacityRatio GPU tests: the strategy-free
streams of tests/fit_workloads.py under RtcrReference (tests/rtcr_reference.py),
and one stream of its own whose nodes hold the two edge cases the shape
function has -- zero memory Allocatable (the resource takes no part although
raw(0) may be positive) and NonZeroRequested beyond capacity (utilisation 100).
Every reference is computed once per (workload, case) and left unchanged."""
import functools

import fit_workloads as W
from ksched import synth
from ksched.objects import Arena, Container, Node, Pod, nodes_array, pods_array
from rtcr_reference import RTCR, SHAPES, WEIGHTS, RtcrReference

Gi, Mi = 1 << 30, 1 << 20


def case(name):
    """"peaked-3-1" -> (shape, cpu weight, memory weight)."""
    shape, w = name.split("-", 1)
    return (SHAPES[shape],) + WEIGHTS[w]


# every shape and every weight pair at least once
CASES = ["binpack-1-1", "falling-3-1", "peaked-1-1", "flat-1-0", "offset-3-1"]


def use(s, name):
    """Set a case on a Scheduler and read it back."""
    shape, wc, wm = case(name)
    s.set_fit_strategy(RTCR, {"cpu": wc, "memory": wm}, shape)
    assert s.get_fit_strategy() == (RTCR, {"cpu": wc, "memory": wm})
    assert s.get_fit_shape() == list(shape)


def two_calls(r, arr, m1, m):
    out = []
    for lo, cnt in ((0, m1), (m1, m - m1)):
        out.append((r.schedule(W.pods_at(arr, lo), cnt), r.states()))
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def group_reference(kind_name, P, name):
    w = W.group_stream(kind_name, P)
    r = RtcrReference(W.CAP_A, case(name))
    W.group_setup(r, w)
    return two_calls(r, w["arr"], w["m1"], w["m"])


@functools.lru_cache(maxsize=None)
def pile_reference(name):
    w = W.pile_stream()
    r = RtcrReference(W.N_PILE, case(name))
    r.upsert(w["nodes"], w["slots"], w["n"])
    return two_calls(r, w["pods"], w["m1"], w["m"])


@functools.lru_cache(maxsize=None)
def hetero_reference(kind_name, name):
    w = W.hetero_stream(kind_name)
    r = RtcrReference(W.N_H, case(name))
    W.hetero_setup(r, w)
    out = (r.schedule(w["ps"].pods, w["m"]), r.states())
    r.close()
    return out


def two_rank_case(cfg):
    return W.hetero_case(W.hetero_stream(cfg["kind_name"]), *hetero_reference(cfg["kind_name"], cfg["name"]),
                         lambda s: use(s, cfg["name"]))


@functools.lru_cache(maxsize=None)
def wide_reference(name):
    from test_gpu_geometry import CAP_B, wide_workload
    w = wide_workload()
    r = RtcrReference(CAP_B, case(name))
    r.upsert(w["nodes"], w["slots"], w["n"])
    out = [(r.schedule(pa, m), r.states()) for pa, m, _, _ in w["batches"]]
    r.close()
    return out


# ------------------------------------------------------------- the edge stream
N_EDGE = 330


@functools.lru_cache(maxsize=None)
def edge_stream():
    """330 nodes: every third has no memory Allocatable, every third so little
    cpu (150m-250m, room for 6 pods) that the non-zero defaults of request-less
    pods (100m, 200Mi) pass its capacity after two of them; 1,300 pods, request-less
    ones and small ones that ask for cpu only, so that every node kind is taken."""
    a = Arena()
    nodes = []
    for i in range(N_EDGE):
        if i % 3 == 0:
            res = {"cpu": (2 + i % 5) * 1000, "memory": 0, "pods": 4}
        elif i % 3 == 1:
            res = {"cpu": 150 + 25 * (i % 5), "memory": (1 + i % 4) * Gi, "pods": 6}
        else:
            res = {"cpu": (1 + i % 4) * 1000, "memory": (2 + i % 3) * Gi, "pods": 3}
        nodes.append(Node(f"e{i}", res))
    na, n = nodes_array(nodes, a)
    pods = []
    for j in range(1300):
        if j % 5 < 3:
            pods.append(Pod(f"be{j}", containers=[Container({})]))
        else:
            pods.append(Pod(f"c{j}", containers=[Container({"cpu": 20 + 10 * (j % 4)})]))
    pa, m = pods_array(pods, a)
    return dict(arena=a, nodes=na, n=n, slots=synth.slot_array(n), pods=pa, m=m, m1=700)


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    w = edge_stream()
    r = RtcrReference(N_EDGE, case(name))
    r.upsert(w["nodes"], w["slots"], w["n"])
    return two_calls(r, w["pods"], w["m1"], w["m"])


@functools.lru_cache(maxsize=None)
def edge_dump_reference(name):
    """A request-less pod's per-node scores against the filled edge cluster:
    (the pod array, its arena, the reference's ks_node_score records)."""
    w = edge_stream()
    a = Arena()
    pa, _ = pods_array([Pod("probe", containers=[Container({})])], a)
    r = RtcrReference(N_EDGE, case(name))
    r.upsert(w["nodes"], w["slots"], w["n"])
    r.schedule(w["pods"], w["m"])
    want = r.plugin_scores(pa)
    r.close()
    return pa, a, want
