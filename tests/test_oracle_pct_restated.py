"""The C++ oracle's percentageOfNodesToScore window against a second,
independent restatement in plain Python (CPU; parity unpinned: neither is the
reference, but they are written separately from upstream v1.31.3's text).

Resource-only pods on untainted, unlabelled nodes, so the profile reduces to
NodeResourcesFit (filter + LeastAllocated), BalancedAllocation and a constant
TaintToleration 3 x 100 (every raw score 0, DefaultNormalizeScore(reverse)
gives 100):

* schedule_one.go#numFeasibleNodesToFind / findNodesThatFitPod /
  findNodesThatPassFilters with one worker: visit from nextStartNodeIndex %
  len(nodes), stop at the (k+1)-th feasible node, nextStartNodeIndex +=
  processed;
* noderesources/fit.go#fitsRequest; least_allocated.go#leastRequestedScore
  and resource_allocation.go (NonZeroRequested, 100m / 200Mi defaults for
  missing requests); balanced_allocation.go (float64 fractions, std = |f0 -
  f1| / 2);
* selectHost: the highest TotalScore, the lowest slot among ties (ksched's
  deterministic tie-break).

The second half (PyWindow) adds absent slots, cordoned nodes and
PreFilterResult pods, and compares pod by pod, nextStartNodeIndex included."""
import random

import pytest

import pyoracle
from helpers import res_array
from ksched.objects import (Arena, Container, Node, NodeSelectorRequirement, NodeSelectorTerm, Pod, nodes_array,
                            pods_array)

Mi, Gi = 1 << 20, 1 << 30
DEF_CPU, DEF_MEM = 100, 200 * Mi


def num_to_find(pct, n):
    if n < 100:
        return n
    p = pct if pct else max(50 - n // 125, 5)
    return max(n * p // 100, 100)


class PyNode:
    def __init__(self, cpu, mem, pods):
        self.ac, self.am, self.ap = cpu, mem, pods
        self.rc = self.rm = self.zc = self.zm = self.np = 0


def requests(pod):
    c = pod.containers[0].requests
    rc, rm = c.get("cpu", 0), c.get("memory", 0)
    zc = c["cpu"] if "cpu" in c else DEF_CPU
    zm = c["memory"] if "memory" in c else DEF_MEM
    return rc, rm, zc, zm


def fits(nd, rc, rm):
    if nd.np + 1 > nd.ap:
        return False
    if rc == 0 and rm == 0:
        return True
    return not ((rc > 0 and rc > nd.ac - nd.rc) or (rm > 0 and rm > nd.am - nd.rm))


def least(req, cap):
    if cap == 0 or req > cap:
        return 0
    return (cap - req) * 100 // cap


def score(nd, rc, rm, zc, zm):
    la_num, la_w = 0, 0
    for cap, req in ((nd.ac, nd.zc + zc), (nd.am, nd.zm + zm)):
        if cap:
            la_num += least(req, cap)
            la_w += 1
    la = la_num // la_w if la_w else 0
    fr = [min(1.0, float(req) / float(cap)) for cap, req in ((nd.ac, nd.rc + rc), (nd.am, nd.rm + rm)) if cap]
    std = abs((fr[0] - fr[1]) / 2) if len(fr) == 2 else 0.0
    ba = int((1 - std) * 100)
    return la + ba + 3 * 100


def py_schedule(nodes, pods, pct):
    nxt, out = 0, []
    n = len(nodes)
    for pod in pods:
        rc, rm, zc, zm = requests(pod)
        k = num_to_find(pct, n)
        s = nxt % n
        feas, processed = [], n
        for j in range(n):
            i = (s + j) % n
            if fits(nodes[i], rc, rm):
                if len(feas) == k:
                    processed = j
                    break
                feas.append(i)
        nxt = (nxt + processed) % n
        if not feas:
            out.append((-1, 0, processed))
            continue
        best = max(feas, key=lambda i: (score(nodes[i], rc, rm, zc, zm), -i))
        nd = nodes[best]
        nd.rc += rc
        nd.rm += rm
        nd.zc += zc
        nd.zm += zm
        nd.np += 1
        out.append((best, len(feas), processed))
    return out, nxt


@pytest.mark.parametrize("seed", range(12))
def test_window_matches_python_restatement(seed):
    rng = random.Random(500 + seed)
    n = rng.choice([60, 150, 320])
    pct = rng.choice([0, 3, 5, 20, 50, 100])
    spec = [(rng.choice([1000, 2000, 4000, 0]), rng.choice([2, 4, 8]) * Gi, rng.choice([1, 3, 110])) for _ in range(n)]
    nodes = [Node(f"n{i}", {"cpu": c, "memory": m, "pods": p}) for i, (c, m, p) in enumerate(spec)]
    pods = []
    for j in range(rng.choice([40, 150])):
        r = rng.random()
        req = {} if r < 0.15 else ({"cpu": rng.randrange(1, 20) * 100} if r < 0.3 else
                                   {"cpu": rng.randrange(1, 20) * 100, "memory": rng.randrange(1, 16) * 128 * Mi})
        pods.append(Pod(f"p{j}", containers=[Container(req)]))
    a = Arena()
    o = pyoracle.Oracle(n, percentage=pct)
    na, _ = nodes_array(nodes, a)
    o.upsert(na, (pyoracle.C.c_uint32 * n)(*range(n)), n)
    pa, m = pods_array(pods, a)
    got = res_array(o.schedule(pa, m), m)
    want, nxt = py_schedule([PyNode(*t) for t in spec], pods, pct)
    for j, (node, feas, processed) in enumerate(want):
        g = got[j]
        assert (int(g["node_index"]), int(g["feasible"]), int(g["evaluated"])) == (node, feas, processed), \
            (seed, n, pct, j, g, (node, feas, processed))
    assert o.next_start == (nxt if pct != 100 else 0)


# ------------------------------------------------- absent slots, cordons, PreFilterResult
#
# A second restatement, wider than py_schedule: a table of slots of which some
# are absent, cordoned nodes (NodeUnschedulable is the first filter, so a
# cordoned node that would not fit either is counted as unschedulable) and
# pods whose required NodeAffinity is `metadata.name In [h]` terms (upstream's
# nodeaffinity PreFilter returns their union as PreFilterResult.NodeNames).
#
#   allNodes   the present nodes in slot order
#   list       allNodes, restricted to the named nodes when the pod names any
#   k          numFeasibleNodesToFind(pct, len(list))
#   visit      from nextStartNodeIndex % len(list), round the list, stopping at
#              the (k+1)-th feasible node
#   processed  feasible kept + visited and rejected + present nodes outside the
#              PreFilterResult (each of the three leaves a feasible node or a
#              recorded status: len(feasibleNodes) + len(NodeToStatusMap))
#   evaluated  = processed
#   nextStartNodeIndex = (nextStartNodeIndex + processed) % len(allNodes);
#              an empty list leaves it where it was


class WNode(PyNode):
    def __init__(self, name, cpu, mem, pods, unsched=False):
        super().__init__(cpu, mem, pods)
        self.name, self.unsched = name, unsched

    def to_node(self):
        return Node(self.name, {"cpu": self.ac, "memory": self.am, "pods": self.ap}, unschedulable=self.unsched)


def named(pod):
    """The node names of a pod whose required terms are all single
    metadata.name In [...] field terms; None for a pod that names none."""
    if not pod.required_terms:
        return None
    out = set()
    for t in pod.required_terms:
        assert not t.match_expressions and len(t.match_fields) == 1
        f = t.match_fields[0]
        assert (f.key, f.operator) == ("metadata.name", "In")
        out.update(f.values)
    return out


class Visit:
    """What one pod's visit did: the result fields and the window's geometry
    (slots, not list positions) for the tests that place it by construction."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def result(self):
        return self.node, self.feasible, self.evaluated, self.unsched, self.prefilter


class PyWindow:
    def __init__(self, capacity, pct):
        self.slots, self.pct, self.nxt, self._present = [None] * capacity, pct, 0, None

    def upsert(self, slot, node):
        self.slots[slot], self._present = node, None

    def delete(self, slot):
        self.slots[slot], self._present = None, None

    def lists(self, pod):
        """allNodes and the pod's list, as slots."""
        if self._present is None:
            self._present = [i for i, nd in enumerate(self.slots) if nd is not None]
        names = named(pod)
        return self._present, self._present if names is None else [i for i in self._present if self.slots[i].name in names]

    def schedule(self, pod):
        rc, rm, zc, zm = requests(pod)
        present, lst = self.lists(pod)
        nl, outside = len(lst), len(present) - len(lst)
        v = Visit(node=-1, feasible=0, evaluated=outside, unsched=0, prefilter=outside, nl=nl, k=0, visited=0,
                  start=None, stop=None, wrapped=False, nxt=self.nxt)
        if nl == 0:
            return v
        v.k = k = num_to_find(self.pct, nl)
        s = self.nxt % nl
        v.start = lst[s]
        feas, visited = [], nl
        for j in range(nl):
            i = lst[(s + j) % nl]
            nd = self.slots[i]
            if nd.unsched:
                v.unsched += 1
            elif fits(nd, rc, rm):
                if len(feas) == k:
                    visited, v.stop = j, i
                    break
                feas.append(i)
        v.visited = visited
        v.wrapped = s + visited + (v.stop is not None) > nl  # a node before the start was looked at
        processed = visited + outside
        v.feasible, v.evaluated = len(feas), processed
        v.nxt = self.nxt = (self.nxt + processed) % len(present)
        if feas:
            v.node = best = max(feas, key=lambda i: (score(self.slots[i], rc, rm, zc, zm), -i))
            nd = self.slots[best]
            nd.rc += rc
            nd.rm += rm
            nd.zc += zc
            nd.zm += zm
            nd.np += 1
        return v


def name_terms(names):
    return [NodeSelectorTerm(match_fields=[NodeSelectorRequirement("metadata.name", "In", [h])]) for h in names]


class OraclePair:
    """pyoracle.Oracle and PyWindow fed the same events, one pod at a time."""

    def __init__(self, capacity, pct):
        self.a, self.cap = Arena(), capacity
        self.o = pyoracle.Oracle(capacity, percentage=pct)
        self.py = PyWindow(capacity, pct)

    def upsert(self, items):  # [(slot, WNode)]
        na, k = nodes_array([nd.to_node() for _, nd in items], self.a)
        self.o.upsert(na, (pyoracle.C.c_uint32 * k)(*[s for s, _ in items]), k)
        for s, nd in items:
            self.py.upsert(s, nd)

    def delete(self, slots):
        self.o.delete((pyoracle.C.c_uint32 * len(slots))(*slots), len(slots))
        for s in slots:
            self.py.delete(s)

    def schedule(self, pod, what):
        pa, _ = pods_array([pod], self.a)
        g = res_array(self.o.schedule(pa, 1), 1)[0]
        v = self.py.schedule(pod)
        got = (int(g["node_index"]), int(g["feasible"]), int(g["evaluated"]), int(g["fail"][0]), int(g["fail"][7]))
        assert got == v.result(), (what, got, v.result())
        assert self.o.next_start == v.nxt, (what, self.o.next_start, v.nxt)
        return v

    def run(self, pods, what):
        return [self.schedule(p, what) for p in pods]


def rand_wnode(rng, name):
    small = rng.random() < 0.05  # a few nodes fill up during the stream; the others stay feasible
    return WNode(name, rng.choice([1000, 2000, 2000, 4000, 4000, 8000, 8000, 0]), rng.choice([2, 4, 8]) * Gi,
                 rng.choice([1, 3]) if small else 10_000, unsched=rng.random() < 0.05)


def rand_wpod(rng, j, names):
    r = rng.random()
    req = {} if r < 0.15 else ({"cpu": rng.randrange(1, 5) * 10} if r < 0.3 else
                               {"cpu": rng.randrange(1, 5) * 10, "memory": rng.randrange(1, 8) * Mi})
    return Pod(f"p{j}", containers=[Container(req)], required_terms=name_terms(names) if names else None)


def window_stream(seed, n, pct, npods):
    """A random stream on n nodes among n + n // 8 slots; returns the visits and
    which of them named nodes."""
    rng = random.Random(9000 + seed)
    cap = n + n // 8
    x = OraclePair(cap, pct)
    serial = iter(range(10 ** 9))
    place = sorted(rng.sample(range(cap), n))
    x.upsert([(s, rand_wnode(rng, f"w{next(serial)}")) for s in place])
    visits, was_named = [], []
    for j in range(npods):
        names = None
        if rng.random() < 0.25:
            live = [nd.name for nd in x.py.slots if nd is not None]
            r = rng.random()
            if r < 0.1:
                names = ["nowhere"]  # a name that matches no present node: an empty list
            elif r < 0.2:
                gone = rng.sample([i for i, nd in enumerate(x.py.slots) if nd is not None], 2)
                names = [x.py.slots[i].name for i in gone]
                x.delete(gone)  # every named node deleted
            else:
                names = rng.sample(live, rng.randint(1, 4)) + (["nowhere"] if r < 0.4 else [])
        visits.append(x.schedule(rand_wpod(rng, j, names), (seed, n, pct, j, names)))
        was_named.append(names is not None)
        if rng.random() < 0.15:  # the list shrinks and grows between pods
            live = [i for i, nd in enumerate(x.py.slots) if nd is not None]
            free = [i for i, nd in enumerate(x.py.slots) if nd is None]
            x.delete(rng.sample(live, min(len(live) - 1, rng.randint(1, 3))))
            x.upsert([(s, rand_wnode(rng, f"w{next(serial)}")) for s in rng.sample(free, min(len(free), rng.randint(1, 3)))])
    x.o.close()
    return visits, was_named


def index_rule_exercised(visits, was_named):
    """A PreFilterResult pod with a non-empty list was followed by a pod whose
    window stopped short of its list: only then does the index that the named
    pod left decide which nodes the next pod sees."""
    return any(a and va.nl and not b and vb.stop is not None
               for a, b, va, vb in zip(was_named, was_named[1:], visits, visits[1:]))


WINDOW_NS, WINDOW_PCTS = [60, 150, 320, 1100], [0, 3, 5, 20, 50]


@pytest.mark.parametrize("seed", range(20))  # 4 and 5 are coprime: every (n, pct) pair once
def test_window_with_holes_cordons_and_prefilter_result(seed):
    n, pct = WINDOW_NS[seed % 4], WINDOW_PCTS[seed % 5]
    visits, was_named = window_stream(seed, n, pct, 120)
    assert any(a and v.nl == 0 for a, v in zip(was_named, visits))  # an empty list was met
    assert any(v.unsched for v in visits)
    if n > 100:  # below minFeasibleNodesToFind every window is the whole list
        assert index_rule_exercised(visits, was_named), (seed, n, pct)


def test_window_at_the_adaptive_floor():
    # 6000 nodes at pct 0: 50 - 6000 / 125 = 2 is below the floor of 5 %, so
    # k = 5 % of the list: 300 at 6000 nodes (299 once churn has taken the list below 6000)
    visits, was_named = window_stream(100, 6000, 0, 40)
    plain = [v for a, v in zip(was_named, visits) if not a]
    assert all(v.k == v.nl * 5 // 100 for v in plain) and any(v.k == 300 for v in plain)
    assert index_rule_exercised(visits, was_named)
