"""Streams that place the percentageOfNodesToScore window by construction
(DESIGN.md §5.8).  Nodes are equal apart from being cordoned and pods are
tiny, so the pattern of cordoned slots is the feasibility pattern and it
survives the stream.  Every stream drives a target `x` that has `py` (the
plain-Python restatement, test_oracle_pct_restated.PyWindow), `upsert([(slot,
WNode)])`, `delete(slots)` and `run(pods, what) -> [Visit]`, and returns the
visits: tests/test_oracle_pct_window.py runs them on the C++ oracle,
tests/test_gpu_pct_window.py on the device, and both assert from the visits
that the stream reached what it exists for."""
import random

from ksched.objects import Container, Pod
from test_oracle_pct_restated import WNode, fits, name_terms, num_to_find, requests

Mi, Gi = 1 << 20, 1 << 30
CHUNK = 1024  # slots per count of the window kernel (WIN_CHUNK)
K = 100       # minFeasibleNodesToFind: k at pct 5 for 100 to 2019 list nodes


def wnode(i, cordoned=False):
    return WNode(f"h{i}", 64_000, 256 * Gi, 100_000, unsched=cordoned)


def tiny(j, names=None):
    return Pod(f"t{j}", containers=[Container({"cpu": 10, "memory": Mi})],
               required_terms=name_terms(names) if names else None)


def on_edge(slot):
    return slot is not None and slot % CHUNK in (0, CHUNK - 1)


def fill(x, slots, feasible):
    feasible = set(feasible)
    x.upsert([(i, wnode(i, i not in feasible)) for i in slots])


def peek(py, pod):
    """The start slot of the pod's visit and its feasible slots in visit order."""
    rc, rm, _, _ = requests(pod)
    _, lst = py.lists(pod)
    s = py.nxt % len(lst)
    order = lst[s:] + lst[:s]
    return order[0], [i for i in order if not py.slots[i].unsched and fits(py.slots[i], rc, rm)]


def steer(x, pod, want, max_deleted):
    """Delete up to max_deleted feasible nodes inside the pod's coming window so
    that the (k+1)-th feasible node, where the visit stops, is a slot that
    `want` accepts.  Only when the window does not wrap: the deleted nodes then
    lie after the start slot and the start keeps its list rank."""
    start, order = peek(x.py, pod)
    nl = len(x.py.lists(pod)[1])
    for d in range(max_deleted + 1):
        k = num_to_find(x.py.pct, nl - d)
        if len(order) - d <= k + 1:
            return False
        head = order[:k + d + 1]
        if head != sorted(head) or start > head[0]:
            return False
        if want(head[-1]):
            if d:
                x.delete(head[1:1 + d])
            return True
    return False


def one_pod_stream(x, npods, want=on_edge, max_deleted=0, tag=""):
    """npods one-pod calls; until a visit has stopped on a slot that `want`
    accepts, nodes are deleted to steer one there (max_deleted at a time)."""
    visits, hit = [], False
    for j in range(npods):
        pod = tiny(j)
        if max_deleted and not hit and j >= 2:
            hit = steer(x, pod, want, max_deleted)
        visits += x.run([pod], f"{tag} pod {j}")
    return visits


# ------------------------------------------------------------ slot counts

SLOT_COUNTS = [101, 115, 1023, 1024, 1025, 2049, 3001]
PATTERNS = ["all", "third", "last130", "mid", "k", "k+1"]


def spread_with_edges(cap, count, top=None):
    """count slots up to `top` (default: the last slot): every chunk-edge slot,
    `top` itself, and evenly spaced ones between them."""
    top = cap - 1 if top is None else top
    order = sorted({i for i in range(top + 1) if on_edge(i)} | {top})
    order += [round(j * top / (count - 1)) for j in range(count)] + list(range(top + 1))
    return sorted(list(dict.fromkeys(order))[:count])


def pattern_slots(cap, pattern):
    """The feasible slots of a pattern, or None where the table has no such
    pattern of its own (it would repeat `all`)."""
    if pattern == "all":
        return list(range(cap))
    if pattern == "third":
        return [i for i in range(cap) if i % 3]
    if pattern == "last130":
        return list(range(cap - 130, cap)) if cap > 130 else None
    if pattern == "mid":
        return list(range(1000, 1130)) if cap >= 1130 else None
    k = num_to_find(5, cap)  # 100 up to 2019 slots, 102 at 2049, 150 at 3001 (and the same with one slot fewer)
    if cap == k + 1:
        return None if pattern == "k+1" else list(range(1, cap))
    # the highest feasible slot is a chunk edge: the first visit stops there, the next ones on the feasible slots
    # before it; "k" deletes one of them during the stream
    return spread_with_edges(cap, k + 1, max(i for i in range(cap) if on_edge(i)) if cap > CHUNK else None)


SLOT_CASES = [(cap, p) for cap in SLOT_COUNTS for p in PATTERNS if pattern_slots(cap, p) is not None]


def slot_count_stream(x, cap, pattern):
    feasible = pattern_slots(cap, pattern)
    fill(x, range(cap), feasible)
    k = num_to_find(5, cap)
    if pattern == "k" and cap > k + 1:
        # k + 1 feasible nodes for 6 pods, so that the index leaves 0; then one
        # of them is deleted and every later visit finds exactly k
        visits = one_pod_stream(x, 6, tag=f"{cap} {pattern}")
        x.delete([feasible[50]])
        return visits + one_pod_stream(x, 34, tag=f"{cap} {pattern} exact")
    many = len(feasible) > k + 1
    return one_pod_stream(x, 44, max_deleted=k - 1 if many and cap > CHUNK else 0, tag=f"{cap} {pattern}")


def check_slot_count_stream(visits, cap, pattern):
    nf, k = len(pattern_slots(cap, pattern)), num_to_find(5, cap)
    if pattern == "k":
        exact = visits[6:] if cap > k + 1 else visits
        assert all(v.stop is None and v.feasible == v.k == k and v.visited == v.nl for v in exact)
        if cap > k + 1:
            assert all(v.start != 0 and v.wrapped for v in exact)  # a whole list from a start that is not its head
        return
    if nf <= k:  # `third` on 101 / 115 slots, 130 feasible of 3001: every visit takes the whole list
        assert all(v.stop is None and v.feasible == nf and v.visited == v.nl == cap for v in visits)
        return
    assert all(v.stop is not None and v.feasible == v.k for v in visits)
    assert any(v.wrapped for v in visits)
    assert any(v.stop < v.start for v in visits)  # the stopping node before the start node
    if cap > CHUNK:
        assert any(on_edge(v.start) and v.start for v in visits), "no start slot on a chunk edge"
        assert any(on_edge(v.stop) for v in visits), "no stopping slot on a chunk edge"


# ------------------------------------------------------------ list lengths

def named_lengths_stream(x, length):
    """3000 nodes; plain pods alternate with a pod that names `length`
    of them: k follows the list, not the table."""
    cap = 3000
    picked = set(spread_with_edges(cap, length))
    # every 7th of the others cordoned: the plain pods' windows vary in length, so the named list is entered at many ranks
    fill(x, range(cap), [i for i in range(cap) if i % 7 != 3 or i in picked])
    names = [f"h{i}" for i in sorted(picked)]
    visits = []
    for j in range(16):
        visits += x.run([tiny(j, names if j % 2 else None)], f"named {length} pod {j}")
    return visits


def check_named_lengths(visits, length):
    named, plain = visits[1::2], visits[0::2]
    assert all(v.nl == length and v.k == min(length, K) and v.prefilter == 3000 - length for v in named)
    assert all(v.nl == 3000 and v.k == 150 and v.stop is not None for v in plain)
    if length == K + 1:
        assert all(v.stop is not None and v.feasible == K and v.evaluated == 3000 - 1 for v in named)
        assert any(v.stop < v.start for v in named)
    else:
        assert all(v.stop is None and v.feasible == length and v.evaluated == 3000 for v in named)
    assert len({v.start for v in named}) > 4  # the named list was entered at different ranks


def present_lengths_stream(x, length):
    """`length` feasible nodes among 1500 slots, plain pods."""
    fill(x, spread_with_edges(1500, length), range(1500))
    return one_pod_stream(x, 10, tag=f"present {length}")


def check_present_lengths(visits, length):
    assert all(v.nl == length and v.k == min(length, K) for v in visits)
    if length == K + 1:
        assert all(v.stop is not None and v.feasible == K for v in visits)
        assert any(v.stop < v.start for v in visits) and any(v.wrapped for v in visits)
    else:
        assert all(v.stop is None and v.feasible == length and v.nxt == 0 for v in visits)


# ------------------------------------------------------------ holes

def holes_stream(x):
    """3000 slots: those = 1 mod 3 never filled, a fifth of the rest deleted,
    a tenth of the nodes cordoned."""
    rng = random.Random(4711)
    slots = [i for i in range(3000) if i % 3 != 1]
    keep_edges = {i for i in slots if on_edge(i)}
    fill(x, slots, [i for i in slots if i in keep_edges or rng.random() >= 0.1])
    x.delete(rng.sample([i for i in slots if i not in keep_edges], len(slots) // 5))
    return one_pod_stream(x, 44, max_deleted=99, tag="holes")


def check_holes(visits):
    assert all(v.nl <= 1600 and v.stop is not None and v.unsched for v in visits)
    assert any(v.wrapped for v in visits) and any(v.stop < v.start for v in visits)
    assert any(on_edge(v.start) and v.start for v in visits) and any(on_edge(v.stop) for v in visits)


# ------------------------------------------------------------ PreFilterResult, then plain pods

def prefilter_then_plain_stream(x):
    """1500 nodes, every 7th cordoned: named pods (1-4 names, one of them
    unknown; once with every named node deleted) alternate with plain pods."""
    rng = random.Random(1789)
    n = 1500
    fill(x, range(n), [i for i in range(n) if i % 7])
    visits, kinds = [], []
    for j in range(28):
        names, kind = None, "plain"
        if j % 2:
            live = [i for i, nd in enumerate(x.py.slots) if nd is not None]
            picked = rng.sample(live, rng.randint(1, 4))
            names, kind = [f"h{i}" for i in picked], "named"
            if j % 6 == 1:
                names, kind = names + ["h-unknown"], "named"
            if j == 9:
                x.delete(picked)
                kind = "gone"
            if j == 15:
                names, kind = ["h-unknown"], "gone"
        visits += x.run([tiny(j, names)], f"prefilter/plain pod {j} ({kind})")
        kinds.append(kind)
    return visits, kinds


def check_prefilter_then_plain(visits, kinds):
    before = 0
    for v, kind in zip(visits, kinds):
        if kind == "plain":
            assert v.stop is not None and v.nxt != before  # a window shorter than the list moved the index
        elif kind == "named":
            assert 1 <= v.nl <= 4 and v.evaluated == v.nl + v.prefilter and v.nxt == before
        else:
            assert v.nl == 0 and v.feasible == 0 and v.nxt == before
        before = v.nxt
    assert kinds.count("gone") == 2


# ------------------------------------------------------------ more than 1024 chunks

BIG_CAP = 1_048_576 + 2048 + 7  # 1027 chunks: the window kernel's threads take two chunks each
BIG_STRIDE = 741  # of the nodes between the placed groups


def big_present():
    placed = list(range(300)) + list(range(1_048_576 - 300, 1_048_576 + 300)) + list(range(BIG_CAP - 200, BIG_CAP))
    return sorted(set(placed) | set(range(5000, 1_040_000, BIG_STRIDE)))


def big_stream(x, npods=25):
    present = big_present()
    fill(x, present, [s for r, s in enumerate(present) if r % 3 != 2])
    # at pct 5 with a third of the nodes cordoned a lap takes 13 1/3 windows, so no window ends within the last 7
    # slots by itself: the 14th is steered there by deleting some 40 nodes inside it
    return one_pod_stream(x, npods, lambda s: s // CHUNK == BIG_CAP // CHUNK, max_deleted=60, tag="big")


def check_big(visits):
    ends = [s for v in visits for s in (v.start, v.stop)]
    assert all(v.stop is not None and v.k == v.nl * 5 // 100 > K for v in visits)
    assert any(s // CHUNK % 2 == 1 for s in ends), "no start / stop in the second chunk of a thread's pair"
    assert any(s // CHUNK == BIG_CAP // CHUNK for s in ends), "no start / stop in the final partial chunk"
    assert any(v.wrapped for v in visits) and any(v.stop < v.start for v in visits)


# ------------------------------------------------------------ adaptive floor

def adaptive_floor_stream(x):
    """6000 nodes at pct 0 (50 - 6000 / 125 is below the floor of 5 %: k =
    300), every 4th cordoned; one batch of 60 pods."""
    fill(x, range(6000), [i for i in range(6000) if i % 4])
    return x.run([tiny(j) for j in range(60)], "adaptive floor")


def check_adaptive_floor(visits):
    assert all(v.k == 300 and v.feasible == 300 and v.stop is not None for v in visits)
    assert any(v.wrapped for v in visits)
