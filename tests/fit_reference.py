"""Reference for NodeResourcesFit scoring strategies other than the oracle's.

The CPU oracle (oracle/) knows one NodeResourcesFit configuration,
{LeastAllocated, cpu 1, memory 1}.  The reference for every other strategy is
composed from the oracle's own per-plugin surface, pod by pod:

  * oracle.plugin_scores(pod): per slot the filter status, every plugin's
    score and TotalScore under the default strategy;
  * oracle.node_states(slots) and oracle_pod_requests(pod): Allocatable,
    NonZeroRequested and the pod's non-zero requests -- the inputs of
    NodeResourcesFit's score;
  * the strategy's score per node (fit_scores below: upstream v1.31.3
    noderesources/{least,most}_allocated.go and resource_allocation.go,
    restated in numpy int64);
  * total' = total - w_fit x least_allocated + w_fit x fit';
  * schedulePod's outcome from them (feasible count, failure histogram, single
    feasible node, max total' with the lowest slot), then oracle.commit.

With the default strategy the composition reproduces oracle.schedule field for
field (tests/test_fit_reference.py), which is what lets the GPU tests trust it
for the others.  It does not model a NodeAffinity PreScore parse error (the
oracle's KS_POD_ERROR); the generators the tests use produce no such pod, and
a stream that held one would fail the default-strategy comparison.
"""
import ctypes as C

import numpy as np

import pyoracle
from helpers import STATE_DT
from ksched import _abi

LEAST, MOST = "LeastAllocated", "MostAllocated"
DEFAULT = (LEAST, 1, 1)
# the strategies the GPU tests run: (type, cpu weight, memory weight)
STRATEGIES = {"most-1-1": (MOST, 1, 1), "most-3-1": (MOST, 3, 1), "least-1-3": (LEAST, 1, 3), "most-1-0": (MOST, 1, 0)}


def resource_score(most, requested, capacity):
    """leastRequestedScore / mostRequestedScore of one resource, int64 arrays.
    capacity == 0 gives 0 here; fit_scores leaves such a resource out."""
    requested = np.asarray(requested, dtype=np.int64)
    capacity = np.asarray(capacity, dtype=np.int64)
    cap = np.where(capacity == 0, 1, capacity)
    if most:
        s = np.minimum(requested, capacity) * 100 // cap  # non-negative: // is Go's truncation
    else:
        s = np.where(requested > capacity, 0, (capacity - requested) * 100 // cap)
    return np.where(capacity == 0, 0, s).astype(np.int64)


def fit_scores(strategy, cap_cpu, cap_mem, req_cpu, req_mem):
    """resourceAllocationScorer.score per node: sum(score x weight) over the
    listed resources with non-zero allocatable, divided (int64 truncation) by
    their summed weight; 0 when no weight is left."""
    kind, wc, wm = strategy
    most = kind == MOST
    cap_cpu = np.asarray(cap_cpu, dtype=np.int64)
    cap_mem = np.asarray(cap_mem, dtype=np.int64)
    num = np.zeros(cap_cpu.shape, dtype=np.int64)
    den = np.zeros(cap_cpu.shape, dtype=np.int64)
    for w, cap, req in ((wc, cap_cpu, req_cpu), (wm, cap_mem, req_mem)):
        if w == 0:  # not listed
            continue
        on = cap != 0
        num += np.where(on, resource_score(most, req, cap) * w, 0)
        den += np.where(on, w, 0)
    return np.where(den == 0, 0, num // np.where(den == 0, 1, den)).astype(np.int64)


def pod_requests(pod_ptr):
    """(req cpu, req mem, non-zero cpu, non-zero mem) of one ks_pod."""
    out = (C.c_int64 * 4)()
    assert pyoracle.lib().oracle_pod_requests(pod_ptr, out) == 0
    return [int(x) for x in out]


def pod_at(arr, i):
    """Pointer to pod i of a ks_pod array or pointer."""
    base = C.cast(arr, C.c_void_p).value
    return C.cast(base + i * C.sizeof(_abi.KsPod), C.POINTER(_abi.KsPod))


def scores_np(raw, n):
    """ks_node_score[n] as a numpy record array (field names of the struct)."""
    size = C.sizeof(_abi.KsNodeScore)
    buf = np.frombuffer(C.string_at(C.addressof(raw), n * size), dtype=np.uint8).reshape(n, size)
    out = np.zeros(n, dtype=[(name, "<i8") for name, _ in _abi.KsNodeScore._fields_ if not name.startswith("_")])
    for name, ctype in _abi.KsNodeScore._fields_:
        if name.startswith("_"):
            continue
        off = getattr(_abi.KsNodeScore, name).offset
        w = C.sizeof(ctype)
        out[name] = buf[:, off:off + w].copy().view("<i4" if w == 4 else "<i8")[:, 0]
    return out


class FitReference:
    """A pyoracle.Oracle that schedules under a NodeResourcesFit strategy.
    (L / o: the oracle library and handle, as pyoracle.Oracle names them.)"""

    def __init__(self, capacity, strategy=DEFAULT, weights=(1, 1, 3, 2, 1, 2)):
        self.oracle = pyoracle.Oracle(capacity, weights)
        self.L, self.o = self.oracle.L, self.oracle.o
        self.capacity = capacity
        self.w_fit = weights[0]
        self.strategy = strategy
        self._slots = (C.c_uint32 * capacity)(*range(capacity))
        for name in ("upsert", "delete", "add_pods", "remove_pods", "node_states", "close"):
            setattr(self, name, getattr(self.oracle, name))

    def set_strategy(self, strategy):
        self.strategy = strategy

    def states(self):
        """Every slot's ks_node_state (helpers.STATE_DT)."""
        out = (_abi.KsNodeState * self.capacity)()
        assert self.L.oracle_node_states(self.o, self._slots, self.capacity, out) == 0
        return np.frombuffer(C.string_at(C.addressof(out), self.capacity * C.sizeof(_abi.KsNodeState)),
                             dtype=STATE_DT).copy()

    def plugin_scores(self, pod_ptr):
        """Per slot: the oracle's ks_node_score fields with least_allocated and
        total_score under the strategy in force."""
        sc = scores_np(self.oracle.plugin_scores(pod_ptr), self.capacity)
        st = self.states()
        _, _, zc, zm = pod_requests(pod_ptr)
        fit = fit_scores(self.strategy, st["alloc_cpu"], st["alloc_mem"], st["nz_cpu"] + zc, st["nz_mem"] + zm)
        feas = sc["status"] == -1
        sc["total_score"] = np.where(feas, sc["total_score"] - self.w_fit * sc["least_allocated"] + self.w_fit * fit,
                                     sc["total_score"])
        sc["least_allocated"] = np.where(feas, fit, sc["least_allocated"])
        return sc

    def keys(self, pod_ptr):
        """As helpers.oracle_keys: packed keys of the feasible nodes, descending, and their count."""
        sc = self.plugin_scores(pod_ptr)
        feas = np.nonzero(sc["status"] == -1)[0]
        keys = ((sc["total_score"][feas].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | (
            np.uint64(0xFFFFFFFF) - feas.astype(np.uint64))
        return np.sort(keys)[::-1], len(feas)

    def schedule_one(self, pod_ptr):
        r = _abi.KsResult()
        r.node_index = -1
        sc = self.plugin_scores(pod_ptr)
        status = sc["status"]
        r.evaluated_nodes = int((status != -2).sum())
        feas = np.nonzero(status == -1)[0]
        r.feasible_nodes = len(feas)
        hist = np.bincount(status[status >= 0], minlength=len(r.fail_counts))
        for k in range(len(r.fail_counts)):
            r.fail_counts[k] = int(hist[k])
        if len(feas) == 0:
            r.status = 1  # KS_POD_UNSCHEDULABLE
            return r
        if len(feas) == 1:
            r.flags |= 1  # KS_RESULT_SINGLE_FEASIBLE
        tot = sc["total_score"][feas]
        best = int(feas[np.argmax(tot)])  # argmax: the first (lowest slot) of the maxima
        r.node_index = best
        r.total_score = int(sc["total_score"][best])
        r.status = 0
        self.oracle.commit(pod_ptr, best)
        return r

    def schedule(self, arr, n):
        out = (_abi.KsResult * max(1, n))()
        for i in range(n):
            out[i] = self.schedule_one(pod_at(arr, i))
        return out
