"""Reference for NodeResourcesFit strategies that list extended resources.

Upstream v1.31.3 noderesources/resource_allocation.go
(calculateResourceAllocatableRequest), restated in numpy
int64.  Per listed resource r and node:

  * cpu, memory: Allocatable, and NonZeroRequested + the pod's non-zero request;
  * a scalar resource (an extended vendor/x name, hugepages-*,
    attachable-volumes-*, a kubernetes.io/-prefixed native name): when the pod's
    request for it is 0 the resource is bypassed -- it adds nothing to the sum
    and nothing to the weight sum; otherwise Allocatable.ScalarResources[r] (0
    when the node lacks it) and Requested.ScalarResources[r] + the pod's
    request (Requested, not NonZeroRequested; the request is PodRequests'
    value, the one the fit filter compares);
  * Allocatable == 0 leaves the resource out.

The oracle's ks_node_state carries no extended state, so XfitReference keeps
its own per-slot mirror of extended Allocatable and Requested by name, fed by
every cache event and by its own commits.  The pod's extended requests come
from pod_xrequests, a restatement of resourcehelper.PodRequests (containers'
sum, init containers' max with sidecars; ks_pod has no extended overhead).
Everything else is composed as tests/fit_reference.py describes.
"""
import numpy as np

from fit_reference import MOST, pod_at, pod_requests, resource_score, scores_np
from rtcr_reference import RtcrReference, raw, round_half_away

GPU, NIC, HUGE = "amd.com/gpu", "example.com/nic", "hugepages-2Mi"


def _extended(container):
    return [(container.extended[j].name.decode(), int(container.extended[j].value))
            for j in range(container.n_extended)]


def pod_xrequests(pod_ptr):
    """{name: value > 0} of one ks_pod: PodRequests over the resources beyond
    cpu and memory."""
    p = pod_ptr[0]
    total, side, init = {}, {}, {}
    for i in range(p.n_containers):
        for name, v in _extended(p.containers[i]):
            total[name] = total.get(name, 0) + v
    for i in range(p.n_init_containers):
        k = p.init_containers[i]
        if k.restart_always:  # a sidecar runs on: it counts with the containers and under every later init container
            for name, v in _extended(k):
                total[name] = total.get(name, 0) + v
                side[name] = side.get(name, 0) + v
            use = dict(side)
        else:
            use = dict(side)
            for name, v in _extended(k):
                use[name] = use.get(name, 0) + v
        for name, v in use.items():
            init[name] = max(init.get(name, 0), v)
    for name, v in init.items():
        total[name] = max(total.get(name, 0), v)
    return {name: v for name, v in total.items() if v > 0}


def combine(kind, resources):
    """The node score from [(weight, capacity, requested)] int64 arrays, the
    listed resources that take part for this pod.  kind: LeastAllocated /
    MostAllocated, or a RequestedToCapacityRatio shape."""
    shape = None if isinstance(kind, str) else kind
    zero = np.zeros(np.asarray(resources[0][1]).shape, dtype=np.int64)
    num, den = zero, zero  # (no resource left: 0)
    for w, cap, req in resources:
        if w == 0:  # not listed
            continue
        cap = np.asarray(cap, dtype=np.int64)
        req = np.asarray(req, dtype=np.int64)
        if shape is None:
            s = resource_score(kind == MOST, req, cap)
            on = cap != 0
        else:
            util = np.where(req > cap, 100, req * 100 // np.where(cap == 0, 1, cap))
            s = np.where(cap == 0, 0, raw(shape, util))
            on = s > 0
        num, den = num + np.where(on, s * w, 0), den + np.where(on, w, 0)
    safe = np.where(den == 0, 1, den)
    q = num // safe if shape is None else round_half_away(num, safe)
    return np.where(den == 0, 0, q).astype(np.int64)


class XfitReference(RtcrReference):
    """RtcrReference whose strategy may list extended resources:
    extended = {name: weight}.  strategy is fit_reference's (type, wc, wm) or
    rtcr_reference's (shape, wc, wm); weights of 0 leave cpu / memory out."""

    def __init__(self, capacity, strategy=("LeastAllocated", 1, 1), extended=None, weights=(1, 1, 3, 2, 1, 2)):
        super().__init__(capacity, strategy, weights)
        for name in ("upsert", "delete", "add_pods", "remove_pods"):  # FitReference binds the oracle's: the methods below
            del self.__dict__[name]
        self.extended = dict(extended or {})
        self.present = np.zeros(capacity, dtype=bool)
        self.xalloc, self.xreq = {}, {}

    def set_strategy(self, strategy, extended=None):
        self.strategy = strategy
        self.extended = dict(extended or {})

    def _col(self, table, name):
        if name not in table:
            table[name] = np.zeros(self.capacity, dtype=np.int64)
        return table[name]

    # ---- cache events: the oracle's, and the mirror
    def upsert(self, arr, slots, n):
        self.oracle.upsert(arr, slots, n)
        for i in range(n):
            slot = int(slots[i])
            if not self.present[slot]:  # a node absent before starts with nothing requested
                for col in self.xreq.values():
                    col[slot] = 0
                self.present[slot] = True
            for col in self.xalloc.values():
                col[slot] = 0
            for j in range(arr[i].n_extended):
                self._col(self.xalloc, arr[i].extended[j].name.decode())[slot] = int(arr[i].extended[j].value)

    def delete(self, slots, n):
        self.oracle.delete(slots, n)
        for i in range(n):
            slot = int(slots[i])
            self.present[slot] = False
            for col in list(self.xalloc.values()) + list(self.xreq.values()):
                col[slot] = 0

    def _account(self, pod_ptr, slot, sign):
        for name, v in pod_xrequests(pod_ptr).items():
            self._col(self.xreq, name)[slot] += sign * v

    def add_pods(self, arr, slots, n):
        self.oracle.add_pods(arr, slots, n)
        for i in range(n):
            self._account(pod_at(arr, i), int(slots[i]), +1)

    def remove_pods(self, arr, slots, n):
        self.oracle.remove_pods(arr, slots, n)
        for i in range(n):
            self._account(pod_at(arr, i), int(slots[i]), -1)

    # ---- the strategy
    def fit(self, pod_ptr):
        """NodeResourcesFit's score of every slot for the pod."""
        st = self.states()
        _, _, zc, zm = pod_requests(pod_ptr)
        kind, wc, wm = self.strategy
        res = [(wc, st["alloc_cpu"], st["nz_cpu"] + zc), (wm, st["alloc_mem"], st["nz_mem"] + zm)]
        want = pod_xrequests(pod_ptr)
        zero = np.zeros(self.capacity, dtype=np.int64)
        for name, w in self.extended.items():
            if want.get(name, 0) == 0:  # bypassed for this pod
                continue
            res.append((w, self.xalloc.get(name, zero), self.xreq.get(name, zero) + want[name]))
        return combine(kind, res)

    def plugin_scores(self, pod_ptr):
        sc = scores_np(self.oracle.plugin_scores(pod_ptr), self.capacity)
        fit = self.fit(pod_ptr)
        feas = sc["status"] == -1
        sc["total_score"] = np.where(feas, sc["total_score"] - self.w_fit * sc["least_allocated"] + self.w_fit * fit,
                                     sc["total_score"])
        sc["least_allocated"] = np.where(feas, fit, sc["least_allocated"])
        return sc

    def schedule_one(self, pod_ptr):
        r = super().schedule_one(pod_ptr)
        if r.status == 0:  # the commit's AssumePod
            self._account(pod_ptr, int(r.node_index), +1)
        return r


def ext_array(extended):
    """(ks_fit_resource array, count, keep-alive) of {name: weight}."""
    from ksched import _abi
    names = [k.encode() for k in extended]
    arr = (_abi.KsFitResource * max(1, len(names)))(*[_abi.KsFitResource(b, int(w), 0)
                                                      for b, w in zip(names, extended.values())])
    return arr, len(names), names
