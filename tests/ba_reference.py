"""Reference for NodeResourcesBalancedAllocation over a list of resources.

Upstream v1.31.3 noderesources/balanced_allocation.go#balancedResourceScorer
and resource_allocation.go, restated in numpy float64,
one IEEE operation per step in Go's order.  The list is walked in order, per
node and per resource:

  * cpu, memory: Allocatable, and Requested (not NonZeroRequested) + the pod's
    request;
  * a scalar resource: bypassed when the pod's PodRequests for it is 0, else
    Allocatable.ScalarResources[r] and Requested.ScalarResources[r] + the
    request;
  * Allocatable == 0 leaves the resource out; otherwise fraction =
    float64(req) / float64(alloc), clamped to 1, appended to the fractions and
    added to totalFraction, both in list order.

Zero or one fraction: std = 0.  Two: |f0 - f1| / 2.  More: mean = total / n,
sum += (f - mean)(f - mean) in list order from 0, std = sqrt(sum / n).  Score
= int64((1 - std) * 100).

BaReference composes it on top of XfitReference (tests/xfit_reference.py, whose
mirror holds the extended node state): balanced_allocation is replaced on the
feasible nodes and total' = total - w_ba x ba + w_ba x ba'.
"""
import numpy as np

from fit_reference import pod_requests
from xfit_reference import XfitReference, pod_xrequests

DEFAULT_LIST = ("cpu", "memory")


def ba_scores(entries):
    """The score per node from [(alloc, req)] int64 arrays: the resources that
    take part for the pod, in list order."""
    shape = np.asarray(entries[0][0]).shape if entries else (1,)
    n = np.zeros(shape, dtype=np.int64)
    tot = np.zeros(shape, dtype=np.float64)
    first = np.zeros(shape, dtype=np.float64)
    last = np.zeros(shape, dtype=np.float64)
    fr = []
    for alloc, req in entries:
        alloc = np.asarray(alloc, dtype=np.int64)
        req = np.asarray(req, dtype=np.int64)
        on = alloc != 0
        f = req.astype(np.float64) / np.where(on, alloc, 1).astype(np.float64)
        f = np.where(f > 1.0, 1.0, f)
        first = np.where(on & (n == 0), f, first)
        last = np.where(on, f, last)
        tot = np.where(on, tot + f, tot)
        n = n + on
        fr.append((on, f))
    nf = np.where(n == 0, 1, n).astype(np.float64)
    mean = tot / nf
    s = np.zeros(shape, dtype=np.float64)
    for on, f in fr:
        d = f - mean
        s = np.where(on, s + d * d, s)
    std = np.where(n > 2, np.sqrt(s / nf), np.where(n == 2, np.abs((first - last) / 2.0), 0.0))
    return ((1.0 - std) * 100.0).astype(np.int64)


class BaReference(XfitReference):
    """XfitReference whose BalancedAllocation walks `balanced`, an ordered
    list of names (None: [cpu, memory])."""

    def __init__(self, capacity, strategy=("LeastAllocated", 1, 1), extended=None, balanced=None,
                 weights=(1, 1, 3, 2, 1, 2)):
        super().__init__(capacity, strategy, extended, weights)
        self.w_ba = weights[1]
        self.balanced = list(balanced or DEFAULT_LIST)

    def set_balanced(self, balanced):
        self.balanced = list(balanced or DEFAULT_LIST)

    def ba(self, pod_ptr):
        """BalancedAllocation's score of every slot for the pod."""
        st = self.states()
        rc, rm, _, _ = pod_requests(pod_ptr)
        want = pod_xrequests(pod_ptr)
        zero = np.zeros(self.capacity, dtype=np.int64)
        entries = []
        for name in self.balanced:
            if name == "cpu":
                entries.append((st["alloc_cpu"], st["req_cpu"] + rc))
            elif name == "memory":
                entries.append((st["alloc_mem"], st["req_mem"] + rm))
            elif want.get(name, 0) != 0:  # else bypassed for this pod
                entries.append((self.xalloc.get(name, zero), self.xreq.get(name, zero) + want[name]))
        return ba_scores(entries)

    def plugin_scores(self, pod_ptr):
        sc = super().plugin_scores(pod_ptr)
        ba = self.ba(pod_ptr)
        feas = sc["status"] == -1
        sc["total_score"] = np.where(feas, sc["total_score"] - self.w_ba * sc["balanced_allocation"] + self.w_ba * ba,
                                     sc["total_score"])
        sc["balanced_allocation"] = np.where(feas, ba, sc["balanced_allocation"])
        return sc
