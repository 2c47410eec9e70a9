"""Reference for NodeResourcesFit's RequestedToCapacityRatio strategy.

A numpy int64 restatement of upstream v1.31.3
noderesources/requested_to_capacity_ratio.go, helper/shape_score.go and
resource_allocation.go, and a FitReference
(tests/fit_reference.py) that composes the oracle's per-plugin surface with it:
FitReference.plugin_scores is the one method the strategy enters.

A shape is a tuple of (utilization, score) points, scores 0..10 as configured;
raw() works on the scores x 10, as upstream does after
MaxNodeScore / MaxCustomPriorityScore.
"""
import numpy as np

from fit_reference import FitReference, pod_requests, scores_np

RTCR = "RequestedToCapacityRatio"

# the shapes the tests run
SHAPES = {
    "binpack": ((0, 0), (100, 10)),
    "falling": ((0, 10), (30, 0)),           # truncation toward zero on a falling segment
    "peaked": ((0, 0), (50, 10), (100, 0)),  # a node's key rises, then falls, as it fills
    "flat": ((40, 7),),
    "offset": ((20, 2), (80, 9)),
}
WEIGHTS = {"1-1": (1, 1), "3-1": (3, 1), "1-0": (1, 0)}


def trunc_div(a, b):
    """Go's int64 division: the quotient truncated toward zero (numpy's //
    floors, which differs for a negative numerator).  b > 0."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    q = np.abs(a) // b
    return np.where(a < 0, -q, q).astype(np.int64)


def raw(shape, p):
    """helper.BuildBrokenLinearFunction(shape x 10)(p), int64 arrays."""
    p = np.asarray(p, dtype=np.int64)
    xs = np.array([x for x, _ in shape], dtype=np.int64)
    ys = np.array([y for _, y in shape], dtype=np.int64) * 10
    out = np.full(p.shape, ys[-1], dtype=np.int64)  # past the last point
    done = np.zeros(p.shape, dtype=bool)
    for i in range(len(xs)):
        hit = ~done & (p <= xs[i])  # the first point with p <= x_i
        if i == 0:
            v = np.full(p.shape, ys[0], dtype=np.int64)
        else:
            v = ys[i - 1] + trunc_div((ys[i] - ys[i - 1]) * (p - xs[i - 1]), xs[i] - xs[i - 1])
        out = np.where(hit, v, out)
        done |= hit
    return out


def table(shape):
    """raw(p) for p = 0..100: what ks_fit_shape_table fills."""
    return raw(shape, np.arange(101))


def round_half_away(n, d):
    """int64(math.Round(float64(n) / float64(d))) for n >= 0, d > 0: half away
    from zero, in integers: floor((2 n + d) / (2 d))."""
    return (2 * n + d) // (2 * d)


def rtcr_scores(shape, wc, wm, cap_cpu, cap_mem, req_cpu, req_mem):
    """The node score per node: per listed resource with non-zero Allocatable
    s_r = raw(100) when requested > capacity, else raw(requested * 100 /
    capacity); then round(sum s_r w_r / sum w_r) over the resources with
    s_r > 0, 0 when there is none."""
    cap_cpu = np.asarray(cap_cpu, dtype=np.int64)
    num = np.zeros(cap_cpu.shape, dtype=np.int64)
    den = np.zeros(cap_cpu.shape, dtype=np.int64)
    for w, cap, req in ((wc, cap_cpu, req_cpu), (wm, cap_mem, req_mem)):
        if w == 0:  # not listed
            continue
        cap = np.asarray(cap, dtype=np.int64)
        req = np.asarray(req, dtype=np.int64)
        safe = np.where(cap == 0, 1, cap)
        util = np.where(req > cap, 100, req * 100 // safe)  # non-negative: // is Go's truncation
        s = np.where(cap == 0, 0, raw(shape, util))
        num += np.where(s > 0, s * w, 0)
        den += np.where(s > 0, w, 0)
    return np.where(den == 0, 0, round_half_away(num, np.where(den == 0, 1, den))).astype(np.int64)


class RtcrReference(FitReference):
    """FitReference under RequestedToCapacityRatio: strategy = (shape, wc, wm),
    or a (type, wc, wm) of fit_reference for the other two types."""

    def plugin_scores(self, pod_ptr):
        if isinstance(self.strategy[0], str):
            return super().plugin_scores(pod_ptr)
        shape, wc, wm = self.strategy
        sc = scores_np(self.oracle.plugin_scores(pod_ptr), self.capacity)
        st = self.states()
        _, _, zc, zm = pod_requests(pod_ptr)
        fit = rtcr_scores(shape, wc, wm, st["alloc_cpu"], st["alloc_mem"], st["nz_cpu"] + zc, st["nz_mem"] + zm)
        feas = sc["status"] == -1
        sc["total_score"] = np.where(feas, sc["total_score"] - self.w_fit * sc["least_allocated"] + self.w_fit * fit,
                                     sc["total_score"])
        sc["least_allocated"] = np.where(feas, fit, sc["least_allocated"])
        return sc
