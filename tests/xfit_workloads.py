"""Workloads of the tests of NodeResourcesFit strategies that list extended
resources: shared by the CPU test of the reference (tests/test_xfit_reference.py,
which also checks that listing the resource changes these streams' schedules)
and the GPU tests (tests/test_gpu_xfit.py).  A stream is driven through a pair
object with the interface of tests/test_gpu_spread.py Pair (upsert / delete /
add / schedule / dump_equal / states_equal), as fit_workloads.chain_stream is.
"""
import ctypes as C
import random

import numpy as np

from fit_reference import LEAST, MOST
from helpers import res_array
from ksched.objects import Arena, Container, Pod, nodes_array, pods_array
from rtcr_reference import SHAPES
from xfit_reference import GPU, HUGE, NIC, XfitReference

Gi, Mi = 1 << 30, 1 << 20

# (strategy of fit_reference / rtcr_reference, extended {name: weight})
CASES = {
    "most-1-1-gpu3": ((MOST, 1, 1), {GPU: 3}),
    "least-gpu1": ((LEAST, 0, 0), {GPU: 1}),                      # the extended resource alone
    "least-2-0-nic1-gpu5": ((LEAST, 2, 0), {NIC: 1, GPU: 5}),
    "binpack-1-1-gpu3": ((SHAPES["binpack"], 1, 1), {GPU: 3}),
    "peaked-1-1-gpu2-nic1": ((SHAPES["peaked"], 1, 1), {GPU: 2, NIC: 1}),  # table scores of 0: the divisor varies
    "falling-1-0-gpu1-nic3": ((SHAPES["falling"], 1, 0), {GPU: 1, NIC: 3}),
}
# nodes, capacity: nodes spread over the whole capacity -- a partial last
# workgroup of 1,024 and empty lanes in every wave
SIZES = {"small": (300, 512), "large": (2500, 4096)}


def spread_slots(n, cap):
    return [i * cap // n for i in range(n)]


def set_strategy(s, strategy, extended):
    """A case on a ksched.Scheduler."""
    kind, wc, wm = strategy
    w = {k: v for k, v in (("cpu", wc), ("memory", wm)) if v}
    w.update(extended)
    if isinstance(kind, str):
        s.set_fit_strategy(kind, w)
    else:
        s.set_fit_strategy("RequestedToCapacityRatio", w, kind)


def xfit_nodes(rng, n, slot0=0):
    from test_gpu_spread import IMAGES, rand_nodes
    out = rand_nodes(rng, n, 6, slot0)
    for nd in out:
        if rng.random() < 0.75:
            nd.extended[GPU] = rng.choice([2, 4, 8, 8])
        if rng.random() < 0.6:
            nd.extended[NIC] = rng.randint(1, 4)
        if rng.random() < 0.5:
            nd.extended[HUGE] = rng.choice([256, 1024]) * Mi
        if rng.random() < 0.3:
            nd.extended["ephemeral-storage"] = rng.choice([50, 20 * 1024]) * Gi  # unlisted: beyond 2^44 is fine
        nd.images = rng.sample(IMAGES, rng.randint(0, 3))
    return out


def xfit_pod(rng, j):
    """One pod of the mixed stream; its kind by j so every kind appears in
    every batch."""
    from test_gpu_spread import IMAGES, rand_ipa_pod, rand_pod
    kind = j % 10
    if kind == 0:
        return rand_pod(rng, j, spread_frac=0.0)  # nothing extended: the round kernels, the bypass
    if kind == 1:
        p = rand_pod(rng, j, spread_frac=1.0)  # spread constraints, nothing extended: the chain's bypass
        return p
    if kind == 6:
        p = rand_pod(rng, j, spread_frac=1.0)
    elif kind == 7:
        p = rand_ipa_pod(rng, j, frac=1.0, spread_frac=0.0)
    else:
        p = rand_pod(rng, j, spread_frac=0.0)
    c = p.containers[0]
    c.requests[GPU] = rng.choice([1, 1, 2, 4])
    if kind == 3:
        c.requests[NIC] = 1
    elif kind == 4:
        c.requests[HUGE] = 256 * Mi  # unlisted: filter only
    elif kind == 5:
        del c.requests[GPU]
        c.requests[NIC] = rng.choice([1, 2])
    elif kind == 8:
        c.image = rng.choice(IMAGES)[0]
    elif kind == 9:
        # an init container's maximum and a sidecar's sum
        p.init_containers = [Container({GPU: rng.choice([1, 2])}, restart_policy_always=True),
                             Container({GPU: rng.choice([2, 4]), NIC: 1})]
    return p


def bound_pods(rng, n_pods, j0):
    out = []
    for j in range(n_pods):
        req = {"cpu": rng.randrange(1, 20) * 100, "memory": rng.randrange(1, 32) * 128 * Mi}
        if rng.random() < 0.5:
            req[GPU] = rng.choice([1, 2, 6])  # also on nodes with fewer (or none): Requested above Allocatable
        if rng.random() < 0.2:
            req[NIC] = 1
        out.append(Pod(f"b{j0 + j}", containers=[Container(req)], labels={"app": rng.choice(["web", "api"])}))
    return out


BATCHES, PER_BATCH = 3, 70


def sweep_stream(x, seed, size, dumps=True):
    """Three batches of the mixed stream over prefilled nodes; nodes fill up,
    so later pods fail NodeResourcesFit on the extended resource.  Returns
    the pods and the results of every batch."""
    n, cap = SIZES[size]
    rng = random.Random(seed)
    slots = spread_slots(n, cap)
    x.upsert(xfit_nodes(rng, n), slots)
    pre = bound_pods(rng, n // 2, 50_000)
    x.add(pre, [rng.choice(slots) for _ in pre])
    pods, res = [], []
    for b in range(BATCHES):
        batch = [xfit_pod(rng, b * 1000 + j) for j in range(PER_BATCH)]
        res.append(x.schedule(batch, f"sweep seed {seed} {size} batch {b}"))
        pods += batch
        x.states_equal(f"sweep seed {seed} {size} batch {b}")
        if dumps:
            x.dump_equal(xfit_pod(rng, 90_002 + 10 * b), f"sweep seed {seed} {size}: dump of a requesting pod {b}")
            x.dump_equal(xfit_pod(rng, 90_001 + 10 * b), f"sweep seed {seed} {size}: dump of a spread pod, bypass {b}")
    x.dump_equal(xfit_pod(rng, 95_000), f"sweep seed {seed} {size}: dump of a plain pod")
    return pods, res


def replicated_case(seed, make_ref, configure):
    """A two-rank case (tests/chain_multirank_main.py) at the small size: prefilled nodes, then two batches of
    the mixed stream, which the chain runs replicated.  make_ref(capacity) is the case's reference,
    configure(scheduler) sets its strategy and lists on a rank."""
    n, cap = SIZES["small"]
    rng = random.Random(seed)
    a = Arena()
    slots = spread_slots(n, cap)
    na, k = nodes_array(xfit_nodes(rng, n), a)
    sl = (C.c_uint32 * k)(*slots)
    pre = bound_pods(rng, n // 2, 60_000)
    ba, nb = pods_array(pre, a)
    bs = (C.c_uint32 * nb)(*[rng.choice(slots) for _ in pre])
    batches = [pods_array([xfit_pod(rng, b * 1000 + j) for j in range(60)], a) for b in range(2)]
    ref = make_ref(cap)
    ref.upsert(na, sl, k)
    ref.add_pods(ba, bs, nb)
    want = np.concatenate([res_array(ref.schedule(pa, m), m) for pa, m in batches])
    states = ref.states()
    ref.close()

    def setup(s):
        configure(s)
        s.upsert_nodes_raw(na, sl, k)
        assert s.lib.ks_pods_add(s.ctx, ba, bs, nb) == 0

    return dict(capacity=cap, pods_per_round=64, setup=setup, batches=batches, want=want, states=states, arena=a)


def two_rank_case(cfg):
    strategy, extended = CASES[cfg["case"]]
    return replicated_case(91, lambda cap: XfitReference(cap, strategy, extended),
                           lambda s: set_strategy(s, strategy, extended))


def requests_extended(pod, names):
    cs = list(pod.containers) + list(pod.init_containers)
    return any(c.requests.get(nm, 0) > 0 for c in cs for nm in names)
