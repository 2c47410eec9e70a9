"""One two-rank case of libksched under a balanced list (run as a subprocess by
tests/test_gpu_ba.py, as tests/xfit_multirank_main.py is): two contexts of
world_size 2 share an in-process communicator, each driven by its own thread,
both set the same strategy and list and see the same cache events; the one-pod
chain runs replicated.  Every rank's results and node states must equal the
composed reference (tests/ba_reference.py).

Prints one JSON line: {"ok": true, ...} or {"ok": false, "error": ...}.
"""
import ctypes as C
import json
import os
import random
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("k8s-1m_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import ba_workloads as W  # noqa: E402
import xfit_workloads as X  # noqa: E402
from ba_reference import BaReference  # noqa: E402
from helpers import res_array, states_np  # noqa: E402
from ksched import Scheduler  # noqa: E402
from ksched.objects import Arena, nodes_array, pods_array  # noqa: E402

P = 64


def main(cfg):
    strategy, extended, balanced = W.CASES[cfg["case"]]
    n, cap = X.SIZES["small"]
    rng = random.Random(93)
    a = Arena()
    slots = X.spread_slots(n, cap)
    na, k = nodes_array(X.xfit_nodes(rng, n), a)
    sl = (C.c_uint32 * k)(*slots)
    pre = X.bound_pods(rng, n // 2, 60_000)
    ba, nb = pods_array(pre, a)
    bs = (C.c_uint32 * nb)(*[rng.choice(slots) for _ in pre])
    batches = [pods_array([X.xfit_pod(rng, b * 1000 + j) for j in range(60)], a) for b in range(2)]

    ref = BaReference(cap, strategy, extended, balanced)
    ref.upsert(na, sl, k)
    ref.add_pods(ba, bs, nb)
    want = [res_array(ref.schedule(pa, m), m) for pa, m in batches]
    states = ref.states()
    ref.close()

    world = 2
    ranks = [Scheduler(cap, device=0, pods_per_round=P, world_size=world, rank=r) for r in range(world)]
    Scheduler.comm_init_local(ranks)
    for s in ranks:
        W.configure(s, cfg["case"])
        s.upsert_nodes_raw(na, sl, k)
        assert s.lib.ks_pods_add(s.ctx, ba, bs, nb) == 0
    out = [[None] * len(batches) for _ in range(world)]
    errs = []

    def drive(r):
        try:
            s = ranks[r]
            for i, (pa, m) in enumerate(batches):
                out[r][i] = res_array(s.schedule_raw(pa, m), m)
            s.allreduce_max([float(r)])  # host barrier through the group
        except Exception as e:  # noqa: BLE001 -- reported to the parent
            errs.append(f"rank {r}: {e!r}")

    th = [threading.Thread(target=drive, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=100)
    if any(t.is_alive() for t in th):
        return {"ok": False, "error": "a rank thread did not finish in 100 s"}
    if errs:
        return {"ok": False, "error": "; ".join(errs)}
    w = np.concatenate(want)
    for r in range(world):
        got = np.concatenate(out[r])
        if not np.array_equal(got, w):
            bad = np.nonzero(got != w)[0]
            i = int(bad[0])
            return {"ok": False, "error": f"rank {r}: {len(bad)}/{len(w)} results differ; first pod {i}: "
                                          f"got {got[i]} want {w[i]}"}
        if not np.array_equal(states_np(ranks[r].lib.ks_node_states, ranks[r].ctx, cap), states):
            return {"ok": False, "error": f"rank {r}: node state differs from the reference"}
    for s in ranks:
        s.close()
    return {"ok": True, "scheduled": int((w["status"] == 0).sum())}


if __name__ == "__main__":
    print(json.dumps(main(json.loads(sys.argv[1]))), flush=True)
