"""The NodePorts stream on a two-rank world (run as a subprocess by
tests/test_gpu_ports.py, as tests/ba_multirank_main.py is): two contexts of
world_size 2 share an in-process communicator, each driven by its own thread,
and see the same cache events; the one-pod chain runs replicated, so every rank
keeps its own dictionary and used-ports column and applies every commit.  Every
rank's results, node states and used ports must equal PortsReference's
(tests/ports_reference.py).

Prints one JSON line: {"ok": true, ...} or {"ok": false, "error": ...}.
"""
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("k8s-1m_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import ports_workloads as W  # noqa: E402
from helpers import res_array, states_np  # noqa: E402
from ksched import Scheduler  # noqa: E402
from ksched.objects import Arena, nodes_array, pods_array  # noqa: E402

P = 64


def main(cfg):
    n = cfg["n"]
    ref = W.reference_run(n)
    ns, ps = W.stream(W.SEEDS[n], n)
    a = Arena()
    na, k = nodes_array(ns, a)
    sl = W.u32(range(k))
    half = len(ps) // 2
    batches = [pods_array(ps[:half], a), pods_array(ps[half:], a)]

    world = 2
    ranks = [Scheduler(n, device=0, pods_per_round=P, world_size=world, rank=r) for r in range(world)]
    Scheduler.comm_init_local(ranks)
    for s in ranks:
        s.upsert_nodes_raw(na, sl, k)
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
    w = ref["res"]
    for r in range(world):
        got = np.concatenate(out[r])
        if not np.array_equal(got, w):
            bad = np.nonzero(got != w)[0]
            i = int(bad[0])
            return {"ok": False, "error": f"rank {r}: {len(bad)}/{len(w)} results differ; first pod {i}: "
                                          f"got {got[i]} want {w[i]}"}
        if not np.array_equal(states_np(ranks[r].lib.ks_node_states, ranks[r].ctx, n), ref["states"]):
            return {"ok": False, "error": f"rank {r}: node state differs from the reference"}
        used = [sorted(ranks[r].node_used_ports(s)) for s in range(n)]
        if used != ref["used"]:
            return {"ok": False, "error": f"rank {r}: used ports differ from the reference's mirror"}
    for s in ranks:
        s.close()
    return {"ok": True, "scheduled": int((w["status"] == 0).sum()), "port_fails": int(w["_pad"].sum())}


if __name__ == "__main__":
    print(json.dumps(main(json.loads(sys.argv[1]))), flush=True)
