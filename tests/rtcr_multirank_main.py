"""One two-rank case of libksched under RequestedToCapacityRatio (run as a
subprocess by tests/test_gpu_rtcr_spread.py, as tests/fit_multirank_main.py
is): two contexts of world_size 2 share an in-process communicator, each driven
by its own thread, both set the same weights and shape; every rank's results
and node states must equal the composed reference (tests/rtcr_reference.py).

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

import fit_workloads as W  # noqa: E402
import rtcr_workloads as R  # noqa: E402
from helpers import res_array, states_np  # noqa: E402
from ksched import Scheduler  # noqa: E402


def main(cfg):
    kind_name, name = cfg["kind_name"], cfg["name"]
    w = W.hetero_stream(kind_name)
    want, states = R.hetero_reference(kind_name, name)
    m, calls, world = w["m"], 2, 2
    want = res_array(want, m)
    ranks = [Scheduler(W.N_H, device=0, pods_per_round=W.P_H, world_size=world, rank=r) for r in range(world)]
    Scheduler.comm_init_local(ranks)
    for s in ranks:
        R.use(s, name)
        W.hetero_setup(s, w)
    cuts = [m * i // calls for i in range(calls + 1)]
    out = [[None] * calls for _ in range(world)]
    errs = []

    def drive(r):
        try:
            s = ranks[r]
            for i in range(calls):
                a, b = cuts[i], cuts[i + 1]
                out[r][i] = res_array(s.schedule_raw(W.pods_at(w["ps"].pods, a), b - a), b - a)
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
    for r in range(world):
        got = np.concatenate(out[r])
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = int(bad[0])
            return {"ok": False, "error": f"rank {r}: {len(bad)}/{m} results differ; first pod {i}: "
                                          f"got {got[i]} want {want[i]}"}
        if not np.array_equal(states_np(ranks[r].lib.ks_node_states, ranks[r].ctx, W.N_H), states):
            return {"ok": False, "error": f"rank {r}: node state differs from the reference"}
    for s in ranks:
        s.close()
    return {"ok": True, "scheduled": int((want["status"] == 0).sum())}


if __name__ == "__main__":
    print(json.dumps(main(json.loads(sys.argv[1]))), flush=True)
