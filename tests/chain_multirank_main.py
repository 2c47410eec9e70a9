"""One two-rank case of a one-pod-chain family (run as a subprocess by the
family's GPU test, as tests/multirank_main.py is by tests/test_gpu_multirank.py):
two contexts of world_size 2 share an in-process communicator, each driven by
its own thread, both set up alike and fed the same batches; every rank's
results and node states must equal the family's reference.

The argument is {"family": ..., ...}; the family's workload module answers
two_rank_case(cfg) with
  capacity, pods_per_round: of each rank's context;
  setup(scheduler): the family's configuration and the cache events before the batches;
  batches: [(ks_pod array, count)], scheduled in order;
  want, states: the reference's results of all batches and its node states;
  check(scheduler) (optional): what else must hold on every rank -- an error text, or None;
  report (optional): fields for the result line.

Prints one JSON line: {"ok": true, ...} or {"ok": false, "error": ...}.
"""
import importlib
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("k8s-1m_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

from helpers import res_array, states_np  # noqa: E402
from ksched import Scheduler  # noqa: E402

FAMILIES = {"fit": "fit_workloads", "rtcr": "rtcr_workloads", "xfit": "xfit_workloads", "ba": "ba_workloads",
            "ports": "ports_workloads", "chain_edges": "chain_edge_cases"}


def main(cfg):
    case = importlib.import_module(FAMILIES[cfg["family"]]).two_rank_case(cfg)
    cap, batches, want = case["capacity"], case["batches"], case["want"]
    world = 2
    ranks = [Scheduler(cap, device=0, pods_per_round=case["pods_per_round"], world_size=world, rank=r)
             for r in range(world)]
    Scheduler.comm_init_local(ranks)
    for s in ranks:
        case["setup"](s)
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
    for r in range(world):
        got = np.concatenate(out[r])
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = int(bad[0])
            return {"ok": False, "error": f"rank {r}: {len(bad)}/{len(want)} results differ; first pod {i}: "
                                          f"got {got[i]} want {want[i]}"}
        if not np.array_equal(states_np(ranks[r].lib.ks_node_states, ranks[r].ctx, cap), case["states"]):
            return {"ok": False, "error": f"rank {r}: node state differs from the reference"}
        err = case["check"](ranks[r]) if "check" in case else None
        if err:
            return {"ok": False, "error": f"rank {r}: {err}"}
    for s in ranks:
        s.close()
    return dict({"ok": True, "scheduled": int((want["status"] == 0).sum())}, **case.get("report", {}))


if __name__ == "__main__":
    print(json.dumps(main(json.loads(sys.argv[1]))), flush=True)
