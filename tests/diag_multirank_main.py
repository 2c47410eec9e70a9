"""ks_diagnose on two in-process ranks (run as a subprocess by
tests/test_gpu_diag.py, as tests/chain_multirank_main.py is by its families):
two contexts of world_size 2 share an in-process communicator, each driven by
its own thread; a third, one-rank context holds the same cache.  Multi-rank
contexts replicate the node table for the one-pod path, so each rank's
diagnosis of every pod must equal the one-rank context's (and, for the
geometry cluster, the closed-form answer).

Prints one JSON line: {"ok": true, "diagnosed": pods, "reasons": distinct reasons seen} or
{"ok": false, "error": ...}.
"""
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("k8s-1m_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import diag_cases as DC  # noqa: E402
from ksched import Scheduler  # noqa: E402
from ksched.objects import Arena  # noqa: E402
from test_gpu_diag import geometry_nodes, geometry_pod, geometry_want, u32  # noqa: E402

CASES = ["taint_first_in_node_order", "fit_every_reason_at_once", "prefilter_result", "node_affinity_conflict",
         "spread_two_constraints_first_decides", "ipa_first_failing_check_is_reported", "node_unschedulable",
         "spread_min_domains", "ipa_existing_pods_anti_affinity"]


def clusters():
    """[(capacity, setup(scheduler), pod, closed-form answer or None)]"""
    out = []
    for name in CASES:
        nodes, bound, pod, _ = DC.CASES[name]()

        def setup(s, nodes=nodes, bound=bound):
            s.upsert_nodes(nodes, list(range(len(nodes))))
            if bound:
                s.add_pods([p for p, _ in bound], [sl for _, sl in bound])
        out.append((len(nodes), setup, pod, None))
    slots = list(range(1025))
    a = Arena()
    arr = geometry_nodes(slots, a)
    out.append((len(slots), lambda s: s.upsert_nodes_raw(arr, u32(slots), len(slots)), geometry_pod(), geometry_want(slots)))
    return out


def main():
    world = 2
    diagnosed, reasons = 0, set()
    for cap, setup, pod, closed in clusters():
        ranks = [Scheduler(cap, device=0, world_size=world, rank=r) for r in range(world)]
        Scheduler.comm_init_local(ranks)
        single = Scheduler(cap, device=0)
        for s in ranks + [single]:
            setup(s)
        want = single.diagnose(pod)
        got, errs = [None] * world, []

        def drive(r):
            try:
                got[r] = ranks[r].diagnose(pod)
                ranks[r].allreduce_max([float(r)])  # host barrier through the group
            except Exception as e:  # noqa: BLE001 -- reported to the parent
                errs.append(f"rank {r}: {e!r}")

        th = [threading.Thread(target=drive, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=60)
        if any(t.is_alive() for t in th):
            return {"ok": False, "error": "a rank thread did not finish in 60 s"}
        if errs:
            return {"ok": False, "error": "; ".join(errs)}
        for r in range(world):
            if got[r] != want:
                return {"ok": False, "error": f"{pod.name}: rank {r} answers {got[r]}, one rank {want}"}
        if closed is not None and any(getattr(want, k) != v for k, v in closed.items()):
            return {"ok": False, "error": f"geometry: {want} is not {closed}"}
        diagnosed += 1
        reasons |= set(want.reasons)
        for s in ranks + [single]:
            s.close()
    return {"ok": True, "diagnosed": diagnosed, "reasons": len(reasons)}


if __name__ == "__main__":
    print(json.dumps(main()), flush=True)
