"""ks_diagnose_pods on two in-process ranks (run as a subprocess by
tests/test_gpu_diag_pods.py, as tests/diag_multirank_main.py is): two contexts
of world_size 2 share an in-process communicator, each driven by its own
thread; a third, one-rank context holds the same cache.  Each rank answers
from its own replica of the node table, so its diagnose_many of a list must
equal the one-rank context's diagnose of every pod of the list.

Prints one JSON line: {"ok": true, "diagnosed": pods, "kernel_pods": ..., "chain_pods": ...} or
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
from ksched.objects import Arena, Container, Pod, Toleration  # noqa: E402
from test_gpu_diag import geometry_nodes, geometry_pod, u32  # noqa: E402

CASES = ["taint_first_in_node_order", "fit_every_reason_at_once", "prefilter_result", "node_affinity_conflict",
         "spread_two_constraints_first_decides", "ipa_first_failing_check_is_reported"]
Mi = 1 << 20


def plain_pods(m):
    out = [Pod(f"q{i}", containers=[Container({"cpu": 100 + i, "memory": 128 * Mi})],
               tolerations=[Toleration("a", "Exists")] if i % 2 else []) for i in range(m)]
    return out + [geometry_pod()]


def clusters():
    """[(capacity, setup(scheduler), pods)]"""
    out = []
    for name in CASES:
        nodes, bound, pod, _ = DC.CASES[name]()

        def setup(s, nodes=nodes, bound=bound):
            s.upsert_nodes(nodes, list(range(len(nodes))))
            if bound:
                s.add_pods([p for p, _ in bound], [sl for _, sl in bound])
        out.append((len(nodes), setup, [pod] + plain_pods(3) + [pod]))
    slots = list(range(1025))
    a = Arena()
    arr = geometry_nodes(slots, a)
    spread = DC.CASES["spread_two_constraints_first_decides"]()[2]
    out.append((len(slots), lambda s: s.upsert_nodes_raw(arr, u32(slots), len(slots)), plain_pods(70) + [spread]))
    return out


def main():
    world = 2
    diagnosed = kernel_pods = chain_pods = 0
    for cap, setup, pods in clusters():
        ranks = [Scheduler(cap, device=0, world_size=world, rank=r) for r in range(world)]
        Scheduler.comm_init_local(ranks)
        single = Scheduler(cap, device=0)
        for s in ranks + [single]:
            setup(s)
        want = [single.diagnose(p) for p in pods]
        got, ctr, errs = [None] * world, [None] * world, []

        def drive(r):
            try:
                got[r] = ranks[r].diagnose_many(pods)
                ctr[r] = ranks[r].diagnose_pods_counters()
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
            for i, (g, w) in enumerate(zip(got[r], want)):
                if g != w:
                    return {"ok": False, "error": f"{pods[i].name}: rank {r} answers {g}, one rank {w}"}
        if single.diagnose_many(pods) != want:
            return {"ok": False, "error": "the one-rank context's diagnose_many differs from its diagnose"}
        diagnosed += len(pods)
        kernel_pods += ctr[0][0]
        chain_pods += ctr[0][1]
        for s in ranks + [single]:
            s.close()
    return {"ok": True, "diagnosed": diagnosed, "kernel_pods": kernel_pods, "chain_pods": chain_pods}


if __name__ == "__main__":
    print(json.dumps(main()), flush=True)
