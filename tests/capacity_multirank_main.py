"""ks_capacity_pods on two in-process ranks (run as a subprocess by
tests/test_gpu_capacity.py, as tests/diag_pods_multirank_main.py is): two
contexts of world_size 2 share an in-process communicator, each driven by its
own thread; a third, one-rank context holds the same cache.  Each rank answers
from its own replica of the node table, so its capacity_many of a list must
equal the one-rank context's capacity of every pod of the list, and the
closed form of tests/capacity_reference.py.

Prints one JSON line: {"ok": true, "answered": pods, "kernel_pods": ..., "chain_pods": ...} or
{"ok": false, "error": ...}.
"""
import json
import os
import random
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("k8s-1m_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import capacity_reference as CR  # noqa: E402
import diag_reference as R  # noqa: E402
from ksched import Scheduler  # noqa: E402
from ksched.objects import Container, Pod, Toleration  # noqa: E402

FIELDS = ("num_all_nodes", "eligible_nodes", "nodes_with_room", "max_per_node", "replicas", "bound_by")
Mi = 1 << 20


def main():
    world, n = 2, 700
    rng = random.Random(7)
    nodes = CR.rand_cluster(rng, n)
    pre, where = CR.rand_prefill(rng, n)
    pods = [Pod(f"q{i}", containers=[Container({"cpu": 100 + 10 * i, "memory": (64 + i) * Mi})],
                tolerations=[Toleration("dedicated", "Exists")] if i % 2 else [],
                node_selector={"zone": "z2"} if i % 5 == 0 else {}) for i in range(30)]
    pods += list(CR.shapes().values())
    ranks = [Scheduler(n, device=0, world_size=world, rank=r) for r in range(world)]
    Scheduler.comm_init_local(ranks)
    single = Scheduler(n, device=0)
    ref = R.DiagReference(n)
    ref.upsert(nodes, list(range(n)))
    ref.add(pre, where)
    for s in ranks + [single]:
        s.upsert_nodes(nodes, list(range(n)))
        s.add_pods(pre, where)
    flat = lambda c: tuple(getattr(c, k) for k in FIELDS)
    want = [flat(single.capacity(p)) for p in pods]
    for p, w in zip(pods, want):
        r = CR.capacity(ref, p, [CR.GPU, CR.DISK])
        if w != tuple(r[k] for k in FIELDS):
            return {"ok": False, "error": f"{p.name}: one rank answers {w}, the reference {r}"}
    got, ctr, errs = [None] * world, [None] * world, []

    def drive(r):
        try:
            got[r] = ranks[r].capacity_many(pods)
            ctr[r] = ranks[r].capacity_counters()
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
            if flat(g) != w:
                return {"ok": False, "error": f"{pods[i].name}: rank {r} answers {flat(g)}, one rank {w}"}
    for s in ranks + [single]:
        s.close()
    return {"ok": True, "answered": len(pods), "kernel_pods": ctr[0][0], "chain_pods": ctr[0][1]}


if __name__ == "__main__":
    print(json.dumps(main()), flush=True)
