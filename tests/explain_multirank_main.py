"""ks_explain on two in-process ranks (run as a subprocess by
tests/test_gpu_explain.py, as tests/diag_multirank_main.py is by its test): two
contexts of world_size 2 share an in-process communicator, each driven by its
own thread; a third, one-rank context holds the same cache.  Multi-rank
contexts replicate the node table for the one-pod path, so each rank's answer
for every pod must equal the one-rank context's, which must equal want(k) of
its own ks_plugin_scores.

Prints one JSON line: {"ok": true, "explained": pods, "candidates": records compared} or
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

import numpy as np  # noqa: E402

from ksched import Scheduler  # noqa: E402
from ksched.objects import Arena, pods_array  # noqa: E402
from test_gpu_explain import (assert_explains, explain_raw, level_nodes, level_pod, level_templates, pref_pod,  # noqa: E402
                              soften, u32)
from test_gpu_spread import rand_ipa_pod, rand_nodes, rand_pod, rand_res_nodes, rand_res_pod  # noqa: E402

K = 32


def clusters():
    """[(capacity, setup(scheduler), pods)]"""
    out = []
    a = Arena()
    slots = list(range(1025))
    arr = level_nodes(level_templates(a), slots, [(i * 37) % 100 for i in slots], a)
    out.append((1025, lambda s: s.upsert_nodes_raw(arr, u32(slots), len(slots)), [level_pod()]))
    rng = random.Random(91)
    n = 400
    nodes = soften(rng, rand_res_nodes(rng, n))
    bound = [rand_ipa_pod(rng, 10_000 + j, frac=0.3, spread_frac=0.0) for j in range(n)]
    where = [rng.randrange(n) for _ in bound]

    def setup(s):
        s.upsert_nodes(nodes, list(range(n)))
        s.add_pods(bound, where)
    pods = [pref_pod(rng, 1), rand_pod(rng, 2, spread_frac=1.0), rand_ipa_pod(rng, 3, frac=1.0), rand_res_pod(rng, 4),
            rand_res_pod(rng, 5), rand_pod(rng, 6, spread_frac=1.0), rand_ipa_pod(rng, 7, frac=1.0), pref_pod(rng, 8)]
    out.append((n, setup, pods))
    return out


def main():
    world = 2
    explained = candidates = 0
    a = Arena()
    for cap, setup, pods in clusters():
        ranks = [Scheduler(cap, device=0, world_size=world, rank=r) for r in range(world)]
        Scheduler.comm_init_local(ranks)
        single = Scheduler(cap, device=0)
        for s in ranks + [single]:
            setup(s)
        for pod in pods:
            pa, _ = pods_array([pod], a)
            try:
                assert_explains(single, pa, [K], pod.name)
            except AssertionError as e:
                return {"ok": False, "error": f"one rank, {pod.name}: {e}"}
            want = explain_raw(single, pa, K)
            got, errs = [None] * world, []

            def drive(r):
                try:
                    got[r] = explain_raw(ranks[r], pa, K)
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
                (e, slots, recs), (we, wslots, wrecs) = got[r], want
                same = bytes(e) == bytes(we) and slots == wslots and np.array_equal(recs, wrecs)
                if not same:
                    return {"ok": False, "error": f"{pod.name}: rank {r} answers {slots[:8]}, one rank {wslots[:8]}"}
            explained += 1
            candidates += len(want[1])
        for s in ranks + [single]:
            s.close()
    return {"ok": True, "explained": explained, "candidates": candidates}


if __name__ == "__main__":
    print(json.dumps(main()), flush=True)
