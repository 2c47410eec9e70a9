"""ks_batch_forget on two ranks (run as one subprocess by
tests/test_gpu_forget.py, as tests/chain_multirank_main.py is by its families):
two contexts of world_size 2 share an in-process communicator, each driven by
its own thread.  Both ranks schedule a batch, both forget the same list, both
schedule the next batch; a one-rank twin is fed the same nodes and batches and
forgets the same pods through ks_pods_remove.  Every rank's results and node
states must equal the twin's.

The batches hold pods the round kernels shard over the ranks and pods of the
one-pod chain, which runs replicated (tests/forget_workloads.py chain_batch).
Every context lists the extended resources in its scoring configuration
(forget_workloads.LISTED), so the second batch's scores -- and with them its
results -- read the Requested columns the forget wrote.

Prints one JSON line: {"ok": true, ...} or {"ok": false, "error": ...}.
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

import forget_workloads as W  # noqa: E402
from helpers import res_array, states_np  # noqa: E402
from ksched import Scheduler  # noqa: E402
from ksched.objects import Arena, nodes_array, pods_array  # noqa: E402


def main():
    cap, world, P = 130, 2, 64
    a = Arena()
    na, k = nodes_array(W.chain_nodes(cap), a)
    sl = W.u32(range(k))
    batches = [pods_array(W.chain_batch(51 + i, f"m{i}", plain=60)[0], a) for i in range(2)]

    # the one-rank twin: ks_pods_remove with the pods and the slots of their results
    twin = Scheduler(cap, device=0, pods_per_round=P, **W.LISTED)
    twin.upsert_nodes_raw(na, sl, k)
    pa, m = batches[0]
    want = [res_array(twin.schedule_raw(pa, m), m)]
    lost = W.seven_eighths(random.Random(52), want[0])
    assert twin.lib.ks_pods_remove(twin.ctx, W.subset(pa, lost), W.u32(want[0]["node_index"][lost]), len(lost)) == 0
    mid = states_np(twin.lib.ks_node_states, twin.ctx, cap)
    want.append(res_array(twin.schedule_raw(*batches[1]), batches[1][1]))
    end = states_np(twin.lib.ks_node_states, twin.ctx, cap)
    twin.close()

    ranks = [Scheduler(cap, device=0, pods_per_round=P, world_size=world, rank=r, **W.LISTED) for r in range(world)]
    Scheduler.comm_init_local(ranks)
    for s in ranks:
        s.upsert_nodes_raw(na, sl, k)
    out = [{} for _ in range(world)]
    errs = []

    def drive(r):
        try:
            s = ranks[r]
            held = []
            for i, (pb, mb) in enumerate(batches):
                b = s.prepare(pb, mb)
                held.append(b)
                s.run(b)
                out[r][f"res{i}"] = res_array(s.results(b, mb), mb)
                if i == 0:
                    out[r]["skipped"] = s.forget(b, lost)
                    out[r]["ctr"] = s.forget_counters()
                    out[r]["mid"] = states_np(s.lib.ks_node_states, s.ctx, cap)
            out[r]["end"] = states_np(s.lib.ks_node_states, s.ctx, cap)
            s.allreduce_max([float(r)])  # host barrier through the group
            for b in held:
                s.free(b)
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
        o = out[r]
        for i in range(2):
            if not np.array_equal(o[f"res{i}"], want[i]):
                bad = np.nonzero(o[f"res{i}"] != want[i])[0]
                return {"ok": False, "error": f"rank {r}: batch {i}: {len(bad)} results differ from the twin's; "
                                              f"first pod {int(bad[0])}"}
        if o["skipped"] != 0 or o["ctr"][0] != len(lost) or o["ctr"][3] != 1:
            return {"ok": False, "error": f"rank {r}: skipped {o['skipped']}, counters {o['ctr']}"}
        if not np.array_equal(o["mid"], mid):
            return {"ok": False, "error": f"rank {r}: node states after the forget differ from the twin's"}
        if not np.array_equal(o["end"], end):
            return {"ok": False, "error": f"rank {r}: node states after the next batch differ from the twin's"}
    for s in ranks:
        s.close()
    return {"ok": True, "forgotten": len(lost), "forgotten_solo": int(out[0]["ctr"][2]),
            "forgotten_plain": int(out[0]["ctr"][0] - out[0]["ctr"][2]),
            "scheduled_after": int((want[1]["status"] == 0).sum())}


if __name__ == "__main__":
    print(json.dumps(main()), flush=True)
