#!/usr/bin/env python3
"""Per-pod wall time of ks_capacity_pods beside ks_diagnose_pods
of the same pods -- one pass of the same shape without the quotients and the
64-bit sums -- in one process on one build, the two calls alternating.

Two 1M-node clusters, as tools/diag_pods_rate.py builds them: the bench's C3
cluster (heterogeneous nodes, prefilled twice) and the C4 cluster (labels and
taints).  Lists:

  resource   distinct resource-only pods on C3 (no two compile alike)
  label      the C4 stream's label / taint pods on C4
  single     one ks_capacity_pod call without and with per_node beside one
             ks_diagnose, on C3
  fill       the "instead of" figure: replicas of one small shape placed by
             ks_schedule on a scratch context of --fill-nodes nodes until the
             first unschedulable result, beside one ks_capacity_pod there; the
             fill's time is measured at that size and NOT extrapolated here

--reps timed repetitions after one untimed; every call ends in a device
synchronise, so the host clock around it is its time.  One JSON line per
measurement, and all of them in profiles/capacity_rate.json.

  python3 tools/capacity_rate.py
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/capacity_rate.py --reps 3 --sizes 4096 --lists resource,label
      # the kernels' own times: one launch of n / 64 groups per call

Reported, not targeted.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "k8s-1m_amd"))

from ksched import Scheduler, _abi, synth  # noqa: E402
from ksched.objects import Arena, Container, Pod, Toleration, pods_array  # noqa: E402

Mi = 1 << 20
KWOK = [Toleration("kwok.x-k8s.io/node", "Equal", "fake", "NoSchedule")]
RESULTS = []


def us(xs):
    return {"min": round(min(xs), 2), "median": round(statistics.median(xs), 2), "max": round(max(xs), 2)}


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


def pod_at(arr, j):
    return C.cast(C.addressof(arr.contents if hasattr(arr, "contents") else arr) + j * C.sizeof(_abi.KsPod),
                  C.POINTER(_abi.KsPod))


def measure(s, name, arr, n, reps):
    lib, ctx = s.lib, s.ctx
    dout = (_abi.KsPodDiagnosis * n)()
    cap = n * _abi.DIAG_MAX_REASONS
    rows = (_abi.KsReason * cap)()
    total = C.c_uint32()
    cout = (_abi.KsPodCapacity * n)()
    first = pod_at(arr, 0)
    t_diag, t_cap = [], []
    for rep in range(reps + 1):  # the first round warms both calls up and is not timed
        t0 = time.perf_counter()
        st = lib.ks_diagnose_pods(ctx, first, n, dout, rows, cap, C.byref(total))
        t1 = time.perf_counter()
        assert st == 0, lib.ks_last_error(ctx)
        st = lib.ks_capacity_pods(ctx, first, n, cout)
        t2 = time.perf_counter()
        assert st == 0, lib.ks_last_error(ctx)
        if rep:
            t_diag.append(1e6 * (t1 - t0) / n)
            t_cap.append(1e6 * (t2 - t1) / n)
    # the two calls agree where they overlap
    assert all(cout[j].c.nodes_with_room == dout[j].d.feasible_nodes for j in range(n))
    dp, cp = us(t_diag), us(t_cap)
    emit({"list": name, "n": n, "reps": reps, "diagnose_us_per_pod": dp, "capacity_us_per_pod": cp,
          "capacity_median_over_diagnose_median": round(cp["median"] / dp["median"], 2),
          "capacity_counters": s.capacity_counters(), "diagnose_counters": s.diagnose_pods_counters(),
          "replicas_last": int(cout[n - 1].c.replicas), "eligible_last": int(cout[n - 1].c.eligible_nodes)})


def measure_single(s, arr, reps):
    import numpy as np

    lib, ctx = s.lib, s.ctx
    d, cnt = _abi.KsDiagnosis(), C.c_uint32()
    one = (_abi.KsReason * _abi.DIAG_MAX_REASONS)()
    c = _abi.KsCapacity()
    pn = np.zeros(int(s.capacity), dtype=np.uint32)
    ptr = pn.ctypes.data_as(C.POINTER(C.c_uint32))
    pod = pod_at(arr, 0)
    t = {"diagnose": [], "capacity": [], "capacity_per_node": []}
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        assert lib.ks_diagnose(ctx, pod, C.byref(d), one, _abi.DIAG_MAX_REASONS, C.byref(cnt)) == 0
        t1 = time.perf_counter()
        assert lib.ks_capacity_pod(ctx, pod, C.byref(c), None) == 0
        t2 = time.perf_counter()
        assert lib.ks_capacity_pod(ctx, pod, C.byref(c), ptr) == 0
        t3 = time.perf_counter()
        if rep:
            t["diagnose"].append(1e6 * (t1 - t0))
            t["capacity"].append(1e6 * (t2 - t1))
            t["capacity_per_node"].append(1e6 * (t3 - t2))
    assert int(pn.astype(np.uint64).sum()) == c.replicas and c.nodes_with_room == d.feasible_nodes
    emit({"list": "single", "reps": reps, "us_per_call": {k: us(v) for k, v in t.items()},
          "replicas": int(c.replicas), "nodes_with_room": int(c.nodes_with_room)})


def measure_fill(nodes):
    """One fill of a small shape by ks_schedule on a scratch context, beside the closed form there."""
    s = cluster(synth.HETERO, nodes, True)
    pod = Pod("fill", tolerations=KWOK, containers=[Container({"cpu": 2000, "memory": 4096 * Mi})])
    keep = Arena()
    batch = 4096
    arr, _ = pods_array([pod] * batch, keep)
    t0 = time.perf_counter()
    want = s.capacity(pod)
    t1 = time.perf_counter()
    placed = 0
    while True:
        raw = s.schedule_raw(arr, batch)
        k = sum(1 for i in range(batch) if raw[i].status == 0)
        placed += k
        if k < batch:
            break
    t2 = time.perf_counter()
    assert placed == want.replicas, (placed, want.replicas)
    emit({"list": "fill", "nodes": nodes, "replicas": placed, "capacity_call_us": round(1e6 * (t1 - t0), 1),
          "fill_by_ks_schedule_ms": round(1e3 * (t2 - t1), 1),
          "fill_pods_per_s": round(placed / (t2 - t1)) if t2 > t1 else None,
          "note": "measured at this node count and shape; not extrapolated"})
    s.close()


def cluster(kind, nodes, fill_twice):
    s = Scheduler(nodes)
    nd = synth.nodes(kind, nodes, 1)
    s.upsert_nodes_raw(nd.nodes, synth.slot_array(nodes), nodes)
    for seed in (3, 4) if fill_twice else (3,):
        pre = synth.prefill(kind, nodes, 1, seed, 0.5)
        assert s.lib.ks_pods_add(s.ctx, pre.pods, pre.slot_ptr, pre.n_pods) == 0, s.lib.ks_last_error(s.ctx)
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--lists", default="resource,label,single,fill")
    ap.add_argument("--fill-nodes", type=int, default=20_000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "capacity_rate.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    lists = a.lists.split(",")
    top = max(sizes)
    keep = Arena()
    if {"resource", "single"} & set(lists):
        with cluster(synth.HETERO, a.nodes, True) as s:
            pods = [Pod(f"r{i}", tolerations=KWOK, containers=[Container({"cpu": 100 + 7 * i, "memory": (64 + i % 97) * Mi})])
                    for i in range(top)]
            arr, _ = pods_array(pods, keep)
            if "resource" in lists:
                for n in sizes:
                    measure(s, "resource", arr, n, a.reps)
            if "single" in lists:
                measure_single(s, arr, a.reps)
    if "label" in lists:
        with cluster(synth.LABELED, a.nodes, False) as s:
            lp = synth.pods(synth.LABELED, top, 7)
            measure(s, "label", lp.pods, min(256, top), a.reps)
    if "fill" in lists:
        measure_fill(a.fill_nodes)
    if a.out:
        Path(a.out).write_text(json.dumps({"tool": "tools/capacity_rate.py", "nodes": a.nodes, "reps": a.reps,
                                           "results": RESULTS}, indent=1) + "\n")


if __name__ == "__main__":
    main()
