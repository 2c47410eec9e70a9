#!/usr/bin/env python3
"""Per-pod wall time of ks_diagnose_pods beside a loop of
ks_diagnose over the same pods, in one process on one build.

Two 1M-node clusters, as tools/diag_rate.py builds them: the bench's C3
cluster (heterogeneous nodes prefilled below 50 % cpu, then a second prefill)
and the C4 cluster (labels and taints).  Four pod lists:

  resource   distinct resource-only pods on C3 (no two compile alike)
  label      the C4 stream's label / taint pods on C4
  replicas   one deployment's identical replicas on C3
  per_pod    spread pods on C3: every one takes ks_diagnose's own pass

For every list and n in --sizes the two ways alternate, --reps timed
repetitions each after one untimed; every call ends in a device synchronise,
so the host clock around it is its time.  One JSON line per (list, n):
microseconds per pod (min / median / max over the repetitions) both ways,
their ratio, and ks_debug_diagnose_pods' counters of the last call.

  python3 tools/diag_pods_rate.py
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/diag_pods_rate.py --reps 3 --sizes 4096 --lists resource,label
      # the multi-pod kernel's own time: one launch of n / 64 groups per call

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
# every synthetic node carries the kwok taint and the synthetic pods tolerate it; so do the pods made here
KWOK = [Toleration("kwok.x-k8s.io/node", "Equal", "fake", "NoSchedule")]


def us(xs):
    return {"min": round(min(xs), 2), "median": round(statistics.median(xs), 2), "max": round(max(xs), 2)}


def measure(s, name, arr, n, reps):
    """arr: a ks_pod array of at least n pods."""
    lib, ctx = s.lib, s.ctx
    d, cnt = _abi.KsDiagnosis(), C.c_uint32()
    one = (_abi.KsReason * _abi.DIAG_MAX_REASONS)()
    out = (_abi.KsPodDiagnosis * n)()
    cap = n * _abi.DIAG_MAX_REASONS
    rows = (_abi.KsReason * cap)()
    total = C.c_uint32()
    at = [C.cast(C.addressof(arr.contents if hasattr(arr, "contents") else arr) + j * C.sizeof(_abi.KsPod),
                 C.POINTER(_abi.KsPod)) for j in range(n)]
    t_loop, t_batch = [], []
    for rep in range(reps + 1):  # the first round warms both paths up and is not timed
        t0 = time.perf_counter()
        for j in range(n):
            st = lib.ks_diagnose(ctx, at[j], C.byref(d), one, _abi.DIAG_MAX_REASONS, C.byref(cnt))
            assert st == 0, lib.ks_last_error(ctx)
        t1 = time.perf_counter()
        st = lib.ks_diagnose_pods(ctx, at[0], n, out, rows, cap, C.byref(total))
        t2 = time.perf_counter()
        assert st == 0, lib.ks_last_error(ctx)
        if rep:
            t_loop.append(1e6 * (t1 - t0) / n)
            t_batch.append(1e6 * (t2 - t1) / n)
    # the last pod both ways: the same diagnosis
    lo = out[n - 1].first_reason
    assert [(one[i].reason, one[i].count) for i in range(cnt.value)] == \
        [(rows[lo + i].reason, rows[lo + i].count) for i in range(out[n - 1].d.n_reasons)]
    ctr = s.diagnose_pods_counters()
    lp, bp = us(t_loop), us(t_batch)
    print(json.dumps({"list": name, "n": n, "reps": reps, "loop_us_per_pod": lp, "batch_us_per_pod": bp,
                      "loop_median_over_batch_median": round(lp["median"] / bp["median"], 2),
                      "batch_median_below_loop_min": bp["median"] < lp["min"],
                      "loop_spread_us_per_pod": round(lp["max"] - lp["min"], 2),
                      "counters": ctr, "feasible_nodes_last": int(d.feasible_nodes)}), flush=True)


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
    ap.add_argument("--sizes", default="1,16,256,4096")
    ap.add_argument("--lists", default="resource,label,replicas,per_pod")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    lists = a.lists.split(",")
    top = max(sizes)
    keep = Arena()
    if {"resource", "replicas", "per_pod"} & set(lists):
        with cluster(synth.HETERO, a.nodes, True) as s:
            if "resource" in lists:
                pods = [Pod(f"r{i}", tolerations=KWOK,
                            containers=[Container({"cpu": 100 + 7 * i, "memory": (64 + i % 97) * Mi})])
                        for i in range(top)]
                arr, _ = pods_array(pods, keep)
                for n in sizes:
                    measure(s, "resource", arr, n, a.reps)
            if "replicas" in lists:
                arr, _ = pods_array([Pod(f"d{i}", containers=[Container({"cpu": 500, "memory": 512 * Mi})],
                                         labels={"app": "web"}, tolerations=KWOK) for i in range(top)], keep)
                for n in sizes:
                    measure(s, "replicas", arr, n, a.reps)
            if "per_pod" in lists:
                sp = synth.spread_pods(top, 16, 9)
                for n in sizes:
                    measure(s, "per_pod", sp.pods, n, a.reps)
    if "label" in lists:
        with cluster(synth.LABELED, a.nodes, False) as s:
            lp = synth.pods(synth.LABELED, top, 7)
            for n in sizes:
                measure(s, "label", lp.pods, n, a.reps)


if __name__ == "__main__":
    main()
