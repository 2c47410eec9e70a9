#!/usr/bin/env python3
"""Throughput of the one-pod chain for pods that request a scalar resource the
balanced list names.  bench.py measures the default profile and
has no switch; this tool takes the bench's C3 cluster -- 1M heterogeneous nodes
prefilled below 50 % cpu -- gives every node 8 amd.com/gpu, and schedules pods
that each request one, through the ksched Python API.  Every such pod takes the
one-pod chain (a filter pass over all nodes, a select pass, a commit) with or
without the list, so the two runs differ in the filter pass's
BalancedAllocation arithmetic alone.

  python3 tools/ba_rate.py                              # the default list: the calls every build has
  python3 tools/ba_rate.py --list cpu,memory,amd.com/gpu
  python3 tools/ba_rate.py --root ../parent-checkout    # another tree's library (built there), same tool

One JSON line: pods/s and the chain's time per pod.  Reported, not targeted.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

GPU = b"amd.com/gpu"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent),
                    help="repository root whose built library is measured")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gpus-per-node", type=int, default=8)
    ap.add_argument("--list", default="", help="comma-separated balanced list; empty: the setter is not called")
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.root).resolve() / "k8s-1m_amd"))
    from ksched import Scheduler, _abi, synth
    from ksched.framework import results_to_arrays

    nodes = synth.nodes(synth.HETERO, a.nodes, 1)
    pre = synth.prefill(synth.HETERO, a.nodes, 1, 3, 0.5)
    total = (a.warmup + a.steps) * a.batch
    pods = synth.pods(synth.HETERO, total, 7)
    # the generator knows cpu and memory: point every node and every pod's first container at one shared entry
    node_res = (_abi.KsResource * 1)(_abi.KsResource(GPU, a.gpus_per_node))
    pod_res = (_abi.KsResource * 1)(_abi.KsResource(GPU, 1))
    for i in range(a.nodes):
        nodes.nodes[i].extended = node_res
        nodes.nodes[i].n_extended = 1
    for j in range(total):
        c = pods.pods[j].containers[0]
        c.extended = pod_res
        c.n_extended = 1
    names = [x for x in a.list.split(",") if x]
    with Scheduler(a.nodes) as s:
        if names:
            s.set_balanced_resources(names)
        s.upsert_nodes_raw(nodes.nodes, synth.slot_array(a.nodes), a.nodes)
        assert s.lib.ks_pods_add(s.ctx, pre.pods, pre.slot_ptr, pre.n_pods) == 0, s.lib.ks_last_error(s.ctx)
        for k in range(a.warmup):
            s.schedule_raw(pods.pods_at(k * a.batch), a.batch)
        s.reset_stats()
        scheduled = 0
        t0 = time.perf_counter()
        for k in range(a.warmup, a.warmup + a.steps):
            raw = s.schedule_raw(pods.pods_at(k * a.batch), a.batch)
            scheduled += int((results_to_arrays(raw, a.batch)["status"] == 0).sum())
        elapsed = time.perf_counter() - t0
        st = s.stats()
        n = a.steps * a.batch
        print(json.dumps({"root": a.root, "list": names or ["cpu", "memory"], "nodes": a.nodes, "pods": n,
                          "scheduled": scheduled, "chain_pods": int(st.spread_pods),
                          "pods_per_s": round(n / elapsed, 1), "us_per_pod": round(1e6 * elapsed / n, 2)}), flush=True)


if __name__ == "__main__":
    main()
