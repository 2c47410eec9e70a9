#!/usr/bin/env python3
"""Throughput of the one-pod chain for pods with a host port (NodePorts,
DESIGN §5.13).  bench.py's workloads carry no host ports; this tool takes the
bench's C3 cluster -- 1M heterogeneous nodes prefilled below 50 % cpu -- and
schedules pods that each want one host port, drawn from 8 (ip, protocol, port)
triples so that they stay schedulable, through the ksched Python API.  Every
such pod takes the one-pod chain (a filter pass over all nodes, a select pass,
a commit); the filter pass loads 8 more bytes per node.

The yardstick is the same chain without that load: the same pods without
ports, each requesting one amd.com/gpu of the 8 every node has (--mode gpu).
That mode uses nothing this feature added, so it runs on an older build too.

  python3 tools/ports_rate.py --mode ports   # one host port per pod
  python3 tools/ports_rate.py --mode gpu     # one amd.com/gpu per pod, no ports

One JSON line: pods/s and the chain's time per pod.  Reported, not targeted.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "k8s-1m_amd"))

from ksched import Scheduler, _abi, synth  # noqa: E402
from ksched.framework import results_to_arrays  # noqa: E402

GPU = b"amd.com/gpu"
TRIPLES = [(ip, proto, port) for port in (9100, 8080) for proto in (b"TCP", b"UDP") for ip in (None, b"10.0.0.1")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=["ports", "gpu"], default="ports")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gpus-per-node", type=int, default=8)
    a = ap.parse_args()
    nodes = synth.nodes(synth.HETERO, a.nodes, 1)
    pre = synth.prefill(synth.HETERO, a.nodes, 1, 3, 0.5)
    total = (a.warmup + a.steps) * a.batch
    pods = synth.pods(synth.HETERO, total, 7)
    keep = []
    if a.mode == "gpu":
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
    else:
        keep = [(_abi.KsHostPort * 1)(_abi.KsHostPort(ip, proto, port, 0)) for ip, proto, port in TRIPLES]
        for j in range(total):
            c = pods.pods[j].containers[0]
            c.host_ports = keep[j % len(keep)]
            c.n_host_ports = 1
    with Scheduler(a.nodes) as s:
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
        print(json.dumps({"mode": a.mode, "nodes": a.nodes, "pods": n, "scheduled": scheduled,
                          "chain_pods": int(st.spread_pods), "pods_per_s": round(n / elapsed, 1),
                          "us_per_pod": round(1e6 * elapsed / n, 2)}), flush=True)


if __name__ == "__main__":
    main()
