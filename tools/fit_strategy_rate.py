#!/usr/bin/env python3
"""Throughput of the round kernels under a NodeResourcesFit scoring strategy
(DESIGN §5.9, §5.10).  bench.py measures the default strategy and has no switch; this
tool times the bench's C3 shape -- 1M heterogeneous nodes prefilled below 50 %
cpu, steps of 50,000 resource-only pods at 256 pods per round -- through the
ksched Python API under each strategy asked for, and prints one JSON line per
strategy: pods/s, the parallel commit's passes per round, rounds it handed to
the serial commit (ks_debug_counters [12]-[15]) and the sweep / resolve time
per launch.  The figures are reported, not targeted.  A strategy is
TYPE:CPU_WEIGHT:MEMORY_WEIGHT; RequestedToCapacityRatio takes its shape as a
fourth field of UTILIZATION=SCORE points joined by "/".

  python3 tools/fit_strategy_rate.py [--strategies LeastAllocated:1:1,MostAllocated:1:1]
  python3 tools/fit_strategy_rate.py --strategies MostAllocated:1:1,RequestedToCapacityRatio:1:1:0=0/100=10,RequestedToCapacityRatio:1:1:0=0/50=10/100=0
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "k8s-1m_amd"))

from ksched import Scheduler, synth  # noqa: E402
from ksched.framework import results_to_arrays  # noqa: E402


def counters(s):
    k = (C.c_uint64 * 16)()
    assert s.lib.ks_debug_counters(s.ctx, k) == 0, s.lib.ks_last_error(s.ctx)
    return [int(x) for x in k]


def measure(a, nodes, pre, pods, strategy):
    kind, wc, wm, *rest = strategy.split(":")
    shape = [tuple(int(v) for v in pt.split("=")) for pt in rest[0].split("/")] if rest else None
    with Scheduler(a.nodes, pods_per_round=a.pods_per_round, fit_strategy=kind,
                   fit_resource_weights={"cpu": int(wc), "memory": int(wm)}, fit_shape=shape) as s:
        s.upsert_nodes_raw(nodes.nodes, synth.slot_array(a.nodes), a.nodes)
        assert s.lib.ks_pods_add(s.ctx, pre.pods, pre.slot_ptr, pre.n_pods) == 0, s.lib.ks_last_error(s.ctx)
        for k in range(a.warmup):
            s.schedule_raw(pods.pods_at(k * a.batch), a.batch)
        s.reset_stats()
        s.set_timing(True)
        k0 = counters(s)
        scheduled = 0
        t0 = time.perf_counter()
        for k in range(a.warmup, a.warmup + a.steps):
            raw = s.schedule_raw(pods.pods_at(k * a.batch), a.batch)
            scheduled += int((results_to_arrays(raw, a.batch)["status"] == 0).sum())
        elapsed = time.perf_counter() - t0
        s.set_timing(False)
        st, k1 = s.stats(), counters(s)
        d = [y - x for x, y in zip(k0, k1)]
        rounds = max(1, d[0])
        return {"strategy": strategy, "nodes": a.nodes, "pods": a.steps * a.batch, "scheduled": scheduled,
                "pods_per_s": round(a.steps * a.batch / elapsed, 1), "rounds": d[0], "wasted_rounds": d[3],
                "pods_per_round": round(a.steps * a.batch / rounds, 1),
                "parallel_rounds": d[13], "parallel_passes_per_round": round(d[12] / max(1, d[13]), 2),
                "handed_to_serial": d[14], "one_step_rounds": d[15],
                # HIP-event times of the timed launches (ks_set_timing), as bench.py reports them
                "sweep_ms_per_launch": round(st.sweep_ms / max(1, st.sweep_launches), 4),
                "resolve_ms_per_launch": round(st.resolve_ms / max(1, st.resolve_launches), 4),
                "timed_sweep_launches": int(st.sweep_launches), "timed_resolve_launches": int(st.resolve_launches)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pods-per-round", type=int, default=256)
    ap.add_argument("--strategies", default="LeastAllocated:1:1,MostAllocated:1:1")
    a = ap.parse_args()
    nodes = synth.nodes(synth.HETERO, a.nodes, 1)
    pre = synth.prefill(synth.HETERO, a.nodes, 1, 3, 0.5)
    pods = synth.pods(synth.HETERO, (a.warmup + a.steps) * a.batch, 7)
    for strategy in a.strategies.split(","):
        print(json.dumps(measure(a, nodes, pre, pods, strategy)), flush=True)


if __name__ == "__main__":
    main()
