#!/usr/bin/env python3
"""Time of ks_explain beside the only route to the same answer
the library offered before it: ks_plugin_scores of the same pod, one record per
slot, and a top-k over them on the host (numpy: the packed keys, argpartition,
a sort of the k).

Two clusters of 1M nodes.  "c3": the bench's C3 cluster -- heterogeneous nodes
prefilled below 50 % cpu -- and 8 pods of the C3 stream.  "rising": nodes whose
TotalScore for the pod rises with the slot in 100 levels, the selection's worst
case (every position beats what the list held when its block reached it), and
one plain pod.  Per pod, ks_explain at k = 1, 16 and 128 and the old route at
k = 128 alternate in one session; every call ends in a device synchronise, so
the host clock around it is the call's time.  The first round warms every path
up, is not timed, and checks that both routes give the same candidates.

  python3 tools/explain_rate.py                  # both clusters, 1M nodes
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/explain_rate.py --reps 10   # the kernels' own time

One JSON line per cluster: microseconds per call (median, min, max) and the
bytes each route brings back from the device.  Reported, not targeted.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "k8s-1m_amd"))

from ksched import Scheduler, _abi, synth  # noqa: E402
from ksched.objects import (Arena, Container, LabelSelector, Node, Pod, TopologySpreadConstraint, nodes_array,  # noqa: E402
                            pods_array)

KS = (1, 16, 128)
Mi = 1 << 20
SCORE_DT = np.dtype([(f, "<i4") for f, _ in _abi.KsNodeScore._fields_[:-1]] + [("total_score", "<i8")])


def us(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def host_topk(scores, k):
    """The k best slots of a score dump, by the packed key."""
    sc = np.frombuffer(scores, dtype=SCORE_DT)
    key = (((sc["total_score"] + 1).astype(np.uint64) << np.uint64(32)) |
           (np.uint64(0xFFFFFFFF) - np.arange(len(sc), dtype=np.uint64))) * (sc["status"] == -1)
    k = min(k, len(key))
    top = np.argpartition(key, len(key) - k)[len(key) - k:]
    top = top[np.argsort(key[top])[::-1]]
    return top[key[top] != 0]


def phase(s, name, pod_ptrs, reps, nodes):
    lib, ctx = s.lib, s.ctx
    e = _abi.KsExplanation()
    out = (_abi.KsCandidate * _abi.EXPLAIN_MAX_CANDIDATES)()
    scores = (_abi.KsNodeScore * nodes)()
    t_explain = {k: [] for k in KS}
    t_scores, t_route = [], []
    for rep in range(reps + 1):  # the first round warms every path up and is not timed
        for j, p in enumerate(pod_ptrs):
            for q in range(len(KS)):  # (the k that follows the dump's 40 MB takes its turn)
                k = KS[(q + rep + j) % len(KS)]
                t0 = time.perf_counter()
                st = lib.ks_explain(ctx, p, k, C.byref(e), out)
                t1 = time.perf_counter()
                assert st == 0, lib.ks_last_error(ctx)
                if rep:
                    t_explain[k].append(1e6 * (t1 - t0))
            t0 = time.perf_counter()
            st = lib.ks_plugin_scores(ctx, p, scores)
            t1 = time.perf_counter()
            top = host_topk(scores, KS[-1])
            t2 = time.perf_counter()
            assert st == 0, lib.ks_last_error(ctx)
            if rep:
                t_scores.append(1e6 * (t1 - t0))
                t_route.append(1e6 * (t2 - t0))
            else:
                st = lib.ks_explain(ctx, p, KS[-1], C.byref(e), out)
                assert st == 0 and [int(out[i].slot) for i in range(e.n_candidates)] == [int(x) for x in top], name
    print(json.dumps({"cluster": name, "nodes": nodes, "calls_each": len(t_scores),
                      "ks_explain_us": {f"k{k}": us(t_explain[k]) for k in KS},
                      "ks_plugin_scores_us": us(t_scores), "ks_plugin_scores_plus_host_topk_us": us(t_route),
                      "explain_bytes_back": {f"k{k}": 24 + 64 * k for k in KS},
                      "plugin_scores_bytes_back": nodes * 40,
                      "feasible_nodes": int(e.feasible_nodes), "top_score": int(e.top_score),
                      "top_score_nodes": int(e.top_score_nodes)}), flush=True)


def rising_nodes(n, a):
    """n ks_node whose LeastAllocated score for rising_pod() is slot * 100 // n (BalancedAllocation 100
    throughout); a level is a zone."""
    tmpl = []
    for lv in range(100):
        cpu = -(-100_000 // (100 - lv))
        tmpl.append(Node(f"l{lv}", {"cpu": cpu, "memory": cpu * Mi, "pods": 110}, {"zone": f"z{lv}"}))
    ta, _ = nodes_array(tmpl, a)
    arr = (_abi.KsNode * n)()
    names = [b"r%d" % i for i in range(n)]
    for i in range(n):
        arr[i] = ta[i * 100 // n]
        arr[i].name = names[i]
    a._keep.append((arr, names))
    return arr


def rising_pod():
    return Pod("p", containers=[Container({"cpu": 1000, "memory": 1000 * Mi})])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pods", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--chain-pods", type=int, default=8)
    a = ap.parse_args()
    nodes = synth.nodes(synth.HETERO, a.nodes, 1)
    pods = synth.pods(synth.HETERO, a.pods, 7)
    with Scheduler(a.nodes) as s:
        s.upsert_nodes_raw(nodes.nodes, synth.slot_array(a.nodes), a.nodes)
        pre = synth.prefill(synth.HETERO, a.nodes, 1, 3, 0.5)
        assert s.lib.ks_pods_add(s.ctx, pre.pods, pre.slot_ptr, pre.n_pods) == 0, s.lib.ks_last_error(s.ctx)
        phase(s, "c3", [pods.pods_at(j) for j in range(a.pods)], a.reps, a.nodes)
    arena = Arena()
    with Scheduler(a.nodes) as s:
        s.upsert_nodes_raw(rising_nodes(a.nodes, arena), synth.slot_array(a.nodes), a.nodes)
        pa, _ = pods_array([rising_pod()], arena)
        phase(s, "rising", [pa] * a.pods, a.reps, a.nodes)
        # a few pods of the one-pod chain scheduled last, so that a kernel trace of this run shows the
        # chain's own select pass beside the explain kernels on the same cluster
        # (requests differ: identical pods would go to a replica run)
        chain = [Pod(f"c{j}", containers=[Container({"cpu": 1000 + j, "memory": 1000 * Mi})], labels={"app": "x"},
                     topology_spread=[TopologySpreadConstraint(1, "zone", "ScheduleAnyway", LabelSelector({"app": "x"}))])
                 for j in range(a.chain_pods)]
        res = s.schedule_pods(chain)
        assert all(not isinstance(r, Exception) for r in res)


if __name__ == "__main__":
    main()
