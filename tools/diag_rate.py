#!/usr/bin/env python3
"""Time of ks_diagnose beside what the library offered for the
same question before it: ks_plugin_scores of the same pod, whose per-node
statuses the caller would have to tally (and which carry no reasons).

The bench's C3 cluster -- 1M heterogeneous nodes prefilled below 50 % cpu --
and then the same cluster filled further ("c3+prefill": a second prefill on
top; a few percent of the nodes are then short of cpu, memory or pod slots).
Per phase, a few pods of the C3 stream are each asked both ways, alternating
in one session; every call ends in a device synchronise, so the host clock
around it is the call's time.

  python3 tools/diag_rate.py                     # both phases, 1M nodes
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/diag_rate.py --reps 10   # the kernels' own time

One JSON line per phase: microseconds per call (median, min, max) of both
calls, the bytes each brings back from the device (ks_diagnose: the 400-byte
record plus 4 bytes per node with several untolerated taints; ks_plugin_scores:
one record per slot), and the diagnosis of the last pod.  Reported, not
targeted.
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

DIAG_REC_BYTES = 400          # csrc/ksched_diag.hpp DiagRec
DUMP_BYTES_PER_SLOT = 40      # ks_plugin_scores of a pod on the round kernels' dump: 10 words per slot


def us(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def phase(s, name, pods, n_pods, reps, nodes):
    lib, ctx = s.lib, s.ctx
    d, cnt = _abi.KsDiagnosis(), C.c_uint32()
    reasons = (_abi.KsReason * _abi.DIAG_MAX_REASONS)()
    scores = (_abi.KsNodeScore * nodes)()
    t_diag, t_scores = [], []
    for rep in range(reps + 1):  # the first round warms both paths up and is not timed
        for j in range(n_pods):
            p = pods.pods_at(j)
            t0 = time.perf_counter()
            st = lib.ks_diagnose(ctx, p, C.byref(d), reasons, _abi.DIAG_MAX_REASONS, C.byref(cnt))
            t1 = time.perf_counter()
            assert st == 0, lib.ks_last_error(ctx)
            st = lib.ks_plugin_scores(ctx, p, scores)
            t2 = time.perf_counter()
            assert st == 0, lib.ks_last_error(ctx)
            if rep:
                t_diag.append(1e6 * (t1 - t0))
                t_scores.append(1e6 * (t2 - t1))
    last = {reasons[i].reason.decode(): int(reasons[i].count) for i in range(cnt.value)}
    multi = int(d.plugin_nodes[2]) - sum(c for r, c in last.items() if "untolerated taint" in r)  # (0: all resolved)
    print(json.dumps({"phase": name, "nodes": nodes, "calls_each": len(t_diag), "ks_diagnose_us": us(t_diag),
                      "ks_plugin_scores_us": us(t_scores), "diagnose_bytes_back": DIAG_REC_BYTES,
                      "plugin_scores_bytes_back": nodes * DUMP_BYTES_PER_SLOT, "unresolved_taint_nodes": multi,
                      "feasible_nodes": int(d.feasible_nodes), "reasons": last}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pods", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    nodes = synth.nodes(synth.HETERO, a.nodes, 1)
    pods = synth.pods(synth.HETERO, a.pods, 7)
    with Scheduler(a.nodes) as s:
        s.upsert_nodes_raw(nodes.nodes, synth.slot_array(a.nodes), a.nodes)
        pre = synth.prefill(synth.HETERO, a.nodes, 1, 3, 0.5)
        assert s.lib.ks_pods_add(s.ctx, pre.pods, pre.slot_ptr, pre.n_pods) == 0, s.lib.ks_last_error(s.ctx)
        phase(s, "c3", pods, a.pods, a.reps, a.nodes)
        more = synth.prefill(synth.HETERO, a.nodes, 1, 4, 0.5)
        assert s.lib.ks_pods_add(s.ctx, more.pods, more.slot_ptr, more.n_pods) == 0, s.lib.ks_last_error(s.ctx)
        phase(s, "c3+prefill", pods, a.pods, a.reps, a.nodes)


if __name__ == "__main__":
    main()
