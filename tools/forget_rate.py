#!/usr/bin/env python3
"""Per-pod wall time of ks_batch_forget beside ks_pods_remove
of the same pods, in one process on one build.

One 1M-node heterogeneous cluster.  Batches of --batch pods are scheduled in
the prepare / run / results form; after each, a seeded 7/8 of the placed pods
are forgotten -- what seven of eight shards do with every batch -- through
ks_batch_forget on one batch and through ks_pods_remove on the next, batch by
batch, --reps timed repetitions each after one untimed pair.  Both calls end
in a device synchronise, so the host clock around the call is its time.  For
ks_pods_remove the ks_pod structs of the selection are gathered into one array
before the clock starts: the shim's second marshalling of every pod, which the
new call makes unnecessary, is not charged to it.  The same again with
--small-pod batches, the small-call floor.

One JSON line per batch size: microseconds per forgotten pod (min / median /
max over the repetitions) both ways, their ratio, and ks_debug_forget of the
last call.

  python3 tools/forget_rate.py
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/forget_rate.py --reps 3
      # the forget kernel's own time: one launch per call

Reported, not targeted.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "k8s-1m_amd"))

from ksched import Scheduler, _abi, synth  # noqa: E402

RES_DT = np.dtype([("node_index", "<i4"), ("status", "<i4"), ("rest", "V56")])


def us(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


def measure(s, stream, at, m, reps, rng):
    """2 x (reps + 1) batches of m pods from stream position `at`; returns the next position."""
    lib, ctx = s.lib, s.ctx
    pod_bytes = C.sizeof(_abi.KsPod)
    t_forget, t_remove, n_forgot = [], [], []
    for rep in range(2 * (reps + 1)):
        arr = stream.pods_at(at)
        at += m
        b = s.prepare(arr, m)
        s.run(b)
        raw = s.results(b, m)
        r = np.frombuffer(C.string_at(C.addressof(raw), m * C.sizeof(_abi.KsResult)), dtype=RES_DT)
        placed = np.nonzero(r["status"] == 0)[0]
        lost = np.sort(np.array(rng.sample(range(len(placed)), (7 * len(placed)) // 8), dtype=np.int64))
        idx = placed[lost].astype(np.uint32)
        n = len(idx)
        if rep % 2 == 0:
            skipped = C.c_uint32()
            t0 = time.perf_counter()
            st = lib.ks_batch_forget(ctx, b, idx.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(skipped))
            dt = time.perf_counter() - t0
            assert st == 0 and skipped.value == 0, lib.ks_last_error(ctx)
        else:
            # the selection's ks_pod structs and slots, gathered outside the timed region
            pods = np.frombuffer(C.string_at(C.addressof(arr.contents), m * pod_bytes), dtype=np.uint8).reshape(m, pod_bytes)
            sel = np.ascontiguousarray(pods[idx])
            slots = np.ascontiguousarray(r["node_index"][idx].astype(np.uint32))
            t0 = time.perf_counter()
            st = lib.ks_pods_remove(ctx, sel.ctypes.data_as(C.POINTER(_abi.KsPod)),
                                    slots.ctypes.data_as(C.POINTER(C.c_uint32)), n)
            dt = time.perf_counter() - t0
            assert st == 0, lib.ks_last_error(ctx)
        s.free(b)
        if rep >= 2:  # the first pair warms both paths up and is not timed
            (t_forget if rep % 2 == 0 else t_remove).append(1e6 * dt / n)
            n_forgot.append(n)
    f, p = us(t_forget), us(t_remove)
    print(json.dumps({"batch": m, "forgotten_per_call": int(statistics.median(n_forgot)), "reps": reps,
                      "forget_us_per_pod": f, "pods_remove_us_per_pod": p,
                      "remove_median_over_forget_median": round(p["median"] / f["median"], 2),
                      "forget_median_below_remove_min": f["median"] < p["min"],
                      "forget_call_us_median": round(f["median"] * statistics.median(n_forgot), 1),
                      "pods_remove_call_us_median": round(p["median"] * statistics.median(n_forgot), 1),
                      "counters_last_forget": s.forget_counters()[:4]}), flush=True)
    return at


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=50_000)
    ap.add_argument("--small", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    total = 2 * (a.reps + 1) * (a.batch + a.small)
    stream = synth.pods(synth.HETERO, total, 2)
    rng = random.Random(7)
    with Scheduler(a.nodes) as s:
        nd = synth.nodes(synth.HETERO, a.nodes, 1)
        s.upsert_nodes_raw(nd.nodes, synth.slot_array(a.nodes), a.nodes)
        at = measure(s, stream, 0, a.batch, a.reps, rng)
        measure(s, stream, at, a.small, a.reps, rng)


if __name__ == "__main__":
    main()
