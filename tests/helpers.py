"""Shared comparison helpers for parity tests (oracle vs libksched)."""
import ctypes as C
import threading

import numpy as np

from ksched import _abi

RES_DT = np.dtype([("node_index", "<i4"), ("status", "<i4"), ("total_score", "<i8"), ("feasible", "<u4"),
                   ("evaluated", "<u4"), ("fail", "<u4", (8,)), ("flags", "<u4"), ("_pad", "<u4")])


# The profile's score plugin weights as a tuple: the order of pyoracle.Oracle's
# weights (and of ks_config's fields), then hardPodAffinityWeight.
WEIGHT_PLUGINS = ("NodeResourcesFit", "NodeResourcesBalancedAllocation", "TaintToleration", "NodeAffinity",
                  "ImageLocality", "PodTopologySpread", "InterPodAffinity")
DEFAULT_VECTOR = (1, 1, 3, 2, 1, 2, 2, 1)


def weight_forms(vec):
    """A weight vector (fit, balanced, taint, affinity, image, spread, ipa,
    hard) in both forms: Scheduler's keyword arguments and pyoracle.Oracle's
    weights tuple."""
    vec = tuple(int(v) for v in vec)
    assert len(vec) == 8, vec
    return dict(weights=dict(zip(WEIGHT_PLUGINS, vec[:7])), hard_pod_affinity_weight=vec[7]), vec


def oracle_weights(weights=None, hard=1):
    """Scheduler's weights dict (over the defaults) and hardPodAffinityWeight as pyoracle.Oracle's tuple."""
    w = dict(zip(WEIGHT_PLUGINS, DEFAULT_VECTOR[:7]), **(weights or {}))
    return tuple(int(w[p]) for p in WEIGHT_PLUGINS) + (int(hard),)


def res_array(raw, n):
    return np.frombuffer(C.string_at(C.addressof(raw), n * C.sizeof(_abi.KsResult)), dtype=RES_DT).copy()


def assert_results_equal(got, want, n, what=""):
    g, w = res_array(got, n), res_array(want, n)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        i = int(bad[0])
        raise AssertionError(
            f"{what}: {len(bad)}/{n} results differ; first at pod {i}: got {g[i]} want {w[i]}")


def state_array(states):
    return np.array([(s.alloc_milli_cpu, s.alloc_memory, s.req_milli_cpu, s.req_memory, s.nonzero_milli_cpu,
                      s.nonzero_memory, s.alloc_pods, s.pod_count) for s in states], dtype=np.int64)


def scores_array(scores):
    return np.array([(s.status, s.least_allocated, s.balanced_allocation, s.taint_raw, s.taint_score,
                      s.affinity_raw, s.affinity_score, s.image_locality, s.spread_raw, s.spread_score,
                      s.affinity_pod_raw, s.affinity_pod_score, s.total_score) for s in scores],
                    dtype=np.int64)


def oracle_keys(o, pod_ptr):
    """The oracle's packed keys ((TotalScore + 1) << 32 | ~slot) of the pod's
    feasible nodes against the current state, descending, and their count."""
    sc = scores_array(o.plugin_scores(pod_ptr))
    feas = np.nonzero(sc[:, 0] == -1)[0]
    keys = ((sc[feas, -1].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - feas.astype(np.uint64))
    return np.sort(keys)[::-1], len(feas)


def assert_round_records(s, want, r, m, K):
    """ks_debug_round_record of pods 0..m of a batch that one round resolved,
    against want[i] = oracle_keys at the round-start state and the results r
    (res_array): the listed keys are the oracle's top ones, the bound covers
    the next feasible key, the feasible count matches.  Returns the number of
    keys listed over all pods."""
    out = (C.c_uint64 * (2 + K))()
    listed = 0
    for i in range(m):
        assert s.lib.ks_debug_round_record(s.ctx, i, out) == 0, s.lib.ks_last_error(s.ctx)
        bound, nk = int(out[0]), int(out[1])
        got = np.array(out[2:2 + nk], dtype=np.uint64)
        keys, nfeas = want[i]
        assert int(r["feasible"][i]) == nfeas or r["status"][i] != 0
        assert nk <= len(keys)
        assert np.array_equal(got, keys[:nk]), f"pod {i}: listed keys differ from the oracle's top {nk}"
        if nk < len(keys):
            assert bound >= int(keys[nk]), f"pod {i}: bound below an unlisted feasible key"
        listed += nk
    return listed


STATE_DT = np.dtype([("alloc_cpu", "<i8"), ("alloc_mem", "<i8"), ("req_cpu", "<i8"), ("req_mem", "<i8"),
                     ("nz_cpu", "<i8"), ("nz_mem", "<i8"), ("alloc_pods", "<i4"), ("pod_count", "<i4")])


def states_np(fn, ctx, n):
    """All n slots' ks_node_state via ks_node_states / oracle_node_states(ctx, slots, n, out), as numpy."""
    slots = np.arange(n, dtype=np.uint32)
    out = (_abi.KsNodeState * max(1, n))()
    st = fn(ctx, slots.ctypes.data_as(C.POINTER(C.c_uint32)), n, out)
    assert st == 0, f"node_states failed ({st})"
    return np.frombuffer(C.string_at(C.addressof(out), n * C.sizeof(_abi.KsNodeState)), dtype=STATE_DT).copy()


class OracleTarget:
    """The C++ oracle (oracle/pyoracle.py) behind the C5 stream driver's target
    interface (ksched.stream.GpuTarget): the stream replays against both."""

    def __init__(self, o):
        self.o = o
        for name in ("upsert", "delete", "add_pods", "remove_pods", "schedule"):
            setattr(self, name, getattr(o, name))

    def states(self, slots):
        return self.o.node_states(slots)


def on_threads(fns):
    """Run the callables on threads and return their results (libksched's and
    the oracle's ctypes calls release the GIL, so per-rank setup runs side by
    side); the first error is raised."""
    out, errs = [None] * len(fns), []

    def go(i):
        try:
            out[i] = fns[i]()
        except Exception as e:  # noqa: BLE001 -- re-raised below
            errs.append(e)

    th = [threading.Thread(target=go, args=(i,)) for i in range(len(fns))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return out


class Background:
    """One callable on a thread, its result fetched later (the oracle's 1M-node
    setup overlaps the GPU work)."""

    def __init__(self, fn):
        self._out, self._err = [], []

        def run():
            try:
                self._out.append(fn())
            except Exception as e:  # noqa: BLE001 -- re-raised by get()
                self._err.append(e)
        self._t = threading.Thread(target=run)
        self._t.start()

    def get(self):
        self._t.join()
        if self._err:
            raise self._err[0]
        return self._out[0]
