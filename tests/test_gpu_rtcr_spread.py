"""RequestedToCapacityRatio beyond the one-rank round kernels:
the one-pod chain (PodTopologySpread, InterPodAffinity, extended resources,
ImageLocality) with churn and its score dumps of plain and spread pods, replica
runs under both constraint kinds, 3 virtual shards and a two-rank world,
against the composed reference (tests/rtcr_reference.py), every result field
and every node's state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_workloads as W
import rtcr_workloads as R
from helpers import assert_results_equal, states_np
from ksched import Scheduler
from rtcr_reference import RTCR, RtcrReference
from test_gpu_fit_spread import FitPair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class RtcrPair(FitPair):
    """FitPair under a RequestedToCapacityRatio case: libksched and the
    composed reference fed the same cache events."""

    def __init__(self, n, name, **cfg):
        super().__init__(n, ("LeastAllocated", 1, 1), **cfg)
        self.o.close()
        self.o = RtcrReference(n, R.case(name))
        R.use(self.s, name)


@pytest.mark.parametrize("seed,n,name", [(51, 300, "peaked-1-1"), (51, 300, "flat-1-0"),
                                         (52, 1500, "falling-3-1"), (52, 1500, "offset-1-1")])
def test_chain_streams(seed, n, name):
    x = RtcrPair(n, name, pods_per_round=64)
    W.chain_stream(x, seed, n)  # schedules, churns and compares the dumps of a spread and a plain pod per batch
    assert x.s.stats().spread_pods > 0
    x.close()


@pytest.mark.parametrize("runs", [1, 0])
@pytest.mark.parametrize("variant,name", [("defaults", "peaked-1-1"), ("dns", "binpack-3-1"),
                                          ("defaults", "falling-1-0"), ("dns", "peaked-3-1")])
def test_deployment_replicas(variant, name, runs):
    x = RtcrPair(W.N_DEP, name, options={"spread_replica_runs": runs})
    W.deployment_stream(x, variant)
    st = x.s.stats()
    assert (st.replica_runs > 0 and st.replica_pods > 0) if runs else st.replica_runs == 0, (st.replica_runs,)
    x.close()


@pytest.mark.parametrize("kind_name,name", [("hetero", "binpack-1-1"), ("labeled", "peaked-3-1")])
def test_virtual_shards(kind_name, name):
    w = W.hetero_stream(kind_name)
    want, states = R.hetero_reference(kind_name, name)
    shape, wc, wm = R.case(name)
    with Scheduler(W.N_H, pods_per_round=W.P_H, virtual_shards=3, fit_strategy=RTCR,
                   fit_resource_weights={"cpu": wc, "memory": wm}, fit_shape=shape) as s:
        W.hetero_setup(s, w)
        got = s.schedule_raw(w["ps"].pods, w["m"])
        assert_results_equal(got, want, w["m"], f"{kind_name} stream on 3 virtual shards")
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, W.N_H), states)


@pytest.mark.parametrize("kind_name,name", [("hetero", "peaked-1-1"), ("labeled", "falling-3-1")])
def test_two_ranks(kind_name, name):
    # a two-rank in-process world (tests/test_gpu_multirank.py): each rank sweeps its shard, both set the shape
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "rtcr", "kind_name": kind_name, "name": name}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] > 0
