"""NodeResourcesFit scoring strategies beyond the one-rank round kernels
(DESIGN §5.9): the one-pod chain (PodTopologySpread, InterPodAffinity,
extended resources, ImageLocality) and its score dump, replica runs, virtual
shards and a two-rank world, against the reference composed from the oracle's
per-plugin surface (tests/fit_reference.py), every result field and every
node's state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_workloads as W
from fit_reference import STRATEGIES, FitReference, scores_np
from helpers import assert_results_equal, states_np
from ksched import Scheduler, _abi
from ksched.objects import pods_array
from test_gpu_spread import Pair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class FitPair(Pair):
    """tests/test_gpu_spread.py Pair under a strategy: libksched and the
    composed reference fed the same cache events."""

    def __init__(self, n, strategy, **cfg):
        super().__init__(n, **cfg)
        self.o.close()
        self.o = FitReference(n, strategy)
        kind, wc, wm = strategy
        self.s.set_fit_strategy(kind, {"cpu": wc, "memory": wm})

    def dump_equal(self, pod, what=""):
        pa, _ = pods_array([pod], self.a)
        out = (_abi.KsNodeScore * self.n)()
        assert self.s.lib.ks_plugin_scores(self.s.ctx, pa, out) == 0, self.s.lib.ks_last_error(self.s.ctx)
        g, w = scores_np(out, self.n), self.o.plugin_scores(pa)
        assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])

    def states_equal(self, what=""):
        assert np.array_equal(states_np(self.s.lib.ks_node_states, self.s.ctx, self.n), self.o.states()), what


# the four strategies over the two cluster sizes (the chain's select and both dumps)
@pytest.mark.parametrize("seed,n,strategy_name", [(51, 300, "most-1-1"), (51, 300, "least-1-3"),
                                                  (52, 1500, "most-3-1"), (52, 1500, "most-1-0")])
def test_chain_streams(seed, n, strategy_name):
    x = FitPair(n, STRATEGIES[strategy_name], pods_per_round=64)
    W.chain_stream(x, seed, n)
    assert x.s.stats().spread_pods > 0
    x.close()


@pytest.mark.parametrize("runs", [1, 0])
@pytest.mark.parametrize("variant,strategy_name", [("defaults", "most-1-1"), ("dns", "most-3-1"),
                                                   ("defaults", "least-1-3"), ("dns", "most-1-0")])
def test_deployment_replicas(variant, strategy_name, runs):
    x = FitPair(W.N_DEP, STRATEGIES[strategy_name], options={"spread_replica_runs": runs})
    W.deployment_stream(x, variant)
    st = x.s.stats()
    assert (st.replica_runs > 0 and st.replica_pods > 0) if runs else st.replica_runs == 0, (st.replica_runs,)
    x.close()


@pytest.mark.parametrize("kind_name,strategy_name", [("hetero", "most-1-1"), ("labeled", "most-3-1")])
def test_virtual_shards(kind_name, strategy_name):
    w = W.hetero_stream(kind_name)
    want, states = W.hetero_reference(kind_name, strategy_name)
    kind, wc, wm = STRATEGIES[strategy_name]
    with Scheduler(W.N_H, pods_per_round=W.P_H, virtual_shards=3, fit_strategy=kind,
                   fit_resource_weights={"cpu": wc, "memory": wm}) as s:
        W.hetero_setup(s, w)
        got = s.schedule_raw(w["ps"].pods, w["m"])
        assert_results_equal(got, want, w["m"], f"{kind_name} stream on 3 virtual shards")
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, W.N_H), states)


@pytest.mark.parametrize("kind_name,strategy_name", [("hetero", "most-3-1"), ("labeled", "most-1-1")])
def test_two_ranks(kind_name, strategy_name):
    # a two-rank in-process world (tests/test_gpu_multirank.py): each rank sweeps its shard, both set the strategy
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "fit", "kind_name": kind_name, "strategy_name": strategy_name}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] > 0
