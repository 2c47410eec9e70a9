"""Replica runs (ksched_spread.hip replica_keys_kernel, replica_groups_kernel,
replica_run_kernel; ksched_host.cpp's loop around them) at their
group, taken-node, hostname-count and histogram limits: the workloads of
tests/replica_edge_cases.py through libksched and the oracle, results and node
states bit for bit after every batch, and ks_stats.replica_runs /
replica_pods of every batch against the pair the case derives from the
oracle's results -- which run ended where, and who took the rest.  Then the
same stream with replica runs off: no run, equal results."""
import numpy as np
import pytest

import replica_edge_cases as W
from helpers import assert_results_equal, res_array
from ksched.objects import pods_array
from test_gpu_spread import Pair

pytestmark = pytest.mark.gpu


class OraclePair(Pair):
    """Pair whose schedule() hands back the oracle's results (the device's are held equal to them)."""

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        want = self.o.schedule(pa, m)
        got = self.s.schedule_raw(pa, m)
        assert_results_equal(got, want, m, what)
        return res_array(want, m)


def counters(x):
    st = x.s.stats()
    return int(st.replica_runs), int(st.replica_pods)


def stream(case, runs):
    n = len(case["nodes"])
    x = OraclePair(n, options={"spread_replica_runs": runs})
    x.upsert(case["nodes"], list(range(n)))
    x.add([p for p, _ in case["bound"]], [s for _, s in case["bound"]])
    res, took = [], []
    for s in case["steps"]:
        x.s.reset_stats()
        r = x.schedule(s["pods"], f"{s['what']} runs={runs}")
        x.states_equal(f"{s['what']} runs={runs}")
        took.append(counters(x))
        print(s["what"], "runs" if runs else "chain", took[-1])
        assert took[-1] == (s["expect"](r) if runs else (0, 0)), (s["what"], runs)
        s["pre"](r)
        res.append(r)
    x.close()
    return res, took


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_replica_edge(name):
    case = W.CASES[name]()
    res, took = stream(case, 1)
    assert took == W.STATED[name]
    chain, _ = stream(case, 0)
    for s, a, b in zip(case["steps"], res, chain):
        assert np.array_equal(a, b), s["what"]

