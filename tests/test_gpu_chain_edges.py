"""The one-pod chain (ksched_spread.hip, ksched_diag.hip, ksched_explain.hip)
at its domain-table, prefetch and renumbering edges: the workloads of
tests/chain_edge_cases.py through libksched and the oracle, results, plugin
score dumps and node states bit for bit, the answers known by construction
asserted on the device's results, and ks_debug_topology read back so that
every case proves which side of a limit its key was on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_edge_cases as W
from helpers import scores_array
from scenarios import SPREAD
from test_gpu_spread import Pair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IDS, SCRATCH, RENUMBERED, SHARED = range(4)  # ks_debug_topology words


def scratch_for(ids):
    """spread_scratch: 1024 entries per constraint until a key has more ids, then at least twice that."""
    return W.SCRATCH_MIN if ids <= W.SCRATCH_MIN else max(ids, 2 * W.SCRATCH_MIN)


# ------------------------------------------------------------ 1. wide key, last domain

@pytest.mark.parametrize("P", [256, 2])
@pytest.mark.parametrize("variant", W.WIDE_VARIANTS)
@pytest.mark.parametrize("D", W.WIDE_D)
def test_wide_key(D, variant, P):
    case = W.wide_key(D, variant)
    n, ids = len(case["nodes"]), D + 1
    assert (ids <= W.SP_LDS_DOM) == (D <= 1023)  # 1022, 1023: LDS histogram; 1024, 1025: global atomics
    x = Pair(n, pods_per_round=P)
    assert x.s.debug_topology("cell") == (0, 0, 0, 0)

    def before(x):
        if variant != "dns":
            return
        d = x.s.diagnose(case["pods"][0])
        assert d.num_all_nodes == n and d.feasible_nodes == 1 and d.reasons == {W.WIDE_REASON: n - 1}, d
        e = x.s.explain(case["pods"][0], k=4)
        assert e.feasible_nodes == 1 and [c.slot for c in e.candidates] == [D - 1], e

    W.run_case(x, case, f"wide {D} {variant}", before)
    x.states_equal(f"wide {D} {variant}")
    assert x.s.debug_topology("cell") == (ids, scratch_for(ids), 0, 37)
    x.close()


def test_wide_key_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    cfg = {"family": "chain_edges", "D": 1024, "variant": "dns"}
    p = subprocess.run([sys.executable, os.path.join(HERE, "chain_multirank_main.py"), json.dumps(cfg)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["scheduled"] == 2 and res["ids"] == 1025


# ------------------------------------------------------------ 2. the LDS budget

def budget_pair(P):
    nodes, bound = W.budget_cluster()
    x = Pair(len(nodes), pods_per_round=P)
    x.upsert(nodes, list(range(len(nodes))))
    x.add([p for p, _ in bound], [s for _, s in bound])
    return x


@pytest.mark.parametrize("P", [256, 2])
def test_lds_budget(P):
    pods = W.budget_pods()
    x = budget_pair(P)
    dump = {k: scores_array(x.dump_equal(pods[k], f"budget dump {k}")) for k in "abcdef"}
    assert np.array_equal(dump["a"], dump["c"])  # the constraints' order moves the spill from k4 to k0, nothing else
    assert (dump["a"][:, 0] == SPREAD).sum() > 0
    r = x.schedule([pods[k] for k in "abcdef"], "budget")
    x.states_equal("budget")
    assert (r["status"] == 0).all() and (r["fail"][:, SPREAD] > 0).all()
    for key, ids in W.BUDGET_IDS.items():  # 4 x 1001 = 4004, + 92 = 4096 fits, + 93 does not
        # (the scratch is one size for all keys: (e)'s hostname term brought a key of 1101 ids)
        assert x.s.debug_topology(key)[:2] == (ids, scratch_for(W.BUDGET_N + 1)), key
    assert x.s.debug_topology(W.HOST)[IDS] == W.BUDGET_N + 1
    x.close()
    y = budget_pair(P)
    rc = y.schedule([pods["c"]], "budget reversed")
    assert rc[0] == r[0]
    y.close()


# ------------------------------------------------------------ 3. beyond the prefetch width

@pytest.mark.parametrize("name", sorted(W.PF_CASES))
def test_prefetch_width(name):
    case = W.PF_CASES[name]()
    x = Pair(W.PF_N)
    r = W.run_case(x, case, name)
    assert r["node_index"][0] == 12
    x.states_equal(name)
    x.close()


# ------------------------------------------------------------ 4. churn

@pytest.mark.parametrize("phase", W.CHURN_PHASES)
def test_churn(phase):
    x = Pair(W.CHURN_CAP)
    seen = []

    def probe(step, models, scratch):
        for key, m in models.items():
            got = x.s.debug_topology(key)
            assert got == (m.ids, scratch, m.rebuilds, m.shared), (step, key, got)
        x.states_equal(f"churn step {step}")
        seen.append(x.s.debug_topology("rack"))

    _, info = W.churn_stream(x, phase, probe)
    x.close()
    ids = [t[IDS] for t in seen]
    s, t = info["left_lds"], info["renumbered"]
    # the scratch grows with the first id count above 1024 ...
    assert ids[s - 1] <= W.SP_LDS_DOM < ids[s]
    assert [q[SCRATCH] for q in seen[s - 1:s + 1]] == [W.SCRATCH_MIN, 2 * W.SCRATCH_MIN]
    # ... and the step whose upsert passes 2 x capacity + 1024 renumbers the key: the ids fall back
    limit = W.renumber_above(W.CHURN_CAP)
    assert ids[t - 1] <= limit < ids[t - 1] + W.CHURN_NODES - 1
    assert [q[RENUMBERED] for q in seen[t - 1:t + 1]] == [0, 1] and ids[t] <= W.CHURN_NODES + 1
    assert seen[t][SHARED] == info["shared_then"] == {0: 0, 2: 1}[phase]
    assert seen[-1][RENUMBERED] == 1 and t < W.CHURN_STEPS - 2


# ------------------------------------------------------------ 5. replica-run width

@pytest.mark.parametrize("variant", W.RUN_VARIANTS)
@pytest.mark.parametrize("D", W.RUN_D)
def test_run_width(D, variant):
    case = W.run_width(D, variant)
    n, ids = len(case["nodes"]), D + 1
    assert case["runs"] == (ids <= W.RK_DZ_NONE)  # 2047 ids: the widest key a run takes; 2048: refused
    res = {}
    for runs in (1, 0):
        x = Pair(n, options={"spread_replica_runs": runs})
        res[runs] = W.run_case(x, case, f"run {D} {variant} runs={runs}")
        x.states_equal(f"run {D} {variant} runs={runs}")
        # (the scratch is one size for all keys: the defaults' hostname constraint comes first, with n + 1 ids)
        assert x.s.debug_topology("cell")[:2] == (ids, scratch_for(n + 1 if variant == "defaults" else ids))
        st = x.s.stats()
        took = (int(st.replica_runs), int(st.replica_pods))
        if runs and case["runs"]:
            assert took[0] > 0 and took[1] > 0, took
        else:
            assert took == (0, 0), took
        x.close()
    assert np.array_equal(res[1], res[0])
    assert any(i % D == D - 1 for i in res[1]["node_index"].tolist())  # the highest domain id was taken
