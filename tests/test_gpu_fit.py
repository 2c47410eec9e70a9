"""NodeResourcesFit scoring strategies on the round kernels (ks_set_fit_strategy;
DESIGN §5.9): MostAllocated / LeastAllocated with per-resource weights against
the reference composed from the oracle's per-plugin surface
(tests/fit_reference.py, validated by tests/test_fit_reference.py), every
result field and every node's state.

(a) the sweep's general variants in every geometry: pod groups (the 1M-node
    5 x 52 and 9 x 29 shapes, 2 x 64 with one pod in the last group), 2 / 4 / 8
    nodes per lane, label words 1 / 2 / 4, short lists, FIX re-sweeps;
(b) the fused totals of the wide label / taint variants (round records);
(c) ks_plugin_scores of a plain pod;
(d) the in-order commit under pile-up (MostAllocated raises the winner's key):
    identical pods on nodes that fill mid-round, under every resolve mode, with
    and without the identical-pod classes; the one-step closed form must not
    take such rounds, and takes them again under the default strategy;
(e) a strategy switch on a live context, also between prepare and run;
(f) refusals.
"""
import ctypes as C

import numpy as np
import pytest

import fit_workloads as W
from fit_reference import DEFAULT, LEAST, MOST, STRATEGIES, FitReference, scores_np
from helpers import assert_results_equal, assert_round_records, res_array, states_np
from ksched import Scheduler, _abi
from ksched.objects import Arena, pods_array
from test_gpu_geometry import (CAP_B, GROUPS, KNPL, LANES, LAUNCHES, LWU, PG, SUB, WIDE_BATCHES, counters, geometry,
                               lane_id, record_pods, wide_pods, wide_workload)

pytestmark = pytest.mark.gpu

CTR_ONESTEP = 15  # ks_debug_counters: rounds the identical-pod closed form resolved


def use(s, strategy):
    kind, wc, wm = strategy
    s.set_fit_strategy(kind, {"cpu": wc, "memory": wm})
    assert s.get_fit_strategy() == (kind, {"cpu": wc, "memory": wm})


def all_states(s, cap):
    return states_np(s.lib.ks_node_states, s.ctx, cap)


# ------------------------------------------------------------ (a) pod groups
# kind, (pods per round, groups, pods per group, last group), blocks
GROUP_CASES = {"hetero-5x52": ("hetero", (256, 5, 52, 48), 2), "labeled-9x29": ("labeled", (256, 9, 29, 24), 4),
               "hetero-2x64": ("hetero", (65, 2, 64, 1), 2), "labeled-2x64": ("labeled", (65, 2, 64, 1), 4)}


def run_groups(case, strategy_name, K, options, npl=4):
    kind_name, (P, groups, pg, last), blocks = GROUP_CASES[case]
    assert P - (groups - 1) * pg == last
    ext = W.KINDS[kind_name][1]
    w = W.group_stream(kind_name, P)
    ref = W.group_reference(kind_name, P, strategy_name)
    pairs = 1 if pg == min(P, 64) else groups * blocks
    opts = dict(options, sweep_pairs=pairs, sweep_pairs_ext=pairs)
    with Scheduler(W.CAP_A, pods_per_round=P, topk=K or P, nodes_per_lane=npl, options=opts) as s:
        use(s, W.ALL[strategy_name])
        W.group_setup(s, w)
        for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
            got = s.schedule_raw(W.pods_at(w["arr"], lo), cnt)
            what = f"{case} {strategy_name} K={K} npl={npl} call {call}"
            assert_results_equal(got, ref[call][0], cnt, what)
            assert np.array_equal(all_states(s, W.CAP_A), ref[call][1]), f"{what}: node state differs"
            g = geometry(s, ext)
            assert g[LAUNCHES] > 0 and geometry(s, not ext)[LAUNCHES] == 0, g
            if npl == 4:
                assert (g[KNPL], g[SUB]) == ((2, 2) if ext else (4, 1)), g
                assert (g[GROUPS], g[PG]) == (groups, pg), g
        return counters(s), w["m"]


@pytest.mark.parametrize("strategy_name", sorted(STRATEGIES))
@pytest.mark.parametrize("case", ["hetero-5x52", "labeled-9x29"])
def test_pod_groups_every_strategy(case, strategy_name):
    k, _ = run_groups(case, strategy_name, 0, {})
    assert k[7] > 0, f"no identical pod was skipped {k}"


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_pod_groups_short_lists(case):
    # lists of 4 run out: rounds end early and the next ones start mid-batch
    k, m = run_groups(case, "most-3-1", 4, {})
    P = GROUP_CASES[case][1][0]
    assert k[0] > -(-m // P), f"{k[0]} rounds for {m} pods: no round ended early"


@pytest.mark.parametrize("case", ["hetero-2x64", "labeled-2x64"])
def test_pod_groups_one_pod_last_group(case):
    run_groups(case, "most-1-1", 0, {})


@pytest.mark.parametrize("early", [1, 0])
def test_pod_groups_fix_resweep(early):
    k, _ = run_groups("labeled-9x29", "most-1-1", 0, {"tuple_guess": 0, "early_fix": early})
    assert k[4] > 0, f"no pod was re-swept {k}"


@pytest.mark.parametrize("npl", [2, 8])
def test_resource_only_lanes(npl):
    # the resource-only sweep at 2 and 8 nodes per lane (4: the cases above)
    kind_name, P = "hetero", 256
    w = W.group_stream(kind_name, P)
    ref = W.group_reference(kind_name, P, "most-3-1")
    with Scheduler(W.CAP_A, pods_per_round=P, nodes_per_lane=npl, options={"sweep_pairs": 1}) as s:
        use(s, STRATEGIES["most-3-1"])
        W.group_setup(s, w)
        for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
            got = s.schedule_raw(W.pods_at(w["arr"], lo), cnt)
            assert_results_equal(got, ref[call][0], cnt, f"npl {npl} call {call}")
            assert np.array_equal(all_states(s, W.CAP_A), ref[call][1])
            g = geometry(s, False)
            assert g[LAUNCHES] > 0 and (g[KNPL], g[SUB], g[PG]) == (npl, 1, 64), g


# ----------------------------- every label / taint variant (nodes per lane, words)
dispatched = set()


@pytest.mark.parametrize("lanes", sorted(LANES), ids=lane_id)
def test_label_word_variants(lanes):
    npl, ext_npl = lanes
    knpl = LANES[lanes]
    w = wide_workload()
    ref = W.wide_reference("most-3-1")
    with Scheduler(CAP_B, pods_per_round=128, nodes_per_lane=npl,
                   options={"ext_nodes_per_lane": ext_npl, "sweep_pairs_ext": 1}) as s:
        use(s, STRATEGIES["most-3-1"])
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        for b, (pa, m, _, _) in enumerate(w["batches"]):
            got = s.schedule_raw(pa, m)
            g = geometry(s, True)
            words = 4 if knpl == 8 else WIDE_BATCHES[b][2]
            what = f"npl {npl}/{ext_npl} batch {b}"
            assert g[LAUNCHES] > b and (g[KNPL], g[LWU], g[SUB]) == (knpl, words, npl // knpl), (what, g)
            dispatched.add((g[KNPL], g[LWU]))
            assert_results_equal(got, ref[b][0], m, what)
            assert np.array_equal(all_states(s, CAP_B), ref[b][1]), f"{what}: node state differs"


def test_every_label_variant_ran_under_the_general_strategy():
    assert dispatched == {(2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4), (8, 4)}, dispatched


# ------------------------------------------------------- (b) fused totals
@pytest.mark.parametrize("lanes", [(4, 4), (8, 8)], ids=lane_id)
def test_round_records_wide_variants(lanes):
    npl, ext_npl = lanes
    w = wide_workload()
    n, K = w["n"], 256
    a = Arena()
    pa, m = pods_array(record_pods(), a)
    r = FitReference(CAP_B, STRATEGIES["most-3-1"])
    r.upsert(w["nodes"], w["slots"], n)
    want = [r.keys(W.pods_at(pa, i)) for i in range(m)]  # keys built from total' at the round-start state
    with Scheduler(CAP_B, pods_per_round=16, topk=K, nodes_per_lane=npl,
                   options={"ext_nodes_per_lane": ext_npl, "sweep_pairs_ext": 1}) as s:
        use(s, STRATEGIES["most-3-1"])
        s.upsert_nodes_raw(w["nodes"], w["slots"], n)
        got = s.schedule_raw(pa, m)
        assert_results_equal(got, r.schedule(pa, m), m, f"records npl {npl}/{ext_npl}")
        g = geometry(s, True)
        assert (g[LAUNCHES], g[KNPL], g[LWU]) == (1, LANES[lanes], 4), g
        assert counters(s)[0] == 1
        res = res_array(got, m)
        assert (res["status"] == 0).all()
        assert assert_round_records(s, want, res, m, K) >= m
    r.close()


# ---------------------------------------------------- (c) ks_plugin_scores
@pytest.mark.parametrize("strategy_name", ["most-3-1", "least-1-3"])
def test_plugin_scores_plain_pod(strategy_name):
    w = wide_workload()
    a = Arena()
    pa, _ = pods_array(wide_pods(0, 40, 8)[3:4], a)  # preferred terms: a normalising pod
    r = FitReference(CAP_B, STRATEGIES[strategy_name])
    r.upsert(w["nodes"], w["slots"], w["n"])
    with Scheduler(CAP_B) as s:
        use(s, STRATEGIES[strategy_name])
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        out = (_abi.KsNodeScore * CAP_B)()
        assert s.lib.ks_plugin_scores(s.ctx, pa, out) == 0, s.lib.ks_last_error(s.ctx)
        got, want = scores_np(out, CAP_B), r.plugin_scores(pa)
        assert (want["status"] == -1).sum() > 100
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    r.close()


# ------------------------------------------------- (d) the commit under pile-up
MODES = {"auto": _abi.RESOLVE_AUTO, "serial": _abi.RESOLVE_SERIAL, "parallel": _abi.RESOLVE_PARALLEL}


def run_pile(s, strategy_name):
    w = W.pile_stream()
    ref = W.pile_reference(strategy_name)
    s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
    for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
        got = s.schedule_raw(W.pods_at(w["pods"], lo), cnt)
        assert_results_equal(got, ref[call][0], cnt, f"pile-up {strategy_name} call {call}")
        assert np.array_equal(all_states(s, W.N_PILE), ref[call][1]), f"pile-up {strategy_name}: node state differs"
    r = np.concatenate([res_array(ref[0][0], w["m1"]), res_array(ref[1][0], w["m"] - w["m1"])])
    return r


@pytest.mark.parametrize("dedup", [1, 0])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("K", [256, 8])
def test_pile_up(K, mode, dedup):
    w = W.pile_stream()
    with Scheduler(W.N_PILE, pods_per_round=256, topk=K,
                   options={"resolve_mode": MODES[mode], "dedup_identical_pods": dedup}) as s:
        use(s, STRATEGIES["most-1-1"])
        r = run_pile(s, "most-1-1")
        # nodes fill and the stream outlives them: pods pile up, the tail finds no node
        ok = r["status"] == 0
        assert ok[:700].all() and (~ok).sum() >= 150
        assert np.bincount(r["node_index"][ok]).max() == 3
        k = counters(s)
        assert k[CTR_ONESTEP] == 0, f"the identical-pod closed form resolved a MostAllocated round {k}"
        # back to the default strategy on the same context, over fresh nodes: it takes such rounds again
        use(s, DEFAULT)
        s.delete_slots(list(range(W.N_PILE)))
        run_pile(s, "default")
        k = counters(s)
        if dedup and mode != "serial" and K == 256:
            assert k[CTR_ONESTEP] > 0, f"the closed form no longer resolves LeastAllocated rounds {k}"


@pytest.mark.parametrize("strategy_name", sorted(set(STRATEGIES) - {"most-1-1"}))
def test_pile_up_other_strategies(strategy_name):
    with Scheduler(W.N_PILE, pods_per_round=256) as s:
        use(s, STRATEGIES[strategy_name])
        run_pile(s, strategy_name)
        if STRATEGIES[strategy_name][0] == MOST:
            assert counters(s)[CTR_ONESTEP] == 0


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind_name", sorted(W.KINDS))
def test_heterogeneous_stream(kind_name, mode):
    w = W.hetero_stream(kind_name)
    want, states = W.hetero_reference(kind_name, "most-3-1")
    with Scheduler(W.N_H, pods_per_round=W.P_H, options={"resolve_mode": MODES[mode]}) as s:
        use(s, STRATEGIES["most-3-1"])
        W.hetero_setup(s, w)
        got = s.schedule_raw(w["ps"].pods, w["m"])
        assert_results_equal(got, want, w["m"], f"{kind_name} stream, resolve {mode}")
        assert np.array_equal(all_states(s, W.N_H), states)


# --------------------------------------------------- (e) strategy switch
def test_strategy_switch_on_a_live_context():
    w = W.hetero_stream("hetero")
    P = W.P_H
    r = FitReference(W.N_H)
    W.hetero_setup(r, w)
    with Scheduler(W.N_H, pods_per_round=P) as s:
        W.hetero_setup(s, w)
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1})
        for b, strategy in enumerate([DEFAULT, STRATEGIES["most-1-1"], DEFAULT]):
            use(s, strategy)
            r.set_strategy(strategy)
            ptr = W.pods_at(w["ps"].pods, b * P)
            if b == 2:
                # prepared under MostAllocated, run after the switch: the run's strategy counts
                use(s, STRATEGIES["most-3-1"])
                batch = s.prepare(ptr, P)
                use(s, strategy)
                s.run(batch)
                got = s.results(batch, P)
                s.free(batch)
            else:
                got = s.schedule_raw(ptr, P)
            assert_results_equal(got, r.schedule(ptr, P), P, f"batch {b} under {strategy}")
            assert np.array_equal(all_states(s, W.N_H), r.states()), f"batch {b}: node state differs"
    r.close()


# ------------------------------------------------------------ (f) refusals
def test_refusals():
    lib = _abi.ksched_lib()
    with Scheduler(64) as s:
        for bad in [(2, 1, 1), (-1, 1, 1), (1, 101, 1), (0, 1, 101), (1, 0, 0), (0, -1, 1)]:
            fs = _abi.KsFitStrategy(*bad, 0)
            assert lib.ks_set_fit_strategy(s.ctx, C.byref(fs)) == _abi.KS_ERR_INVALID, bad
        assert lib.ks_set_fit_strategy(s.ctx, None) == _abi.KS_ERR_INVALID
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1})  # refused calls change nothing
        s.set_fit_strategy(MOST, {"cpu": 100, "memory": 7})
        assert s.get_fit_strategy() == (MOST, {"cpu": 100, "memory": 7})
        s.set_fit_strategy(MOST, {"memory": 2})  # a resource left out is not listed
        assert s.get_fit_strategy() == (MOST, {"cpu": 0, "memory": 2})
    with Scheduler(64, percentage_of_nodes_to_score=5) as s:
        for general in [(1, 1, 1), (0, 1, 3), (0, 2, 2)]:
            fs = _abi.KsFitStrategy(*general, 0)
            assert lib.ks_set_fit_strategy(s.ctx, C.byref(fs)) == _abi.KS_ERR_UNSUPPORTED, general
        fs = _abi.KsFitStrategy(0, 1, 1, 0)
        assert lib.ks_set_fit_strategy(s.ctx, C.byref(fs)) == 0  # the default strategy is still accepted
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1})
    with pytest.raises(_abi.KschedError):
        Scheduler(64, percentage_of_nodes_to_score=5, fit_strategy=MOST)
    with Scheduler(64, fit_strategy=MOST, fit_resource_weights={"cpu": 3, "memory": 1}) as s:
        assert s.get_fit_strategy() == (MOST, {"cpu": 3, "memory": 1})
