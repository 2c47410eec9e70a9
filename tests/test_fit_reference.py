"""The reference for NodeResourcesFit scoring strategies (tests/fit_reference.py).

(1) Known answers of the Python scorer, each derived by hand from upstream
    v1.31.3 noderesources/{least,most}_allocated.go and resource_allocation.go.
(2) The composition (per-pod oracle.plugin_scores + node states + the Python
    scorer + oracle.commit) under {LeastAllocated, 1, 1} equals oracle.schedule,
    every result field and every node state, on the streams the GPU tests use.
    That is the condition under which the GPU tests trust it for the other
    strategies, where the only new arithmetic is fit_scores.
"""
import numpy as np
import pytest

import fit_workloads as W
import pyoracle
from fit_reference import LEAST, MOST, fit_scores, resource_score
from helpers import assert_results_equal, states_np

Gi = 1 << 30


def one(strategy, cap_c, cap_m, req_c, req_m):
    return int(fit_scores(strategy, [cap_c], [cap_m], [req_c], [req_m])[0])


def test_kat_most_and_least_allocated():
    """A 4000 m / 8 Gi node with 1000 m / 2 Gi non-zero requested and a
    500 m / 1 Gi pod: requested = 1500 m / 3 Gi.
    MostAllocated: cpu 1500 * 100 / 4000 = 37 (37.5), memory 3 * 100 / 8 = 37
    (37.5); (37 + 37) / 2 = 37.
    LeastAllocated: cpu 2500 * 100 / 4000 = 62 (62.5), memory 5 * 100 / 8 = 62;
    (62 + 62) / 2 = 62."""
    assert one((MOST, 1, 1), 4000, 8 * Gi, 1500, 3 * Gi) == 37
    assert one((LEAST, 1, 1), 4000, 8 * Gi, 1500, 3 * Gi) == 62
    assert one((LEAST, 1, 1), 4000, 8 * Gi, 1500, 3 * Gi) == pyoracle.lib().oracle_least_allocated(
        4000, 8 * Gi, 1000, 2 * Gi, 500, 1 * Gi)


def test_kat_requested_beyond_capacity_clamps():
    """requested 5000 m > 4000 m and 9 Gi > 8 Gi: mostRequestedScore clamps
    requested to capacity (100), leastRequestedScore returns 0."""
    assert one((MOST, 1, 1), 4000, 8 * Gi, 5000, 9 * Gi) == 100
    assert one((LEAST, 1, 1), 4000, 8 * Gi, 5000, 9 * Gi) == 0
    # one resource beyond: cpu 100 / 0, memory 37 / 62 -> (100 + 37) / 2 = 68, (0 + 62) / 2 = 31
    assert one((MOST, 1, 1), 4000, 8 * Gi, 5000, 3 * Gi) == 68
    assert one((LEAST, 1, 1), 4000, 8 * Gi, 5000, 3 * Gi) == 31


def test_kat_zero_allocatable_drops_out_of_the_weight_sum():
    """A node with no memory allocatable: the loop skips the resource, so the
    score is cpu's alone (37 / 1, not 37 / 2); with weights (3, 1) likewise
    3 * 37 / 3.  No allocatable at all: weight sum 0 -> 0."""
    assert one((MOST, 1, 1), 4000, 0, 1500, 3 * Gi) == 37
    assert one((MOST, 3, 1), 4000, 0, 1500, 3 * Gi) == 37
    assert one((LEAST, 1, 3), 0, 8 * Gi, 1500, 3 * Gi) == 62
    assert one((MOST, 1, 1), 0, 0, 1500, 3 * Gi) == 0


def test_kat_weights():
    """Per-resource scores (37, 50) -- cpu 1500 / 4000, memory 4 Gi / 8 Gi --
    under weights (3, 1): (3 * 37 + 50) / 4 = 161 / 4 = 40 (40.25)."""
    assert int(resource_score(True, [1500], [4000])[0]) == 37 and int(resource_score(True, [4 * Gi], [8 * Gi])[0]) == 50
    assert one((MOST, 3, 1), 4000, 8 * Gi, 1500, 4 * Gi) == 40
    # a weight of 0 removes the resource: the other's score alone
    assert one((MOST, 1, 0), 4000, 8 * Gi, 1500, 4 * Gi) == 37
    assert one((MOST, 0, 1), 4000, 8 * Gi, 1500, 4 * Gi) == 50
    assert one((MOST, 0, 7), 4000, 8 * Gi, 1500, 4 * Gi) == 50
    # ... also when the remaining resource has no allocatable: nothing is left
    assert one((MOST, 1, 0), 0, 8 * Gi, 1500, 4 * Gi) == 0


def test_kat_truncation_of_the_weighted_sum():
    """The weighted sum is divided once, not term by term.  Scores (37, 37)
    under weights (1, 2): (37 + 2 * 37) / 3 = 111 / 3 = 37, whereas truncating
    each term gives 37 / 3 + 74 / 3 = 12 + 24 = 36.  And scores (37, 50) under
    (2, 3): (74 + 150) / 5 = 224 / 5 = 44 (44.8)."""
    assert one((MOST, 1, 2), 4000, 8 * Gi, 1500, 3 * Gi) == 37
    assert 37 // 3 + 74 // 3 == 36
    assert one((MOST, 2, 3), 4000, 8 * Gi, 1500, 4 * Gi) == 44


# ------------------------------------------- the composition equals the oracle
def check_default(ref_fn, setup, capacity, calls):
    """ref_fn: the cached reference under the default strategy, [(results,
    states)] per call; the oracle runs the same calls."""
    o = pyoracle.Oracle(capacity)
    setup(o)
    for (want, states), (ptr, cnt) in zip(ref_fn, calls):
        got = o.schedule(ptr, cnt)
        assert_results_equal(got, want, cnt, "composed reference vs oracle.schedule")
        assert np.array_equal(states_np(o.L.oracle_node_states, o.o, capacity), states)
    o.close()


@pytest.mark.parametrize("P", [256, 65])
@pytest.mark.parametrize("kind_name", sorted(W.KINDS))
def test_composed_default_equals_oracle_group_streams(kind_name, P):
    w = W.group_stream(kind_name, P)

    def setup(o):
        o.upsert(w["ns"].nodes, w["slots"], W.N_A)
        o.add_pods(w["pf"].pods, w["pf_slots"], w["pf"].n_pods)
    check_default(W.group_reference(kind_name, P, "default"), setup, W.CAP_A,
                  [(W.pods_at(w["arr"], 0), w["m1"]), (W.pods_at(w["arr"], w["m1"]), w["m"] - w["m1"])])


def test_composed_default_equals_oracle_pile_up():
    w = W.pile_stream()
    check_default(W.pile_reference("default"), lambda o: o.upsert(w["nodes"], w["slots"], w["n"]), W.N_PILE,
                  [(W.pods_at(w["pods"], 0), w["m1"]), (W.pods_at(w["pods"], w["m1"]), w["m"] - w["m1"])])


@pytest.mark.parametrize("kind_name", sorted(W.KINDS))
def test_composed_default_equals_oracle_hetero_stream(kind_name):
    w = W.hetero_stream(kind_name)

    def setup(o):
        o.upsert(w["ns"].nodes, W.synth.slot_array(W.N_H), W.N_H)
        o.add_pods(w["pf"].pods, w["pf"].slot_ptr, w["pf"].n_pods)
    check_default([W.hetero_reference(kind_name, "default")], setup, W.N_H, [(w["ps"].pods, w["m"])])


def test_composed_default_equals_oracle_wide_batches():
    from test_gpu_geometry import wide_workload
    for (want, states), (_, m, owant, ostates) in zip(W.wide_reference("default"), wide_workload()["batches"]):
        assert_results_equal(want, owant, m, "composed reference vs oracle.schedule (wide batches)")
        assert np.array_equal(W.states_matrix(states), ostates)


@pytest.mark.parametrize("seed,n", [(51, 300), (52, 1500)])
def test_composed_default_equals_oracle_chain_streams(seed, n):
    x = W.RefPair(n)
    W.chain_stream(x, seed, n)
    x.close()


@pytest.mark.parametrize("variant", ["defaults", "dns"])
def test_composed_default_equals_oracle_deployments(variant):
    x = W.RefPair(W.N_DEP)
    W.deployment_stream(x, variant)
    x.close()


def test_streams_hold_unschedulable_and_single_feasible_pods():
    """The labeled stream takes every branch of the composition's outcome."""
    w = W.group_stream("labeled", 256)
    r = W.res_array(W.group_reference("labeled", 256, "default")[0][0], w["m1"])
    assert (r["status"] == 1).any() and (r["flags"] & 1).any() and (r["status"] == 0).any()


def test_most_allocated_packs():
    """The strategies differ where they should: on the heterogeneous stream
    MostAllocated lands the pods on far fewer nodes than LeastAllocated."""
    w = W.hetero_stream("hetero")
    least = W.res_array(W.hetero_reference("hetero", "default")[0], w["m"])
    most = W.res_array(W.hetero_reference("hetero", "most-1-1")[0], w["m"])
    used = lambda r: len(set(r["node_index"][r["status"] == 0]))  # noqa: E731
    assert used(most) * 2 < used(least), (used(most), used(least))
