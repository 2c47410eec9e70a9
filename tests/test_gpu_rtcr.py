"""NodeResourcesFit's RequestedToCapacityRatio on the round kernels
(ks_set_fit_strategy_shape) against the reference composed from
the oracle's per-plugin surface (tests/rtcr_reference.py), every result field
and every node's state.  Shapes: bin packing {0:0, 100:10}, falling with
truncation {0:10, 30:0}, peaked {0:0, 50:10, 100:0} (a node's key rises and
then falls as it fills), flat {40:7}, offset {20:2, 80:9}; weights (1, 1),
(3, 1), (1, 0).

(a) the sweep's ten instances under the strategy, checked as a set from
    ks_debug_sweep_geometry: pod groups (5 x 52, 9 x 29, 2 x 64 with one pod in
    the last group) with full and 4-entry lists, 2 / 4 / 8 nodes per lane,
    label words 1 / 2 / 4;
(b) nodes without memory Allocatable and nodes whose NonZeroRequested passes
    their capacity;
(c) ks_plugin_scores of a plain pod;
(d) the in-order commit under pile-up, under every resolve mode, with and
    without the identical-pod classes, at K = 256 and 8; the closed form takes
    LeastAllocated rounds again after a switch back on the same context;
(e) a strategy and a shape switch on a live context, also between prepare and run;
(f) refusals on a context.
"""
import ctypes as C

import numpy as np
import pytest

import fit_workloads as W
import rtcr_workloads as R
from fit_reference import DEFAULT, LEAST, MOST, scores_np
from helpers import assert_results_equal, res_array, states_np
from ksched import Scheduler, _abi
from ksched.objects import Arena, pods_array
from rtcr_reference import RTCR, SHAPES, RtcrReference
from test_gpu_fit import CTR_ONESTEP, GROUP_CASES, MODES
from test_gpu_fit import use as use_plain
from test_gpu_geometry import (CAP_B, GROUPS, KNPL, LANES, LAUNCHES, LWU, PG, SUB, WIDE_BATCHES, counters, geometry,
                               lane_id, wide_pods, wide_workload)

pytestmark = pytest.mark.gpu

# sweep instances dispatched under the strategy: (label / taint columns, nodes per lane, label words)
dispatched = set()


def all_states(s, cap):
    return states_np(s.lib.ks_node_states, s.ctx, cap)


# ------------------------------------------------------------ (a) pod groups
def run_groups(group_case, name, K, npl=4):
    kind_name, (P, groups, pg, last), blocks = GROUP_CASES[group_case]
    ext = W.KINDS[kind_name][1]
    w = W.group_stream(kind_name, P)
    ref = R.group_reference(kind_name, P, name)
    pairs = 1 if pg == min(P, 64) else groups * blocks
    with Scheduler(W.CAP_A, pods_per_round=P, topk=K or P, nodes_per_lane=npl,
                   options={"sweep_pairs": pairs, "sweep_pairs_ext": pairs}) as s:
        R.use(s, name)
        W.group_setup(s, w)
        for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
            got = s.schedule_raw(W.pods_at(w["arr"], lo), cnt)
            what = f"{group_case} {name} K={K} npl={npl} call {call}"
            assert_results_equal(got, ref[call][0], cnt, what)
            assert np.array_equal(all_states(s, W.CAP_A), ref[call][1]), f"{what}: node state differs"
            g = geometry(s, ext)
            assert g[LAUNCHES] > 0 and geometry(s, not ext)[LAUNCHES] == 0, g
            if npl == 4:
                assert (g[KNPL], g[SUB]) == ((2, 2) if ext else (4, 1)), g
                assert (g[GROUPS], g[PG]) == (groups, pg), g
            dispatched.add((ext, g[KNPL], g[LWU] if ext else 0))
        return counters(s), w["m"]


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("group_case", ["hetero-5x52", "labeled-9x29"])
def test_pod_groups_every_shape(group_case, name):
    k, _ = run_groups(group_case, name, 0)
    assert k[7] > 0, f"no identical pod was skipped {k}"


@pytest.mark.parametrize("group_case", sorted(GROUP_CASES))
def test_pod_groups_short_lists(group_case):
    # lists of 4 run out: rounds end early and the next ones start mid-batch
    k, m = run_groups(group_case, "peaked-1-1", 4)
    P = GROUP_CASES[group_case][1][0]
    assert k[0] > -(-m // P), f"{k[0]} rounds for {m} pods: no round ended early"


@pytest.mark.parametrize("group_case", ["hetero-2x64", "labeled-2x64"])
def test_pod_groups_one_pod_last_group(group_case):
    run_groups(group_case, "peaked-1-1", 0)


@pytest.mark.parametrize("npl", [2, 8])
def test_resource_only_lanes(npl):
    w = W.group_stream("hetero", 256)
    ref = R.group_reference("hetero", 256, "falling-3-1")
    with Scheduler(W.CAP_A, pods_per_round=256, nodes_per_lane=npl, options={"sweep_pairs": 1}) as s:
        R.use(s, "falling-3-1")
        W.group_setup(s, w)
        for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
            got = s.schedule_raw(W.pods_at(w["arr"], lo), cnt)
            assert_results_equal(got, ref[call][0], cnt, f"npl {npl} call {call}")
            assert np.array_equal(all_states(s, W.CAP_A), ref[call][1])
            g = geometry(s, False)
            assert g[LAUNCHES] > 0 and (g[KNPL], g[SUB], g[PG]) == (npl, 1, 64), g
            dispatched.add((False, g[KNPL], 0))


@pytest.mark.parametrize("lanes", sorted(LANES), ids=lane_id)
def test_label_word_variants(lanes):
    npl, ext_npl = lanes
    knpl = LANES[lanes]
    w = wide_workload()
    ref = R.wide_reference("peaked-1-1")
    with Scheduler(CAP_B, pods_per_round=128, nodes_per_lane=npl,
                   options={"ext_nodes_per_lane": ext_npl, "sweep_pairs_ext": 1}) as s:
        R.use(s, "peaked-1-1")
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        for b, (pa, m, _, _) in enumerate(w["batches"]):
            got = s.schedule_raw(pa, m)
            g = geometry(s, True)
            words = 4 if knpl == 8 else WIDE_BATCHES[b][2]
            what = f"npl {npl}/{ext_npl} batch {b}"
            assert g[LAUNCHES] > b and (g[KNPL], g[LWU], g[SUB]) == (knpl, words, npl // knpl), (what, g)
            dispatched.add((True, g[KNPL], g[LWU]))
            assert_results_equal(got, ref[b][0], m, what)
            assert np.array_equal(all_states(s, CAP_B), ref[b][1]), f"{what}: node state differs"


def test_all_ten_sweep_instances_ran_under_the_strategy():
    assert dispatched == {(False, 2, 0), (False, 4, 0), (False, 8, 0), (True, 2, 1), (True, 2, 2), (True, 2, 4),
                          (True, 4, 1), (True, 4, 2), (True, 4, 4), (True, 8, 4)}, dispatched


# ------------------------------------------------------- (b) the edge nodes
@pytest.mark.parametrize("mode", ["auto", "serial"])
@pytest.mark.parametrize("name", ["falling-1-1", "offset-3-1", "peaked-1-1"])
def test_zero_allocatable_and_over_capacity_nodes(name, mode):
    w = R.edge_stream()
    ref = R.edge_reference(name)
    # the stream holds both: memory-less nodes that take pods, nodes beyond their cpu capacity
    st = ref[1][1]
    assert ((st["alloc_mem"] == 0) & (st["pod_count"] > 0)).sum() > 50 and (st["nz_cpu"] > st["alloc_cpu"]).sum() > 50
    with Scheduler(R.N_EDGE, pods_per_round=128, options={"resolve_mode": MODES[mode]}) as s:
        R.use(s, name)
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
            got = s.schedule_raw(W.pods_at(w["pods"], lo), cnt)
            assert_results_equal(got, ref[call][0], cnt, f"edge nodes {name} {mode} call {call}")
            assert np.array_equal(all_states(s, R.N_EDGE), ref[call][1]), f"edge nodes {name}: node state differs"
        # and the dump on them: a request-less pod against the filled cluster
        pa, _, want = R.edge_dump_reference(name)
        out = (_abi.KsNodeScore * R.N_EDGE)()
        assert s.lib.ks_plugin_scores(s.ctx, pa, out) == 0, s.lib.ks_last_error(s.ctx)
        g = scores_np(out, R.N_EDGE)
        assert np.array_equal(g, want), np.nonzero(g != want)[0][:5]


# ---------------------------------------------------- (c) ks_plugin_scores
@pytest.mark.parametrize("name", ["falling-3-1", "peaked-1-1", "flat-1-0"])
def test_plugin_scores_plain_pod(name):
    w = wide_workload()
    a = Arena()
    pa, _ = pods_array(wide_pods(0, 40, 8)[3:4], a)  # preferred terms: a normalising pod
    r = RtcrReference(CAP_B, R.case(name))
    r.upsert(w["nodes"], w["slots"], w["n"])
    with Scheduler(CAP_B) as s:
        R.use(s, name)
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        out = (_abi.KsNodeScore * CAP_B)()
        assert s.lib.ks_plugin_scores(s.ctx, pa, out) == 0, s.lib.ks_last_error(s.ctx)
        got, want = scores_np(out, CAP_B), r.plugin_scores(pa)
        assert (want["status"] == -1).sum() > 100
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    r.close()


# ------------------------------------------------- (d) the commit under pile-up
def run_pile(s, ref):
    w = W.pile_stream()
    s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
    for call, (lo, cnt) in enumerate([(0, w["m1"]), (w["m1"], w["m"] - w["m1"])]):
        got = s.schedule_raw(W.pods_at(w["pods"], lo), cnt)
        assert_results_equal(got, ref[call][0], cnt, f"pile-up call {call}")
        assert np.array_equal(all_states(s, W.N_PILE), ref[call][1]), "pile-up: node state differs"
    return np.concatenate([res_array(ref[0][0], w["m1"]), res_array(ref[1][0], w["m"] - w["m1"])])


@pytest.mark.parametrize("dedup", [1, 0])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("K", [256, 8])
def test_pile_up_peaked(K, mode, dedup):
    # the peaked shape: a node's key rises to utilisation 50 and falls beyond it
    with Scheduler(W.N_PILE, pods_per_round=256, topk=K,
                   options={"resolve_mode": MODES[mode], "dedup_identical_pods": dedup}) as s:
        R.use(s, "peaked-1-1")
        r = run_pile(s, R.pile_reference("peaked-1-1"))
        ok = r["status"] == 0
        assert ok[:700].all() and (~ok).sum() >= 150
        assert np.bincount(r["node_index"][ok]).max() == 3
        # back to the default strategy on the same context, over fresh nodes: the closed form takes its rounds again
        use_plain(s, DEFAULT)
        assert s.get_fit_shape() == []
        s.delete_slots(list(range(W.N_PILE)))
        run_pile(s, W.pile_reference("default"))
        k = counters(s)
        if dedup and mode != "serial" and K == 256:
            assert k[CTR_ONESTEP] > 0, f"the closed form no longer resolves LeastAllocated rounds {k}"


@pytest.mark.parametrize("name", ["binpack-3-1", "falling-1-0", "offset-1-1", "flat-1-1"])
def test_pile_up_other_shapes(name):
    with Scheduler(W.N_PILE, pods_per_round=256) as s:
        R.use(s, name)
        run_pile(s, R.pile_reference(name))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind_name,name", [("hetero", "binpack-1-1"), ("labeled", "peaked-3-1")])
def test_heterogeneous_stream(kind_name, name, mode):
    w = W.hetero_stream(kind_name)
    want, states = R.hetero_reference(kind_name, name)
    with Scheduler(W.N_H, pods_per_round=W.P_H, options={"resolve_mode": MODES[mode]}) as s:
        R.use(s, name)
        W.hetero_setup(s, w)
        got = s.schedule_raw(w["ps"].pods, w["m"])
        assert_results_equal(got, want, w["m"], f"{kind_name} stream {name}, resolve {mode}")
        assert np.array_equal(all_states(s, W.N_H), states)


# --------------------------------------------------- (e) strategy switch
def test_strategy_and_shape_switch_on_a_live_context():
    w = W.hetero_stream("hetero")
    P = W.P_H
    r = RtcrReference(W.N_H)
    W.hetero_setup(r, w)
    with Scheduler(W.N_H, pods_per_round=P) as s:
        W.hetero_setup(s, w)
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1}) and s.get_fit_shape() == []
        for b, name in enumerate(["peaked-1-1", "falling-3-1", None]):
            ptr = W.pods_at(w["ps"].pods, b * P)
            if name is None:
                # prepared under one shape, run after a switch to another strategy: the run's counts
                R.use(s, "binpack-1-1")
                batch = s.prepare(ptr, P)
                use_plain(s, (MOST, 1, 1))
                r.set_strategy((MOST, 1, 1))
                s.run(batch)
                got = s.results(batch, P)
                s.free(batch)
            elif b == 1:
                # prepared under the first shape, run under the second
                batch = s.prepare(ptr, P)
                R.use(s, name)
                r.set_strategy(R.case(name))
                s.run(batch)
                got = s.results(batch, P)
                s.free(batch)
            else:
                R.use(s, name)
                r.set_strategy(R.case(name))
                got = s.schedule_raw(ptr, P)
            assert_results_equal(got, r.schedule(ptr, P), P, f"batch {b} under {name}")
            assert np.array_equal(all_states(s, W.N_H), r.states()), f"batch {b}: node state differs"
    r.close()


# ------------------------------------------------------------ (f) refusals
def pts(shape):
    return (_abi.KsFitShapePoint * max(1, len(shape)))(*[_abi.KsFitShapePoint(u, v) for u, v in shape]), len(shape)


def test_refusals():
    lib = _abi.ksched_lib()
    good, n_good = pts(SHAPES["peaked"])
    with Scheduler(64) as s:
        fs = _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, 1, 1, 0)
        # the strategy call itself has no shape
        assert lib.ks_set_fit_strategy(s.ctx, C.byref(fs)) == _abi.KS_ERR_INVALID
        with pytest.raises(_abi.KschedError):
            s.set_fit_strategy(RTCR)
        for bad in [(), ((0, 11),), ((0, -1),), ((101, 5),), ((-1, 5),), ((10, 1), (10, 2)), ((20, 1), (10, 2)),
                    tuple((min(i, 100), 1) for i in range(102))]:
            p, n = pts(bad)
            assert lib.ks_set_fit_strategy_shape(s.ctx, C.byref(fs), p, n) == _abi.KS_ERR_INVALID, bad
        assert lib.ks_set_fit_strategy_shape(s.ctx, C.byref(fs), None, 3) == _abi.KS_ERR_INVALID
        assert lib.ks_set_fit_strategy_shape(s.ctx, None, good, n_good) == _abi.KS_ERR_INVALID
        for w in [(101, 1), (1, 101), (0, 0), (-1, 1)]:
            bw = _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, *w, 0)
            assert lib.ks_set_fit_strategy_shape(s.ctx, C.byref(bw), good, n_good) == _abi.KS_ERR_INVALID, w
        # a shape with another type
        most = _abi.KsFitStrategy(_abi.FIT_MOST_ALLOCATED, 1, 1, 0)
        assert lib.ks_set_fit_strategy_shape(s.ctx, C.byref(most), good, n_good) == _abi.KS_ERR_INVALID
        # refused calls change nothing
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1}) and s.get_fit_shape() == []
        s.set_fit_strategy(RTCR, {"cpu": 100, "memory": 7}, SHAPES["offset"])
        assert s.get_fit_strategy() == (RTCR, {"cpu": 100, "memory": 7})
        assert s.get_fit_shape() == list(SHAPES["offset"])
        n = C.c_uint32()
        out = (_abi.KsFitShapePoint * 1)()
        assert lib.ks_get_fit_shape(s.ctx, out, 1, C.byref(n)) == _abi.KS_ERR_INVALID and n.value == 2  # too small
        assert lib.ks_get_fit_shape(s.ctx, out, 1, None) == _abi.KS_ERR_INVALID
        s.set_fit_strategy(RTCR, {"memory": 2}, [(0, 0), (100, 10)])  # a resource left out is not listed
        assert s.get_fit_strategy() == (RTCR, {"cpu": 0, "memory": 2})
        s.set_fit_strategy(MOST)  # the other types carry no shape
        assert s.get_fit_strategy() == (MOST, {"cpu": 1, "memory": 1}) and s.get_fit_shape() == []
    with Scheduler(64, percentage_of_nodes_to_score=5) as s:
        fs = _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, 1, 1, 0)
        assert lib.ks_set_fit_strategy_shape(s.ctx, C.byref(fs), good, n_good) == _abi.KS_ERR_UNSUPPORTED
        assert s.get_fit_strategy() == (LEAST, {"cpu": 1, "memory": 1})
    with pytest.raises(_abi.KschedError):
        Scheduler(64, percentage_of_nodes_to_score=5, fit_strategy=RTCR, fit_shape=[(0, 0), (100, 10)])
    with Scheduler(64, fit_strategy=RTCR, fit_resource_weights={"cpu": 3, "memory": 1},
                   fit_shape=[(0, 0), (100, 10)]) as s:
        assert s.get_fit_strategy() == (RTCR, {"cpu": 3, "memory": 1}) and s.get_fit_shape() == [(0, 0), (100, 10)]
