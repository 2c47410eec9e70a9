"""The weight vectors and workloads of tests/weight_cases.py on the CPU: what
makes tests/test_gpu_weights.py able to fail.

(a) discrimination: every (workload, vector) pair the GPU tests run with a
    discriminating vector moves at least a tenth of the reference's placements
    away from the default profile's, and a one-hot vector's plugin scores the
    feasible nodes of some pod unequally;
(b) scaling: under c x the default weights every decision is the default
    profile's and every TotalScore c times it;
(c) an independent composition: sum of weight x per-plugin score, from the
    oracle's per-plugin dump, equals the dump's TotalScore on every feasible node;
(d) ks_open's bounds on the eight weight fields (the range check comes before
    ks_open touches a device, so it runs here)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import weight_cases as WC
from helpers import WEIGHT_PLUGINS, scores_array
from ksched import _abi
from ksched.framework import SCORE_FIELDS
from ksched.objects import pods_array


# ---------------------------------------------------------- (a) discrimination
@pytest.mark.parametrize("workload,vec_name", WC.PAIRS, ids=lambda v: str(v))
def test_vector_moves_a_tenth_of_the_placements(workload, vec_name):
    assert vec_name in WC.DISCRIMINATING
    n_moved, n = WC.moved(workload, vec_name)
    print(f"{workload} {vec_name}: {n_moved} of {n} placements differ from the default profile's")
    assert 10 * n_moved >= n, (workload, vec_name, n_moved, n)


def pod_ptr(arr, j):
    return C.cast(C.cast(arr, C.c_void_p).value + j * C.sizeof(_abi.KsPod), C.POINTER(_abi.KsPod))


COLS = {"status": 0, "least_allocated": 1, "balanced_allocation": 2, "taint_score": 4, "affinity_score": 6,
        "image_locality": 7, "spread_score": 9, "affinity_pod_score": 11, "total_score": 12}  # helpers.scores_array


def chain_probe(name, vec, pick):
    """The oracle after a chain workload's events, and dumps of `pick`ed pods
    of its last batch: [(pod, scores_array)]."""
    seen = []

    class Probe(WC.OraclePair):
        def schedule(self, pods, what=""):
            out = []
            for p in pods:
                if pick(p) and len(out) < 6:
                    pa, _ = pods_array([p], self.a)
                    out.append((p, scores_array(self.o.plugin_scores(pa))))
            seen[:] = out or seen
            return super().schedule(pods, what)

    x = Probe(WC.CHAIN[name][1], pyoracle.Oracle(WC.CHAIN[name][1], vec))
    WC.CHAIN[name][0](x)
    x.close()
    assert seen, name
    return seen


def stream_probe(w, vec, idx):
    o = pyoracle.Oracle(w["cap"], vec)
    WC.load(o, w)
    out = [scores_array(o.plugin_scores(pod_ptr(w["pods"], j))) for j in idx]
    o.close()
    return out


def varies(dumps, field):
    """Some dump's feasible nodes take more than one value of the field."""
    return any(len(set(sc[sc[:, 0] == -1, COLS[field]].tolist())) > 1 for sc in dumps)


def test_one_hot_plugins_score_the_feasible_nodes_unequally():
    lab = WC.synth_stream("labeled")
    pref = [j for j in range(lab["m"]) if lab["pods"][j].n_preferred][:8]
    d = stream_probe(lab, WC.DEFAULT, pref + list(range(8)))
    assert varies(d, "taint_score") and varies(d, "affinity_score"), "labeled stream"
    nz = WC.normaliser_stream()
    d = stream_probe(nz, WC.DEFAULT, list(range(10)))
    assert varies(d, "taint_score") and varies(d, "affinity_score"), "normaliser cluster"
    assert varies([sc for _, sc in chain_probe("spread", WC.DEFAULT, lambda p: True)], "spread_score")
    assert varies([sc for _, sc in chain_probe("image", WC.DEFAULT, lambda p: True)], "image_locality")
    assert varies([sc for _, sc in chain_probe("ipa", WC.DEFAULT, lambda p: p.affinity_terms)], "affinity_pod_score")


def test_ipa_weights_change_the_outcome():
    # the InterPodAffinity cases run (hard, ipa) pairs, no named vector: each pair's outcome is its own
    base = WC.chain_reference("ipa", WC.DEFAULT)
    # (a plugin weight of 0 takes hardPodAffinityWeight out with the rest of the plugin's score)
    seen = {}
    for hard in (0, 1, 100):
        for ipa in (0, 2, 17):
            r = WC.chain_reference("ipa", WC.DEFAULT[:6] + (ipa, hard))
            seen.setdefault(tuple(r["total_score"].tolist()), []).append((hard, ipa))
    assert sorted(seen.values()) == [[(0, 0), (1, 0), (100, 0)], [(0, 2)], [(0, 17)], [(1, 2)], [(1, 17)], [(100, 2)],
                                     [(100, 17)]], sorted(seen.values())
    # hard 0 against hard 1, ipa 2: the bound pods' required terms alone move placements
    r = WC.chain_reference("ipa", WC.DEFAULT[:6] + (2, 0))
    assert (r["node_index"] != base["node_index"]).any()


def test_replica_cases_step_the_key_width():
    assert [WC.s_bits(v) for v, _ in WC.REPLICA_CASES.values()] == [b for _, b in WC.REPLICA_CASES.values()]
    assert [b for _, b in WC.REPLICA_CASES.values()] == [1, 7, 9, 10, 11, 22]
    assert WC.s_bits(WC.DEFAULT) == 10
    # each case's outcome on the replica workload is its own
    seen = []
    for name, (vec, _) in WC.REPLICA_CASES.items():
        r = WC.chain_reference("replica", vec)
        key = (r["node_index"].tolist(), r["total_score"].tolist())
        assert key not in seen, name
        seen.append(key)


# ------------------------------------------------------------------ (b) scaling
@pytest.mark.parametrize("workload", WC.WORKLOADS)
def test_scaled_weights_scale_the_totals(workload):
    base = WC.reference(workload, WC.DEFAULT)
    assert (base["status"] == 0).sum() > len(base) // 4
    for name, c in WC.SCALES.items():
        r = WC.reference(workload, WC.VECTORS[name])
        for f in ("node_index", "status", "feasible", "evaluated", "fail", "flags"):
            assert np.array_equal(r[f], base[f]), (workload, name, f)
        assert np.array_equal(r["total_score"], c * base["total_score"]), (workload, name)


def test_cap_all_and_zero_are_range_cases():
    # the symmetric cap decides as the all-ones profile; all zeros ties every feasible node at 0
    for workload in ("hetero", "kwok", "replica"):
        ones, cap = WC.reference(workload, (1,) * 8), WC.reference(workload, WC.CAP_ALL)
        assert np.array_equal(cap["node_index"], ones["node_index"])
        assert np.array_equal(cap["total_score"], 10000 * ones["total_score"])
    z = WC.reference("hetero", WC.ZERO)
    assert (z["total_score"] == 0).all() and (z["status"] == 0).any()
    assert int(WC.reference("hetero", WC.CAP_ALL)["total_score"].max()) > (1 << 21)  # the key's top bits are in use


# ------------------------------------------- (c) an independent composition
def composed(sc, vec, terms):
    """Sum of weight x normalised score over the plugins whose PreScore ran."""
    t = np.zeros(len(sc), dtype=np.int64)
    for k, plugin in enumerate(WEIGHT_PLUGINS):
        if plugin in terms:
            t += vec[k] * sc[:, COLS[SCORE_FIELDS[plugin]]]
    return t


ALWAYS = {"NodeResourcesFit", "NodeResourcesBalancedAllocation", "TaintToleration", "ImageLocality", "InterPodAffinity"}


def terms_of(pod):
    """The score plugins that take part for a ksched.objects.Pod: NodeAffinity
    with preferred terms, PodTopologySpread with a ScheduleAnyway constraint;
    InterPodAffinity's score is 0 where its PreScore skips."""
    t = set(ALWAYS)
    if pod.preferred:
        t.add("NodeAffinity")
    if any(c.when_unsatisfiable == "ScheduleAnyway" for c in pod.topology_spread):
        t.add("PodTopologySpread")
    return t


def check_composition(sc, vec, terms, what):
    """Returns whether the pod had a feasible node to compare on."""
    feas = sc[:, 0] == -1
    got, want = composed(sc, vec, terms)[feas], sc[feas, COLS["total_score"]]
    assert np.array_equal(got, want), (what, got[:4], want[:4])
    return bool(feas.any())


@pytest.mark.parametrize("vec_name", ["PRIME", "SKEW"])
def test_total_is_the_weighted_sum_of_the_plugin_scores(vec_name):
    vec = WC.VECTORS[vec_name]
    # resource-only and label / taint pods of the synth streams
    for kind in ("hetero", "kwok", "labeled"):
        w = WC.synth_stream(kind)
        pref = [j for j in range(w["m"]) if w["pods"][j].n_preferred][:8]
        plain = [j for j in range(w["m"]) if not w["pods"][j].n_preferred][:8]
        assert bool(pref) == (kind == "labeled")
        for group in (pref, plain):
            terms = ALWAYS | ({"NodeAffinity"} if group is pref else set())
            done = sum(check_composition(sc, vec, terms, f"{kind} pod {j}")
                       for j, sc in zip(group, stream_probe(w, vec, group)))
            assert done >= 3 or not group, (kind, done)
    nz = WC.normaliser_stream()
    assert all(check_composition(sc, vec, terms_of(nz["pypods"][j]), f"normaliser pod {j}")
               for j, sc in zip(range(6), stream_probe(nz, vec, list(range(6)))))
    # spread, affinity and image pods of the chain workloads
    n_any = 0
    for name, pick in (("spread", lambda p: p.topology_spread), ("ipa", lambda p: p.affinity_terms),
                       ("image", lambda p: True), ("replica", lambda p: True)):
        done = 0
        for p, sc in chain_probe(name, vec, pick):
            done += check_composition(sc, vec, terms_of(p), f"{name} pod {p.name}")
            n_any += "PodTopologySpread" in terms_of(p)
        assert done >= 3, (name, done)
    assert n_any > 0


# ------------------------------------------------------ (d) ks_open's bounds
FIELDS = ["weight_fit", "weight_balanced", "weight_taint", "weight_affinity", "weight_image",
          "weight_topology_spread", "weight_inter_pod_affinity", "hard_pod_affinity_weight"]


@pytest.mark.parametrize("field", FIELDS)
def test_ks_open_weight_bounds(field):
    lib = _abi.ksched_lib()
    for value, ok in ((0, True), (10000, True), (-1, False), (10001, False)):
        cfg = _abi.KsConfig()
        lib.ks_config_default(C.byref(cfg))
        cfg.node_capacity = 64
        setattr(cfg, field, value)
        ctx = C.c_void_p()
        st = lib.ks_open(C.byref(cfg), C.byref(ctx))
        if st == 0:
            lib.ks_close(ctx)
        if ok:  # accepted: open, or no device in this machine -- never KS_ERR_INVALID
            assert st in (_abi.KS_OK, _abi.KS_ERR_DEVICE), (field, value, st)
        else:
            assert st == _abi.KS_ERR_INVALID and not ctx.value, (field, value, st)
