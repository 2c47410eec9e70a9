"""Score plugin weights other than the default profile's in every kernel
family: each case compares every result field and every
node's state with the oracle (or the composed reference) under the same
weights, and reads back what shows that the intended kernel ran.  The vectors
and workloads are tests/weight_cases.py's; tests/test_weight_cases.py shows on
the CPU that each (workload, vector) pair used here with a discriminating
vector moves at least a tenth of the placements, so a swapped, defaulted or
truncated weight fails these cases.

(a) the resource-only sweep and the in-order commit;
(b) the general NodeResourcesFit variants of the sweep;
(c) the label / taint sweep, its FIX re-sweep and the commit's normalisers;
(d) the one-pod chain: PodTopologySpread, InterPodAffinity, ImageLocality,
    strategy and balanced lists, the percentageOfNodesToScore window;
(e) replica runs at every width of the sort key;
(f) ks_plugin_scores and ks_explain;
(g) two ranks.
"""
import functools
import random

import numpy as np
import pytest

import weight_cases as WC
from helpers import WEIGHT_PLUGINS, res_array, scores_array, states_np, weight_forms
from ksched import Scheduler, _abi
from ksched.objects import pods_array
from test_gpu_geometry import GROUPS, KNPL, LAUNCHES, PG, counters, geometry
from test_gpu_spread import Pair
from test_weight_cases import COLS, composed, terms_of

pytestmark = pytest.mark.gpu

V = WC.VECTORS
ROUNDS, RESWEPT, CPU_SHARED = 0, 4, 9  # ks_debug_counters
P_S = 57  # pods per round of the stream cases: three pod groups of 19 (two batches of 8 and a part)
MODES = {"auto": _abi.RESOLVE_AUTO, "serial": _abi.RESOLVE_SERIAL, "parallel": _abi.RESOLVE_PARALLEL}


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)}/{len(want)} results differ; first at pod {i}: got {got[i]} want {want[i]}")


def run_stream(w, vec, ref, what, m=None, K=0, npl=4, shards=1, options=None, use=None, ext=False):
    """The stream on a context under the vector: results and node states equal
    `ref`'s.  Returns (results, the sweep geometry read back, the counters)."""
    m = w["m"] if m is None else m
    knpl = min(npl, (options or {}).get("ext_nodes_per_lane", 2)) if ext else npl  # the kernel's nodes per lane
    # layout waves (a multiple of 4) of npl x 64 slots; a block holds four kernel waves of knpl x 64
    waves = -(-w["cap"] // (64 * npl * 4)) * 4
    blocks = waves * (npl // knpl) // 4
    # three pod groups per block (with virtual shards: at least that many)
    opts = dict(options or {}, **{"sweep_pairs_ext" if ext else "sweep_pairs": 3 * blocks * shards})
    with Scheduler(w["cap"], pods_per_round=P_S, topk=K, nodes_per_lane=npl, virtual_shards=shards, options=opts,
                   **weight_forms(vec)[0]) as s:
        if use:
            use(s)
        WC.load(s, w)
        got = res_array(s.schedule_raw(w["pods"], m), m)
        assert_same(got, ref[0], what)
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, w["cap"]), ref[1]), f"{what}: node state differs"
        g = geometry(s, ext)
        assert g[LAUNCHES] > 0 and geometry(s, not ext)[LAUNCHES] == 0, (what, g)
        assert g[KNPL] == knpl, (what, g)
        if shards == 1:
            assert (g[GROUPS], g[PG]) == (3, 19), (what, g)
        return got, g, counters(s)


# --------------------------------------- (a) resource-only sweep and commit
@pytest.mark.parametrize("vec_name", ["PRIME", "CAP", "CAP_ALL", "SKEW", "ZERO"])
@pytest.mark.parametrize("kind", ["hetero", "kwok"])
def test_resource_only_stream(kind, vec_name):
    vec = V[vec_name]
    r, _, k = run_stream(WC.synth_stream(kind), vec, WC.synth_reference(kind, vec), f"{kind} {vec_name}")
    assert k[CPU_SHARED] > 0, f"no list entry kept its predecessor's cpu terms {k}"
    if vec_name == "ZERO":
        assert (r["total_score"] == 0).all()
    if vec_name == "CAP_ALL":
        assert int(r["total_score"].max()) > (1 << 21)


@pytest.mark.parametrize("vec_name", ["PRIME", "CAP"])
@pytest.mark.parametrize("npl", [2, 8])
def test_resource_only_lanes(npl, vec_name):
    vec = V[vec_name]
    _, _, k = run_stream(WC.synth_stream("hetero"), vec, WC.synth_reference("hetero", vec), f"npl {npl} {vec_name}",
                         npl=npl)
    assert k[CPU_SHARED] > 0, k


@pytest.mark.parametrize("vec_name", ["PRIME", "CAP"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind", ["hetero", "kwok"])
def test_resolve_modes(kind, mode, vec_name):
    # the commit re-scores live rows on its own: every mode equals the oracle, hence each other
    vec = V[vec_name]
    run_stream(WC.synth_stream(kind), vec, WC.synth_reference(kind, vec), f"{kind} resolve {mode} {vec_name}",
               options={"resolve_mode": MODES[mode]})


@pytest.mark.parametrize("kind", ["hetero", "kwok"])
def test_short_lists(kind):
    # lists of 4 run out: rounds end early and the re-score on live rows decides
    w = WC.synth_stream(kind)
    _, _, k = run_stream(w, WC.PRIME, WC.synth_reference(kind, WC.PRIME), f"{kind} topk 4", K=4)
    assert k[ROUNDS] > -(-w["m"] // P_S), f"{k[ROUNDS]} rounds: no round ended early"


@pytest.mark.parametrize("shards", [2, 5])
@pytest.mark.parametrize("kind", ["hetero", "labeled"])
def test_virtual_shards(kind, shards):
    # the cross-shard merge orders the shards' totals
    run_stream(WC.synth_stream(kind), WC.PRIME, WC.synth_reference(kind, WC.PRIME), f"{kind} {shards} shards",
               shards=shards, ext=kind == "labeled")


@functools.lru_cache(maxsize=None)
def default_profile_run(kind, mode):
    """The stream under the default weights on the same context configuration
    (the existing suite pins it; it equals the oracle here too)."""
    return run_stream(WC.synth_stream(kind), WC.DEFAULT, WC.synth_reference(kind, WC.DEFAULT), f"{kind} default",
                      options={"resolve_mode": MODES[mode]}, ext=kind == "labeled")[0]


@pytest.mark.parametrize("mode", ["auto", "serial"])
@pytest.mark.parametrize("name", sorted(WC.SCALES))
@pytest.mark.parametrize("kind", ["hetero", "labeled"])
def test_scaled_weights_scale_the_totals(kind, name, mode):
    # metamorphic, no trust in the oracle's weighting: c x the default weights decides as the default profile
    # does and every TotalScore is c times its
    c = WC.SCALES[name]
    base = default_profile_run(kind, mode)
    r, _, _ = run_stream(WC.synth_stream(kind), V[name], WC.synth_reference(kind, V[name]), f"{kind} {name}",
                         options={"resolve_mode": MODES[mode]}, ext=kind == "labeled")
    for f in ("node_index", "status", "feasible", "evaluated", "fail", "flags"):
        assert np.array_equal(r[f], base[f]), (kind, name, f)
    assert np.array_equal(r["total_score"], c * base["total_score"]), (kind, name)


# ------------------------------------------------ (b) general Fit variants
@pytest.mark.parametrize("vec_name", ["PRIME", "CAP"])
@pytest.mark.parametrize("strategy", sorted(WC.GF_CASES))
def test_general_fit_variants(strategy, vec_name):
    vec = V[vec_name]
    run_stream(WC.synth_stream("hetero"), vec, WC.gf_reference(strategy, vec), f"{strategy} {vec_name}", m=WC.M_GF,
               use=lambda s: WC.gf_use(s, strategy))


# ------------------------------------------------ (c) label / taint sweep
LABEL_VECTORS = ["PRIME", "CAP", "SKEW", f"ONE_HOT{WC.TAINT}", f"ONE_HOT{WC.AFFINITY}"]


@pytest.mark.parametrize("vec_name", LABEL_VECTORS)
def test_labeled_stream(vec_name):
    vec = V[vec_name]
    run_stream(WC.synth_stream("labeled"), vec, WC.synth_reference("labeled", vec), f"labeled {vec_name}", ext=True)


@pytest.mark.parametrize("vec_name", ["PRIME", "CAP"])
@pytest.mark.parametrize("lanes", [(4, 4), (8, 8), (8, 4)], ids=lambda t: f"npl{t[0]}-ext{t[1]}")
def test_labeled_lanes(lanes, vec_name):
    vec = V[vec_name]
    run_stream(WC.synth_stream("labeled"), vec, WC.synth_reference("labeled", vec), f"labeled {lanes} {vec_name}",
               npl=lanes[0], options={"ext_nodes_per_lane": lanes[1]}, ext=True)


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("vec_name", LABEL_VECTORS)
def test_normaliser_cluster_fix_resweep(vec_name, early):
    # plain normaliser guesses: four pods of five are re-swept in FIX mode, behind the sweep (early_fix 1) or
    # behind the merge (0), and the commit scores with the measured maxima, all under the weights
    vec = V[vec_name]
    w = WC.normaliser_stream()
    _, _, k = run_stream(w, vec, WC.normaliser_reference(vec), f"normaliser {vec_name} early {early}",
                         options={"tuple_guess": 0, "early_fix": early}, ext=True)
    assert k[RESWEPT] >= w["flagged"], f"not every wrongly guessed pod was re-swept {k}"


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("vec_name", ["PRIME", "SKEW"])
def test_labeled_stream_fix_resweep(vec_name, early):
    vec = V[vec_name]
    _, _, k = run_stream(WC.synth_stream("labeled"), vec, WC.synth_reference("labeled", vec),
                         f"labeled {vec_name} early {early}", options={"tuple_guess": 0, "early_fix": early}, ext=True)
    assert k[RESWEPT] > 0, f"no pod was re-swept {k}"


# ----------------------------------------------------- (d) one-pod chain
def chain_pair(name, vec, **cfg):
    """libksched and the workload's reference under the vector, fed the same events."""
    _, n, make, pct = WC.CHAIN[name]
    kw = dict(weight_forms(vec)[0], **cfg)
    if name == "xfit":
        import xfit_workloads
        from test_gpu_xfit import XfitPair
        x = XfitPair(n, *xfit_workloads.CASES[WC.XFIT_CASE], pods_per_round=64, **kw)
    elif name == "ba":
        from test_gpu_ba import BaPair
        x = BaPair(n, WC.BA_CASE, pods_per_round=64, **kw)
    else:
        if pct != 100:
            kw["percentage_of_nodes_to_score"] = pct
        x = Pair(n, **kw)
    if make or pct != 100:
        x.o.close()
        x.o = WC.chain_reference_object(name, vec)
    return x


def run_chain(name, vec, **cfg):
    x = chain_pair(name, vec, **cfg)
    try:
        WC.CHAIN[name][0](x)  # every schedule call, dump and state comparison asserts
        r = np.concatenate(x.res)
        assert_same(r, WC.chain_reference(name, vec), f"{name}: the reference the CPU tests judged")
        st = x.s.stats()
        if name == "pct30":
            assert x.s.next_start_index() == x.o.next_start
        return r, st
    finally:
        x.close()


@pytest.mark.parametrize("vec_name", ["PRIME", "SKEW", f"ONE_HOT{WC.SPREAD}"])
def test_topology_spread(vec_name):
    _, st = run_chain("spread", V[vec_name])
    assert st.spread_pods >= 200 and st.replica_pods == 0, (st.spread_pods, st.replica_pods)


def hand_cases():
    import ipa_cases
    import spread_cases
    return [("spread", k) for k in sorted(spread_cases.CASES)] + [("ipa", k) for k in sorted(ipa_cases.CASES)]


@pytest.mark.parametrize("family,name", hand_cases())
def test_hand_built_cases(family, name):
    # tests/spread_cases.py and tests/ipa_cases.py under PRIME: their hand-derived expectations are the default
    # profile's, so here the oracle under PRIME alone judges results, dumps and node states
    mod = __import__(f"{family}_cases")
    nodes, bound, pods, _, dumps = mod.CASES[name]()
    x = Pair(len(nodes), **weight_forms(WC.PRIME)[0])
    try:
        x.upsert(nodes, list(range(len(nodes))))
        x.add([p for p, _ in bound], [s for _, s in bound])
        for j in sorted(dumps):
            x.dump_equal(pods[j], f"{name} dump {j}")
        x.schedule(pods, name)
        x.states_equal(name)
    finally:
        x.close()


@pytest.mark.parametrize("ipa", [0, 2, 17])
@pytest.mark.parametrize("hard", [0, 1, 100])
def test_inter_pod_affinity(hard, ipa):
    _, st = run_chain("ipa", WC.DEFAULT[:6] + (ipa, hard))
    assert st.spread_pods > 0


@pytest.mark.parametrize("vec_name", ["PRIME", "SKEW"])
def test_inter_pod_affinity_vectors(vec_name):
    run_chain("ipa", V[vec_name])


@pytest.mark.parametrize("vec_name", [f"ONE_HOT{WC.IMAGE}", "PRIME"])
def test_image_locality(vec_name):
    _, st = run_chain("image", V[vec_name])
    assert st.spread_pods > 0


@pytest.mark.parametrize("name", ["xfit", "ba", "pct30"])
def test_strategy_balanced_list_and_window(name):
    r, st = run_chain(name, WC.PRIME)
    assert (r["status"] == 0).sum() > 100 and st.spread_pods > 0


# ------------------------------------------------------- (e) replica runs
@pytest.mark.parametrize("runs", [1, 0])
@pytest.mark.parametrize("case", list(WC.REPLICA_CASES))
def test_replica_runs_key_widths(case, runs):
    # the sort key is 20 + s_bits wide, s_bits the bit length of 100 x (fit + balanced + taint + affinity):
    # 1, 7, 9, 10, 11 and 22 bits.  Runs on and off equal the oracle, hence each other.
    vec, bits = WC.REPLICA_CASES[case]
    assert WC.s_bits(vec) == bits
    r, st = run_chain("replica", vec, options={"spread_replica_runs": runs})
    assert (r["status"] == 0).sum() > 400
    if runs:
        assert st.replica_runs > 0 and st.replica_pods > 0, (st.replica_runs, st.replica_pods)
    else:
        assert st.replica_runs == 0


@pytest.mark.parametrize("runs", [1, 0])
def test_replica_runs_nodes_fill(runs):
    # taken nodes are re-scored with the weights; runs end at Fit losses
    _, st = run_chain("fill", WC.PRIME, options={"spread_replica_runs": runs})
    assert (st.replica_pods > 0) == bool(runs)


# ----------------------------------------------------- (f) read-only calls
def readonly_pods(rng):
    from test_gpu_explain import pref_pod
    from test_gpu_spread import IMAGES, rand_ipa_pod, rand_pod, rand_res_pod
    pods = []
    for j in range(4):
        pods += [rand_pod(rng, 4 * j, spread_frac=1.0), rand_ipa_pod(rng, 4 * j + 1, frac=1.0, spread_frac=0.0),
                 pref_pod(rng, 4 * j + 2)]
        p = rand_res_pod(rng, 4 * j + 3)
        p.containers[0].image = IMAGES[j][0]
        pods.append(p)
    return pods


@pytest.mark.parametrize("vec_name", ["PRIME", "SKEW"])
def test_plugin_scores_and_explain(vec_name):
    from test_gpu_spread import rand_ipa_pod, rand_res_nodes
    vec = V[vec_name]
    rng = random.Random(107)
    n, k = 500, 16
    x = Pair(n, **weight_forms(vec)[0])
    x.upsert(WC.soft_taints(rng, rand_res_nodes(rng, n)), list(range(n)))
    pre = [rand_ipa_pod(rng, 10_000 + j, frac=0.4, spread_frac=0.0) for j in range(n // 2)]
    for p in pre:
        p.affinity_terms = [t for t in p.affinity_terms if t.kind != "anti-affinity"]
    x.add(pre, [rng.randrange(n) for _ in pre])
    assert tuple(x.s.weights[p] for p in WEIGHT_PLUGINS) == vec[:7]
    checked = 0
    for p in readonly_pods(rng):
        sc = scores_array(x.dump_equal(p, f"{vec_name} {p.name}"))  # every record equals the oracle's
        feas = np.nonzero(sc[:, 0] == -1)[0]
        if not len(feas):
            continue
        checked += 1
        terms = terms_of(p)
        assert np.array_equal(composed(sc, vec, terms)[feas], sc[feas, COLS["total_score"]]), p.name
        # the oracle's dump, top k by (-TotalScore, slot), and the size of the top score's tie set
        pa, _ = pods_array([p], x.a)
        want = scores_array(x.o.plugin_scores(pa))
        order = feas[np.lexsort((feas, -want[feas, COLS["total_score"]]))]
        top = int(want[order[0], COLS["total_score"]])
        e = x.s.explain(p, k)
        assert (e.feasible_nodes, e.top_score) == (len(feas), top), p.name
        assert e.top_score_nodes == int((want[feas, COLS["total_score"]] == top).sum()), p.name
        assert [c.slot for c in e.candidates] == [int(v) for v in order[:k]], p.name
        for c in e.candidates:
            assert np.array_equal(scores_array([c.raw])[0], want[c.slot]), (p.name, c.slot)
            by_name = {s.name: s.score for s in c.scores}
            assert c.total_score == sum(x.s.weights[name] * by_name[name] for name in terms), (p.name, c.slot)
    assert checked >= 12
    x.close()


# ------------------------------------------------------------ (g) two ranks
def test_two_ranks():
    from test_gpu_multirank import run_case
    r = run_case(world=2, kind=4, nodes=3000, pods=600, node_seed=4, pod_seed=5, P=64, calls=2,
                 weights=list(WC.PRIME))
    assert r["scheduled"] > 300
