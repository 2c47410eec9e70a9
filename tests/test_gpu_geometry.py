"""The sweep's pod-group and wide-lane variants at small shapes.

The other small GPU tests run the sweep in one corner of its geometry: one
pod per sweep block (pg = 1), the label / taint kernels at 2 nodes per lane,
every execution option at its default.  The geometry the benchmark runs
(dozens of pods per block, a partial last group) is otherwise reached only by
the 50k to 1M-node replays.  Here clusters of 1,500 to 4,100 nodes force it
with sweep_pairs / sweep_pairs_ext, ext_nodes_per_lane and the stream options,
and every case reads back what it ran (ks_debug_sweep_geometry) before it
compares every result field and every node's state with the CPU oracle:

(a) pod groups: groups x pods-per-group shapes up to the LDS bound of 64, with
    partial last groups, early round ends (topk = 4), the dedup list cutting
    a group short, and FIX re-sweeps;
(b) every label / taint instantiation of launch_sweep: (nodes per lane, label
    words) in {2, 4} x {1, 2, 4} and (8, 4), as the dictionary widens over
    three batches on one context;
(c) the round records (every listed node's fused TotalScore) under the wide
    variants;
(d) the hand-built scenarios with their nodes spread over every step of a
    lane and over several blocks;
(e) the stream options (value_sync, resolve_cus, side_cus) over a dozen rounds.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
from helpers import assert_results_equal, assert_round_records, oracle_keys, res_array, state_array
from ksched import Scheduler, _abi, synth
from ksched.objects import (Arena, NodeSelectorRequirement as Req, NodeSelectorTerm as Term,
                            PreferredSchedulingTerm as Pref, Taint, Toleration, nodes_array, pods_array)
from scenarios import SCENARIOS, check, node, pod

pytestmark = pytest.mark.gpu

Gi = 1 << 30
LAUNCHES, KNPL, LWU, SUB, BLOCKS, GROUPS, PG = range(7)  # ks_debug_sweep_geometry words


def geometry(s, ext):
    g = (C.c_uint64 * 8)()
    assert s.lib.ks_debug_sweep_geometry(s.ctx, 1 if ext else 0, g) == 0, s.lib.ks_last_error(s.ctx)
    return [int(x) for x in g]


def counters(s):
    k = (C.c_uint64 * 16)()
    assert s.lib.ks_debug_counters(s.ctx, k) == 0, s.lib.ks_last_error(s.ctx)
    return [int(x) for x in k]


def pods_at(arr, start):
    return C.cast(C.addressof(arr) + start * C.sizeof(_abi.KsPod), C.POINTER(_abi.KsPod))


def all_states(t, cap):
    return state_array(t.node_states(list(range(cap))))


def spread(n, cap):
    """n distinct slots spread evenly over cap.  Slot l of a shard of W layout
    waves sits at step l // (64 W), so a cluster that fills the low slots of
    its capacity leaves a lane's last steps empty (1,500 nodes at 4 per lane:
    step 3 holds nothing); spread over a capacity that is a whole number of
    blocks, the nodes reach every step, and every wave has empty lanes."""
    assert cap >= n
    return (C.c_uint32 * n)(*[i * cap // n for i in range(n)])


# ------------------------------------------------------------ (a) pod groups
N_A, CAP_A = 1500, 2048  # npl 4: 8 layout waves -> 2 blocks (4 at 2 nodes per lane), all with holes
# pods per round, pod groups, pods per group, pods of the last group
SHAPES = [(256, 4, 64, 64), (200, 4, 64, 8), (100, 2, 64, 36), (65, 2, 64, 1), (7, 1, 7, 7), (256, 128, 2, 2),
          (256, 5, 52, 48),   # the 1M-node resource-only shape
          (256, 9, 29, 24)]   # the 1M-node label / taint shape
KINDS = {"hetero": (synth.HETERO, False, 2), "labeled": (synth.LABELED, True, 4)}  # kind, ext, blocks expected


@functools.lru_cache(maxsize=None)
def group_workload(kind_name, P):
    """Nodes, prefill and a pod stream for rounds of P pods, with the oracle's
    results and node states after each of the two calls (computed once).

    The stream is no multiple of P, is split mid-round, and its first round
    holds a run of identical request-less pods, so the round's dedup list is
    shorter than P and ends inside a pod group."""
    kind = KINDS[kind_name][0]
    ns = synth.nodes(kind, N_A, 71)
    slots = spread(N_A, CAP_A)
    pf = synth.prefill(kind, N_A, 71, 72, 0.5)  # names nodes by their index
    pf_slots = (C.c_uint32 * pf.n_pods)(*[slots[pf.slot_ptr[j]] for j in range(pf.n_pods)])
    run = max(3, P // 3)
    head = P // 2 + 1
    m = 2 * P + P // 3 + run
    assert m % P != 0 and head + run <= P
    # every fifth pod of a LABELED stream carries preferred terms (a
    # normalising pod), however short the stream
    src = synth.pods(kind, 8 * (m - run) + 64, 73)
    pref = [i for i in range(src.n_pods) if src.pods[i].n_preferred]
    rest = [i for i in range(src.n_pods) if not src.pods[i].n_preferred]
    assert kind != synth.LABELED or len(pref) >= m
    pick = [pref.pop(0) if pref and j % 5 == 2 else rest.pop(0) for j in range(m - run)]
    be = synth.besteffort_pods(run)
    arr = (_abi.KsPod * m)()
    for j in range(m):
        arr[j] = src.pods[pick[j]] if j < head else be.pods[j - head] if j < head + run else src.pods[pick[j - run]]
    m1 = P + P // 2 + 1
    o = pyoracle.Oracle(CAP_A)
    o.upsert(ns.nodes, slots, N_A)
    o.add_pods(pf.pods, pf_slots, pf.n_pods)
    want1 = o.schedule(pods_at(arr, 0), m1)
    st1 = all_states(o, CAP_A)
    want2 = o.schedule(pods_at(arr, m1), m - m1)
    st2 = all_states(o, CAP_A)
    o.close()
    return dict(ns=ns, slots=slots, pf=pf, pf_slots=pf_slots, arr=arr, m=m, m1=m1, want=(want1, want2), states=(st1, st2), keep=(src, be))


def run_groups(kind_name, shape, K, options):
    P, groups, pg, last = shape
    assert P - (groups - 1) * pg == last and 0 < last <= pg
    _, ext, blocks = KINDS[kind_name]
    w = group_workload(kind_name, P)
    # pg = 64 (and a single group) need at most one (block, group) pair per
    # block; any other group count takes that many pairs per block
    pairs = 1 if pg == min(P, 64) else groups * blocks
    opts = dict(options, sweep_pairs=pairs, sweep_pairs_ext=pairs)
    with Scheduler(CAP_A, pods_per_round=P, topk=K, options=opts) as s:
        s.upsert_nodes_raw(w["ns"].nodes, w["slots"], N_A)
        assert s.lib.ks_pods_add(s.ctx, w["pf"].pods, w["pf_slots"], w["pf"].n_pods) == 0
        m, m1 = w["m"], w["m1"]
        for call, (lo, cnt) in enumerate([(0, m1), (m1, m - m1)]):
            got = s.schedule_raw(pods_at(w["arr"], lo), cnt)
            what = f"{kind_name} {groups}x{pg} P={P} K={K} call {call}"
            assert_results_equal(got, w["want"][call], cnt, what)
            assert np.array_equal(all_states(s, CAP_A), w["states"][call]), f"{what}: node state differs"
            g = geometry(s, ext)
            assert g[LAUNCHES] > 0 and geometry(s, not ext)[LAUNCHES] == 0, g
            assert (g[KNPL], g[SUB], g[BLOCKS]) == ((2, 2, 4) if ext else (4, 1, 2)), g
            assert (g[GROUPS], g[PG]) == (groups, pg), g
        return counters(s), m


@pytest.mark.parametrize("K", ["P", 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: f"P{t[0]}-{t[1]}x{t[2]}")
@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_pod_groups(kind_name, shape, K):
    P = shape[0]
    k, m = run_groups(kind_name, shape, P if K == "P" else K, {})
    assert k[7] > 0, f"no identical pod was skipped: the dedup list cut no group short {k}"
    if K == 4:
        # lists of 4 run out: rounds end early and the next ones start mid-batch
        assert k[0] > -(-m // P), f"{k[0]} rounds for {m} pods: no round ended early"


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: f"P{t[0]}-{t[1]}x{t[2]}")
def test_pod_groups_fix_resweep(shape, early):
    # plain normaliser guesses: wrong ones are re-swept in FIX mode, behind the
    # sweep (early_fix 1) or behind the merge (0)
    k, _ = run_groups("labeled", shape, shape[0], {"tuple_guess": 0, "early_fix": early})
    assert k[4] > 0, f"no pod was re-swept {k}"
    assert k[7] > 0, k


# ------------------------------------- (b) every label / taint sweep variant
N_B, CAP_B = 2100, 4096  # whole blocks at 2, 4 and 8 nodes per lane
RACKS = [f"r{v}" for v in range(200)]
# (nodes_per_lane, ext_nodes_per_lane) -> the label / taint kernel's nodes per lane
LANES = {(4, 2): 2, (4, 4): 4, (8, 4): 4, (8, 8): 8, (2, 8): 2}
ALL_VARIANTS = {(2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4), (8, 4)}  # launch_sweep's label / taint branch
dispatched = set()  # (kernel nodes per lane, label words) the read-back reported, over the module


def lane_id(lanes):
    return f"npl{lanes[0]}-ext{lanes[1]}"


def wide_cluster():
    nodes = []
    for i in range(N_B):
        labels = {"rack": RACKS[i % 200], "zone": f"z{i % 5}", "gen": str(i % 9)}
        if i % 3 == 0:
            labels["ssd"] = ""
        taints = []
        if i % 11 == 0:
            taints.append(Taint("dedicated", "batch", "NoSchedule"))
        if i % 13 == 0:
            taints.append(Taint("maint", "", "NoSchedule"))
        if i % 4 == 0:
            taints.append(Taint("spot", "true", "PreferNoSchedule"))
        if i % 6 == 0:
            taints.append(Taint("old", "true", "PreferNoSchedule"))
        nodes.append(node(f"w{i}", cpu=(8 + 8 * (i % 5)) * 1000, mem=(32 << (i % 4)) * Gi, pods=110,
                          labels=labels, taints=taints))
    return nodes


def wide_pods(batch, R, count):
    """Pods whose label programs reference rack values r0..r{R-1}: In, NotIn,
    Exists, Gt, a metadata.name term, required and preferred terms."""
    T = lambda *reqs, fields=(): Term(list(reqs), list(fields))  # noqa: E731
    vals = RACKS[:R]
    pods = []
    for j in range(count):
        kw = {}
        lo = (j * 7) % R
        some = [vals[(lo + 3 * q) % R] for q in range(1 + j % 9)]
        kind = j % 8
        if kind == 0:
            kw["required_terms"] = [T(Req("rack", "In", some))]
        elif kind == 1:
            kw["required_terms"] = [T(Req("rack", "NotIn", vals[R // 2:] if j % 16 == 1 else some))]
        elif kind == 2:
            kw["required_terms"] = [T(Req("ssd", "Exists"), Req("rack", "In", vals))]
        elif kind == 3:
            kw["preferred"] = [Pref(10 + j % 50, T(Req("rack", "In", some))),
                               Pref(5 + j % 7, T(Req("zone", "In", [f"z{j % 5}"])))]
        elif kind == 4:
            kw["required_terms"] = [T(Req("gen", "Gt" if j % 16 == 4 else "Lt", ["4"]))]
            kw["preferred"] = [Pref(20, T(Req("rack", "NotIn", some)))]
        elif kind == 5:
            name = f"w{(j * 131 + batch) % N_B}"
            kw["required_terms"] = [T(fields=[Req("metadata.name", "In", [name])]),
                                    T(Req("rack", "In", [vals[R - 1], vals[lo]]))]
        elif kind == 6:
            kw["node_selector"] = {"rack": vals[R - 1 - j % 4]}
            kw["tolerations"] = [Toleration("dedicated", "Equal", "batch", "NoSchedule"),
                                 Toleration("spot", "Exists", "", "PreferNoSchedule")]
        else:
            kw["tolerations"] = [Toleration("", "Exists", "", "")]
        cpu = 100 + 37 * (j % 23)
        if j % 24 == 0:  # fits nowhere: rejected with NodeAffinity, taint and fit failure counts
            cpu = 10 ** 7
        if j % 24 == 2:  # no node passes: gen <= 8 everywhere
            kw["required_terms"][0].match_expressions.append(Req("gen", "Gt", ["8"]))
        pods.append(pod(f"b{batch}-{j}", cpu=cpu, mem=(1 + j % 7) * Gi // 4, **kw))
    return pods


WIDE_BATCHES = [(40, 150, 1), (100, 150, 2), (200, 150, 4)]  # rack values referenced so far, pods, label words


@functools.lru_cache(maxsize=None)
def wide_workload():
    a = Arena()
    na, n = nodes_array(wide_cluster(), a)
    slots = spread(n, CAP_B)
    o = pyoracle.Oracle(CAP_B)
    o.upsert(na, slots, n)
    batches = []
    for b, (R, count, _) in enumerate(WIDE_BATCHES):
        pa, m = pods_array(wide_pods(b, R, count), a)
        want = o.schedule(pa, m)
        batches.append((pa, m, want, all_states(o, CAP_B)))
        r = res_array(want, m)
        assert (r["status"] == 0).sum() > m // 2 and (r["status"] == 1).any(), "batch neither places nor rejects"
    o.close()
    return dict(arena=a, nodes=na, n=n, slots=slots, batches=batches)


@pytest.mark.parametrize("pg", [64, 1])
@pytest.mark.parametrize("lanes", sorted(LANES), ids=lane_id)
def test_label_word_variants(lanes, pg):
    npl, ext_npl = lanes
    knpl = LANES[lanes]
    w = wide_workload()
    P = 128
    opts = {"ext_nodes_per_lane": ext_npl}
    if pg == 64:
        opts["sweep_pairs_ext"] = 1  # else the default: a pod per block at this size
    with Scheduler(CAP_B, pods_per_round=P, nodes_per_lane=npl, options=opts) as s:
        s.upsert_nodes_raw(w["nodes"], w["slots"], w["n"])
        for b, (pa, m, want, states) in enumerate(w["batches"]):
            got = s.schedule_raw(pa, m)
            g = geometry(s, True)
            words = 4 if knpl == 8 else WIDE_BATCHES[b][2]
            what = f"npl {npl}/{ext_npl} pg {pg} batch {b}"
            assert g[LAUNCHES] > b and (g[KNPL], g[LWU], g[SUB]) == (knpl, words, npl // knpl), (what, g)
            assert (g[GROUPS], g[PG]) == ((2, 64) if pg == 64 else (P, 1)), (what, g)
            dispatched.add((g[KNPL], g[LWU]))
            assert_results_equal(got, want, m, what)
            assert np.array_equal(all_states(s, CAP_B), states), f"{what}: node state differs"


# --------------------------------- (c) round records under the wide variants
def record_pods():
    """16 pods over disjoint rack sets (no two compete for a node, so one round
    resolves them all) that between them name all 200 rack values.  A pod's
    racks are 12 consecutive ones: rack r is on nodes r + 200 k, so they
    reach every layout wave and thus every sweep block."""
    T = lambda *reqs: Term(list(reqs))  # noqa: E731
    pods = []
    for i in range(16):
        mine = [RACKS[r] for r in range(200) if (r // 12) % 16 == i]
        kw = {"required_terms": [T(Req("rack", "In", mine))]}
        if i % 2:
            kw["preferred"] = [Pref(30, T(Req("rack", "In", mine[:3]))), Pref(7, T(Req("zone", "NotIn", ["z1"])))]
        if i % 3 == 0:
            kw["tolerations"] = [Toleration("spot", "Exists", "", "PreferNoSchedule")]
        if i % 4 == 0:
            kw["required_terms"] = [T(Req("rack", "In", mine), Req("gen", "Gt", ["2"]))]
        pods.append(pod(f"rec{i}", cpu=500 + 100 * i, mem=(1 + i % 3) * Gi, **kw))
    return pods


@pytest.mark.parametrize("lanes", [(4, 4), (8, 8)], ids=lane_id)
def test_round_records_wide_variants(lanes):
    npl, ext_npl = lanes
    w = wide_workload()
    n, K = w["n"], 256
    a = Arena()
    pa, m = pods_array(record_pods(), a)
    o = pyoracle.Oracle(CAP_B)
    o.upsert(w["nodes"], w["slots"], n)
    want = [oracle_keys(o, pods_at(pa.contents, i)) for i in range(m)]  # round-start state
    with Scheduler(CAP_B, pods_per_round=16, topk=K, nodes_per_lane=npl,
                   options={"ext_nodes_per_lane": ext_npl, "sweep_pairs_ext": 1}) as s:
        s.upsert_nodes_raw(w["nodes"], w["slots"], n)
        got = s.schedule_raw(pa, m)
        assert_results_equal(got, o.schedule(pa, m), m, f"records npl {npl}/{ext_npl}")
        g = geometry(s, True)
        assert (g[LAUNCHES], g[KNPL], g[LWU], g[GROUPS], g[PG]) == (1, LANES[lanes], 4, 1, 16), g
        dispatched.add((g[KNPL], g[LWU]))
        assert counters(s)[0] == 1, "round 0 stopped early and its records were re-swept"
        r = res_array(got, m)
        assert (r["status"] == 0).all()
        listed = assert_round_records(s, want, r, m, K)
        # every block holds feasible nodes of every pod and lists its best one
        assert g[BLOCKS] >= 2 and listed >= m * g[BLOCKS], f"only {listed} keys listed over {m} pods"
    o.close()


# ----------------------------- (d) scenarios spread over steps and blocks
SPREAD_WAVES = 8  # layout waves: two sweep blocks at one kernel wave per layout wave


def spread_slots(n, npl):
    """n distinct slots spread evenly over a capacity of 64 * waves * npl.  A
    slot's step is slot // (64 * waves) and its layout wave slot % waves."""
    cap = 64 * SPREAD_WAVES * npl
    return [i * cap // n + (i * 5) % SPREAD_WAVES for i in range(n)], cap


def test_spread_slots_cover_steps_and_blocks():
    for npl in (4, 8):
        steps = set()
        for name in SCENARIOS:
            n = len(SCENARIOS[name]()[0])
            slots, cap = spread_slots(n, npl)
            assert len(set(slots)) == n and max(slots) < cap and slots == sorted(slots)
            steps |= {sl // (64 * SPREAD_WAVES) for sl in slots}
            assert len({(sl % SPREAD_WAVES) // 4 for sl in slots}) == 2, (name, slots)
        assert steps == set(range(npl))


@pytest.mark.parametrize("lanes", [(4, 2), (4, 4), (8, 8)], ids=lane_id)
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_spread_over_steps(name, lanes):
    npl, ext_npl = lanes
    nodes, pods, exp = SCENARIOS[name]()
    a = Arena()
    na, n = nodes_array(nodes, a)
    pa, m = pods_array(pods, a)
    sl, cap = spread_slots(n, npl)
    slots = (C.c_uint32 * n)(*sl)
    o = pyoracle.Oracle(cap)
    o.upsert(na, slots, n)
    want = o.schedule(pa, m)
    with Scheduler(cap, nodes_per_lane=npl,
                   options={"ext_nodes_per_lane": ext_npl, "sweep_pairs": 1, "sweep_pairs_ext": 1}) as s:
        s.upsert_nodes_raw(na, slots, n)
        got = s.schedule_raw(pa, m)
        assert np.array_equal(all_states(s, cap), all_states(o, cap)), f"{name}: node state differs"
        ran = 0
        for ext in (False, True):
            g = geometry(s, ext)
            if g[LAUNCHES]:
                knpl = LANES[lanes] if ext else npl
                assert (g[KNPL], g[SUB], g[GROUPS], g[PG]) == (knpl, npl // knpl, 4, 64), (ext, g)
                assert g[BLOCKS] == SPREAD_WAVES * g[SUB] // 4, g
                if ext:
                    dispatched.add((g[KNPL], g[LWU]))
                ran += 1
        assert ran, "no sweep was launched"
    o.close()
    assert_results_equal(got, want, m, name)
    # the scenario's expectations name nodes by their index: now at slots[index]
    moved = [dict(e, node=sl[e["node"]]) if e.get("node") is not None else e for e in exp]
    check(res_array(got, m), moved)


# ------------------------------------------------------- (e) stream options
N_E, M_E, P_E = 2000, 1500, 128
STREAM_OPTIONS = [{"value_sync": 0}, {"resolve_cus": 0}, {"side_cus": 8},
                  {"side_cus": 8, "resolve_cus": 4, "value_sync": 0}]


@functools.lru_cache(maxsize=None)
def stream_workload(kind_name):
    kind = KINDS[kind_name][0]
    ns = synth.nodes(kind, N_E, 81)
    ps = synth.pods(kind, M_E, 82)
    pf = synth.prefill(kind, N_E, 81, 83, 0.5)
    o = pyoracle.Oracle(N_E)
    o.upsert(ns.nodes, synth.slot_array(N_E), N_E)
    o.add_pods(pf.pods, pf.slot_ptr, pf.n_pods)
    want = o.schedule(ps.pods, M_E)
    states = all_states(o, N_E)
    o.close()
    return ns, ps, pf, want, states


@pytest.mark.parametrize("options", STREAM_OPTIONS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("kind_name,early", [("hetero", 1), ("labeled", 1), ("labeled", 0)])
def test_stream_options(kind_name, early, options):
    ext = KINDS[kind_name][1]
    ns, ps, pf, want, states = stream_workload(kind_name)
    with Scheduler(N_E, pods_per_round=P_E, options=dict(options, early_fix=early)) as s:
        s.upsert_nodes_raw(ns.nodes, synth.slot_array(N_E), N_E)
        assert s.lib.ks_pods_add(s.ctx, pf.pods, pf.slot_ptr, pf.n_pods) == 0
        got = s.schedule_raw(ps.pods, M_E)
        what = f"{kind_name} early_fix {early} {options}"
        assert_results_equal(got, want, M_E, what)
        assert np.array_equal(all_states(s, N_E), states), f"{what}: node state differs"
        g = geometry(s, ext)
        # a dozen rounds or more, so every hand-off recurs; the default geometry
        assert g[LAUNCHES] >= -(-M_E // P_E) and geometry(s, not ext)[LAUNCHES] == 0, g
        assert (g[KNPL], g[GROUPS], g[PG]) == (2 if ext else 4, P_E, 1), g
        assert counters(s)[0] >= 12


# ------------------------------------------------------------ module check
def test_every_label_variant_was_dispatched():
    # runs last in this module: the cases above reported, from the read-back,
    # every instantiation of launch_sweep's label / taint branch
    assert dispatched == ALL_VARIANTS, f"never dispatched: {sorted(ALL_VARIANTS - dispatched)}"
