"""ks_diagnose_pods on the GPU (ksched_diag_batch.hip): every
answer against ks_diagnose's for the same pod and, where the test has one,
against the closed-form answer or tests/diag_reference.py; which path answered
is read from ks_debug_diagnose_pods' counters: [0] the multi-pod kernel's
pods, [1] the per-pod pass's, [2] identical pods, [3] pods run again after a
full list, [4] launches, [5] pods per group, [6] positions per launch turn."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import diag_reference as R
from helpers import states_np
from ksched import Scheduler, _abi
from ksched.objects import Arena, Container, Node, Pod, Taint, Toleration, pods_array
from test_gpu_diag import (DiagPair, assert_same, geometry_nodes, geometry_pod, geometry_want, u32)
from test_gpu_spread import rand_ipa_pod, rand_nodes, rand_pod, rand_res_nodes, rand_res_pod

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Gi, Mi = 1 << 30, 1 << 20
TAINT = R.TAINT
BIG = {"cpu": 4000, "memory": 8 * Gi, "pods": 110}


def geometry_pods(m, first=0):
    """geometry_pod() with cpu requests 100 + i: one expected answer, no two pods identical."""
    out = []
    for i in range(first, first + m):
        p = geometry_pod()
        p.name = f"p{i}"
        p.containers = [Container({"cpu": 100 + i, "memory": 128 * Mi})]
        out.append(p)
    return out


# ----------------------------------------------------------------- geometry
@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_geometry(n):
    a = Arena()
    slots = list(range(n))
    want = geometry_want(slots)
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        G = s.diagnose_pods_counters()[5]
        assert G >= 2
        for m in sorted({1, 2, 63, 64, 65, G - 1, G, G + 1, 2 * G + 3}):
            got = s.diagnose_many(geometry_pods(m))
            assert len(got) == m
            for i, d in enumerate(got):
                assert_same(d, want, (n, m, i))
            c = s.diagnose_pods_counters()
            assert c[0] == m and c[1] == 0 and c[2] == 0, (n, m, c)
            assert c[4] == 1 and c[7] == 0, (n, m, c)  # one launch: every pod reads the label columns
            # slot 3 of every seven carries two untolerated taints: the list holds 4 x n pairs
            assert (c[3] > 0) == (m * len([x for x in slots if x % 7 == 3]) > 4 * n), (n, m, c)


def test_geometry_grid_stride_second_turn():
    # just above the positions one launch covers in a turn: the loop's second step, its last wave partly past the end
    a = Arena()
    with Scheduler(1) as s0:
        turn = s0.diagnose_pods_counters()[6]
    assert 0 < turn <= 600_000
    n = turn + 100
    slots = list(range(n))
    want = geometry_want(slots)
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        got = s.diagnose_many(geometry_pods(3))
        for i, d in enumerate(got):
            assert_same(d, want, i)
        c = s.diagnose_pods_counters()
        assert c[0] == 3 and c[1] == 0 and c[3] == 0 and c[6] == turn < n, c


# ------------------------------------------------------------------- taints
def test_whole_taint_dictionary():
    n = 70
    nodes = [Node(f"n{i}", BIG, {}, [Taint(f"k{i % 63}", f"v{i % 63}")]) for i in range(n)]
    pods = [Pod(f"p{i}", containers=[Container({"cpu": 10 + i})],
                tolerations=[Toleration(f"k{i % 63}", "Equal", f"v{i % 63}")] if i < 63 else []) for i in range(65)]
    with Scheduler(n) as s:
        s.upsert_nodes(nodes, list(range(n)))
        got = s.diagnose_many(pods)
        c = s.diagnose_pods_counters()
        assert c[0] == 65 and c[1] == 0 and c[2] == 0 and c[3] == 0, c
        for i, d in enumerate(got):
            assert d == s.diagnose(pods[i]), i
            want = {TAINT % (f"k{b}", f"v{b}"): (2 if b < 7 else 1) for b in range(63) if i >= 63 or b != i}
            assert d.reasons == want and d.feasible_nodes == (0 if i >= 63 else 2 if i < 7 else 1), i


def test_several_untolerated_taints():
    # dictionary bits follow first appearance: x 0, y 1, z 2; the last node lists them as z, x, y
    nodes = [Node("n0", BIG, {}, [Taint("x", "")]), Node("n1", BIG, {}, [Taint("y", "")]),
             Node("n2", BIG, {}, [Taint("z", "")]), Node("n3", BIG, {}, [Taint("z", ""), Taint("x", ""), Taint("y", "")])]
    subsets = [[], ["x"], ["y"], ["z"], ["x", "y"], ["x", "z"], ["y", "z"], ["x", "y", "z"]]
    pods = [Pod(f"p{i}", tolerations=[Toleration(k, "Exists") for k in ks]) for i, ks in enumerate(subsets)]
    with Scheduler(4) as s:
        s.upsert_nodes(nodes, [0, 1, 2, 3])
        got = s.diagnose_many(pods)
        c = s.diagnose_pods_counters()
        assert c[0] == 8 and c[1] == 0 and c[3] == 0, c
        assert got[0].reasons == {TAINT % ("x", ""): 1, TAINT % ("y", ""): 1, TAINT % ("z", ""): 2}
        assert got[3].reasons == {TAINT % ("x", ""): 2, TAINT % ("y", ""): 1}  # z tolerated: n3 reports x
        assert got[7].reasons == {} and got[7].feasible_nodes == 4
        for p, d in zip(pods, got):
            assert d == s.diagnose(p), p.name


def test_shared_list_overflows():
    # 64 nodes with three untolerated taints each, in rotating order; the list holds 4 x 64 pairs, so the fifth
    # distinct pod's entries no longer fit: those pods are run again, one at a time
    n = 64
    keys = ["x", "y", "z", "w"]
    nodes = [Node(f"n{i}", BIG, {}, [Taint(keys[(i + k) % 4], "") for k in range(3)]) for i in range(n)]
    pods = [Pod(f"p{i}", containers=[Container({"cpu": 10 + i})],
                tolerations=[Toleration("w", "Exists")] if i % 3 == 0 else []) for i in range(12)]
    with Scheduler(n) as s:
        s.upsert_nodes(nodes, list(range(n)))
        got = s.diagnose_many(pods)
        c = s.diagnose_pods_counters()
        assert c[0] == 12 and c[1] == 0 and c[3] > 0, c
        for p, d in zip(pods, got):
            assert d == s.diagnose(p), p.name
            assert sum(d.reasons.values()) == n and d.plugin_nodes[2] == n


# ---------------------------------------------------- random streams, parity
def many_stream(x, rng, make_pod, batches, per_batch, what):
    """Per batch: diagnose_many against the reference and against diagnose, entry by entry; then the batch is
    scheduled on both.  Returns the counters [0..3] summed over the batches."""
    total = [0, 0, 0, 0]
    for b in range(batches):
        pods = [make_pod(rng, b * 1000 + j) for j in range(per_batch)]
        got = x.s.diagnose_many(pods)
        c = x.s.diagnose_pods_counters()
        assert c[0] + c[1] + c[2] == len(pods), (what, b, c)
        total = [t + v for t, v in zip(total, c[:4])]
        for j, (p, d) in enumerate(zip(pods, got)):
            assert_same(d, x.ref.diagnose(p), f"{what} batch {b} pod {j} (reference)")
            assert d == x.s.diagnose(p), f"{what} batch {b} pod {j} (diagnose)"
        x.schedule_equal(pods, f"{what} batch {b}")
    return total


@pytest.mark.parametrize("seed,n,batches,per_batch", [(41, 300, 3, 40), (42, 1500, 2, 20)])
def test_random_stream_resources(seed, n, batches, per_batch):
    rng = random.Random(seed)
    x = DiagPair(n, pods_per_round=64)
    x.upsert(rand_res_nodes(rng, n), list(range(n)))
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(2 * n)]  # a crowded cluster: NodeResourcesFit has work
    for p in pre:
        p.topology_spread = []
    x.add(pre, [rng.randrange(n) for _ in pre])
    total = many_stream(x, rng, rand_res_pod, batches, per_batch, f"seed {seed}")
    assert total[0] > 0 and total[1] > 0, total
    x.close()


@pytest.mark.parametrize("seed,n,zones,batches,per_batch", [(51, 300, 3, 3, 40), (52, 1200, 10, 2, 20)])
def test_random_stream_affinity(seed, n, zones, batches, per_batch):
    rng = random.Random(seed)
    x = DiagPair(n, pods_per_round=64)
    x.upsert(rand_nodes(rng, n, zones), list(range(n)))
    pre = [rand_ipa_pod(rng, 10_000 + j, frac=0.15, spread_frac=0.0) for j in range(n // 2)]
    x.add(pre, [rng.randrange(n) for _ in pre])

    # one-pod-chain pods and plain pods interleaved: the output order is the input order.  The plain pods live in
    # a namespace of their own: in the stream's namespaces a bound pod's term with an empty selector matches every
    # incoming pod, which then carries an InterPodAffinity record
    def make(g, j):
        if j % 2:
            return rand_ipa_pod(g, j, frac=0.6, spread_frac=0.5)
        req = {"cpu": g.randrange(1, 40) * 50, "memory": g.randrange(1, 64) * 64 * Mi}
        return Pod(f"plain{j}", namespace="plain", containers=[Container(req)],
                   node_selector={"disk": "ssd"} if g.random() < 0.3 else {})
    total = many_stream(x, rng, make, batches, per_batch, f"seed {seed}")
    assert total[0] > 0 and total[1] > 0, total
    x.close()


# ------------------------------------------------------------ identical pods
def test_identical_pods_are_diagnosed_once():
    a = Arena()
    n = 200
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        distinct = geometry_pods(5, first=1)
        copies = geometry_pods(1) * 100
        pods = copies[:30] + distinct[:2] + copies[30:70] + distinct[2:] + copies[70:]
        got = s.diagnose_many(pods)
        c = s.diagnose_pods_counters()
        assert c[0] == 6 and c[1] == 0 and c[2] == 99, c
        want = geometry_want(slots)
        for i, d in enumerate(got):
            assert_same(d, want, i)
        first = got[0]
        assert all(d == first for p, d in zip(pods, got) if p is copies[0])


# -------------------------------------------------------------------- errors
def test_refusals_and_edge_arguments():
    a = Arena()
    n = 70
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        lib, ctx = s.lib, s.ctx
        pods = geometry_pods(2) + [Pod("v", unmodelled=["volumes"])] + geometry_pods(2, first=2)
        pa, m = pods_array(pods, a)
        chk = (C.c_int32 * m)()
        want_st = lib.ks_pods_check(ctx, pa, m, chk)
        assert want_st == _abi.KS_ERR_UNSUPPORTED and list(chk) == [0, 0, want_st, 0, 0]
        out = (_abi.KsPodDiagnosis * m)()
        rows = (_abi.KsReason * (m * _abi.DIAG_MAX_REASONS))()
        cnt = C.c_uint32(0)
        assert lib.ks_diagnose_pods(ctx, pa, m, out, rows, len(rows), C.byref(cnt)) == want_st
        err = lib.ks_last_error(ctx).decode()
        assert err.startswith("pod 2:") and "volumes" in err.lower(), err
        assert [o.status for o in out] == [0, 0, want_st, 0, 0] and cnt.value == 4 * 7
        assert out[2].d.n_reasons == 0 and out[2].d.num_all_nodes == 0
        assert [o.first_reason for o in out if not o.status] == [0, 7, 14, 21]
        assert all(o.d.n_reasons == 7 for o in out if not o.status)
        with pytest.raises(_abi.KschedError) as e:
            s.diagnose_many(pods)
        assert e.value.status == want_st
        got = s.diagnose_many(pods, strict=False)
        assert got[2] is None
        for i in (0, 1, 3, 4):
            assert_same(got[i], geometry_want(slots), i)
        # cap one below the need: KS_ERR_INVALID with *n_reasons (and every diagnosis) set
        pa, m = pods_array(geometry_pods(3), a)
        out = (_abi.KsPodDiagnosis * m)()
        assert lib.ks_diagnose_pods(ctx, pa, m, out, rows, 20, C.byref(cnt)) == _abi.KS_ERR_INVALID
        assert cnt.value == 21 and [o.d.n_reasons for o in out] == [7, 7, 7] and out[1].d.num_all_nodes == n
        assert lib.ks_diagnose_pods(ctx, pa, m, out, None, 0, C.byref(cnt)) == _abi.KS_ERR_INVALID and cnt.value == 21
        assert lib.ks_diagnose_pods(ctx, pa, m, out, rows, 21, C.byref(cnt)) == 0 and cnt.value == 21
        assert [rows[i].plugin for i in range(7)] == [rows[7 + i].plugin for i in range(7)] == [0, 2, 2, 3, 4, 4, 4]
        # n == 0
        cnt.value = 9
        assert lib.ks_diagnose_pods(ctx, None, 0, None, None, 0, C.byref(cnt)) == 0 and cnt.value == 0
        assert s.diagnose_many([]) == []
        # null arguments
        for args in ((None, pa, m, out, rows, 21, C.byref(cnt)), (ctx, None, m, out, rows, 21, C.byref(cnt)),
                     (ctx, pa, m, None, rows, 21, C.byref(cnt)), (ctx, pa, m, out, None, 21, C.byref(cnt)),
                     (ctx, pa, m, out, rows, 21, None)):
            assert lib.ks_diagnose_pods(*args) == _abi.KS_ERR_INVALID
        assert lib.ks_debug_diagnose_pods(ctx, None) == _abi.KS_ERR_INVALID
        # the context still answers
        assert_same(s.diagnose_many(geometry_pods(1))[0], geometry_want(slots))


# ------------------------------------------------------------ no side effects
def test_no_side_effects_and_window_does_not_matter():
    rng = random.Random(61)
    n = 400
    nodes = rand_res_nodes(rng, n)
    for nd in nodes:
        nd.images = []
    pre = [rand_res_pod(rng, 50_000 + j) for j in range(n)]
    for p in pre:
        p.topology_spread, p.init_containers = [], []
    where = [rng.randrange(n) for _ in pre]
    probes = [rand_res_pod(rng, j) for j in range(24)]
    x100, x5 = DiagPair(n), DiagPair(n, percentage_of_nodes_to_score=5)
    for x in (x100, x5):
        x.upsert(nodes, list(range(n)))
        x.add(pre, where)
    first = [Pod(f"f{j}", containers=[Container({"cpu": 10})]) for j in range(3)]
    x5.s.schedule_pods(first)  # moves nextStartNodeIndex off zero
    x100.s.schedule_pods(first)
    start = x5.s.next_start_index()
    assert start != 0
    before100 = states_np(x100.s.lib.ks_node_states, x100.s.ctx, n)
    before5 = states_np(x5.s.lib.ks_node_states, x5.s.ctx, n)
    d100, d5 = x100.s.diagnose_many(probes), x5.s.diagnose_many(probes)
    assert d100 == d5  # a FitError is over every present node, whatever the window
    assert d100 == [x100.s.diagnose(p) for p in probes]
    c100, c5 = x100.s.diagnose_pods_counters(), x5.s.diagnose_pods_counters()
    assert c100[0] > 0 and c100[1] > 0, c100
    assert c5[0] == 0 and c5[1] + c5[2] == len(probes), c5  # with a window every pod is a one-pod-chain pod
    assert x5.s.next_start_index() == start
    assert np.array_equal(states_np(x100.s.lib.ks_node_states, x100.s.ctx, n), before100)
    assert np.array_equal(states_np(x5.s.lib.ks_node_states, x5.s.ctx, n), before5)
    # a following batch equals the reference's (which saw no diagnose call at all)
    x100.ref.schedule(first)
    x100.schedule_equal([rand_res_pod(rng, 7000 + j) for j in range(60)], "after diagnose_many")
    for x in (x100, x5):
        x.close()


def test_domain_scratch_is_left_clean():
    # one-pod-chain pods back to back: their prep passes share the domain scratch; spread pods scheduled
    # afterwards equal the reference's results
    rng = random.Random(62)
    n = 300
    x = DiagPair(n, pods_per_round=64)
    x.upsert(rand_nodes(rng, n, 4), list(range(n)))
    pre = [rand_pod(rng, 20_000 + j, spread_frac=0.0) for j in range(n)]
    x.add(pre, [rng.randrange(n) for _ in pre])
    probes = [rand_pod(rng, j, spread_frac=1.0) for j in range(30)]
    got = x.s.diagnose_many(probes)
    c = x.s.diagnose_pods_counters()
    assert c[1] >= 20 and c[0] == 0, c
    for p, d in zip(probes, got):
        assert_same(d, x.ref.diagnose(p), p.name)
    x.schedule_equal([rand_pod(rng, 1000 + j, spread_frac=1.0) for j in range(60)], "after diagnose_many")
    x.close()


def test_host_port_dictionary_is_not_consumed():
    big = {"cpu": 64000, "memory": 256 * Gi, "pods": 200}
    port_pod = lambda j, port: Pod(f"p{j}", containers=[Container({"cpu": 10})], host_ports=[(None, "TCP", port)])
    with Scheduler(4) as s:
        s.upsert_nodes([Node(f"n{i}", big) for i in range(4)], [0, 1, 2, 3])
        s.add_pods([port_pod(900, 8000)], [1])
        # 64 fresh triples and a held one, between plain pods, diagnosed only
        pods = [Pod("a", containers=[Container({"cpu": 10})])] + [port_pod(j, 1000 + j) for j in range(64)] + \
            [port_pod(99, 8000), Pod("b", containers=[Container({"cpu": 20})])]
        got = s.diagnose_many(pods)
        c = s.diagnose_pods_counters()
        # (a fresh triple conflicts with nothing: the pods asking for one compile alike and are diagnosed once)
        assert c[0] == 2 and c[1] >= 2 and c[1] + c[2] == 65, c
        assert all(d.feasible_nodes == 4 and d.reasons == {} for d in got[:65] + got[66:])
        assert got[65].reasons == {R.PORTS: 1} and got[65].node_ports_nodes == 1 and got[65].feasible_nodes == 3
        assert s.node_used_ports(0) == [] and s.node_used_ports(1) == [("0.0.0.0", "TCP", 8000)]
        # the dictionary still has room for 63 more triples: none of the diagnosed ones was interned
        res = s.schedule_pods([port_pod(100 + j, 2000 + j) for j in range(63)])
        assert all(not isinstance(r, Exception) for r in res)


def test_strings_of_an_earlier_diagnose_stay_valid():
    a = Arena()
    n = 70
    slots = list(range(n))
    with Scheduler(n) as s:
        s.upsert_nodes_raw(geometry_nodes(slots, a), u32(slots), n)
        lib, ctx = s.lib, s.ctx
        pa1, _ = pods_array([geometry_pod()], a)
        d, cnt = _abi.KsDiagnosis(), C.c_uint32(0)
        one = (_abi.KsReason * 16)()
        assert lib.ks_diagnose(ctx, pa1, C.byref(d), one, 16, C.byref(cnt)) == 0 and cnt.value == 7
        ptr = lambda r: C.c_void_p.from_buffer(r, _abi.KsReason.reason.offset).value  # the pointer itself
        addr = [ptr(one[i]) for i in range(7)]
        text = [one[i].reason for i in range(7)]
        # a call with other reasons (a pod that tolerates a and asks for too much memory)
        other = Pod("o", containers=[Container({"cpu": 10, "memory": 64 * Gi})], tolerations=[Toleration("a", "Exists")])
        pa, m = pods_array([other] + geometry_pods(3), a)
        out = (_abi.KsPodDiagnosis * m)()
        rows = (_abi.KsReason * (m * _abi.DIAG_MAX_REASONS))()
        total = C.c_uint32(0)
        assert lib.ks_diagnose_pods(ctx, pa, m, out, rows, len(rows), C.byref(total)) == 0
        mine = [(ptr(rows[i]), rows[i].reason) for i in range(total.value)]
        assert not set(addr) & {p for p, _ in mine}  # storage of its own
        assert [one[i].reason for i in range(7)] == text
        assert [ptr(one[i]) for i in range(7)] == addr
        # ... and the other way round: a ks_diagnose leaves this call's strings
        assert lib.ks_diagnose(ctx, pa1, C.byref(d), one, 16, C.byref(cnt)) == 0
        assert [(ptr(rows[i]), rows[i].reason) for i in range(total.value)] == mine


# ------------------------------------------------------------------ two ranks
def test_two_ranks():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    p = subprocess.run([sys.executable, os.path.join(HERE, "diag_pods_multirank_main.py")], capture_output=True,
                       text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert res["ok"], res["error"]
    assert res["diagnosed"] >= 30 and res["kernel_pods"] > 0 and res["chain_pods"] > 0


# ---------------------------------------------------------- submitted batches
def test_waits_for_submitted_batches():
    rng = random.Random(71)
    n = 2000
    a = Arena()
    nodes = rand_res_nodes(rng, n)
    with Scheduler(n, pods_per_round=64) as s:
        s.upsert_nodes(nodes, list(range(n)))
        batches = [[rand_res_pod(rng, b * 1000 + j) for j in range(150)] for b in range(3)]
        arrs = [pods_array(p, a) for p in batches]
        probes = [rand_res_pod(rng, 9000 + j) for j in range(20)]
        hs = []
        for pa, m in arrs:
            h = s.prepare(pa, m)
            assert s.lib.ks_batch_submit(s.ctx, h) == 0, s.lib.ks_last_error(s.ctx)
            hs.append(h)
        got = s.diagnose_many(probes)  # while the batches are in flight
        for h in hs:
            assert s.lib.ks_batch_wait(s.ctx, h) == 0, s.lib.ks_last_error(s.ctx)
            s.free(h)
        assert got == [s.diagnose(p) for p in probes]
        assert any(d.reasons for d in got)
