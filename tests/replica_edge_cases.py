"""Workloads that put a replica run (ksched_spread.hip replica_keys_kernel,
replica_groups_kernel, replica_run_kernel) on its limits: 512
groups, 512 taken nodes, hostname counts of 0..254, the 512-entry histogram of
domain offsets of DoNotSchedule runs, no feasible node, every candidate
blocked, pods of more than two selector classes, nodes lacking a key and a
single feasible node.  Plain Python over Node / Pod objects, small clusters
built by hand: tests/test_oracle_replica_edges.py runs them on the CPU oracle
alone and holds each to the condition that makes it mean something,
tests/test_gpu_replica_edges.py on the device next to the oracle.

A case is a dict: nodes, bound [(pod, slot)] and steps, one batch each.  A
step is a dict: pods, what, pre(r) -- the condition on the oracle's results r
-- and expect(r) -> (replica_runs, replica_pods), what ks_stats must show for
the batch.  expect restates ksched_host.cpp's loop over a sequence of identical
pods (host_loop below) with the rule by which the case's runs end, fed with
the oracle's results, never the device's."""
import numpy as np

from ksched.objects import (Container, LabelSelector, Node, Pod, TopologySpreadConstraint as TSC,
                            system_default_spread)
from scenarios import AFFINITY, SPREAD

Gi, Mi = 1 << 30, 1 << 20
ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"
SEL = LabelSelector({"app": "web"})
DNS, ANYWAY = "DoNotSchedule", "ScheduleAnyway"
PIN = {"pin": "y"}

RUN_GROUPS = 512    # ksched_kernels.hpp: (domain, hostname count) groups a run holds; more: refused
RUN_TOUCHED = 512   # ksched_kernels.hpp: distinct nodes one run takes, then it ends
RUN_MIN_PODS = 4    # ksched_kernels.hpp: shorter sequences take the per-pod chain
RK_HK_NONE = 255    # ksched_kernels.hpp: hostname counts 0..254; 255: the node lacks the key
RUN_HIST = 512      # ksched_spread.hip: offsets above the start's minimum a DoNotSchedule run tracks
END, FIT, FULL = 0, 1, 2  # ksched_kernels.hpp RunStop
SINGLE = 1          # ksched.h KS_RESULT_SINGLE_FEASIBLE


def node(i, labels=None, host=True, cpu=64000):
    """64 cpu, 256 GiB, 400 pods: no case here ends on a Fit loss."""
    lab = {HOST: f"n{i}"} if host else {}
    lab.update(labels or {})
    return Node(f"n{i}", {"cpu": cpu, "memory": 256 * Gi, "pods": 400}, lab)


def replicas(name, m, spread, labels=None, defaulted=False, **kw):
    """m identical pods (only the names differ)."""
    return [Pod(f"{name}-{j}", containers=[Container({"cpu": 100, "memory": 128 * Mi})],
                labels=dict(labels or {"app": "web"}), topology_spread=list(spread), spread_defaulted=defaulted, **kw)
            for j in range(m)]


def defaults(m, name="web", sel=SEL, labels=None, **kw):
    return replicas(name, m, system_default_spread(sel), labels, True, **kw)


def prefilled(slot, k, labels=None):
    return [(Pod(f"b{slot}-{j}", containers=[Container({"cpu": 10})], labels=dict(labels or {"app": "web"})), slot)
            for j in range(k)]


def step(pods, what, expect=None, pre=None):
    return dict(pods=pods, what=what, expect=expect, pre=pre or (lambda r: None))


def host_loop(m, run):
    """ksched_host.cpp's loop over m identical pods.  run(hi) -> (pods, RunStop)
    of the run that starts at pod hi; 0 pods: refused.  A sequence of fewer
    than RUN_MIN_PODS pods takes the chain; so does the rest after a refused
    run and after a run that a Fit loss (or every candidate blocked) ended
    short of RUN_MIN_PODS pods.  Any other stop starts the next run."""
    hi = runs = 0
    while m - hi >= RUN_MIN_PODS:
        done, stop = run(hi)
        assert 0 <= done <= m - hi
        if done == 0:
            break
        runs, hi = runs + 1, hi + done
        if stop == FIT and done < RUN_MIN_PODS:
            break
    return runs, hi


def whole(r):
    """One run takes the batch."""
    return host_loop(len(r), lambda hi: (len(r) - hi, END))


def refused(r):
    return host_loop(len(r), lambda hi: (0, END))


def all_scheduled(r):
    assert (r["status"] == 0).all(), np.nonzero(r["status"])[0][:5]


# ------------------------------------------------------------ 1. taken-node cap

TOUCHED_N = 560
TOUCHED_M = [RUN_TOUCHED, RUN_TOUCHED + 1, RUN_TOUCHED + RUN_MIN_PODS - 1, RUN_TOUCHED + RUN_MIN_PODS]


def touched_cap(m):
    """m replicas that each take a fresh node: a run ends after its 512th
    taken node unless that pod is the sequence's last."""
    nodes = [node(i, {ZONE: f"z{i % 3}"}) for i in range(TOUCHED_N)]

    def pre(r):
        all_scheduled(r)
        assert len(set(r["node_index"].tolist())) == m <= TOUCHED_N

    def expect(r):
        slots = r["node_index"].tolist()

        def run(hi):
            seen = set()
            for k, s in enumerate(slots[hi:]):
                seen.add(s)
                if len(seen) == RUN_TOUCHED and hi + k + 1 < m:
                    return k + 1, FULL
            return m - hi, END
        return host_loop(m, run)

    return dict(nodes=nodes, bound=[], steps=[step(replicas("web", m, [TSC(1, HOST, ANYWAY, SEL)]), f"touched {m}",
                                                   expect, pre)])


# ------------------------------------------------------------ 2. hostname count crossing 255

CROSS_SLOTS = (5, 9)
CROSS_FILL = [(250, 252), (254, 254), (255, 100), (253, 0)]
CROSS_M = 12


def cross_index(fill, slots):
    """Index of the first pod whose commit raises a node's own count to
    RK_HK_NONE (None: no count gets there; -1: one is there before the batch)."""
    cnt = dict(zip(CROSS_SLOTS, fill))
    if max(cnt.values()) >= RK_HK_NONE:
        return -1
    for j, s in enumerate(slots):
        cnt[s] += 1
        if cnt[s] == RK_HK_NONE:
            return j
    return None


def hostname_cross(fill):
    """Two candidate nodes that hold fill matching pods: the commit that
    raises a count to 255 ends the run (RUN_FULL), replica_keys_kernel refuses
    the next one (a count beyond 254), the chain takes the rest."""
    nodes = [node(i, dict({ZONE: f"z{i % 3}"}, **(PIN if i in CROSS_SLOTS else {}))) for i in range(64)]
    bound = [b for s, k in zip(CROSS_SLOTS, fill) for b in prefilled(s, k)]

    def pre(r):
        all_scheduled(r)
        assert set(r["node_index"].tolist()) <= set(CROSS_SLOTS) and (r["feasible"] == 2).all()

    def expect(r):
        slots = r["node_index"].tolist()
        j = cross_index(fill, slots)

        def run(hi):
            if j is None:
                return CROSS_M - hi, END
            if hi > j:  # a count of 255 at the start
                return 0, END
            return j + 1 - hi, FULL
        return host_loop(CROSS_M, run)

    return dict(nodes=nodes, bound=bound, fill=fill,
                steps=[step(defaults(CROSS_M, node_selector=PIN), f"cross {fill}", expect, pre)])


# ------------------------------------------------------------ 3. every candidate blocked

BLOCKED = [(1, 10, 2), (3, 12, 6)]  # maxSkew, replicas, how many the skew lets through


def blocked(skew, m, ok):
    """z0 is an eligible domain (nodeAffinityPolicy Ignore) without a candidate:
    its count, the minimum, stays 0, and z1 and z2 take maxSkew pods each.  The
    run ends before the first pod that finds every candidate blocked (RUN_FIT);
    a run that starts there has no feasible node and answers every pod left."""
    nodes = [node(i, dict({ZONE: f"z{i % 3}"}, **(PIN if i % 3 else {}))) for i in range(90)]
    spread = [TSC(skew, ZONE, DNS, SEL, node_affinity_policy="Ignore"), TSC(1, HOST, ANYWAY, SEL)]

    def pre(r):
        assert r["status"].tolist() == [0] * ok + [1] * (m - ok)
        assert (r["fail"][ok:, SPREAD] > 0).all() and (r["feasible"][ok:] == 0).all()

    def expect(r):
        st = r["status"].tolist()

        def run(hi):
            if st[hi]:  # no feasible node at the start: the F == 0 branch
                assert all(st[hi:])
                return m - hi, END
            k = st[hi:].index(1) if 1 in st[hi:] else m - hi
            return k, (FIT if hi + k < m else END)
        return host_loop(m, run)

    return dict(nodes=nodes, bound=[], steps=[step(replicas("web", m, spread, node_selector=PIN),
                                                   f"blocked {skew}", expect, pre)])


# ------------------------------------------------------------ 4. the offset histogram

HIST_START = RUN_HIST - 4  # z0's count before the batch: four commits below the histogram's end
HIST_M, HIST_M2 = 10, 6


def hist_start():
    """(a) z0 holds 508 matching pods, z1 (eligible, no candidate) none: the
    count is entered at offset 508, and the commit that finds it at 511 ends
    the run; every later run meets a domain beyond the histogram and ends after
    one pod.  (b) then maxSkew 515 blocks every candidate at the start, with
    skew-rejected candidates present and no ScheduleAnyway constraint."""
    nodes = [node(i, dict({ZONE: f"z{i % 2}"}, **({} if i % 2 else PIN))) for i in range(40)]
    fill = [0, 2, 4, 6]
    assert HIST_START % len(fill) == 0 and HIST_START // len(fill) < RK_HK_NONE - HIST_M
    bound = [b for s in fill for b in prefilled(s, HIST_START // len(fill))]
    a = [TSC(600, ZONE, DNS, SEL, node_affinity_policy="Ignore"), TSC(1, HOST, ANYWAY, SEL)]
    b = [TSC(HIST_START + HIST_M - 3, ZONE, DNS, SEL, node_affinity_policy="Ignore")]
    assert HIST_START + HIST_M + 1 - 0 > b[0].max_skew  # count + self - minimum: blocked

    def pre_a(r):
        all_scheduled(r)
        assert (r["feasible"] == 20).all() and all(s % 2 == 0 for s in r["node_index"].tolist())

    def expect_a(r):
        def run(hi):  # every pod so far went to z0
            at_end = RUN_HIST - 1 - (HIST_START + hi)  # commits before the one that finds offset 511
            k = max(at_end, 0) + 1
            return (k, FULL) if k <= HIST_M - hi else (HIST_M - hi, END)
        return host_loop(HIST_M, run)

    def pre_b(r):
        assert (r["status"] == 1).all() and (r["feasible"] == 0).all()
        assert (r["fail"][:, SPREAD] == 20).all() and (r["fail"][:, AFFINITY] == 20).all()

    return dict(nodes=nodes, bound=bound,
                steps=[step(replicas("web", HIST_M, a, node_selector=PIN), "hist start", expect_a, pre_a),
                       step(replicas("late", HIST_M2, b, node_selector=PIN), "hist blocked", whole, pre_b)])


HIST_SKEW = [RUN_HIST - 1, RUN_HIST, RUN_HIST + 1]
HIST_THR_M = 12


def hist_threshold(skew):
    """Three empty zones take the pods in turn, so the minimum rises with every
    third commit; the threshold's offset is then the minimum's + maxSkew - 1
    (the pods count themselves), and the run ends when that reaches RUN_HIST."""
    nodes = [node(i, {ZONE: f"z{i % 3}"}) for i in range(30)]
    spread = [TSC(skew, ZONE, DNS, SEL), TSC(1, HOST, ANYWAY, SEL)]

    def pre(r):
        all_scheduled(r)
        assert [s % 3 for s in r["node_index"].tolist()] == [j % 3 for j in range(HIST_THR_M)]

    def expect(r):
        rises = max(1, RUN_HIST - (skew - 1))  # rises of the minimum until its offset + maxSkew - 1 >= RUN_HIST
        return host_loop(HIST_THR_M, lambda hi: (min(3 * rises, HIST_THR_M - hi), FULL))

    return dict(nodes=nodes, bound=[], steps=[step(replicas("web", HIST_THR_M, spread), f"hist skew {skew}",
                                                   expect, pre)])


UNBLOCK_M = 12
UNBLOCK = {2: [20, 20, 30], 1: [20, 10, 20]}  # maxSkew: the first three pods' feasible counts


def hist_unblock(skew):
    """z2 starts two above z0 and z1, so its ten candidates are blocked.  The
    second commit raises the minimum to 1, and the run takes the candidates of
    the domains at the new threshold's offset (s_nhist) off the blocked count:
    under maxSkew 2 those are z2's, and the third pod finds all 30 nodes
    feasible; under maxSkew 1 they are z0's and z1's, which their own first
    pods had blocked, while z2 stays blocked."""
    nodes = [node(i, {ZONE: f"z{i % 3}"}) for i in range(30)]
    bound = prefilled(2, 1) + prefilled(5, 1)
    spread = [TSC(skew, ZONE, DNS, SEL), TSC(1, HOST, ANYWAY, SEL)]

    def pre(r):
        all_scheduled(r)
        assert r["feasible"].tolist()[:3] == UNBLOCK[skew]
        assert r["fail"][:3, SPREAD].tolist() == [30 - f for f in UNBLOCK[skew]]
        assert sorted(s % 3 for s in r["node_index"].tolist()[:2]) == [0, 1]

    return dict(nodes=nodes, bound=bound, steps=[step(replicas("web", UNBLOCK_M, spread), f"hist unblock {skew}",
                                                      whole, pre)])

# ------------------------------------------------------------ 5. more than two selector classes

CLS_SELECTORS = [{"tier": "fe"}, {"team": "x"}, {"env": "p"}]
CLS_WEB, CLS_FOLLOW = 40, 30


def classes(web_labels=True):
    """The web pods match four selector classes: their own and the three that
    earlier deployments created.  The follow-up deployments spread on those
    three, so their placements show whether every web commit was counted in
    every class column.  web_labels False: the same stream with web pods that
    match their own class only (what the follow-ups do without those counts)."""
    nodes = [node(i, {ZONE: f"z{i % 4}"}, cpu=[16000, 32000, 64000][i % 3]) for i in range(60)]
    first = [p for q, lab in enumerate(CLS_SELECTORS) for p in defaults(4, f"first{q}", LabelSelector(lab), lab)]
    lab = {"app": "web"}
    if web_labels:
        for s in CLS_SELECTORS:
            lab.update(s)
    steps = [step(first, "classes first", lambda r: (len(CLS_SELECTORS), len(r)), all_scheduled),
             step(defaults(CLS_WEB, labels=lab), "classes web", whole, all_scheduled)]
    for q, s in enumerate(CLS_SELECTORS):
        sel = LabelSelector(s)
        own = [TSC(1, HOST, ANYWAY, sel), TSC(1, ZONE, ANYWAY, sel)]
        steps.append(step(replicas(f"follow{q}", CLS_FOLLOW, own, s), f"classes follow {q}", whole, all_scheduled))
    return dict(nodes=nodes, bound=[], steps=steps)


# ------------------------------------------------------------ 6. group cap

GROUP_N, GROUP_M = 520, 8
GROUP_G = [RUN_GROUPS, RUN_GROUPS + 1]


def group_cap(G):
    """G racks, every one a group of candidates: 512 fill the run's group table
    (the sort of the group starts has no padding entry), 513 refuse the run."""
    nodes = [node(i, {"rack": f"r{i % G}", ZONE: f"z{i % 3}"}) for i in range(GROUP_N)]

    def pre(r):
        all_scheduled(r)
        assert (r["feasible"] == GROUP_N).all() and len({nd.labels["rack"] for nd in nodes}) == G
        assert r["node_index"].tolist() == list(range(GROUP_M))

    return dict(nodes=nodes, bound=[], steps=[step(replicas("web", GROUP_M, [TSC(2, "rack", ANYWAY, SEL)]),
                                                   f"groups {G}", whole if G <= RUN_GROUPS else refused, pre)])


# ------------------------------------------------------------ 7. missing labels, one feasible node

BARE_N, BARE_M, SOLO_SLOT, SOLO_M = 120, 40, 11, 6


def bare_nodes():
    no_host = lambda i: i % 7 == 0  # noqa: E731
    no_zone = lambda i: i % 5 == 0  # noqa: E731
    nodes = [node(i, dict({} if no_zone(i) else {ZONE: f"z{i % 3}"}, **({"solo": "y"} if i == SOLO_SLOT else {})),
                  host=not no_host(i)) for i in range(BARE_N)]
    assert not no_host(SOLO_SLOT) and not no_zone(SOLO_SLOT)
    return nodes, {i for i in range(BARE_N) if no_host(i) or no_zone(i)}


def missing_labels():
    """Under the system defaults a node lacking a key is scored (one lacking the
    zone counts under ""); under the pod's own constraints it is ignored."""
    nodes, bare = bare_nodes()
    own = [TSC(2, ZONE, ANYWAY, SEL), TSC(1, HOST, ANYWAY, SEL)]

    def pre_defaults(r):
        all_scheduled(r)
        assert (r["feasible"] == BARE_N).all() and set(r["node_index"].tolist()) & bare

    def pre_own(r):
        all_scheduled(r)
        assert (r["feasible"] == BARE_N).all() and not set(r["node_index"].tolist()) & bare

    return dict(nodes=nodes, bound=[], steps=[step(defaults(BARE_M), "bare defaults", whole, pre_defaults),
                                              step(replicas("own", BARE_M, own), "bare own", whole, pre_own)])


def single_feasible():
    nodes, _ = bare_nodes()

    def pre(r):
        all_scheduled(r)
        assert (r["node_index"] == SOLO_SLOT).all() and (r["feasible"] == 1).all() and (r["flags"] & SINGLE).all()

    return dict(nodes=nodes, bound=[], steps=[step(defaults(SOLO_M, node_selector={"solo": "y"}), "single", whole,
                                                   pre)])


# ------------------------------------------------------------ 8. no feasible node, long

NONE_N, NONE_M = 20, 600


def no_node():
    """More pods than the workgroup has threads, none with a feasible node:
    the result loop strides."""
    nodes = [node(i, {ZONE: f"z{i % 3}"}) for i in range(NONE_N)]
    assert NONE_M > RUN_TOUCHED

    def pre(r):
        assert (r["status"] == 1).all() and (r["feasible"] == 0).all() and (r["fail"][:, AFFINITY] == NONE_N).all()

    return dict(nodes=nodes, bound=[], steps=[step(defaults(NONE_M, node_selector={"no": "such"}), "no node", whole,
                                                   pre)])


CASES = {f"touched-{m}": (lambda m=m: touched_cap(m)) for m in TOUCHED_M}
CASES.update({f"cross-{a}-{b}": (lambda f=(a, b): hostname_cross(f)) for a, b in CROSS_FILL})
CASES.update({f"blocked-{s}": (lambda a=(s, m, ok): blocked(*a)) for s, m, ok in BLOCKED})
CASES["hist-start"] = hist_start
CASES.update({f"hist-skew-{s}": (lambda s=s: hist_threshold(s)) for s in HIST_SKEW})
CASES.update({f"hist-unblock-{s}": (lambda s=s: hist_unblock(s)) for s in UNBLOCK})
CASES["classes"] = classes
CASES.update({f"groups-{g}": (lambda g=g: group_cap(g)) for g in GROUP_G})
CASES["missing-labels"] = missing_labels
CASES["single-feasible"] = single_feasible
CASES["no-node"] = no_node

# the pairs worked out by hand from the kernel's limits and the host's loop (DESIGN §5.7 lists the reasoning);
# expect() must arrive at the same from the oracle's results
STATED = {"touched-512": [(1, 512)], "touched-513": [(1, 512)], "touched-515": [(1, 512)], "touched-516": [(2, 516)],
          "cross-255-100": [(0, 0)], "blocked-1": [(1, 2)], "blocked-3": [(2, 12)], "hist-start": [(4, 7), (1, 6)],
          "hist-skew-511": [(2, 12)], "hist-skew-512": [(3, 9)], "hist-skew-513": [(3, 9)],
          "groups-512": [(1, 8)], "groups-513": [(0, 0)], "single-feasible": [(1, 6)], "no-node": [(1, 600)],
          "cross-250-252": [(1, 7)], "cross-254-254": [(1, 1)], "cross-253-0": [(1, 12)],
          "hist-unblock-1": [(1, 12)], "hist-unblock-2": [(1, 12)], "missing-labels": [(1, 40), (1, 40)],
          "classes": [(3, 12), (1, 40), (1, 30), (1, 30), (1, 30)]}
assert sorted(STATED) == sorted(CASES)


def run_steps(x, case):
    """Feed a case to the target (test_gpu_spread.Pair's interface); per step,
    the results x.schedule returned."""
    x.upsert(case["nodes"], list(range(len(case["nodes"]))))
    x.add([p for p, _ in case["bound"]], [s for _, s in case["bound"]])
    return [x.schedule(s["pods"], s["what"]) for s in case["steps"]]
