"""The workloads of tests/chain_edge_cases.py on the CPU oracle alone: the
answers stated there by construction (chosen slots, closed-form raw scores,
the order of a pod's constraints not mattering) and the conditions the inputs
must meet for the device tests to prove anything (filters that reject, pods
that schedule, a deciding record that decides)."""
import ctypes as C

import numpy as np
import pytest

import chain_edge_cases as W
import pyoracle
from helpers import res_array, scores_array
from ksched.objects import Arena, nodes_array, pods_array
from scenarios import POD_AFFINITY, SPREAD


def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


class OracleOnly:
    """The oracle behind the interface the streams drive (test_gpu_spread.Pair's)."""

    def __init__(self, n):
        self.n, self.a, self.o = n, Arena(), pyoracle.Oracle(n)

    def upsert(self, nodes, slots):
        na, k = nodes_array(nodes, self.a)
        self.o.upsert(na, u32(slots), k)

    def add(self, pods, slots):
        if pods:
            pa, k = pods_array(pods, self.a)
            self.o.add_pods(pa, u32(slots), k)

    def schedule(self, pods, what=""):
        pa, m = pods_array(pods, self.a)
        return res_array(self.o.schedule(pa, m), m)

    def dump_equal(self, pod, what=""):
        pa, _ = pods_array([pod], self.a)
        return self.o.plugin_scores(pa)

    def close(self):
        self.o.close()


def run(case, pods=None, what=""):
    x = OracleOnly(len(case["nodes"]))
    r = W.run_case(x, dict(case, pods=pods, exp=[], dumps={}) if pods else case, what)
    x.close()
    return r


# ------------------------------------------------------------ 1. wide key

@pytest.mark.parametrize("variant", W.WIDE_VARIANTS)
@pytest.mark.parametrize("D", W.WIDE_D)
def test_wide_key(D, variant):
    run(W.wide_key(D, variant), what=f"wide {D} {variant}")


# ------------------------------------------------------------ 2. LDS budget

def budget_setup():
    nodes, bound = W.budget_cluster()
    x = OracleOnly(len(nodes))
    x.upsert(nodes, list(range(len(nodes))))
    x.add([p for p, _ in bound], [s for _, s in bound])
    return x


def test_budget_id_counts_are_the_packing():
    nodes, _ = W.budget_cluster()
    for key, ids in W.BUDGET_IDS.items():
        assert len({nd.labels[key] for nd in nodes}) + 1 == ids, key


def test_budget_stream_conditions():
    x = budget_setup()
    pods = W.budget_pods()
    r = x.schedule([pods[k] for k in "abcdef"], "budget")
    assert (r["status"] == 0).sum() * 2 >= len(r)
    assert (r["fail"][:, SPREAD] > 0).all()         # every pod: some nodes first rejected by PodTopologySpread
    assert r["fail"][4, POD_AFFINITY] > 0           # (e): ... and some by InterPodAffinity
    assert (r["feasible"][r["status"] == 0] > 0).all()
    x.close()


def test_budget_constraint_order_does_not_matter():
    pods = W.budget_pods()
    res, dump = {}, {}
    for k in "ac":
        x = budget_setup()
        dump[k] = scores_array(x.dump_equal(pods[k]))
        res[k] = x.schedule([pods[k]], k)[0]
        x.close()
    assert np.array_equal(dump["a"], dump["c"])
    assert res["a"] == res["c"] and res["a"]["status"] == 0
    assert (dump["a"][:, 0] == SPREAD).sum() == res["a"]["fail"][SPREAD] > 0


# ------------------------------------------------------------ 3. prefetch width

@pytest.mark.parametrize("name", sorted(W.PF_CASES))
def test_prefetch_width(name):
    case = W.PF_CASES[name]()
    n_rec = int(name.rsplit("-", 1)[1])
    p = case["pods"][0]
    if name.startswith("spread"):
        assert len(p.topology_spread) == n_rec > W.SP_PF
    else:
        assert len(p.affinity_terms) + (1 if "bound" in name else 0) == n_rec > W.AF_PF
    r = run(case, what=name)
    assert r["node_index"][0] == 12
    # without the record at index >= 4 the answer is another: that record is what decides
    ctl = run(case, pods=case["control"], what=name + " control")
    assert ctl["status"][0] == 0 and ctl["node_index"][0] == 0 and ctl["feasible"][0] == W.PF_N


# ------------------------------------------------------------ 4. churn

@pytest.mark.parametrize("phase", W.CHURN_PHASES)
def test_churn_stream(phase):
    x = OracleOnly(W.CHURN_CAP)
    res, info = W.churn_stream(x, phase)
    x.close()
    r = np.concatenate(res)
    assert len(r) == 4 * (W.CHURN_STEPS + 1)
    assert (r["status"] == 0).sum() * 2 >= len(r)
    assert (r["fail"][:, SPREAD] > 0).any() and (r["fail"][:, POD_AFFINITY] > 0).any()
    # the rack key leaves LDS (and the scratch grows), is renumbered once, and the stream goes on after it
    assert 1 < info["left_lds"] < info["renumbered"] < W.CHURN_STEPS - 2
    assert info["scratch"] == 2 * W.SCRATCH_MIN
    assert info["rack_ids"] < W.SP_LDS_DOM
    assert info["shared_then"] == {0: 0, 2: 1}[phase]  # the rebuild meets `shared` at 0 and above 0


# ------------------------------------------------------------ 5. replica-run width

@pytest.mark.parametrize("variant", W.RUN_VARIANTS)
@pytest.mark.parametrize("D", W.RUN_D)
def test_run_width(D, variant):
    case = W.run_width(D, variant)
    r = run(case, what=f"run {D} {variant}")
    assert (r["status"] == 0).all() and (r["feasible"] <= 52).all()
    assert case["runs"] == (D <= 2046)
    nodes = r["node_index"].tolist()
    # the candidates carry the table's two ends: the first and the last cell are both taken
    assert any(i % D == D - 1 for i in nodes) and any(i % D == 0 for i in nodes)
    # one replica in each of the deployment's 40 cells without a web pod (dns: maxSkew 1 over a minimum of 0)
    assert sorted(i % D for i in nodes) == [c for c in list(range(10)) + list(range(D - 32, D)) if c not in (3, D - 3)]
    if variant == "dns":
        assert (r["fail"][:, SPREAD] > 0).all()
