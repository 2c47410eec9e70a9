"""tests/diag_reference.py on its own (CPU): the hand-derived answers of
tests/diag_cases.py, one or more per row of the reason table, and the
restated pieces by themselves.  No product code computes anything here."""
import pytest

import diag_cases as DC
import diag_reference as R
from ksched.objects import Container, Pod, Taint, Toleration


def reference_for(name):
    nodes, bound, pod, want = DC.CASES[name]()
    ports = name == "node_ports"
    ref = R.DiagReference(len(nodes), DC.PORT_PAIRS if ports else (), DC.PORT_IPS if ports else ())
    ref.upsert(nodes, list(range(len(nodes))))
    ref.add([p for p, _ in bound], [s for _, s in bound])
    return ref, pod, want


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_known_answers(name):
    ref, pod, want = reference_for(name)
    got = ref.diagnose(pod)
    ref.close()
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)
    assert got["num_all_nodes"] == len(ref.nodes)
    assert got["node_ports_nodes"] == want.get("node_ports_nodes", 0)
    assert got["prefilter_msg"] == want.get("prefilter_msg")
    # a node is counted once per reason; outside NodeResourcesFit a failing node carries exactly one
    fit = sum(c for r, c in got["reasons"].items() if r.startswith("Insufficient") or r == "Too many pods")
    others = sum(got["reasons"].values()) - fit
    assert others == sum(got["plugin_nodes"]) - got["plugin_nodes"][4] + got["node_ports_nodes"]
    assert fit >= got["plugin_nodes"][4]
    assert got["feasible_nodes"] + sum(got["plugin_nodes"]) + got["node_ports_nodes"] == got["num_all_nodes"]


def test_every_table_row_has_a_case():
    seen = set()
    for name in DC.CASES:
        seen |= set(DC.CASES[name]()[3]["reasons"])
    fixed = {R.UNSCHEDULABLE, R.NODE_NAME, R.AFFINITY, R.CONFLICT, R.PREFILTERED, R.PORTS, R.TOO_MANY_PODS,
             R.INSUFFICIENT % "cpu", R.INSUFFICIENT % "memory", R.INSUFFICIENT % "ephemeral-storage",
             R.INSUFFICIENT % "amd.com/gpu", R.SPREAD_LABEL, R.SPREAD_SKEW, R.IPA_AFF, R.IPA_ANTI, R.IPA_EXIST}
    assert fixed <= seen
    assert any(r.startswith("node(s) had untolerated taint {") for r in seen)


def test_tolerations():
    t = Taint("k", "v", "NoSchedule")
    assert R.tolerates(Toleration("k", "Equal", "v"), t) and R.tolerates(Toleration("k", "Exists"), t)
    assert R.tolerates(Toleration("", "Exists"), t) and R.tolerates(Toleration("k", "Equal", "v", "NoSchedule"), t)
    assert not R.tolerates(Toleration("k", "Equal", "w"), t) and not R.tolerates(Toleration("k", "Exists", "", "NoExecute"), t)
    assert not R.tolerates(Toleration("j", "Exists"), t)


def test_pod_requests():
    p = Pod("p", containers=[Container({"cpu": 100, "x/y": 1}), Container({"cpu": 50})],
            init_containers=[Container({"cpu": 400}), Container({"x/y": 3}, restart_policy_always=True),
                             Container({"cpu": 10, "x/y": 1})], overhead={"cpu": 7})
    # containers 150 / 1, the sidecar adds 3 to x/y; init maxima: 400 cpu; x/y max(3, 3 + 1) = 4
    assert R.pod_requests(p) == {"cpu": 407, "x/y": 4}


def test_message():
    assert R.message(12, {"Insufficient memory": 2, "Insufficient cpu": 10}) == \
        "0/12 nodes are available: 10 Insufficient cpu, 2 Insufficient memory."
    assert R.message(3, {}) == "0/3 nodes are available:"
    assert R.message(3, {"x": 3}, "pod affinity terms conflict") == "0/3 nodes are available: pod affinity terms conflict."
