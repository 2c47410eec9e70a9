"""What tests/test_gpu_chain_variants.py rests on, shown on PortsReference
alone (no GPU): under each of the ten contexts of ports_workloads.CONTEXTS the
65-node stream with the 16 chain-variant pods schedules at least one pod of
each of the four kinds (host port or none, anti-affinity term or none) and
fails at least one pod with NodePorts, so no filter instance the GPU test means
to reach can go unlaunched, and a build that ignored a pod's ports or its
terms could not pass."""
import pytest

import ports_workloads as W


def test_ten_contexts():
    # GF 0 / 1 / 2, XF under GF >= 1, BAL under each: every combination the chain's launch tells apart
    gf = lambda ref: 0 if "strategy" not in ref else 1 if ref["strategy"][0] == W.MOST else 2
    keys = {(gf(ref), "extended" in ref, "balanced" in ref) for ref, _ in W.CONTEXTS.values()}
    assert len(W.CONTEXTS) == len(keys) == 10
    for (ref, cfg) in W.CONTEXTS.values():
        assert ("extended" in ref) == ("fit_resource_weights" in cfg) and ("balanced" in ref) == ("balanced_resources" in cfg)
        assert "strategy" in ref or "extended" not in ref  # XF needs a general strategy


@pytest.mark.parametrize("name", list(W.CONTEXTS))
def test_every_kind_is_scheduled_and_a_pod_fails_node_ports(name):
    ref = W.variants_reference(name)
    r, pods = ref["res"], ref["pods"]
    extras = range(len(pods) - 16, len(pods))
    for ports, anti in W.KINDS:
        mine = [j for j in extras if bool(pods[j].host_ports) == ports and bool(pods[j].affinity_terms) == anti]
        assert len(mine) == 4
        assert all(pods[j].containers[0].requests[W.GPU] == 1 for j in mine)
        assert any(r["status"][j] == 0 for j in mine), (name, ports, anti)
    # an unschedulable pod with NodePorts in its diagnosis
    assert ((r["status"] != 0) & (r["_pad"] > 0)).any(), name
    # one probe of each kind
    assert [(bool(p.host_ports), bool(p.affinity_terms)) for p in ref["probes"]] == W.KINDS
