"""Every kernel variant the one-pod chain's launch can choose (ksched_spread.hip
launch_spread_pod: the filter instances by AFF, GF, XF, BAL and PORTS, and
the select instances of a score dump), against PortsReference bit for bit.

65 nodes: one wave plus one lane.  Under each of the ten contexts of
ports_workloads.CONTEXTS the 65-node NodePorts stream is followed by 16 pods
of four kinds -- with or without a host port (PORTS), with or without a
required anti-affinity term (AFF) -- that each request one amd.com/gpu, so
they meet XF and BAL wherever the context lists the resource.
tests/test_chain_variants_reference.py shows on the reference alone that a pod
of every kind is scheduled and a pod fails NodePorts in every context.
"""
import numpy as np
import pytest

import ports_workloads as W
from helpers import res_array, states_np
from ksched import Scheduler
from ksched.objects import Arena, nodes_array, pods_array
from test_gpu_ports import assert_res, dump, used_ports

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(W.CONTEXTS))
def test_chain_variants(name):
    n = 65
    ref = W.variants_reference(name)
    a = Arena()
    with Scheduler(n, pods_per_round=64, **W.CONTEXTS[name][1]) as s:
        na, k = nodes_array(ref["nodes"], a)
        s.upsert_nodes_raw(na, W.u32(range(k)), k)
        pa, m = pods_array(ref["pods"], a)
        assert_res(res_array(s.schedule_raw(pa, m), m), ref["res"], name)
        assert np.array_equal(states_np(s.lib.ks_node_states, s.ctx, n), ref["states"]), name
        assert used_ports(s, n) == ref["used"], name
        for p, want in zip(ref["probes"], ref["dumps"]):  # the dump path: the select instances
            got = dump(s, p, n, a)
            assert np.array_equal(got, want), (name, p.name, np.nonzero(got != want)[0][:5])
        assert s.stats().spread_pods >= 16  # the extra pods took the chain
