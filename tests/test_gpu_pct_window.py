"""The geometry of the percentageOfNodesToScore window on the GPU (DESIGN.md
§5.8): spread_wcount_kernel / spread_window_kernel with the start node and the
stopping node placed by construction (tests/pct_window_cases.py) -- on the
edges of the 1024-slot chunks, in a table that is no multiple of 16 slots, at
the `all` boundary (exactly k / k + 1 feasible nodes, lists of 99 / 100 / 101
nodes), with the stopping node before the start node, behind a PreFilterResult
pod, and in a table of more than 1024 chunks, where each thread of the window
kernel sums and searches two chunks.

Two references, both bit-exact: the C++ oracle (every result field, the
nodes' states and nextStartNodeIndex after each call, through PctPair) and the
plain-Python restatement of tests/test_oracle_pct_restated.py (node, feasible
and evaluated counts, the NodeUnschedulable and PreFilterResult counts and the
index), from whose visits each stream also asserts that it reached what it
was built for.  Parity unpinned: neither reference is upstream's text."""
import ctypes as C

import numpy as np
import pytest

import pct_window_cases as W
from helpers import STATE_DT
from ksched import _abi
from test_gpu_pct import PctPair
from test_oracle_pct_restated import PyWindow

pytestmark = pytest.mark.gpu


class Tri(PctPair):
    """libksched, the oracle and the Python restatement fed the same events."""

    def __init__(self, n, pct, states_of=None):
        super().__init__(n, pct)
        self.py = PyWindow(n, pct)
        self.states_of = states_of  # the slots whose states are compared after each call (default: all)

    def upsert(self, items):
        super().upsert([nd.to_node() for _, nd in items], [s for s, _ in items])
        for s, nd in items:
            self.py.upsert(s, nd)

    def delete(self, slots):
        super().delete(list(slots))
        for s in slots:
            self.py.delete(s)

    def some_states_equal(self, what):
        sl = np.asarray(self.states_of, dtype=np.uint32)
        out = []
        for fn, ctx in ((self.s.lib.ks_node_states, self.s.ctx), (self.o.L.oracle_node_states, self.o.o)):
            buf = (_abi.KsNodeState * len(sl))()
            assert fn(ctx, sl.ctypes.data_as(C.POINTER(C.c_uint32)), len(sl), buf) == 0
            out.append(np.frombuffer(buf, dtype=STATE_DT).copy())
        assert np.array_equal(out[0], out[1]), what

    def run(self, pods, what):
        r = self.schedule(pods, what)  # the device against the oracle, every field
        visits = [self.py.schedule(p) for p in pods]
        for j, v in enumerate(visits):
            got = (int(r["node_index"][j]), int(r["feasible"][j]), int(r["evaluated"][j]), int(r["fail"][j][0]),
                   int(r["fail"][j][7]))
            assert got == v.result(), (what, j, got, v.result())
        if self.states_of is None:
            self.states_equal(what)
        else:
            self.some_states_equal(what)
        self.check_start(what)
        assert self.s.next_start_index() == self.py.nxt, (what, self.s.next_start_index(), self.py.nxt)
        return visits


@pytest.mark.parametrize("cap,pattern", W.SLOT_CASES)
def test_window_slot_counts(cap, pattern):
    x = Tri(cap, 5)
    W.check_slot_count_stream(W.slot_count_stream(x, cap, pattern), cap, pattern)
    x.close()


@pytest.mark.parametrize("length", [99, 100, 101])
def test_window_named_list_lengths(length):
    x = Tri(3000, 5)
    W.check_named_lengths(W.named_lengths_stream(x, length), length)
    x.close()


@pytest.mark.parametrize("length", [99, 100, 101])
def test_window_present_list_lengths(length):
    x = Tri(1500, 5)
    W.check_present_lengths(W.present_lengths_stream(x, length), length)
    x.close()


def test_window_holes():
    x = Tri(3000, 5)
    W.check_holes(W.holes_stream(x))
    x.close()


def test_window_prefilter_result_then_plain_pods():
    # a named pod's PreFilterResult exclusions count as processed: it leaves
    # nextStartNodeIndex where it was, and the plain pod after it takes the
    # window that the plain pod before it left.  (With the index advanced by
    # the named list's length instead, the kernel fails here at the first
    # named pod against the oracle and the restatement.)
    x = Tri(1500, 5)
    W.check_prefilter_then_plain(*W.prefilter_then_plain_stream(x))
    x.close()


def test_window_more_than_1024_chunks():
    # 1027 chunks: spread_window_kernel's threads take two chunks each (cpt 2)
    # and the last chunk has 7 slots.  States are compared on the present
    # slots and their neighbours after each call, on every slot at the end
    present = W.big_present()
    near = sorted({s for p in present for s in (p - 1, p, p + 1) if 0 <= s < W.BIG_CAP})
    x = Tri(W.BIG_CAP, 5, states_of=near)
    W.check_big(W.big_stream(x))
    x.states_equal("big, every slot")
    x.close()


def test_window_adaptive_floor():
    x = Tri(6000, 0)
    W.check_adaptive_floor(W.adaptive_floor_stream(x))
    x.close()
