"""The workloads of tests/replica_edge_cases.py on the CPU oracle alone: the
condition each case needs for the device test to prove anything (pods that
land where the limit is, status patterns, counts that cross), and the
(replica_runs, replica_pods) pairs the cases derive from the oracle's results
against the ones stated by hand."""
import numpy as np
import pytest

import replica_edge_cases as W
from test_oracle_chain_edges import OracleOnly


def run(case):
    x = OracleOnly(len(case["nodes"]))
    res = W.run_steps(x, case)
    x.close()
    return res


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_case_conditions(name):
    case = W.CASES[name]()
    res = run(case)
    pairs = []
    for s, r in zip(case["steps"], res):
        assert len(r) == len(s["pods"])
        s["pre"](r)
        pairs.append(s["expect"](r))
    assert pairs == W.STATED[name]
    print(name, pairs)


def test_constants_sit_where_the_cases_need_them():
    assert W.TOUCHED_M == [512, 513, 515, 516] and W.GROUP_G == [512, 513] and W.HIST_SKEW == [511, 512, 513]
    assert W.HIST_START == 508 and W.RK_HK_NONE == 255


# ------------------------------------------------------------ 2. hostname count crossing 255

@pytest.mark.parametrize("fill", W.CROSS_FILL)
def test_cross_index(fill):
    case = W.hostname_cross(fill)
    r, = run(case)
    j = W.cross_index(fill, r["node_index"].tolist())
    pair = case["steps"][0]["expect"](r)
    if fill == (255, 100):
        assert j == -1 and pair == (0, 0)
    elif fill == (253, 0):
        # no count gets to 255 here: the hostname constraint sends every pod to the empty node, whatever the
        # rest of the score says (2 x 100 against at most 100 + 100), so the run keeps a candidate at 253,
        # two below the field's end, and takes the whole batch
        assert j is None and (r["node_index"] == W.CROSS_SLOTS[1]).all() and pair == (1, W.CROSS_M)
    else:
        # a node's own count reaches 255 at pod j, within the batch: the run ends after that commit
        assert j is not None and 0 <= j < W.CROSS_M and pair == (1, j + 1)
    if fill == (250, 252):
        assert r["node_index"].tolist()[:8] == [5, 5, 5, 9, 5, 9, 5, 9] and j == 6


# ------------------------------------------------------------ 5. more than two selector classes

def test_classes_follow_ups_depend_on_the_web_labels():
    with_labels, without = run(W.classes()), run(W.classes(web_labels=False))
    moved = [int((a["node_index"] != b["node_index"]).sum()) for a, b in zip(with_labels[2:], without[2:])]
    assert len(moved) == len(W.CLS_SELECTORS)
    assert all(3 * k >= W.CLS_FOLLOW for k in moved), moved
    # the batches before them are the same without the labels: the web pods' own class decides those
    for a, b in zip(with_labels[:2], without[:2]):
        assert np.array_equal(a["node_index"], b["node_index"])
    print("moved", moved)
