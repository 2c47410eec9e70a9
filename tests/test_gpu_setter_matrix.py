"""The scoring configuration's four setters (ks_set_fit_strategy,
ks_set_fit_strategy_shape, ks_set_fit_strategy_resources and
ks_set_balanced_resources) as one table: the status each argument combination
returns, the ks_last_error text it leaves (a refusal without a text of its own
leaves the earlier one), in the order the checks fire -- an invalid type before
the weights, an invalid shape before the refusal of a window -- and, after
every call, what the four getters answer: the arguments of an accepted call,
the earlier configuration after a refused one.

Two contexts of capacity 64 with four nodes, one of which holds example.com/huge
at 2^44 (the bound of the exact range); the second scores half the nodes
(percentage_of_nodes_to_score 50), which admits the default configuration alone.
"""
import ctypes as C

import pytest

from ksched import Scheduler, _abi
from ksched.objects import Node

pytestmark = pytest.mark.gpu

Gi = 1 << 30
OK, INV, UNS, RNG = _abi.KS_OK, _abi.KS_ERR_INVALID, _abi.KS_ERR_UNSUPPORTED, _abi.KS_ERR_RANGE
LEAST, MOST, RTCR = _abi.FIT_LEAST_ALLOCATED, _abi.FIT_MOST_ALLOCATED, _abi.FIT_REQUESTED_TO_CAPACITY_RATIO
GPU, NIC, HUGE, EPH = "amd.com/gpu", "example.com/nic", "example.com/huge", "ephemeral-storage"
BINPACK, PEAKED = [(0, 0), (100, 10)], [(0, 0), (50, 10), (100, 2)]
NINE = [(f"example.com/r{i}", 1) for i in range(9)]
FIT_NAME = "(empty, cpu / memory / pods, repeated or not a scalar resource)"
BAL_NAME = "(empty, pods, repeated or not cpu, memory or a scalar resource)"
HUGE_RANGE = f"a node's allocatable of {HUGE} outside the exact range"

# (setter, arguments, status, the error text it sets or None).  fit: (type, cpu, memory); shape: + points or
# None; resources: + points or None, [(name, weight)]; balanced: names.  In order on one context.
FULL = [
    ("fit", (7, 1, 1), INV, None),                                    # a bad type
    ("fit", (RTCR, 1, 1), INV, None),                                 # ... which this setter takes RequestedToCapacityRatio for
    ("fit", (7, 101, 0), INV, None),
    ("fit", (LEAST, 101, 1), INV, None),                              # weights out of range
    ("fit", (LEAST, 1, -1), INV, None),
    ("fit", (MOST, 0, 0), INV, None),                                 # both zero
    ("fit", (MOST, 3, 1), OK, None),
    ("fit", (LEAST, 0, 100), OK, None),
    ("shape", (MOST, 1, 1, BINPACK), INV, None),                      # a shape given to another strategy
    ("shape", (7, 1, 1, None), INV, None),                            # no shape: ks_set_fit_strategy's answer
    ("shape", (LEAST, 2, 1, None), OK, None),
    ("shape", (RTCR, 1, 1, None), INV, None),                         # RequestedToCapacityRatio without a shape
    ("shape", (RTCR, 1, 1, [(50, 5), (50, 6)]), INV, None),           # a bad shape
    ("shape", (RTCR, 1, 1, [(0, 11)]), INV, None),
    ("shape", (RTCR, 0, 0, BINPACK), INV, None),                      # both zero
    ("shape", (RTCR, 101, 0, [(0, 11)]), INV, None),
    ("shape", (RTCR, 2, 1, BINPACK), OK, None),
    ("resources", (MOST, 1, 2, None, []), OK, None),                  # no list: falls through
    ("resources", (RTCR, 1, 0, PEAKED, []), OK, None),
    ("resources", (MOST, 1, 1, BINPACK, []), INV, None),
    ("resources", (9, 1, 1, None, [(GPU, 1)]), INV, None),            # a bad type before the weights
    ("resources", (LEAST, 101, 1, None, [(GPU, 1)]), INV, None),
    ("resources", (LEAST, 0, 0, None, [(GPU, 1)]), OK, None),         # both zero beside a list
    ("resources", (MOST, 1, 1, BINPACK, [(GPU, 1)]), INV, None),      # a shape given to another strategy
    ("resources", (RTCR, 1, 1, [(60, 1), (40, 2)], [(GPU, 1)]), INV, None),
    ("resources", (RTCR, 1, 1, None, [(GPU, 1)]), INV, None),
    ("resources", (RTCR, 1, 1, [(0, 11)], NINE), INV, None),          # a bad shape before the names
    ("resources", (LEAST, 1, 1, None, NINE), INV, "more than 8 extended resources in the strategy"),
    ("resources", (LEAST, 1, 1, None, [(GPU, 1), (GPU, 2)]), INV, f"strategy resource 1: name '{GPU}' {FIT_NAME}"),
    ("resources", (LEAST, 1, 1, None, [("cpu", 1)]), INV, f"strategy resource 0: name 'cpu' {FIT_NAME}"),
    ("resources", (LEAST, 1, 1, None, [(GPU, 1), ("pods", 1)]), INV, f"strategy resource 1: name 'pods' {FIT_NAME}"),
    ("resources", (LEAST, 1, 1, None, [("gpu", 1)]), INV, f"strategy resource 0: name 'gpu' {FIT_NAME}"),
    ("resources", (LEAST, 1, 1, None, [(GPU, 0)]), INV, f"strategy resource {GPU}: weight 0 outside 1..100"),
    ("resources", (LEAST, 1, 1, None, [(NIC, 101)]), INV, f"strategy resource {NIC}: weight 101 outside 1..100"),
    ("resources", (LEAST, 1, 1, None, [(GPU, 1), (EPH, 1)]), UNS, "ephemeral-storage in the strategy's resources"),
    ("resources", (MOST, 1, 1, None, [(GPU, 1), (HUGE, 1)]), RNG, HUGE_RANGE),  # an over-range column
    ("resources", (RTCR, 1, 1, PEAKED, [(HUGE, 1)]), RNG, HUGE_RANGE),
    ("resources", (RTCR, 1, 1, PEAKED, [(GPU, 3), ("example.com/absent", 100)]), OK, None),
    ("resources", (MOST, 100, 0, None, [(NIC, 2)]), OK, None),
    ("balanced", ["cpu", GPU], UNS, "a balanced list without cpu or memory"),
    ("balanced", [GPU], UNS, "a balanced list without cpu or memory"),
    ("balanced", ["cpu", "memory", "pods"], INV, f"balanced resource 2: name 'pods' {BAL_NAME}"),
    ("balanced", ["cpu", "memory", "cpu"], INV, f"balanced resource 2: name 'cpu' {BAL_NAME}"),
    ("balanced", ["", "memory"], INV, f"balanced resource 0: name '' {BAL_NAME}"),
    ("balanced", ["cpu", "memory", EPH], UNS, "ephemeral-storage in the balanced list"),
    ("balanced", ["cpu", "memory"] + [nm for nm, _ in NINE], INV, "more than 8 scalar resources in the balanced list"),
    ("balanced", ["cpu", "memory", HUGE], RNG, HUGE_RANGE),
    ("balanced", [GPU, "cpu", "memory"], OK, None),
    ("balanced", ["memory", "cpu"], OK, None),                        # another order is a list of its own
    ("balanced", ["cpu", "memory"], OK, None),                        # the default, by its names
    ("balanced", ["cpu", NIC, "memory", GPU], OK, None),
    ("balanced", [], OK, None),                                       # ... and by none
    ("fit", (LEAST, 1, 1), OK, None),
]

# ... and on a context with a window (percentage_of_nodes_to_score < 100)
WINDOW = [
    ("fit", (7, 1, 1), INV, None),
    ("fit", (MOST, 0, 0), INV, None),
    ("fit", (MOST, 1, 1), UNS, None),                                 # a non-default setting
    ("fit", (LEAST, 2, 1), UNS, None),
    ("fit", (LEAST, 1, 1), OK, None),
    ("shape", (RTCR, 1, 1, [(50, 5), (50, 6)]), INV, None),           # an invalid shape before the refusal
    ("shape", (RTCR, 1, 1, BINPACK), UNS, None),
    ("shape", (LEAST, 1, 1, None), OK, None),
    ("resources", (LEAST, 1, 1, None, [(GPU, 0)]), INV, f"strategy resource {GPU}: weight 0 outside 1..100"),
    ("resources", (LEAST, 1, 1, None, [(EPH, 1)]), UNS, "ephemeral-storage in the strategy's resources"),
    ("resources", (LEAST, 1, 1, None, [(HUGE, 1)]), UNS, None),       # the refusal before the read-back
    ("resources", (LEAST, 1, 1, None, [(GPU, 1)]), UNS, None),
    ("resources", (LEAST, 1, 1, None, []), OK, None),
    ("balanced", ["cpu", GPU], UNS, "a balanced list without cpu or memory"),
    ("balanced", ["cpu", "memory", GPU], UNS, None),
    ("balanced", ["memory", "cpu"], UNS, None),
    ("balanced", ["cpu", "memory"], OK, None),
    ("balanced", [], OK, None),
]


def points(pts):
    if pts is None:
        return None, 0
    return (_abi.KsFitShapePoint * max(1, len(pts)))(*[_abi.KsFitShapePoint(u, v) for u, v in pts]), len(pts)


def call(s, setter, args):
    """The status of one setter call with the table's arguments."""
    if setter == "balanced":
        arr = (C.c_char_p * max(1, len(args)))(*[nm.encode() for nm in args])
        return s.lib.ks_set_balanced_resources(s.ctx, arr if args else None, len(args))
    fs = _abi.KsFitStrategy(args[0], args[1], args[2], 0)
    if setter == "fit":
        return s.lib.ks_set_fit_strategy(s.ctx, C.byref(fs))
    arr, n = points(args[3])
    if setter == "shape":
        return s.lib.ks_set_fit_strategy_shape(s.ctx, C.byref(fs), arr, n)
    ext = args[4]
    res = (_abi.KsFitResource * max(1, len(ext)))(*[_abi.KsFitResource(nm.encode(), w, 0) for nm, w in ext])
    return s.lib.ks_set_fit_strategy_resources(s.ctx, C.byref(fs), arr, n, res if ext else None, len(ext))


def getters(s):
    """(type, cpu, memory), the shape, the extended resources and the balanced list in force, through the C getters."""
    fs = _abi.KsFitStrategy()
    assert s.lib.ks_get_fit_strategy(s.ctx, C.byref(fs)) == OK
    n = C.c_uint32()
    pts = (_abi.KsFitShapePoint * _abi.FIT_SHAPE_MAX_POINTS)()
    assert s.lib.ks_get_fit_shape(s.ctx, pts, _abi.FIT_SHAPE_MAX_POINTS, C.byref(n)) == OK
    shape = [(pts[i].utilization, pts[i].score) for i in range(n.value)]
    res = (_abi.KsFitResource * _abi.FIT_MAX_RESOURCES)()
    assert s.lib.ks_get_fit_resources(s.ctx, res, _abi.FIT_MAX_RESOURCES, C.byref(n)) == OK
    ext = [(res[i].name.decode(), res[i].weight) for i in range(n.value)]
    names = (C.c_char_p * _abi.BALANCED_MAX_RESOURCES)()
    assert s.lib.ks_get_balanced_resources(s.ctx, names, _abi.BALANCED_MAX_RESOURCES, C.byref(n)) == OK
    return (fs.type, fs.weight_cpu, fs.weight_memory), shape, ext, [names[i].decode() for i in range(n.value)]


def accepted(config, setter, args):
    """The getters' answer after an accepted call, from the one before it."""
    fit, shape, ext, balanced = config
    if setter == "balanced":
        # the default list reads back as its names, however it was set
        return fit, shape, ext, (list(args) if args and args != ["cpu", "memory"] else ["cpu", "memory"])
    pts = list(args[3]) if setter != "fit" and args[0] == RTCR else []
    return tuple(args[:3]), pts, (list(args[4]) if setter == "resources" else []), balanced


def run_table(s, table):
    config = getters(s)
    assert config == ((LEAST, 1, 1), [], [], ["cpu", "memory"])
    wrong = []
    for i, (setter, args, status, text) in enumerate(table):
        before = s.lib.ks_last_error(s.ctx)
        got, err = call(s, setter, args), s.lib.ks_last_error(s.ctx)
        if got == OK:
            config = accepted(config, setter, args)
        print(i, setter, args, "->", got, err)
        if (got, err, getters(s)) != (status, before if text is None else text.encode(), config):
            wrong.append((i, setter, args, got, err, getters(s)))
    assert not wrong, wrong


def nodes():
    base = {"cpu": 8000, "memory": 16 * Gi, "pods": 110}
    return [Node("n0", dict(base)), Node("n1", dict(base), extended={GPU: 4, NIC: 2}), Node("n2", dict(base), extended={GPU: 2}),
            Node("n3", dict(base), extended={HUGE: 1 << 44})]


def test_setter_status_matrix():
    with Scheduler(64) as s:
        s.upsert_nodes(nodes(), [0, 1, 2, 63])
        run_table(s, FULL)


def test_setter_status_matrix_under_a_window():
    with Scheduler(64, percentage_of_nodes_to_score=50) as s:
        s.upsert_nodes(nodes(), [0, 1, 2, 63])
        run_table(s, WINDOW)
