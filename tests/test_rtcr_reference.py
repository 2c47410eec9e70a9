"""RequestedToCapacityRatio on the CPU: the restatement's known answers
(tests/rtcr_reference.py; values of SURVEY.md Appendix A, derived by hand),
ks_fit_shape_table -- the table the kernels read -- against it, the refusals
that need no device, and the C header's new struct and enum value against the
ctypes mirror."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from fit_reference import LEAST, fit_scores
from ksched import _abi
from rtcr_reference import SHAPES, raw, round_half_away, rtcr_scores, table, trunc_div

ROOT = Path(__file__).resolve().parent.parent


def one(shape, wc, wm, cap, req):
    """Node score of one node: cap / req are (cpu, memory)."""
    return int(rtcr_scores(shape, wc, wm, [cap[0]], [cap[1]], [req[0]], [req[1]])[0])


# ------------------------------------------------------------- the restatement
def test_truncation_is_toward_zero():
    assert trunc_div([-100, -199, 100, 199, -1, 0], 100).tolist() == [-1, -1, 1, 1, 0, 0]
    assert (np.array([-199]) // 100).tolist() == [-2]  # what numpy's own division would have given


def test_shape_known_answers():
    f = SHAPES["falling"]  # {0:100, 30:0}
    assert raw(f, [1, 15, 29, 30, 31, 100]).tolist() == [97, 50, 4, 0, 0, 0]  # floor would give 96 at 1
    p = SHAPES["peaked"]  # {0:0, 50:100, 100:0}
    assert raw(p, [0, 25, 50, 75, 99, 100]).tolist() == [0, 50, 100, 50, 2, 0]
    o = SHAPES["offset"]  # {20:20, 80:90}
    assert raw(o, [0, 20, 21, 50, 80, 81, 100]).tolist() == [20, 20, 21, 55, 90, 90, 90]
    assert set(table(SHAPES["flat"]).tolist()) == {70}
    assert table(SHAPES["binpack"]).tolist() == list(range(101))


def test_node_score_known_answers():
    b = SHAPES["binpack"]  # raw(p) = p
    # resource scores (30, 45): round(37.5) = 38, truncation would give 37
    assert one(b, 1, 1, (100, 100), (30, 45)) == 38
    # (100, 0): a zero score leaves the weight sum
    assert one(b, 1, 1, (100, 100), (100, 0)) == 100
    assert one(b, 1, 1, (100, 100), (0, 0)) == 0
    # requested > capacity is utilisation 100
    assert one(b, 1, 1, (100, 100), (250, 40)) == 70
    # weights: (3 x 30 + 45) / 4 = 33.75 -> 34; a resource not listed
    assert one(b, 3, 1, (100, 100), (30, 45)) == 34
    assert one(b, 1, 0, (100, 100), (30, 45)) == 30
    assert one(b, 0, 1, (100, 100), (30, 45)) == 45
    assert round_half_away(np.array([75, 5, 1, 149]), np.array([2, 2, 2, 2])).tolist() == [38, 3, 1, 75]


def test_zero_allocatable_resource_takes_no_part():
    f = SHAPES["falling"]  # raw(0) = 100 > 0: a memory-less node must not score memory's utilisation 0
    assert one(f, 1, 1, (1000, 0), (150, 0)) == 50
    assert one(f, 1, 1, (1000, 0), (150, 12345)) == 50
    assert one(f, 1, 1, (1000, 1000), (150, 0)) == 75  # with memory Allocatable it does
    assert one(f, 1, 1, (0, 0), (0, 0)) == 0


def test_not_least_allocated():
    """{0:10, 100:0} with weights (1, 1) is not LeastAllocated: the utilisation
    is truncated before the shape, the mean is rounded, a zero score drops out."""
    s = ((0, 10), (100, 0))
    # where they must agree: utilisations that divide exactly, positive scores of even sum
    caps, reqs = [], []
    for k in range(1, 40):
        for jc, jm in ((10, 20), (33, 41), (98, 2), (0, 64), (7, 7)):
            caps.append((100 * k, 300 * k))
            reqs.append((jc * k, 3 * jm * k))
    cc, cm = np.array(caps).T
    rc, rm = np.array(reqs).T
    assert np.array_equal(rtcr_scores(s, 1, 1, cc, cm, rc, rm), fit_scores((LEAST, 1, 1), cc, cm, rc, rm))
    la = lambda cap, req: int(fit_scores((LEAST, 1, 1), [cap[0]], [cap[1]], [req[0]], [req[1]])[0])
    # rounding against truncation: scores (70, 55) -> 62.5
    assert (one(s, 1, 1, (100, 100), (30, 45)), la((100, 100), (30, 45))) == (63, 62)
    # the zero-score rule: scores (100, 0)
    assert (one(s, 1, 1, (100, 100), (0, 100)), la((100, 100), (0, 100))) == (100, 50)
    # the utilisation's own truncation: 1 of 3 is utilisation 33 -> 67, LeastAllocated 200 / 3 = 66
    assert (one(s, 1, 0, (3, 100), (1, 0)), la((3, 100), (1, 0))) == (67, 83)
    assert int(fit_scores((LEAST, 1, 0), [3], [100], [1], [0])[0]) == 66


# ------------------------------------------------------- ks_fit_shape_table
def lib_table(shape):
    lib = _abi.ksched_lib()
    pts = (_abi.KsFitShapePoint * max(1, len(shape)))(*[_abi.KsFitShapePoint(u, v) for u, v in shape])
    out = (C.c_uint8 * 101)()
    st = lib.ks_fit_shape_table(pts, len(shape), out)
    return st, list(out)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_table_known_shapes(name):
    st, got = lib_table(SHAPES[name])
    assert st == 0
    assert got == table(SHAPES[name]).tolist()


def test_shape_table_random_shapes():
    rng = random.Random(5)
    for _ in range(3000):
        n = rng.choice([1, 2, 2, 3, 4, 8, 30, 101])
        xs = sorted(rng.sample(range(101), n))
        shape = tuple((x, rng.randrange(11)) for x in xs)
        st, got = lib_table(shape)
        assert st == 0 and got == table(shape).tolist(), shape


def test_shape_table_refusals():
    lib = _abi.ksched_lib()
    out = (C.c_uint8 * 101)()
    assert lib.ks_fit_shape_table(None, 0, out) == _abi.KS_ERR_INVALID
    assert lib.ks_fit_shape_table(None, 2, out) == _abi.KS_ERR_INVALID
    pts = (_abi.KsFitShapePoint * 1)(_abi.KsFitShapePoint(0, 0))
    assert lib.ks_fit_shape_table(pts, 0, out) == _abi.KS_ERR_INVALID  # empty
    assert lib.ks_fit_shape_table(pts, 1, None) == _abi.KS_ERR_INVALID
    for bad in [((0, 11),), ((0, -1),), ((101, 5),), ((-1, 5),), ((10, 1), (10, 2)), ((20, 1), (10, 2)),
                tuple((min(i, 100), 1) for i in range(102))]:
        assert lib_table(bad)[0] == _abi.KS_ERR_INVALID, bad
    assert lib_table(tuple((i, i % 11) for i in range(101)))[0] == 0  # 101 points: the most there can be


def test_shape_calls_reject_null_arguments():
    lib = _abi.ksched_lib()
    fs = _abi.KsFitStrategy(_abi.FIT_REQUESTED_TO_CAPACITY_RATIO, 1, 1, 0)
    pts = (_abi.KsFitShapePoint * 2)(_abi.KsFitShapePoint(0, 0), _abi.KsFitShapePoint(100, 10))
    n = C.c_uint32()
    assert lib.ks_set_fit_strategy_shape(None, C.byref(fs), pts, 2) == _abi.KS_ERR_INVALID
    assert lib.ks_get_fit_shape(None, pts, 2, C.byref(n)) == _abi.KS_ERR_INVALID
    assert lib.ks_abi_version() == 6


# ------------------------------------------------------------ header mirror
C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
int main(void) {
  printf("size %zu\n", sizeof(ks_fit_shape_point));
  printf("utilization %zu\n", offsetof(ks_fit_shape_point, utilization));
  printf("score %zu\n", offsetof(ks_fit_shape_point, score));
  printf("RTCR %d\n", (int)KS_FIT_REQUESTED_TO_CAPACITY_RATIO);
  printf("strategy %zu\n", sizeof(ks_fit_strategy));
  return 0;
}
"""


def test_shape_point_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got.pop("size") == C.sizeof(_abi.KsFitShapePoint) == 8
    assert got.pop("strategy") == C.sizeof(_abi.KsFitStrategy) == 16  # unchanged
    assert got.pop("RTCR") == _abi.FIT_REQUESTED_TO_CAPACITY_RATIO == _abi.FIT_TYPES["RequestedToCapacityRatio"] == 2
    assert [f for f, _ in _abi.KsFitShapePoint._fields_] == list(got)
    for field, off in got.items():
        assert getattr(_abi.KsFitShapePoint, field).offset == off, field
    assert "ks_fit_shape_point" not in _abi.STRUCTS and "ks_fit_strategy" not in _abi.STRUCTS
    for sym in ("ks_set_fit_strategy_shape", "ks_get_fit_shape", "ks_fit_shape_table"):
        assert sym in _abi.KSCHED_SYMBOLS


# ------------------------------------------------- the composed reference
def test_reference_on_the_edge_stream():
    """The stream of tests/rtcr_workloads.py that holds memory-less nodes and
    nodes filled beyond their cpu capacity: under the default strategy the
    composition is the oracle's own schedule there, and under a shape the
    stream reaches both kinds of node."""
    import pyoracle
    import rtcr_workloads as R
    from fit_reference import DEFAULT
    from helpers import assert_results_equal, res_array
    from rtcr_reference import RtcrReference
    w = R.edge_stream()
    r = RtcrReference(R.N_EDGE, DEFAULT)
    o = pyoracle.Oracle(R.N_EDGE)
    for t in (r, o):
        t.upsert(w["nodes"], w["slots"], w["n"])
    assert_results_equal(r.schedule(w["pods"], w["m"]), o.schedule(w["pods"], w["m"]), w["m"], "edge stream, default")
    r.close()
    o.close()
    for name in ("falling-1-1", "peaked-1-1"):
        ref = R.edge_reference(name)
        st = ref[1][1]
        assert ((st["alloc_mem"] == 0) & (st["pod_count"] > 0)).sum() > 50, name
        assert (st["nz_cpu"] > st["alloc_cpu"]).sum() > 50, name
        res = np.concatenate([res_array(ref[0][0], w["m1"]), res_array(ref[1][0], w["m"] - w["m1"])])
        assert (res["status"] == 0).all()
    # the two shapes schedule differently: the stream tells them apart
    a, b = R.edge_reference("falling-1-1"), R.edge_reference("peaked-1-1")
    assert not np.array_equal(res_array(a[0][0], w["m1"])["node_index"], res_array(b[0][0], w["m1"])["node_index"])
