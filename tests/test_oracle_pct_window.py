"""The streams of tests/pct_window_cases.py on the CPU: the C++ oracle against
the plain-Python restatement after every pod, and each stream's own check that
it placed the window where it was built to (chunk edges, the `all` boundary,
the wrap) -- the same streams that tests/test_gpu_pct_window.py runs on the
device."""
import pytest

import pct_window_cases as W
from test_oracle_pct_restated import OraclePair


@pytest.mark.parametrize("cap,pattern", W.SLOT_CASES)
def test_slot_count_streams(cap, pattern):
    W.check_slot_count_stream(W.slot_count_stream(OraclePair(cap, 5), cap, pattern), cap, pattern)


@pytest.mark.parametrize("length", [99, 100, 101])
def test_list_lengths(length):
    W.check_named_lengths(W.named_lengths_stream(OraclePair(3000, 5), length), length)
    W.check_present_lengths(W.present_lengths_stream(OraclePair(1500, 5), length), length)


def test_holes():
    W.check_holes(W.holes_stream(OraclePair(3000, 5)))


def test_prefilter_result_then_plain_pods():
    W.check_prefilter_then_plain(*W.prefilter_then_plain_stream(OraclePair(1500, 5)))


def test_more_than_1024_chunks():
    W.check_big(W.big_stream(OraclePair(W.BIG_CAP, 5)))


def test_adaptive_floor():
    W.check_adaptive_floor(W.adaptive_floor_stream(OraclePair(6000, 0)))
