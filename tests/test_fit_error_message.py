"""ks_fit_error_message alone (pure host code, no context, no GPU):
FitError.Error() without the PostFilter part -- the header, the PreFilter
message form, equal strings merged, "<count> <reason>" sorted bytewise as Go's
sort.Strings sorts them, and the cap / len convention."""
import ctypes as C

from ksched import _abi
from ksched.framework import fit_error_message

INV = _abi.KS_ERR_INVALID


def rows(pairs):
    return (_abi.KsReason * max(1, len(pairs)))(*[_abi.KsReason(0, c, r.encode()) for r, c in pairs])


def call(n_all, pairs, pm=None, cap=None):
    lib = _abi.ksched_lib()
    n = C.c_size_t(12345)
    cap = 4096 if cap is None else cap
    buf = C.create_string_buffer(b"\xff" * 8, max(cap, 8)) if cap else None
    st = lib.ks_fit_error_message(n_all, pm, rows(pairs), len(pairs), buf, cap, C.byref(n))
    return st, n.value, (buf.value.decode() if buf is not None and st == 0 else None)


def test_issue_example():
    st, n, msg = call(1000000, [("Insufficient memory", 12), ("node(s) had untolerated taint {dedicated: infra}", 3),
                                ("Insufficient cpu", 999985)])
    assert st == 0
    assert msg == ("0/1000000 nodes are available: 12 Insufficient memory, "
                   "3 node(s) had untolerated taint {dedicated: infra}, 999985 Insufficient cpu.")
    assert n == len(msg)


def test_sorted_as_strings_not_numbers():
    # "10 ..." < "2 ..." bytewise; "9 a" after both; an upper-case letter before a lower-case one
    _, _, msg = call(30, [("Insufficient memory", 2), ("Insufficient cpu", 10), ("a", 9), ("Too many pods", 10)])
    assert msg == "0/30 nodes are available: 10 Insufficient cpu, 10 Too many pods, 2 Insufficient memory, 9 a."


def test_equal_strings_merge_before_sorting():
    # 6 + 5 = 11 sorts before 2; merged rows need not be adjacent
    _, _, msg = call(13, [("Insufficient cpu", 6), ("Insufficient memory", 2), ("Insufficient cpu", 5)])
    assert msg == "0/13 nodes are available: 11 Insufficient cpu, 2 Insufficient memory."


def test_bytes_above_ascii_sort_after_it():
    _, _, msg = call(2, [("1 é", 1), ("1 z", 1)])  # equal counts: the reasons decide; 'z' (0x7a) < 0xc3
    assert msg == "0/2 nodes are available: 1 1 z, 1 1 é."


def test_no_reasons():
    st, n, msg = call(7, [])
    assert (st, msg) == (0, "0/7 nodes are available:") and n == len(msg)
    lib = _abi.ksched_lib()
    ln = C.c_size_t()
    buf = C.create_string_buffer(64)
    assert lib.ks_fit_error_message(0, None, None, 0, buf, 64, C.byref(ln)) == 0  # null reasons with n == 0
    assert buf.value == b"0/0 nodes are available:"


def test_prefilter_message_replaces_the_histogram():
    _, _, msg = call(5, [("pod affinity terms conflict", 5)], pm=b"pod affinity terms conflict")
    assert msg == "0/5 nodes are available: pod affinity terms conflict."
    _, _, msg = call(5, [("x", 5)], pm=b"")  # an empty message is no message
    assert msg == "0/5 nodes are available: 5 x."


def test_cap_and_len():
    pairs = [("Insufficient cpu", 3)]
    want = "0/3 nodes are available: 3 Insufficient cpu."
    st, n, _ = call(3, pairs, cap=0)  # sizing call: null buffer
    assert (st, n) == (INV, len(want))
    st, n, _ = call(3, pairs, cap=len(want))  # no room for the terminator
    assert (st, n) == (INV, len(want))
    st, n, msg = call(3, pairs, cap=len(want) + 1)
    assert (st, n, msg) == (0, len(want), want)
    # a refused call leaves the buffer alone
    lib = _abi.ksched_lib()
    buf = C.create_string_buffer(b"keep", 8)
    ln = C.c_size_t()
    assert lib.ks_fit_error_message(3, None, rows(pairs), 1, buf, 8, C.byref(ln)) == INV
    assert buf.value == b"keep"


def test_null_arguments():
    lib = _abi.ksched_lib()
    ln = C.c_size_t()
    buf = C.create_string_buffer(64)
    one = rows([("x", 1)])
    assert lib.ks_fit_error_message(1, None, one, 1, buf, 64, None) == INV           # len
    assert lib.ks_fit_error_message(1, None, None, 1, buf, 64, C.byref(ln)) == INV   # reasons with n > 0
    assert lib.ks_fit_error_message(1, None, one, 1, None, 64, C.byref(ln)) == INV   # buf with cap > 0
    null_reason = (_abi.KsReason * 1)(_abi.KsReason(0, 1, None))
    assert lib.ks_fit_error_message(1, None, null_reason, 1, buf, 64, C.byref(ln)) == INV


def test_python_wrapper():
    assert fit_error_message(4, {"b": 1, "a": 3}) == "0/4 nodes are available: 1 b, 3 a."
    assert fit_error_message(4, [("a", 1), ("a", 2)]) == "0/4 nodes are available: 3 a."
    assert fit_error_message(4, {"a": 4}, "msg") == "0/4 nodes are available: msg."
