"""CPU tests of the delta-tier history import's surface: the library exports the entry points and
they refuse a NULL handle, the Python `into` keyword is checked before the library is touched, and
the known-answer of the GPU invariant test follows from merge_max alone."""
import ctypes

import numpy as np
import pytest

from tests.import_helpers import merge_max, merge_max_fast


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_entry_points_refuse_a_null_handle(lib):
    from foundationdb_amd import conflict_set as C

    out = ctypes.c_int64(-7)
    ko = np.zeros(1, np.int64)
    assert lib.fdbcs_history_import_delta(None, None, -1, None, -1, 0, None, ko.ctypes.data, None, 0,
                                          ctypes.byref(out)) == C.FDBCS_E_INVALID
    assert lib.fdbcs_history_import_delta_pending(None, None, None, -1, None, -1, ctypes.byref(out)) == C.FDBCS_E_INVALID
    path, base, before, after = ctypes.c_int32(-7), ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert lib.fdbcs_history_import_info(None, ctypes.byref(path), ctypes.byref(base), ctypes.byref(before),
                                         ctypes.byref(after)) == C.FDBCS_E_INVALID
    assert (out.value, path.value, base.value, before.value, after.value) == (-7,) * 5  # nothing written


def test_into_is_checked_before_the_library_is_touched(monkeypatch):
    from foundationdb_amd import conflict_set as C

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(C, "load_library", no_library)
    cs = C.ConflictSet.__new__(C.ConflictSet)  # no handle: nothing may reach the C-ABI
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int64))
    for bad in ("nonsense", "", "Delta", None, 1):
        with pytest.raises(ValueError):
            cs.merge_history(*empty, into=bad)
        with pytest.raises(ValueError):
            cs.merge_pending_export(cs, into=bad)
    for good in ("base", "delta"):  # accepted: the call goes on to the library
        with pytest.raises(AssertionError, match="the library was loaded"):
            cs.merge_history(*empty, into=good)


def test_known_answer_of_the_invariant_test():
    """tests/test_gpu_import_delta.py::test_invariant_known_answer: base a < b < c < d at 10, 50, 10,
    10, the single segment [a, d) at 30 imported over [a, d).  The base's 50 stays."""
    a, b, c, d = b"a", b"b", b"c", b"d"
    own = (0, [a, b, c, d], [10, 50, 10, 10])
    imp = (0, [a, d], [30, 0])
    want = (0, [a, b, c, d], [30, 50, 30, 10])
    assert merge_max(own, imp, a, d) == merge_max_fast(own, imp, a, d) == want
    # with a committed write [a, a + 0) at 60 before the import (its closing boundary: a hole in the delta)
    own = (0, [a, a + b"\x00", b, c, d], [60, 10, 50, 10, 10])
    want = (0, [a, a + b"\x00", b, c, d], [60, 30, 50, 30, 10])
    assert merge_max(own, imp, a, d) == merge_max_fast(own, imp, a, d) == want
    # the point reads: a read at snapshot s of key k conflicts iff H'(k) > s
    at = lambda st, k: ([st[0]] + [v for kk, v in zip(st[1], st[2]) if kk <= k])[-1]
    st = merge_max((0, [a, b, c, d], [10, 50, 10, 10]), imp, a, d)
    assert at(st, b) > 40 and not at(st, a) > 35 and at(st, a) > 25 and not at(st, d) > 25
