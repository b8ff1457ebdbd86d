"""CPU test of the iops sample's C-ABI boundary: without a device, the new entry points refuse a
NULL handle before they touch anything."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_null_handles_are_invalid(lib):
    from foundationdb_amd import conflict_set as C

    n, nb, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
    off = (ctypes.c_int64 * 1)()
    assert lib.fdbcs_batch_set_iops_sample(None, 20000, 0) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_iops_sample(None, ctypes.byref(n), ctypes.byref(nb)) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_iops_sample_read(None, None, 0, ctypes.cast(off, ctypes.c_void_p), None, None, 0) \
        == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_iops_sample_timing(None, ctypes.byref(ms)) == C.FDBCS_E_INVALID
