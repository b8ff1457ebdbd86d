"""CPU test of the device add's C-ABI boundary: without a device, the new entry points exist and
refuse a NULL handle before they touch anything."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_null_handles_are_invalid(lib):
    from foundationdb_amd import conflict_set as C
    from foundationdb_amd.packing import DevicePackedBatch

    dpb = DevicePackedBatch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0).c_struct()
    t, r, w, tb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    a, b = ctypes.c_double(), ctypes.c_double()
    assert lib.fdbcs_batch_add_packed_device(None, ctypes.byref(dpb), None, 0) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_device_add_info(None, ctypes.byref(t), ctypes.byref(r), ctypes.byref(w),
                                           ctypes.byref(tb)) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_device_add_timing(None, ctypes.byref(a), ctypes.byref(b)) == C.FDBCS_E_INVALID


def test_device_packed_batch_holds_addresses_only():
    """packing.py stays importable without torch: the struct is pointers and sizes."""
    from foundationdb_amd.packing import DevicePackedBatch

    c = DevicePackedBatch(3, 4, 5, 99, 0x1000, 0, 0x2000, 0x3000, 0x4001, 0x5000).c_struct()
    assert (c.n_txn, c.n_reads, c.n_writes, c.key_bytes_len) == (3, 4, 5, 99)
    assert c.report_conflicting_keys is None and c.key_bytes == 0x4001
