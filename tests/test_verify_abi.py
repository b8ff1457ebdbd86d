"""CPU test of the stored-state check's C-ABI boundary: without a device the entry points exist, the
ctypes mirrors have the C layouts, and a NULL handle or report is refused before anything is touched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_symbols_exist(lib):
    for name in ("fdbcs_history_verify", "fdbcs_history_verify_timing", "fdbcs_history_verify_sizes"):
        assert getattr(lib, name) is not None


def test_ctypes_structs_have_the_c_sizes(lib):
    from foundationdb_amd import conflict_set as C

    rep, ov = ctypes.c_int64(), ctypes.c_int64()
    assert lib.fdbcs_history_verify_sizes(ctypes.byref(rep), ctypes.byref(ov)) == C.FDBCS_OK
    assert (rep.value, ov.value) == (ctypes.sizeof(C._CVerifyReport), ctypes.sizeof(C._CVerifyOverride)) == (600, 40)
    assert lib.fdbcs_history_verify_sizes(None, ctypes.byref(ov)) == C.FDBCS_E_INVALID
    assert len(C.VERIFY_CLASSES) == 12 and len(C.VERIFY_ARRAYS) == 11
    o = C.VerifyOverride("tail_word", 0, 7, xor_lo=-1).c_struct()
    assert (o.what, o.index, o.xor_lo, o.xor_hi) == (11, 7, (1 << 64) - 1, 0)


def test_null_handle_and_null_report_are_invalid(lib):
    from foundationdb_amd import conflict_set as C

    out = C._CVerifyReport()
    a, b = ctypes.c_double(), ctypes.c_double()
    assert lib.fdbcs_history_verify(None, 0, None, ctypes.byref(out)) == C.FDBCS_E_INVALID
    assert lib.fdbcs_history_verify_timing(None, ctypes.byref(a), ctypes.byref(b)) == C.FDBCS_E_INVALID
    # a non-NULL handle with a NULL report: refused on the arguments alone, the handle is never read
    fake = ctypes.create_string_buffer(64)
    assert lib.fdbcs_history_verify(ctypes.addressof(fake), 0, None, None) == C.FDBCS_E_INVALID


def test_no_device_fails_at_construction(lib):
    import torch

    from foundationdb_amd import conflict_set as C

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(C.FdbcsError) as e:
        C.ConflictSet(0)
    assert e.value.status == C.FDBCS_E_NODEVICE


def test_report_accessors():
    from foundationdb_amd import conflict_set as C

    r = C._CVerifyReport()
    r.tier[1].n = 5
    r.tier[1].cls[4].examined, r.tier[1].cls[4].violations, r.tier[1].cls[4].first = 9, 2, 3
    for t in range(2):
        for c in range(12):
            if (t, c) != (1, 4):
                r.tier[t].cls[c].first = -1
    rep = C.VerifyReport._of(r)
    assert not rep.ok and rep.violations(1, "dominance") == 2 and rep.first(1, "dominance") == 3
    assert rep.first(0, "order") == -1 and rep.examined(1, 4) == 9
    assert rep.as_dict()["tiers"][1]["dominance"] == {"examined": 9, "violations": 2, "first": 3}
    assert C.VerifyReport._of(C._CVerifyReport()).ok
