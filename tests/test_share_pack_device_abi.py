"""The share pack from device memory, host side of its C-ABI (no GPU needed): the four entry points
exist and refuse a NULL handle, and fdbcs_share_bytes_bound, the stride a caller that holds only
device arrays sizes its all-gather with, bounds fdbcs_share_bytes of every batch of its sizes."""
import ctypes

import numpy as np
import pytest

from foundationdb_amd import build, conflict_set as C
from foundationdb_amd import workloads as W

NAMES = ["fdbcs_share_bytes_bound", "fdbcs_batch_share_pack_device", "fdbcs_batch_share_pack_info",
         "fdbcs_batch_share_pack_timing"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return C.load_library()


def test_entry_points_exist_with_signatures(lib):
    for name in NAMES:
        assert name in C.SIGNATURES and getattr(lib, name) is not None
    header = open(build.ROOT + "/" + build.PUBLIC_HEADER).read()
    assert all(f" {name}(" in header for name in NAMES)


def test_null_handle_is_invalid(lib):
    n, t, d = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
    dpb = C._CPackedBatchDev()
    assert lib.fdbcs_batch_share_pack_device(None, ctypes.byref(dpb), None, 0, None, 0) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_share_pack_info(None, ctypes.byref(n), ctypes.byref(t), ctypes.byref(t), ctypes.byref(t),
                                           ctypes.byref(n)) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_share_pack_timing(None, ctypes.byref(d), ctypes.byref(d)) == C.FDBCS_E_INVALID


def test_bound_refuses_negative_sizes_and_a_null_output(lib):
    n = ctypes.c_int64()
    for args in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        assert lib.fdbcs_share_bytes_bound(*args, ctypes.byref(n)) == C.FDBCS_E_INVALID
        with pytest.raises(C.FdbcsError) as e:
            C.share_bytes_bound(*args)
        assert e.value.status == C.FDBCS_E_INVALID
    assert lib.fdbcs_share_bytes_bound(1, 1, 1, 1, None) == C.FDBCS_E_INVALID


def test_bound_of_the_empty_share_is_320(lib):
    assert C.share_bytes_bound(0, 0, 0, 0) == 320
    assert len(C.share_pack(W.random_small_batch(np.random.default_rng(0), 0))) == 320


def test_bound_covers_the_exact_size_of_random_batches(lib):
    rng = np.random.default_rng(13)
    exact_hits = long_keys = 0
    for i in range(300):
        T = int(rng.integers(0, 12))
        pb = W.random_small_batch(rng, T, alphabet=5, max_len=40, now=10, staleness=5)
        exact = len(C.share_pack(pb))
        bound = C.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, len(pb.key_bytes))
        assert bound >= exact, (i, bound, exact)
        assert bound % 64 == 0
        # with no tails the bound counts the prefixes' bytes as tail bytes; it is exact for no keys
        exact_hits += bound == exact
        long_keys += int((np.diff(pb.key_offsets) > 16).sum())
    assert exact_hits > 0 and long_keys > 1000


def test_bound_is_monotone_in_each_argument(lib):
    rng = np.random.default_rng(14)
    for _ in range(200):
        a = [int(rng.integers(0, 3000)) for _ in range(3)] + [int(rng.integers(0, 100000))]
        base = C.share_bytes_bound(*a)
        for k in range(4):
            for step in (1, 15, 64, 1000):
                b = list(a)
                b[k] += step
                assert C.share_bytes_bound(*b) >= base, (a, b)
