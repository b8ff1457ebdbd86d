"""CPU tests of the read-version query: the plain-Python model (tests/read_versions_model.py)
against the semantic oracle, and the C-ABI boundary without a device.

The model is what every GPU test of the query compares with, so it is pinned here first, against the
oracle's own point lookup and against the oracle's own detect: a read-only batch whose snapshot is
V_r never conflicts, the same batch at V_r - 1 always does."""
import ctypes
import inspect

import numpy as np
import pytest

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests import read_versions_model as M

CONFLICT, COMMITTED = 0, 2
PREFIX = b"\x15tenant\x00orders\x00\x02\x02"  # 17 bytes: longer keys part only past the 16-byte prefix words
LENGTHS = (0, 1, 1, 2, 2, 3, 3, 17, 19, 24, 25, 40)


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


def rand_key(rng, alphabet):
    n = int(rng.choice(LENGTHS))
    tail = bytes(int(x) for x in rng.integers(0, alphabet, size=n if n < 17 else n - 17))
    return tail if n < 17 else PREFIX + tail


def build_state(oracle_mod, seed):
    """An oracle after 6 write batches over keys of 0 to 40 bytes, versions 100 .. 150 over a header
    of 40, oldest version 10: (oracle, keys, versions, header)."""
    rng = np.random.default_rng(seed)
    alphabet = int(rng.integers(2, 5))
    o = oracle_mod.OracleConflictSet()
    header = 40
    o.clear(header)
    o.set_oldest_version(10)
    for i in range(6):
        now = 100 + 10 * i
        txns = []
        for _ in range(16):
            a, b = sorted((rand_key(rng, alphabet), rand_key(rng, alphabet)))
            # mostly single keys, and only these in the last batches: a wide write leaves one segment
            # of all it covers
            if i >= 3 or rng.random() < 0.7:
                b = a + b"\x00"
            txns.append(CommitTransaction([], [KeyRange(a, b)], now, False))
        v, _ = o.detect(PackedBatch.from_transactions(txns), now, 10)
        assert (v == COMMITTED).all()
    keys, vers = o.dump_history()
    assert len(keys) >= 10 and len(set(vers.tolist())) >= 3
    return o, keys, vers.tolist(), header, rng, alphabet


def probe_keys(keys, rng, alphabet):
    out = [b"", b"\x00"]
    for k in keys:
        out += [k, k + b"\x00", k[:-1], k[:-1] + bytes([max(k[-1], 1) - 1]) if k else b""]
    out += [rand_key(rng, alphabet) for _ in range(60)]
    return sorted(set(out))


@pytest.mark.parametrize("seed", range(6))
def test_model_point_reads_equal_the_oracle(oracle_mod, seed):
    o, keys, vers, header, rng, alphabet = build_state(oracle_mod, seed)
    probes = probe_keys(keys, rng, alphabet)
    assert len(probes) > 50
    for k in probes:
        assert M.version_at(keys, vers, header, k) == o.version_at(k), k
        assert M.version_at(keys, vers, header, k, 10) == o.version_at(k), k  # nothing lies below the floor
    assert M.version_at(keys, vers, header, b"") in (header, vers[0])
    # the floor: every version below it reads floor - 1, the others as they are
    for k in probes[::7]:
        v = o.version_at(k)
        assert M.version_at(keys, vers, header, k, 125) == (v if v >= 125 else 124)
    assert M.read_version(keys, vers, header, keys[0], keys[0]) == header  # b == the first boundary
    assert M.read_version(keys, vers, header, b"", b"") == header


@pytest.mark.parametrize("seed", range(6))
def test_verdict_property_against_the_oracles_detect(oracle_mod, seed):
    """Reads that are degenerate, at b"", at and beside boundaries, ending at boundaries and wide:
    one transaction per read and snapshot, every verdict compared."""
    o, keys, vers, header, rng, alphabet = build_state(oracle_mod, seed)
    probes = probe_keys(keys, rng, alphabet)
    ranges = [(k, k) for k in probes[::3]] + [(b"", b""), (b"", b"\x00"), (b"", keys[0]), (b"", keys[-1] + b"\xff")]
    for i, k in enumerate(keys):
        ranges += [(k, k + b"\x00"), (k, keys[min(i + 1, len(keys) - 1)]), (k, keys[min(i + 3, len(keys) - 1)])]
        if k:
            ranges += [(k[:-1], k), (k[:-1], k + b"\x00")]
    for _ in range(150):
        a, b = sorted(rng.choice(len(probes), size=2))
        ranges.append((probes[a], probes[b]))
    ranges = [r for r in ranges if r[0] <= r[1]]
    V = M.read_versions(keys, vers, header, ranges)
    assert V == M.read_versions(keys, vers, header, ranges, o.oldest_version)
    assert len(V) == len(ranges) > 200 and min(V) - 1 >= o.oldest_version  # no snapshot below is TooOld
    assert sum(a == b for a, b in ranges) >= 20 and len(set(V)) >= 3
    txns = [CommitTransaction([KeyRange(a, b)], [], v - d, False) for d in (0, 1) for (a, b), v in zip(ranges, V)]
    want = np.repeat(np.array([COMMITTED, CONFLICT], np.uint8), len(ranges))
    got, _ = o.detect(PackedBatch.from_transactions(txns), 200, o.oldest_version)
    assert len(got) == len(want) == 2 * len(ranges)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(ranges[i % len(ranges)], V[i % len(ranges)], int(got[i])) for i in bad[:5]]
    assert (got == CONFLICT).mean() >= 0.3 and (got == COMMITTED).mean() >= 0.3


# ---- the C-ABI boundary

@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


NEW_SYMBOLS = ("fdbcs_batch_read_versions", "fdbcs_batch_read_versions_device", "fdbcs_batch_read_versions_timing")


def test_symbols_are_exported_and_declared(lib):
    from foundationdb_amd import build, conflict_set as C

    raw = ctypes.CDLL(C.LIB_PATH)
    with open(build.ROOT + "/" + build.PUBLIC_HEADER) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert getattr(raw, name) is not None
        assert name in C.SIGNATURES and f"int {name}(fdbcs_batch* b" in header


def test_null_handles_are_invalid(lib):
    from foundationdb_amd import conflict_set as C

    out = np.zeros(4, np.int64)
    a, b = ctypes.c_double(), ctypes.c_double()
    assert lib.fdbcs_batch_read_versions(None, C.NO_FLOOR, out.ctypes.data, 4) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_read_versions_device(None, 0, out.ctypes.data, 4) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_read_versions_timing(None, ctypes.byref(a), ctypes.byref(b)) == C.FDBCS_E_INVALID
    assert (out == 0).all()


def test_python_wrappers_have_the_stated_signatures():
    from foundationdb_amd import conflict_set as C

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]

    assert params(C.ConflictBatch.read_versions) == [("floor", None)]
    assert params(C.ConflictBatch.read_versions_device) == [("dev_out_ptr", inspect.Parameter.empty),
                                                             ("cap", inspect.Parameter.empty), ("floor", None)]
    assert params(C.ConflictBatch.read_versions_timing) == []
    assert params(C.ConflictSet.read_versions) == [("ranges", inspect.Parameter.empty), ("floor", None)]
    assert params(C.ConflictSet.version_at) == [("key", inspect.Parameter.empty), ("floor", None)]
