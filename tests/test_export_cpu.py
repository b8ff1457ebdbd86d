"""CPU tests of the history export's definition: the canonical form over the oracle's dump agrees
with point lookups, does not depend on GC at floor = oldest version, and the library exports the
entry points."""
import ctypes

import numpy as np

from foundationdb_amd import workloads as W
from tests.export_helpers import NO_FLOOR, canon


def _value_at(hdr, ks, vs, key):
    """The canonical step function read at `key`."""
    v = hdr
    for k, x in zip(ks, vs):
        if k > key:
            break
        v = x
    return v


def _states(oracle, gc, seeds=range(6), batches=30):
    for seed in seeds:
        rng = np.random.default_rng(4200 + seed)
        o = oracle.OracleConflictSet()
        if seed % 3 == 0:
            o.clear(4)
        now = 20
        for _ in range(batches):
            pb = W.random_small_batch(rng, int(rng.integers(2, 12)), alphabet=4, max_len=3, now=now, staleness=30,
                                      max_writes=1)
            o.detect(pb, now, now - int(rng.integers(25, 45)), gc=gc)
            now += int(rng.integers(1, 5))
        yield seed, (4 if seed % 3 == 0 else 0), o


def test_canon_agrees_with_version_at(oracle_built):
    rng = np.random.default_rng(1)
    for seed, header, o in _states(oracle_built, True):
        keys, vers = o.dump_history()
        probes = [b""] + keys + [k + b"\x00" for k in keys] + [
            bytes(int(x) for x in rng.integers(0, 4, size=int(rng.integers(0, 5)))) for _ in range(60)]
        for floor in (NO_FLOOR, o.oldest_version, o.oldest_version + 3):
            cl = lambda v: v if (floor == NO_FLOOR or v >= floor) else floor - 1
            hdr, ks, vs = canon(keys, vers, header, floor)
            assert ks == sorted(set(ks)) and all(a != b for a, b in zip([hdr] + vs, vs))
            for p in probes:
                assert _value_at(hdr, ks, vs, p) == cl(o.version_at(p)), (seed, floor, p)
            # clipped: header H_f(lo), boundaries strictly inside (lo, hi)
            for _ in range(25):
                lo, hi = sorted((probes[int(rng.integers(len(probes)))], probes[int(rng.integers(len(probes)))]))
                h2, k2, v2 = canon(keys, vers, header, floor, lo, hi)
                assert h2 == cl(o.version_at(lo)), (seed, lo, hi)
                assert all(lo < k < hi for k in k2)
                assert all(a != b for a, b in zip([h2] + v2, v2))
                for p in probes:
                    if lo <= p < hi:
                        assert _value_at(h2, k2, v2, p) == cl(o.version_at(p)), (seed, lo, hi, p)
                assert canon(keys, vers, header, floor, lo, lo)[1:] == ([], [])
                assert canon(keys, vers, header, floor, lo, None)[0] == h2
                assert canon(keys, vers, header, floor, None, hi)[0] == cl(header)


def test_canon_is_gc_neutral_at_the_oldest_version(oracle_built):
    total = 0
    for (seed, header, a), (_, _, b) in zip(_states(oracle_built, True, range(12)),
                                           _states(oracle_built, False, range(12))):
        assert a.oldest_version == b.oldest_version
        ca = canon(*a.dump_history(), header, a.oldest_version)
        cb = canon(*b.dump_history(), header, b.oldest_version)
        assert ca == cb, seed
        total += len(ca[1])
    assert total > 50  # the states are not empty


def test_export_symbols_bound_and_reject_null():
    from foundationdb_amd import build, conflict_set

    build.build()
    L = conflict_set.load_library()
    assert conflict_set.NO_FLOOR == -(1 << 63)
    for name in ("fdbcs_history_export", "fdbcs_history_export_read"):
        assert name in conflict_set.SIGNATURES
        assert getattr(L, name).argtypes == conflict_set.SIGNATURES[name][1]
    n, nb, hdr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = L.fdbcs_history_export(None, None, -1, None, -1, conflict_set.NO_FLOOR, ctypes.byref(n), ctypes.byref(nb),
                                ctypes.byref(hdr))
    assert rc == conflict_set.FDBCS_E_INVALID
    off = np.zeros(1, np.int64)
    rc = L.fdbcs_history_export_read(None, None, 0, ctypes.c_void_p(off.ctypes.data), None, 0)
    assert rc == conflict_set.FDBCS_E_INVALID
