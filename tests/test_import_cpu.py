"""CPU tests of the history import's definition: merge_max (tests/import_helpers.py) agrees with
point lookups in the semantic oracle, the max of two histories is the history of the resolver that
saw both write streams, and the library exports the entry points."""
import ctypes

import numpy as np

from foundationdb_amd import workloads as W
from tests.export_helpers import NO_FLOOR, canon
from tests.import_helpers import merge_max, merge_max_fast, pack, shifted


def _value_at(hdr, ks, vs, key):
    v = hdr
    for k, x in zip(ks, vs):
        if k > key:
            break
        v = x
    return v


def _state(oracle, seed, batches=30):
    """A random small state as test_export_cpu.py builds them: (header, oracle)."""
    rng = np.random.default_rng(7300 + seed)
    o = oracle.OracleConflictSet()
    header = 4 if seed % 3 == 0 else 0
    if header:
        o.clear(header)
    now = 20
    for _ in range(batches):
        pb = W.random_small_batch(rng, int(rng.integers(2, 12)), alphabet=4, max_len=3, now=now, staleness=30,
                                  max_writes=1)
        o.detect(pb, now, now - int(rng.integers(25, 45)), gc=bool(seed & 1))
        now += int(rng.integers(1, 5))
    return header, o


def _is_canonical(state):
    hdr, ks, vs = state
    return ks == sorted(set(ks)) and all(a != b for a, b in zip([hdr] + vs, vs))


def test_merge_max_agrees_with_version_at(oracle_built):
    rng = np.random.default_rng(11)
    cases = changed = 0
    for pair in range(12):
        h1, o1 = _state(oracle_built, 2 * pair)
        h2, o2 = _state(oracle_built, 2 * pair + 1)
        k1, v1 = o1.dump_history()
        k2, v2 = o2.dump_history()
        own = canon(k1, v1, h1, NO_FLOOR)
        probes = sorted(set([b""] + k1 + k2 + [k + b"\x00" for k in k1 + k2]))
        for c in range(20):
            lo = hi = None
            if c % 5 != 0:
                lo = probes[int(rng.integers(len(probes)))]
            if c % 5 != 1:
                hi = probes[int(rng.integers(len(probes)))]
            if lo is not None and hi is not None and lo > hi:
                lo, hi = hi, lo
            # the import: the whole history, or (the hand-over) the export of the range itself
            imp = canon(k2, v2, h2, NO_FLOOR) if c & 1 else canon(k2, v2, h2, NO_FLOOR, lo, hi)
            got = merge_max(own, imp, lo, hi)
            assert _is_canonical(got), (pair, lo, hi)
            assert got == merge_max_fast(own, imp, lo, hi)
            assert got[0] == (max(h1, imp[0]) if lo is None else h1)
            for p in probes + [lo, hi]:
                if p is None:
                    continue
                inside = (lo is None or p >= lo) and (hi is None or p < hi)
                want = max(o1.version_at(p), o2.version_at(p)) if inside else o1.version_at(p)
                assert _value_at(*got, p) == want, (pair, lo, hi, p)
            cases += 1
            changed += got != own
            # idempotent, and a no-op on an empty range
            assert merge_max(got, imp, lo, hi) == got
            if lo is not None:
                assert merge_max(own, imp, lo, lo) == own
    assert cases == 240 and changed > cases // 2, (cases, changed)


def test_max_of_two_write_streams_is_their_union(oracle_built):
    """Write-only batches (every transaction commits) alternate between A and B by version and all go
    to U: max(B, A) is U's history, over the whole key space and over a range."""
    rng = np.random.default_rng(5)
    vacuous = 0  # seeds where B alone already is U: the merge would show nothing
    for seed in range(10):
        a, b, u = (oracle_built.OracleConflictSet() for _ in range(3))
        header = 3 if seed % 2 else 0
        if header:
            for o in (a, b, u):
                o.clear(header)
        now = 20
        for i in range(24):
            pb = W.random_small_batch(rng, int(rng.integers(1, 4)), max_reads=0, max_writes=1, alphabet=8, max_len=3,
                                      now=now, staleness=5)
            for o in ((a, b)[i & 1], u):
                v, _ = o.detect(pb, now, 0, gc=False)
                assert (v == 2).all()
            now += int(rng.integers(1, 4))
        oldest = 30  # the first few batches' versions clamp to 29
        for o in (a, b, u):
            o.set_oldest_version(oldest)
        ca, cb, cu = (canon(*o.dump_history(), header, oldest) for o in (a, b, u))
        assert merge_max(cb, ca) == cu, seed
        assert merge_max(ca, cb) == cu, seed
        vacuous += cb == cu or ca == cu or not cu[1]
        keys = sorted(set(cu[1]) | {k + b"\x00" for k in cu[1]})
        for _ in range(8):
            lo, hi = sorted((keys[int(rng.integers(len(keys)))], keys[int(rng.integers(len(keys)))]))
            got = merge_max(cb, canon(*a.dump_history(), header, oldest, lo, hi), lo, hi)
            for p in [b""] + keys:
                want = cu if lo <= p < hi else cb
                assert _value_at(*got, p) == _value_at(*want, p), (seed, lo, hi, p)
    assert vacuous < 5  # as for merge_max above: more than half of the cases show something


def test_pack_and_shifted():
    state = (3, [b"", b"a", b"a\x00", b"b" * 40], [5, 2, 9, 1])
    kb, ko, vv, hdr = pack(state)
    raw = kb.tobytes()
    assert [raw[ko[i]:ko[i + 1]] for i in range(len(vv))] == state[1]
    assert vv.tolist() == state[2] and hdr == 3 and ko[0] == 0 and ko[-1] == len(kb)
    assert pack((7, [], []))[1].tolist() == [0]
    for shift in range(1, 9):
        st = shifted(state, shift, 77)
        assert st[1] == sorted(st[1]) and len(st[1]) == 5 and st[1][1] == b"\x00" * shift and st[2][1] == 77
        assert pack(st)[1][2] == shift


def test_import_symbols_bound_and_reject_null():
    from foundationdb_amd import build, conflict_set

    build.build()
    L = conflict_set.load_library()
    for name in ("fdbcs_history_import", "fdbcs_history_import_pending"):
        assert name in conflict_set.SIGNATURES
        assert getattr(L, name).argtypes == conflict_set.SIGNATURES[name][1]
    VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert conflict_set.SIGNATURES["fdbcs_history_import"][1] == [VP, VP, I32, VP, I32, I64, VP, VP, VP, I64,
                                                                  ctypes.POINTER(I64)]
    assert conflict_set.SIGNATURES["fdbcs_history_import_pending"][1] == [VP, VP, VP, I32, VP, I32, ctypes.POINTER(I64)]
    out = ctypes.c_int64()
    off = np.zeros(1, np.int64)
    rc = L.fdbcs_history_import(None, None, -1, None, -1, 0, None, ctypes.c_void_p(off.ctypes.data), None, 0,
                                ctypes.byref(out))
    assert rc == conflict_set.FDBCS_E_INVALID
    assert L.fdbcs_history_import_pending(None, None, None, -1, None, -1, ctypes.byref(out)) == conflict_set.FDBCS_E_INVALID
    assert hasattr(conflict_set.ConflictSet, "merge_history") and hasattr(conflict_set.ConflictSet, "merge_pending_export")
