"""GPU tests of the device-side history digest (ConflictSet.digest).  In every state
    cs.digest(lo, hi, floor) == digest_arrays(*cs.dump_history(lo, hi, floor))
and, where the semantic oracle runs beside the set, the same digest equals the plain-Python model
(tests/digest_model.py) over the oracle's canonical form.  The states are built the way
tests/test_gpu_export.py builds its own."""
import ctypes

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests import digest_model as M
from tests.export_helpers import NO_FLOOR, Pair, canon
from tests.helpers import EngineDriver
from tests.test_digest_cpu import LADDER_KEYS, LADDER_VERS, arrays
from tests.test_gpu_export import P14, c2_pair, c2_sequence, prefix_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


def check(C, cs, lo=None, hi=None, floor=None, want=None, what=None):
    """The digest taken first (so it never leans on an export's leftovers), then the export of the
    same arguments through the host entry, then the model over `want` = (header, keys, versions)."""
    d = cs.digest(lo, hi, floor)
    assert isinstance(d, C.HistoryDigest)
    assert d == C.digest_arrays(*cs.dump_history(lo, hi, floor)), (what, lo, hi, floor)
    if want is not None:
        assert tuple(d) == M.digest(*want), (what, lo, hi, floor)
    return d


def check_pair(p, lo=None, hi=None, floor=None, what=None):
    return check(p.e.C, p.cs, lo, hi, floor, p.reference(lo, hi, floor), what)


def write_batch(ranges, now):
    """One transaction that writes `ranges` and reads nothing: it always commits."""
    return PackedBatch.from_transactions([CommitTransaction([], [KeyRange(a, b) for a, b in ranges], now, False)])


# ---- empty states

def test_empty_states_on_a_set_never_exported(engine):
    C = engine
    cs = C.ConflictSet()
    assert tuple(cs.digest()) == (0, 0, 0, (0, 0))  # before any export allocated anything
    assert tuple(cs.digest(b"a", b"b", NO_FLOOR)) == (0, 0, 0, (0, 0))
    cs.clear(42)
    assert tuple(cs.digest()) == (0, 0, 42, (0, 0))
    assert tuple(cs.digest(floor=100)) == (0, 0, 99, (0, 0))  # the header is clamped as the export's
    assert tuple(cs.digest(b"k" * 20, None, NO_FLOOR)) == (0, 0, 42, (0, 0))
    ms_kernels, ms_host = cs.digest_timing()
    assert ms_kernels > 0 and ms_host >= ms_kernels
    check(C, cs, want=(42, [], []))
    cs.close()
    # a loaded set, still never exported: the model directly
    cs = C.ConflictSet()
    order = sorted(range(len(LADDER_KEYS)), key=lambda i: LADDER_KEYS[i])
    keys, vers = [LADDER_KEYS[i] for i in order], [LADDER_VERS[i] for i in order]
    cs.load_history(*arrays(keys, vers), 5)
    assert tuple(cs.digest(floor=NO_FLOOR)) == M.digest(5, keys, vers)
    cs.close()


# ---- both tiers with holes, several tiles

@pytest.mark.parametrize("gc_interval", [0, 3])
def test_two_tiers_with_holes_multi_tile(engine, oracle_mod, gc_interval):
    p, seq = c2_pair(engine, oracle_mod, gc_interval)
    assert tuple(p.cs.digest()) == M.digest(*p.reference())  # loaded, never exported
    hidden = 0
    for i, (pb, now, no) in enumerate(seq):
        p.detect(pb, now, no)
        size = p.cs.history_size()
        assert size >= 2600  # three tiles of the merged stream
        d = check_pair(p, what=i)
        assert d.n > 2 * 1024  # kept boundaries in every tile: tile edges depend on the predecessor
        assert p.cs.history_size() == size
        assert p.cs.digest() == d
        hidden += size - p.cs.digest(floor=NO_FLOOR).n
    # equal keys in both tiers and base boundaries under delta segments: elements that are not kept
    assert hidden > 0


# ---- a floor that makes long runs equal across tile edges

def test_clamp_coalescing_across_tiles(engine):
    C = engine
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 256, size=(5000, 16), dtype=np.uint8), axis=0)
    n = len(keys)
    assert n > 4 * 1024
    vers = rng.integers(0, 100, size=n, dtype=np.int64)
    ko = np.arange(n + 1, dtype=np.int64) * 16
    cs = C.ConflictSet()
    cs.load_history(keys.reshape(-1), ko, vers, 3)
    klist = [keys[i].tobytes() for i in range(n)]
    assert tuple(cs.digest(floor=10 ** 6)) == (0, 0, 10 ** 6 - 1, (0, 0))
    ns = []
    for floor in (99, 50, NO_FLOOR):  # 99: only 1 version in 100 survives, runs longer than a tile's share
        ns.append(check(C, cs, floor=floor, want=canon(klist, vers, 3, floor), what=floor).n)
    assert 0 < ns[0] < 200 and ns[0] < ns[1] < ns[2]
    cs.close()


# ---- prefix ties, zero padding, the empty key, long keys

@pytest.mark.parametrize("gc_interval", [0, 1])
def test_prefix_ties_and_zero_padding(engine, oracle_mod, gc_interval):
    total = 0
    for seed in range(6):
        p = Pair(engine, oracle_mod, gc_interval=gc_interval)
        for i, (pb, now, no) in enumerate(prefix_sequence(seed)):
            p.detect(pb, now, no)
            d = check_pair(p, what=(seed, i))
        total += d.n
    assert total >= 60  # the final states are not degenerate


@pytest.mark.parametrize("gc_interval", [0, 1])
def test_long_keys_and_the_empty_key(engine, oracle_mod, gc_interval):
    """Keys of 17, 23, 24, 25 and 100 bytes in both tiers, k beside k + b'\\0', keys that differ only
    past byte 16 and past byte 24, and the empty key as a boundary."""
    order = sorted(range(len(LADDER_KEYS)), key=lambda i: LADDER_KEYS[i])
    keys = [LADDER_KEYS[i] for i in order if LADDER_KEYS[i]]
    vers = [30 + i for i in range(len(keys))]
    p = Pair(engine, oracle_mod, gc_interval=gc_interval)
    p.load_history(*arrays(keys, vers), 9)
    check_pair(p, floor=NO_FLOOR, what="loaded")
    by = {len(k): k for k in keys}
    now = 100
    # the same long keys again (equal keys in both tiers with gc_interval 0), their k + b'\0' ends,
    # new keys that part from them only in the tail, and the empty key
    for ranges in ([(by[L], by[L] + b"\x00") for L in (17, 24, 100)] + [(b"", b"\x00")],
                   [(by[23], by[23] + b"\x00"), (by[25][:24] + b"\x00", by[25]), (by[100][:99], by[100][:99] + b"\x01")],
                   [(by[100] + b"\x00" * 7, by[100] + b"\x00" * 8), (by[16], by[17][:16] + b"\x00")]):
        p.detect(write_batch(ranges, now), now, 0)
        d = check_pair(p, what=now)
        check_pair(p, floor=NO_FLOOR, what=now)
        now += 10
    hdr, ks, _ = p.reference()
    assert ks[0] == b"" and {17, 23, 24, 25, 100, 107, 108} <= {len(k) for k in ks} and d.n == len(ks)
    # clips whose bounds are long keys themselves
    for lo, hi in ((by[17], by[100]), (by[100], by[100] + b"\x00" * 8), (by[25][:24], None), (None, by[23] + b"\x00")):
        check_pair(p, lo, hi, what=("clip", lo, hi))


# ---- range clips

def _clip_cases(p, long_probe):
    _, ks, _ = p.reference()
    assert len(ks) >= 6
    present = set(ks)
    mid = len(ks) // 2
    between = next(ks[i] + b"\x00" for i in range(mid, len(ks)) if ks[i] + b"\x00" not in present)
    above = ks[-1] + b"\xff"
    cases = [
        (ks[mid], ks[-2]),            # lo equal to a boundary; hi equal to a boundary (excluded)
        (between, above),             # lo strictly between two boundaries; hi above the last
        (b"", ks[mid]),               # lo below the first boundary
        (ks[2], ks[2]),               # lo == hi at a boundary
        (between, between),           # lo == hi between boundaries
        (above, above + b"\x01"),     # lo above every key
        (above, None),
        (long_probe[0], long_probe[1]),
        (ks[mid], None), (between, None), (None, ks[mid]), (None, between), (None, above),
        (b"", None), (None, b""),
    ]
    for lo, hi in cases:
        d = check_pair(p, lo, hi, what=("clip", lo, hi))
        if lo is not None and (lo == hi or lo == above):
            assert d.n == 0 and d.key_bytes == 0 and d.sum == (0, 0)
            assert d.header_version == p.reference(lo, None)[0]  # H_f(lo)
    with pytest.raises(p.e.C.FdbcsError) as ei:
        p.cs.digest(ks[mid], ks[2])
    assert ei.value.status == p.e.C.FDBCS_E_INVALID
    check_pair(p, what="after the refused digest")


def test_range_clip_two_tiers(engine, oracle_mod):
    p, seq = c2_pair(engine, oracle_mod, 3)
    for pb, now, no in seq:
        p.detect(pb, now, no)
    _, ks, _ = p.reference()
    _clip_cases(p, (ks[10] + b"\x00\x05\x06", ks[len(ks) - 10] + b"\x01\x00\x00\xff"))


@pytest.mark.parametrize("gc_interval", [0, 1])
def test_range_clip_prefix_ties(engine, oracle_mod, gc_interval):
    p = Pair(engine, oracle_mod, gc_interval=gc_interval)
    for pb, now, no in prefix_sequence(3):
        p.detect(pb, now, no)
    # bounds longer than 16 bytes inside the shared prefix, the second between lengths of one run
    _clip_cases(p, (P14 + b"\x00\x00\x01", P14 + b"\xff\x01\x00\x00\x00"))
    check_pair(p, P14 + b"\x01\x00\x00", P14 + b"\x01\x00\x00\x00", what="bounds differing by a trailing zero")


# ---- invariance

def test_invariance_and_one_more_write(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    sets = []
    for gc in (1, 0):
        d = EngineDriver(C, gc_interval=gc)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        for pb, now, no in seq[:5]:
            d.detect(pb, now, no)
        sets.append(d)
    a, b = sets
    assert a.cs.history_size() != b.cs.history_size()  # the tiers differ, the canonical history does not
    want = a.cs.digest()
    assert want.n > 2 * 1024 and b.cs.digest() == want
    # a restored checkpoint
    r = C.ConflictSet()
    r.load_history(*a.cs.dump_history())
    r.set_oldest_version(a.cs.oldest_version)
    assert r.digest() == want
    # the receiver of a device-to-device hand-over of everything
    m = C.ConflictSet()
    m.clear(0)
    m.set_oldest_version(a.cs.oldest_version)
    a.cs.export_history()
    m.merge_pending_export(a.cs)
    assert m.digest() == want
    # one more committed write inside [lo, hi): that range's digest moves, a disjoint one's does not
    dump = a.cs.dump_history()
    raw, off = dump[0].tobytes(), dump[1]
    key = lambda i: raw[off[i]:off[i + 1]]
    n = len(dump[2])
    lo, mid, hi = key(n // 4), key(n // 2), key(3 * n // 4)
    inside, outside = a.cs.digest(lo, mid), a.cs.digest(mid, hi)
    assert inside.n > 100 and outside.n > 100 and b.cs.digest(lo, mid) == inside
    now = seq[4][1] + 500
    w = key(n // 3)
    a.detect(write_batch([(w, w + b"\x00")], now), now, seq[4][2])
    assert a.cs.digest(lo, mid) != inside
    assert a.cs.digest(mid, hi) == outside
    assert b.cs.digest(lo, mid) == inside and a.cs.digest() != b.cs.digest()
    b.detect(write_batch([(w, w + b"\x00")], now), now, seq[4][2])
    assert a.cs.digest() == b.cs.digest()
    for d in sets:
        d.cs.close()
    r.close()
    m.close()


# ---- read-only

def test_read_only_and_pending_export_survives(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    twins = []
    for _ in range(2):
        d = EngineDriver(C, gc_interval=3)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        for pb, now, no in seq[:3]:
            d.detect(pb, now, no)
        twins.append(d)
    a, twin = twins  # twin is never digested
    size = a.cs.history_size()
    dump = a.cs.dump_history()
    raw, off = dump[0].tobytes(), dump[1]
    n = len(dump[2])
    k1, k2, k3 = (raw[off[i]:off[i + 1]] for i in (n // 4, n // 2, 3 * n // 4))
    want_a = twin.cs.dump_history(k1, k2)
    # export range A, digest range B (and the whole set), then read: A's result
    na, nba, hdra = a.cs.export_history(k1, k2)
    db = a.cs.digest(k2, k3)
    dall = a.cs.digest()
    got = a.cs.read_export(na, nba)
    assert hdra == want_a[3] and all((x == y).all() for x, y in zip(got, want_a[:3]))
    assert db == C.digest_arrays(*twin.cs.dump_history(k2, k3)) and dall == C.digest_arrays(*dump)
    assert a.cs.history_size() == size == twin.cs.history_size()
    for pb, now, no in seq[3:6]:
        a.cs.digest()
        va, ca = a.detect(pb, now, no)
        vt, ct = twin.detect(pb, now, no)
        assert (va == vt).all() and ca == ct
        assert a.cs.history_size() == twin.cs.history_size()
    assert a.cs.digest() == C.digest_arrays(*twin.cs.dump_history())
    for d in twins:
        d.cs.close()


# ---- errors

def test_errors(engine, oracle_mod):
    C = engine
    L = C.load_library()
    cs = C.ConflictSet()
    cs.clear(42)
    rng = np.random.default_rng(8)
    pb = W.random_small_batch(rng, 50, alphabet=3, max_len=3, now=60, staleness=10)
    b = C.ConflictBatch(cs, None)
    b.add_packed(pb)
    b.detect_async(60, 50)
    with pytest.raises(C.FdbcsError) as ei:
        cs.digest()
    assert ei.value.status == C.FDBCS_E_STATE
    v = b.wait()
    b.close()
    o = oracle_mod.OracleConflictSet()
    o.clear(42)
    vo, _ = o.detect(pb, 60, 50)
    assert (v == vo).all()  # the batch is unharmed
    keys, vers = o.dump_history()
    want = canon(keys, vers, 42, o.oldest_version)
    assert check(C, cs, want=want).n == len(want[1]) > 0
    with pytest.raises(C.FdbcsError) as ei:
        cs.digest(b"b", b"a")
    assert ei.value.status == C.FDBCS_E_INVALID
    assert L.fdbcs_history_digest(cs.handle, None, -1, None, -1, C.NO_FLOOR, None) == C.FDBCS_E_INVALID
    d = C._CDigest()
    assert L.fdbcs_history_digest(cs.handle, None, 1, None, -1, C.NO_FLOOR, ctypes.byref(d)) == C.FDBCS_E_INVALID
    assert check(C, cs, want=want).n == len(want[1])
    cs.close()
