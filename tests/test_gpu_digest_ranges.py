"""GPU tests of the partitioned history digest (ConflictSet.digest_ranges), of split_keys and of
diverging_ranges.  The reference of digest_ranges is the single-range call this change leaves alone:
in every state and for every range i
    cs.digest_ranges(bounds, ...)[i] == cs.digest(s_i, s_{i+1}, floor)
                                     == digest_arrays(*cs.dump_history(s_i, s_{i+1}, floor))
and where the semantic oracle runs beside the set, the plain-Python model of the partition
(tests/digest_ranges_model.py) over the oracle's canonical form.  The scan tile is 1024 stream
elements, so the sets are small: 3,000 boundaries in the base alone (three tiles, their edges at known
keys) and the 8,000 and more of the two-tier sequence tests/test_gpu_export.py shares (eight tiles,
holes in the delta).  The states are built the way tests/test_gpu_digest.py builds its own."""
import ctypes
import gc

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from tests import digest_ranges_model as R
from tests.export_helpers import NO_FLOOR, Pair, canon, split_dump
from tests.helpers import EngineDriver
from tests.test_digest_cpu import LADDER_KEYS, LADDER_VERS, arrays
from tests.test_gpu_digest import write_batch
from tests.test_gpu_export import P14, c2_pair, c2_sequence, prefix_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


def check(C, cs, bounds, open_lo=False, open_hi=False, floor=None, want=None, what=None, dumps=True):
    """digest_ranges taken first (it never leans on another call's leftovers), then per range the
    single digest and the digest of the export of the same arguments, the count identity against the
    whole span's digest, and the model over `want` = (header, keys, versions) of the whole history."""
    got = cs.digest_ranges(bounds, floor, open_lo, open_hi)
    rs = R.ranges(bounds, open_lo, open_hi)
    assert len(got) == len(rs)
    for i, (d, (lo, hi)) in enumerate(zip(got, rs)):
        assert isinstance(d, C.HistoryDigest)
        assert d == cs.digest(lo, hi, floor), (what, i, lo, hi, floor)
        if dumps:
            assert d == C.digest_arrays(*cs.dump_history(lo, hi, floor)), (what, i, lo, hi, floor)
    span = split_dump(cs.dump_history(rs[0][0], rs[-1][1], floor))
    assert len(span[1]) == sum(d.n for d in got) + R.bound_hits(span[1], bounds, open_lo, open_hi), what
    assert got == C.digest_arrays_ranges(*arrays(span[1], span[2]), span[0], bounds, open_lo, open_hi), what
    if want is not None:
        assert [tuple(d) for d in got] == R.digest_ranges(*want, bounds, open_lo, open_hi), what
    return got


def stream_keys(cs):
    """The canonical keys without a floor: boundary keys of the set, a subset of the merged stream."""
    return split_dump(cs.dump_history(floor=NO_FLOOR))[1]


# ---- empty states, a set never exported or digested

def test_empty_states_on_a_set_never_exported(engine):
    C = engine
    cs = C.ConflictSet()
    assert [tuple(d) for d in cs.digest_ranges([], open_lo=True, open_hi=True)] == [(0, 0, 0, (0, 0))]
    ms_kernels, ms_host = cs.digest_timing()  # the last call of either kind
    assert ms_kernels > 0 and ms_host >= ms_kernels
    assert [tuple(d) for d in cs.digest_ranges([b"a", b"b" * 20], NO_FLOOR, True, True)] == [(0, 0, 0, (0, 0))] * 3
    cs.clear(42)
    assert [tuple(d) for d in cs.digest_ranges([b"a", b"b"], 100)] == [(0, 0, 99, (0, 0))]  # clamped as the export's
    check(C, cs, [b"", b"k" * 20, b"z"], True, True, NO_FLOOR, want=(42, [], []))
    cs.close()
    # a loaded set, still never exported or digested: the model directly
    cs = C.ConflictSet()
    order = sorted(range(len(LADDER_KEYS)), key=lambda i: LADDER_KEYS[i])
    keys, vers = [LADDER_KEYS[i] for i in order], [LADDER_VERS[i] for i in order]
    cs.load_history(*arrays(keys, vers), 5)
    got = cs.digest_ranges(keys, NO_FLOOR, True, True)
    assert [tuple(d) for d in got] == R.digest_ranges(5, keys, vers, keys, True, True)
    assert [d.header_version for d in got] == [5] + vers and not any(d.n for d in got)
    check(C, cs, [k + b"\x00" for k in keys], True, True, NO_FLOOR, want=(5, keys, vers))
    cs.close()


# ---- base only: the stream is the loaded array, so tile edges are known keys

@pytest.fixture(scope="module")
def base_only():
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 256, size=(3000, 16), dtype=np.uint8), axis=0)
    n = len(keys)
    assert 2 * 1024 + 500 < n <= 3000
    vers = rng.integers(0, 100, size=n, dtype=np.int64)
    return keys, np.arange(n + 1, dtype=np.int64) * 16, vers, [keys[i].tobytes() for i in range(n)]


def test_base_only_partitions(engine, base_only):
    C = engine
    keys, ko, vers, kl = base_only
    n = len(kl)
    cs = C.ConflictSet()
    cs.load_history(keys.reshape(-1), ko, vers, 3)
    for floor in (NO_FLOOR, 50):
        w = canon(kl, vers.tolist(), 3, floor)
        # K = 1 in every form
        check(C, cs, [], True, True, floor, w, "whole")
        check(C, cs, [kl[700]], True, False, floor, w, "K=1 open lo")
        check(C, cs, [kl[700]], False, True, floor, w, "K=1 open hi")
        check(C, cs, [kl[700], kl[2100]], False, False, floor, w, "K=1 closed")
        # bounds on the tile edges of the stream from below every key (positions 1023 | 1024, 2047 | 2048)
        check(C, cs, [kl[1023], kl[1024], kl[2047], kl[2048]], True, True, floor, w, "tile edges")
        check(C, cs, [kl[1024], kl[2048]], True, True, floor, w, "tile starts")
        # ... and of the stream from a closed low end: element j + 1 + 1024 t opens tile t
        check(C, cs, [kl[99], kl[99 + 1024], kl[100 + 1024], kl[100 + 2048], kl[n - 1]], False, False, floor, w, "shifted")
        # bounds below every key and above every key, equal neighbours, both open ends
        lowest, above = b"", kl[-1] + b"\xff"
        assert lowest < kl[0]
        check(C, cs, [lowest, lowest, kl[5], kl[5], kl[5], kl[1500] + b"\x00", kl[1500] + b"\x00", above, above + b"\x01"],
              True, True, floor, w, "outside and equal")
        check(C, cs, [above, above + b"\x00"], True, True, floor, w, "above only")
        check(C, cs, [lowest, kl[0]], True, False, floor, w, "below only")
    # a floor that coalesces across tile edges: 1 version in 100 survives, runs longer than a tile's share
    assert 0 < cs.digest(floor=99).n < 200
    check(C, cs, [kl[i] for i in range(64, n, 128)], True, True, 99, canon(kl, vers.tolist(), 3, 99), "coalesced")
    cs.close()


def test_base_only_more_bounds_than_a_tile(engine, base_only):
    """1,300 bounds over the three tiles: every key of the middle tile's first 1,100 elements is a
    bound or has one right behind it (a tile of many one-element and empty bins, every wave
    straddling bounds), the outer tiles hold a few wide bins, and bins span both tile edges."""
    C = engine
    keys, ko, vers, kl = base_only
    cs = C.ConflictSet()
    cs.load_history(keys.reshape(-1), ko, vers, 3)
    bounds = sorted([kl[i] for i in range(1000, 2100, 2)] + [kl[i] + b"\x00" for i in range(1001, 2100, 2)]
                    + [kl[i] for i in (10, 500, 2300, 2301, 2500)] + [kl[i] for i in range(2600, 2795)])
    assert len(bounds) == 1300
    for floor in (NO_FLOOR, 50):
        got = check(C, cs, bounds, True, True, floor, canon(kl, vers.tolist(), 3, floor), "many", dumps=(floor == 50))
        assert sum(d.n > 0 for d in got) > 300
    cs.close()


# ---- both tiers with holes, several tiles

@pytest.mark.parametrize("gc_interval", [0, 3])
def test_two_tiers_with_holes_multi_tile(engine, oracle_mod, gc_interval):
    p, seq = c2_pair(engine, oracle_mod, gc_interval)
    C = engine
    rng = np.random.default_rng(77)
    for i, (pb, now, no) in enumerate(seq):
        p.detect(pb, now, no)
        size = p.cs.history_size()
        assert size >= 2600  # three tiles of the merged stream
        ks = stream_keys(p.cs)
        # a few wide ranges after every batch, at the oldest version and without a floor
        few = sorted(ks[int(j)] for j in rng.integers(0, len(ks), size=6)) + [ks[-1] + b"\x01"]
        got = check(C, p.cs, few, True, True, None, p.reference(), (i, "few"))
        assert sum(d.n for d in got) > 2 * 1024  # kept boundaries in every tile
        # (without a floor the oracle's state depends on its GC: the set's own calls are the reference)
        check(C, p.cs, few[1:4], False, False, NO_FLOOR, None, (i, "few, closed"), dumps=False)
        assert p.cs.history_size() == size
        if i in (2, 7):
            # more bounds than a tile holds elements: boundary keys, keys right behind them, and the
            # keys of the batch just merged (delta boundaries, equal keys in both tiers with gc 0)
            many = sorted(set(ks[::8]) | {k + b"\x00" for k in ks[1::16]} | set(ks[1200:1500]))
            assert len(many) > 1024
            got = check(C, p.cs, many, True, True, None, p.reference(), (i, "many"), dumps=(i == 2))
            assert sum(d.n > 0 for d in got) > 300
            check(C, p.cs, many, False, False, NO_FLOOR, None, (i, "many, no floor"), dumps=False)


def test_equal_keys_in_both_tiers_as_bounds(engine, oracle_mod):
    """A delta boundary and a base boundary at the same key, that key being a bound; and holes."""
    C = engine
    (kb, ko, vers), _ = c2_sequence()
    p = Pair(engine, oracle_mod, gc_interval=0)
    p.load_history(kb, ko, vers, 7)
    raw = kb.tobytes()
    key = lambda i: raw[ko[i]:ko[i + 1]]
    picks = [key(i) for i in (5, 1023, 1024, 1500, 2047, 2048, len(vers) - 2)]
    now = 200000
    # each write [k, k + 0) puts boundaries k and k + 0 into the delta above the base's k
    p.detect(write_batch([(k, k + b"\x00") for k in picks], now), now, 0)
    size = p.cs.history_size()
    assert size > len(vers)  # the delta tier holds the writes
    ends = [k + b"\x00" for k in picks]
    for bounds in (picks, ends, sorted(picks + ends), [picks[3]] * 3, [picks[1], picks[1], picks[2]]):
        for floor in (NO_FLOOR, None):
            check(C, p.cs, bounds, True, True, floor, p.reference(floor=floor), ("tie", len(bounds), floor))
    # a write that ends at a boundary key leaves a hole there
    now += 1000
    p.detect(write_batch([(key(700), key(1100)), (key(2040), key(2060))], now), now, 0)
    check(C, p.cs, [key(i) for i in (650, 700, 900, 1100, 1101, 2040, 2050, 2060)], True, True, NO_FLOOR,
          p.reference(floor=NO_FLOOR), "holes")
    assert p.cs.history_size() > len(vers)  # still two tiers: nothing was compacted


# ---- long keys (the long-key search) and prefix ties

@pytest.mark.parametrize("gc_interval", [0, 1])
def test_long_keys_and_long_bounds(engine, oracle_mod, gc_interval):
    """Keys of 17 - 108 bytes in both tiers, k beside k + b'\\0', keys that differ only past byte 16
    and past byte 24, the empty key; every one of them, and keys parting from them in the tail, a bound."""
    C = engine
    order = sorted(range(len(LADDER_KEYS)), key=lambda i: LADDER_KEYS[i])
    keys = [LADDER_KEYS[i] for i in order if LADDER_KEYS[i]]
    vers = [30 + i for i in range(len(keys))]
    p = Pair(engine, oracle_mod, gc_interval=gc_interval)
    p.load_history(*arrays(keys, vers), 9)
    by = {len(k): k for k in keys}
    now = 100
    for ranges in ([(by[L], by[L] + b"\x00") for L in (17, 24, 100)] + [(b"", b"\x00")],
                   [(by[23], by[23] + b"\x00"), (by[25][:24] + b"\x00", by[25]), (by[100][:99], by[100][:99] + b"\x01")],
                   [(by[100] + b"\x00" * 7, by[100] + b"\x00" * 8), (by[16], by[17][:16] + b"\x00")]):
        p.detect(write_batch(ranges, now), now, 0)
        ks = stream_keys(p.cs)
        probes = sorted(set(ks) | {k + b"\x00" for k in ks} | {k[:-1] for k in ks if len(k) > 16}
                        | {by[100][:40] + b"\xff" * 30, by[25][:24]})
        for floor in (None, NO_FLOOR):
            check(C, p.cs, probes, True, True, floor, p.reference(floor=floor), (now, "all"))
            check(C, p.cs, ks, False, False, floor, p.reference(floor=floor), (now, "keys"), dumps=False)
        now += 10
    assert {17, 23, 24, 25, 100, 107, 108} <= {len(k) for k in ks} and ks[0] == b""
    assert max(len(b) for b in probes) == 109


@pytest.mark.parametrize("gc_interval", [0, 1])
def test_prefix_ties(engine, oracle_mod, gc_interval):
    C = engine
    total = 0
    for seed in range(3):
        p = Pair(engine, oracle_mod, gc_interval=gc_interval)
        for i, (pb, now, no) in enumerate(prefix_sequence(seed)):
            p.detect(pb, now, no)
            if i % 3 != 0:
                continue
            ks = stream_keys(p.cs)
            # every boundary and the key a trailing zero away, bounds longer than 16 bytes inside the
            # shared prefix, bounds that differ by a trailing zero
            probes = sorted(set(ks) | {k + b"\x00" for k in ks}
                            | {P14 + b"\x00\x00\x01", P14 + b"\x01\x00\x00", P14 + b"\x01\x00\x00\x00", P14 + b"\xff\x01\x00\x00\x00"})
            got = check(C, p.cs, probes, True, True, None, p.reference(), (seed, i))
            check(C, p.cs, probes[1:], False, False, NO_FLOOR, None, (seed, i), dumps=False)
            got = check(C, p.cs, probes[2::5], True, True, None, p.reference(), (seed, i, "wide"))
        total += sum(d.n for d in got)
    assert total >= 30  # the final states are not degenerate


# ---- the greatest partition

def test_65536_ranges_on_a_small_set(engine):
    """65,536 ranges over 600 boundaries: every entry against the host form over one export (the
    single digest 65,536 times would take a quarter of a minute), and against the single digest for
    every range that holds a boundary and every 64th of the others.  65,537 ranges are refused."""
    C = engine
    rng = np.random.default_rng(12)
    vals = np.unique(rng.integers(0, 65535 * 65535, size=600))
    kl = [int(v).to_bytes(4, "big") for v in vals]
    vers = [int(v) for v in rng.integers(1, 1 << 40, size=len(kl))]
    d = EngineDriver(C, gc_interval=0)
    d.load_history(*arrays(kl, vers), 2)
    w = kl[100]
    d.detect(write_batch([(w, w + b"\x00"), (kl[300], kl[310])], 1 << 41), 1 << 41, 0)  # a delta tier too
    cs = d.cs
    bounds = [(i * 65535).to_bytes(4, "big") for i in range(65537)]
    got = cs.digest_ranges(bounds, NO_FLOOR)
    assert len(got) == 65536
    span = split_dump(cs.dump_history(bounds[0], bounds[-1], NO_FLOOR))
    assert got == C.digest_arrays_ranges(*arrays(span[1], span[2]), span[0], bounds)
    assert sum(x.n for x in got) + R.bound_hits(span[1], bounds) == len(span[1]) > 500
    for i, x in enumerate(got):
        if x.n or i % 64 == 0:
            assert x == cs.digest(bounds[i], bounds[i + 1], NO_FLOOR), i
    for open_lo, open_hi in ((True, False), (False, True)):
        with pytest.raises(C.FdbcsError) as ei:
            cs.digest_ranges(bounds, NO_FLOOR, open_lo, open_hi)
        assert ei.value.status == C.FDBCS_E_NOMEM
    assert cs.digest_ranges(bounds[:9], NO_FLOOR) == got[:8]
    cs.close()


# ---- read-only, a pending export, the statuses, the resources

def _twins(C, batches):
    (kb, ko, vers), seq = c2_sequence()
    twins = []
    for _ in range(2):
        d = EngineDriver(C, gc_interval=3)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        for pb, now, no in seq[:batches]:
            d.detect(pb, now, no)
        twins.append(d)
    return twins, seq


def test_read_only_and_pending_export_survives(engine, oracle_mod):
    C = engine
    (a, twin), seq = _twins(C, 3)  # twin is never digested or split
    size = a.cs.history_size()
    ks = stream_keys(twin.cs)
    n = len(ks)
    k1, k2, k3 = ks[n // 4], ks[n // 2], ks[3 * n // 4]
    want_a = twin.cs.dump_history(k1, k2)
    # export range A, digest ranges and take split keys elsewhere, then read: A's result
    na, nba, hdra = a.cs.export_history(k1, k2)
    got = a.cs.digest_ranges(ks[::40], None, True, True)
    keys = a.cs.split_keys(k2, k3, 50)
    assert len(keys) == 50
    read = a.cs.read_export(na, nba)
    assert hdra == want_a[3] and all((x == y).all() for x, y in zip(read, want_a[:3]))
    dump = twin.cs.dump_history()
    assert got == C.digest_arrays_ranges(*dump, ks[::40], True, True)
    assert a.cs.history_size() == size == twin.cs.history_size()
    for pb, now, no in seq[3:6]:
        a.cs.digest_ranges(ks[::100], None, True, True)
        a.cs.split_keys(None, None, 100)
        va, ca = a.detect(pb, now, no)
        vt, ct = twin.detect(pb, now, no)
        assert (va == vt).all() and ca == ct
        assert a.cs.history_size() == twin.cs.history_size()
    assert a.cs.digest_ranges([k2], None, True, True) == C.digest_arrays_ranges(*twin.cs.dump_history(), [k2], True, True)
    for d in (a, twin):
        d.cs.close()


def test_statuses(engine):
    C = engine
    L = C.load_library()
    cs = C.ConflictSet()
    cs.clear(42)
    rng = np.random.default_rng(8)
    pb = W.random_small_batch(rng, 50, alphabet=3, max_len=3, now=60, staleness=10)
    b = C.ConflictBatch(cs, None)
    b.add_packed(pb)
    b.detect_async(60, 50)
    for call in (lambda: cs.digest_ranges([b"a"], None, True, True), lambda: cs.split_keys(None, None, 4)):
        with pytest.raises(C.FdbcsError) as ei:
            call()
        assert ei.value.status == C.FDBCS_E_STATE
    b.wait()
    b.close()
    whole = cs.digest()
    assert cs.digest_ranges([], None, True, True) == [whole] and whole.n > 0
    for bounds, open_lo, open_hi in (([b"b", b"a"], True, True), ([b"a"], False, False), ([], True, False), ([], False, False),
                                     ([b"a", b"b", b"a\x00"], False, False)):
        with pytest.raises(C.FdbcsError) as ei:
            cs.digest_ranges(bounds, None, open_lo, open_hi)
        assert ei.value.status == C.FDBCS_E_INVALID, bounds
    out = (C._CDigest * 4)()
    bb, bo, _ = arrays([b"a", b"b"], [0, 0])
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    call = lambda n, by, off, res: L.fdbcs_history_digest_ranges(cs.handle, n, by, off, 0, 0, C.NO_FLOOR, res)
    assert call(2, vp(bb), vp(bo), ctypes.addressof(out)) == C.FDBCS_OK
    assert call(2, vp(bb), vp(bo), None) == C.FDBCS_E_INVALID
    assert call(-1, vp(bb), vp(bo), ctypes.addressof(out)) == C.FDBCS_E_INVALID
    assert call(2, vp(bb), None, ctypes.addressof(out)) == C.FDBCS_E_INVALID
    assert call(2, None, vp(bo), ctypes.addressof(out)) == C.FDBCS_E_INVALID
    bad = np.array([1, 1, 2], np.int64)
    assert call(2, vp(bb), vp(bad), ctypes.addressof(out)) == C.FDBCS_E_INVALID
    bad = np.array([0, 2, 1], np.int64)
    assert call(2, vp(bb), vp(bad), ctypes.addressof(out)) == C.FDBCS_E_INVALID
    # split_keys: the export's statuses
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    with pytest.raises(C.FdbcsError) as ei:
        cs.split_keys(b"b", b"a", 4)
    assert ei.value.status == C.FDBCS_E_INVALID
    with pytest.raises(C.FdbcsError) as ei:
        cs.split_keys(None, None, -1)
    assert ei.value.status == C.FDBCS_E_INVALID
    with pytest.raises(C.FdbcsError) as ei:
        cs.split_keys(None, None, 65537)
    assert ei.value.status == C.FDBCS_E_NOMEM
    ko = np.zeros(8, np.int64)
    assert L.fdbcs_history_split_keys_read(cs.handle, None, 0, vp(ko), 8) == C.FDBCS_E_STATE  # nothing pending
    assert L.fdbcs_history_split_keys(cs.handle, None, -1, None, -1, 4, ctypes.byref(n), ctypes.byref(nb)) == C.FDBCS_OK
    assert 0 < n.value <= 4 and nb.value > 0
    kb = np.zeros(nb.value, np.uint8)
    assert L.fdbcs_history_split_keys_read(cs.handle, vp(kb), nb.value - 1, vp(ko), 8) == C.FDBCS_E_NOMEM
    assert L.fdbcs_history_split_keys_read(cs.handle, vp(kb), nb.value, vp(ko), n.value - 1) == C.FDBCS_E_NOMEM
    assert L.fdbcs_history_split_keys_read(cs.handle, vp(kb), nb.value, vp(ko), 8) == C.FDBCS_OK  # the result stayed
    assert ko[n.value] == nb.value
    assert L.fdbcs_history_split_keys_read(cs.handle, vp(kb), nb.value, vp(ko), 8) == C.FDBCS_E_STATE  # released
    assert cs.digest() == whole
    cs.close()


def test_resources_come_back(engine):
    C = engine
    gc.collect()
    base = C.live_resources()
    (kb, ko, vers), seq = c2_sequence()
    d = EngineDriver(C, gc_interval=0)
    d.load_history(kb, ko, vers, 7)
    d.detect(*seq[0])
    before = C.live_resources()
    ks = d.cs.split_keys(None, None, 2000)
    d.cs.digest_ranges(ks, None, True, True)
    grown = C.live_resources()
    assert grown[0] > before[0] and grown[3] == before[3]
    d.cs.digest_ranges(ks[::2], None, True, True)
    d.cs.split_keys(ks[3], None, 100)
    assert C.live_resources() == grown  # grow-only: smaller calls allocate nothing
    d.cs.close()
    del d
    gc.collect()
    assert C.live_resources() == base


# ---- split_keys

def _check_split(cs, lo, hi, want, boundary_keys=None):
    """boundary_keys: the keys of the tier the picks must come from, where the test knows them."""
    keys = cs.split_keys(lo, hi, want)
    assert len(keys) <= want
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert all((lo is None or k > lo) and (hi is None or k < hi) for k in keys)
    assert boundary_keys is None or set(keys) <= boundary_keys
    return keys


def test_split_keys(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    d = EngineDriver(C, gc_interval=0)
    d.load_history(kb, ko, vers, 7)
    raw = kb.tobytes()
    base_keys = [raw[ko[i]:ko[i + 1]] for i in range(len(vers))]
    assert _check_split(d.cs, None, None, 0, set()) == []
    assert _check_split(d.cs, None, None, 65536, set(base_keys)) == base_keys  # every boundary of the only tier
    got = _check_split(d.cs, None, None, 255, set(base_keys))
    assert len(got) == 255
    ranks = [base_keys.index(k) for k in got]
    gaps = np.diff([-1] + ranks + [len(base_keys)])
    assert gaps.max() - gaps.min() <= len(base_keys) // 255 + 2  # evenly spaced
    ms_kernels, ms_host = d.cs.split_keys_timing()
    assert ms_kernels > 0 and ms_host >= ms_kernels
    for pb, now, no in seq[:3]:
        d.detect(pb, now, no)
    # both tiers hold boundaries now; over a wide range the base holds more, and every pick is one of its keys
    known = set(base_keys)
    k1, k2 = base_keys[1000], base_keys[1400]
    got = _check_split(d.cs, k1, k2, 1000, known)
    assert len(got) == 399  # fewer than asked for: what the fuller tier holds there
    assert _check_split(d.cs, k1, k2, 7, known) == [base_keys[1001 + ((2 * k + 1) * 399) // 14] for k in range(7)]
    assert _check_split(d.cs, k1, k1, 5) == []                    # an empty range
    assert _check_split(d.cs, k1, k1 + b"\x00", 5) == []
    assert _check_split(d.cs, base_keys[-1] + b"\xff", None, 5) == []
    assert len(_check_split(d.cs, None, base_keys[3], 5)) >= 3    # keys 0 .. 2 at the least
    assert len(_check_split(d.cs, base_keys[-4], None, 5)) >= 3
    # a pending export survives
    want = d.cs.dump_history(k1, k2)
    na, nba, _ = d.cs.export_history(k1, k2)
    assert len(_check_split(d.cs, None, None, 100, known)) == 100
    read = d.cs.read_export(na, nba)
    assert all((x == y).all() for x, y in zip(read, want[:3]))
    d.cs.close()


@pytest.mark.parametrize("gc_interval", [0, 1])
def test_split_keys_long_keys_byte_exact(engine, oracle_mod, gc_interval):
    order = sorted(range(len(LADDER_KEYS)), key=lambda i: LADDER_KEYS[i])
    keys = [LADDER_KEYS[i] for i in order]
    vers = [30 + i for i in range(len(keys))]
    d = EngineDriver(engine, gc_interval=gc_interval)
    d.load_history(*arrays(keys, vers), 9)
    assert d.cs.split_keys(None, None, 100) == [k for k in keys]  # the empty key, 100 bytes, every length
    by = {len(k): k for k in keys}
    now = 100
    d.detect(write_batch([(by[100] + b"\x00" * 7, by[100] + b"\x00" * 8), (by[17], by[17] + b"\x00"),
                          (by[25][:24] + b"\x00", by[25]), (b"", b"\x00")], now), now, 0)
    ks = stream_keys(d.cs)  # all versions differ: every boundary is canonical
    assert {107, 108} <= {len(k) for k in ks}
    got = d.cs.split_keys(None, None, 100)
    # the fuller tier's boundaries, byte for byte among the exported keys
    assert len(got) >= 8 and set(got) <= set(ks) and all(a < b for a, b in zip(got, got[1:]))
    lo, hi = by[100], by[100] + b"\x00" * 9
    got = d.cs.split_keys(lo, hi, 5)
    assert got == [k for k in ks if lo < k < hi] and len(got) == 2 and [len(k) for k in got] == [107, 108]
    d.cs.close()


# ---- diverging_ranges

def _differences(a, b, floor=None):
    """Boundary keys at which two sets' canonical histories, read as step functions, differ."""
    da, db = (split_dump(x.dump_history(floor=floor)) for x in (a, b))
    return R.differing_keys(da, db)


def _check_located(a, b, got, fanout, leaf, floor=None):
    inside = lambda k, r: (r[0] is None or k >= r[0]) and (r[1] is None or k < r[1])
    for r, nxt in zip(got, got[1:]):
        assert r[1] is not None and nxt[0] is not None and r[1] <= nxt[0]
    for lo, hi in got:
        x, y = a.digest(lo, hi, floor), b.digest(lo, hi, floor)
        assert x != y, (lo, hi)  # nothing that is equal
        assert (x.n <= leaf and y.n <= leaf) or not a.split_keys(lo, hi, 1)
    diff = _differences(a, b, floor)
    for k in diff:
        assert sum(inside(k, r) for r in got) == 1, k
    return diff


def test_diverging_ranges_one_extra_write(engine, oracle_mod):
    C = engine
    (a, b), seq = _twins(C, 4)
    assert a.cs.diverging_ranges(b.cs) == []
    assert a.cs.diverging_ranges(b.cs, fanout=4, leaf=2) == []
    ks = stream_keys(a.cs)
    w = ks[len(ks) // 3]
    now = seq[3][1] + 500
    a.detect(write_batch([(w, w + b"\x00")], now), now, seq[3][2])
    for fanout, leaf in ((256, 64), (4, 2), (16, 0)):
        got = a.cs.diverging_ranges(b.cs, fanout=fanout, leaf=leaf)
        diff = _check_located(a.cs, b.cs, got, fanout, leaf)
        assert w in diff and len(diff) <= 2 and 1 <= len(got) <= 2
        assert got == [r for r in got if any((r[0] is None or k >= r[0]) and (r[1] is None or k < r[1]) for k in diff)]
        # from the other side: the same keys, bisected on b's split keys
        _check_located(b.cs, a.cs, b.cs.diverging_ranges(a.cs, fanout=fanout, leaf=leaf), fanout, leaf)
    # inside a span that does not hold the write: nothing
    assert a.cs.diverging_ranges(b.cs, ks[len(ks) // 2], None) == []
    assert a.cs.diverging_ranges(b.cs, None, ks[len(ks) // 4]) == []
    assert a.cs.diverging_ranges(b.cs, ks[len(ks) // 4], ks[len(ks) // 2]) != []
    b.detect(write_batch([(w, w + b"\x00")], now), now, seq[3][2])
    assert a.cs.diverging_ranges(b.cs) == []
    for d in (a, b):
        d.cs.close()


def test_diverging_ranges_after_a_hand_over(engine, oracle_mod):
    """A receiver merges a pending export of everything, then a detect runs on the giving side only."""
    C = engine
    (a, _twin), seq = _twins(C, 3)
    _twin.cs.close()
    m = C.ConflictSet()
    m.clear(0)
    m.set_oldest_version(a.cs.oldest_version)
    a.cs.export_history()
    m.merge_pending_export(a.cs)
    assert a.cs.diverging_ranges(m) == [] and m.diverging_ranges(a.cs) == []
    pb, now, no = seq[3]
    a.detect(pb, now, no)
    m.set_oldest_version(a.cs.oldest_version)
    floor = a.cs.oldest_version
    got = a.cs.diverging_ranges(m, fanout=32, leaf=8)
    diff = _check_located(a.cs, m, got, 32, 8, floor)
    assert len(diff) > 100 and len(got) > 50  # the batch's writes, spread over the key space
    got2 = m.diverging_ranges(a.cs, floor=floor, fanout=32, leaf=8)
    _check_located(m, a.cs, got2, 32, 8, floor)
    a.cs.close()
    m.close()
