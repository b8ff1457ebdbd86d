"""GPU tests of the device-side history export (ConflictSet.dump_history): after every batch the
exported state equals the canonical form of the semantic oracle's step function at floor = oldest
version, whatever the tiers hold (empty delta, everything in the delta, holes over the base), with
range clips, a load_history round trip, and the entry points' state rules."""
import ctypes

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests.export_helpers import NO_FLOOR, Pair, canon, split_dump
from tests.helpers import EngineDriver, load_json, scenario_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


# ---- the sequences several tests share

C2P = W.C2Params(txns=600, history=8000, version_step=1000, window=5000, staleness=3000)
_c2_cache = {}


def c2_sequence():
    """(history arrays, [(batch, now, new_oldest)] x 8): a loaded base, then merges that leave holes."""
    if not _c2_cache:
        _c2_cache["hist"] = W.c2_history(C2P, 3, 100000)
        rng = np.random.default_rng(31)
        _c2_cache["seq"] = [(W.c2_batch(C2P, rng, now), now, now - 5000) for now in range(101000, 109000, 1000)]
    return _c2_cache["hist"], _c2_cache["seq"]


def c2_pair(engine, oracle_mod, gc_interval):
    (kb, ko, vers), seq = c2_sequence()
    p = Pair(engine, oracle_mod, gc_interval=gc_interval)
    p.load_history(kb, ko, vers, 7)
    p.set_oldest_version(95000)
    return p, seq


P14 = b"\x07" * 14


def _key(rng):
    return P14 + bytes(int(x) for x in rng.choice([0, 1, 255], size=int(rng.integers(0, 6))))


def _rg(rng, point):
    a = _key(rng)
    if rng.random() < point:
        return KeyRange(a, a + b"\x00")
    b = _key(rng)
    a, b = min(a, b), max(a, b)
    return KeyRange(a, b)


def prefix_sequence(seed):
    """10 batches of 40 transactions over keys of 14 - 19 bytes behind a 14-byte shared prefix: ties
    on the 16-byte prefix words decided by length and tails, boundaries differing by a trailing zero."""
    rng = np.random.default_rng(seed)
    seq = []
    for b in range(10):
        now = 100 + 5 * b
        txns = [CommitTransaction([_rg(rng, .5) for _ in range(int(rng.integers(0, 3)))],
                                  [_rg(rng, .85) for _ in range(int(rng.integers(0, 3)))],
                                  int(now - rng.integers(0, 12)), False) for _ in range(40)]
        seq.append((PackedBatch.from_transactions(txns), now, now - 30))
    return seq


# ---- 1

@pytest.mark.parametrize("gc_interval,delta_limit", [(1, 0), (0, 0), (3, 0)])
def test_kat_scenarios_state(engine, oracle_mod, gc_interval, delta_limit):
    """(1, 0) compacts every batch (empty delta at export), (0, 0) never (everything in the delta over
    an empty base)."""
    for scn in load_json("kat_scenarios.json"):
        p = Pair(engine, oracle_mod, gc_interval=gc_interval, delta_limit=delta_limit)
        for i, (pb, now, no, expect, _) in enumerate(scenario_batches(scn)):
            if scn.get("clear_before") == i:
                p.clear(scn["clear_version"])
                p.check(what=(scn["name"], "clear"))
            v = p.detect(pb, now, no)
            assert v.tolist() == expect
            p.check(what=(scn["name"], i))


# ---- 2

@pytest.mark.parametrize("gc_interval", [0, 3])
def test_two_tiers_with_holes_multi_tile(engine, oracle_mod, gc_interval):
    p, seq = c2_pair(engine, oracle_mod, gc_interval)
    p.check(what="loaded")
    for i, (pb, now, no) in enumerate(seq):
        p.detect(pb, now, no)
        size = p.cs.history_size()
        got = p.check(what=i)
        assert len(got[1]) > 2 * 1024  # several scan tiles: look-back and tile edges
        assert p.cs.history_size() == size
        again = split_dump(p.cs.dump_history())
        assert again == got
        assert p.cs.history_size() == size


# ---- 3

def test_clamp_coalescing_across_tiles(engine):
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 256, size=(5000, 16), dtype=np.uint8), axis=0)
    n = len(keys)
    assert n > 4 * 1024
    vers = rng.integers(0, 100, size=n, dtype=np.int64)
    ko = np.arange(n + 1, dtype=np.int64) * 16
    cs = engine.ConflictSet()
    cs.load_history(keys.reshape(-1), ko, vers, 3)
    klist = [keys[i].tobytes() for i in range(n)]
    hdr, ks, vs = split_dump(cs.dump_history(floor=10 ** 6))
    assert (hdr, ks, vs) == (10 ** 6 - 1, [], [])
    for floor in (50, NO_FLOOR):
        want = canon(klist, vers, 3, floor)
        assert split_dump(cs.dump_history(floor=floor)) == want
        v = vers.copy() if floor == NO_FLOOR else np.where(vers >= floor, vers, floor - 1)
        keep = v != np.concatenate([[3 if floor == NO_FLOOR or 3 >= floor else floor - 1], v[:-1]])
        assert want[1] == [klist[i] for i in np.flatnonzero(keep)] and want[2] == v[keep].tolist()
    cs.close()


# ---- 4

@pytest.mark.parametrize("gc_interval", [0, 1])
def test_prefix_ties_and_zero_padding(engine, oracle_mod, gc_interval):
    total = 0
    for seed in range(20):
        p = Pair(engine, oracle_mod, gc_interval=gc_interval)
        for i, (pb, now, no) in enumerate(prefix_sequence(seed)):
            p.detect(pb, now, no)
            got = p.check(what=(seed, i))
        total += len(got[1])
    assert total >= 200  # the final states are not degenerate


# ---- 5

def test_long_keys(engine, oracle_mod, monkeypatch):
    monkeypatch.setenv("FDBCS_SPLIT_CHECK", "1")
    cp = W.C4Params(txns=400, users=800, items=300, history=20_000, window=12_000, staleness=4_000)
    kb, ko, vers = W.c4_history(cp, seed=4, start_version=100_000)
    assert 15_000 < len(vers) <= 20_000
    p = Pair(engine, oracle_mod, gc_interval=2)
    p.load_history(kb, ko, vers)
    p.check(what="loaded", floor=NO_FLOOR)
    rng = np.random.default_rng(5)
    now = 100_000
    for i in range(3):
        now += cp.version_step
        p.detect(W.c4_batch(cp, rng, now), now, now - cp.window)
        p.check(what=i)


@pytest.mark.parametrize("gc_interval,delta_limit", [(0, 0), (0, 40), (3, 0)])
def test_long_shared_prefix_and_empty_key(engine, oracle_mod, gc_interval, delta_limit):
    """Every key behind a 60-byte shared prefix (all order decisions in the tails), and the empty key
    as a boundary."""
    rng = np.random.default_rng(77 + gc_interval + delta_limit)
    prefix = bytes(rng.integers(0, 256, 60, dtype=np.uint8))
    p = Pair(engine, oracle_mod, gc_interval=gc_interval, delta_limit=delta_limit)
    now = 10
    for i in range(12):
        pb = W.random_small_batch(rng, int(rng.integers(20, 120)), alphabet=3, max_len=5, now=now, staleness=12,
                                  max_reads=4, max_writes=3)
        txns = []
        for t in pb.to_transactions():
            f = lambda r: KeyRange(prefix + bytes(r.begin), prefix + bytes(r.end))
            txns.append(CommitTransaction([f(r) for r in t.read_conflict_ranges],
                                          [f(r) for r in t.write_conflict_ranges], t.read_snapshot,
                                          t.report_conflicting_keys))
        if i % 5 == 0:
            txns.append(CommitTransaction([], [KeyRange(b"", b"\x01")], now, False))
        p.detect(PackedBatch.from_transactions(txns), now, now - int(rng.integers(0, 10)))
        got = p.check(what=i)
        if i == 0:
            assert got[1][0] == b""
        now += int(rng.integers(1, 4))


# ---- 6

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
        (long_probe[0], long_probe[1]),
        (ks[mid], None), (between, None), (None, ks[mid]), (None, between), (None, above),
        (b"", None), (None, b""),
    ]
    for lo, hi in cases:
        got = p.check(lo, hi, what=("clip", lo, hi))
        if lo is not None and lo == hi:
            assert got[1] == []
    with pytest.raises(p.e.C.FdbcsError) as ei:
        p.cs.dump_history(ks[mid], ks[2])
    assert ei.value.status == p.e.C.FDBCS_E_INVALID
    p.check(what="after the refused export")


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
    p.check(P14 + b"\x01\x00\x00", P14 + b"\x01\x00\x00\x00", what="bounds differing by a trailing zero")


# ---- 7

def test_round_trip(engine, oracle_mod):
    """A set loaded from another's export continues exactly like it (and like the oracle)."""
    for p, seq in (c2_pair(engine, oracle_mod, 3), (Pair(engine, oracle_mod, gc_interval=0), prefix_sequence(4))):
        half = len(seq) // 2
        for pb, now, no in seq[:half]:
            p.detect(pb, now, no)
        d2 = EngineDriver(engine, gc_interval=2)
        d2.cs.load_history(*p.cs.dump_history())
        d2.cs.set_oldest_version(p.cs.oldest_version)
        for pb, now, no in seq[half:]:
            pb = PackedBatch(pb.read_snapshot, np.ones(pb.n_txn, np.uint8), pb.read_offsets, pb.write_offsets,
                             pb.key_bytes, pb.key_offsets)  # every transaction reports its conflicting reads
            v2, c2 = d2.detect(pb, now, no)
            v1, c1 = p.e.detect(pb, now, no)
            vo, co = p.o.detect(pb, now, no)
            assert (v1 == vo).all() and (v2 == vo).all()
            assert c1 == co and c2 == co
            assert any(co.values()) or not (vo == 0).any()
        assert split_dump(d2.cs.dump_history()) == split_dump(p.cs.dump_history())
        p.check(what="final")


# ---- 8

def test_state_and_edges(engine, oracle_mod):
    C = engine
    L = C.load_library()
    cs = C.ConflictSet()
    assert split_dump(cs.dump_history()) == (0, [], [])
    cs.clear(42)
    assert split_dump(cs.dump_history()) == (42, [], [])
    assert split_dump(cs.dump_history(b"a", b"b", NO_FLOOR)) == (42, [], [])
    # an unwaited batch: the export refuses, the batch is unharmed
    o = oracle_mod.OracleConflictSet()
    o.clear(42)
    rng = np.random.default_rng(8)
    pb = W.random_small_batch(rng, 50, alphabet=3, max_len=3, now=60, staleness=10)
    b = C.ConflictBatch(cs, None)
    b.add_packed(pb)
    b.detect_async(60, 50)
    with pytest.raises(C.FdbcsError) as ei:
        cs.dump_history()
    assert ei.value.status == C.FDBCS_E_STATE
    v = b.wait()
    b.close()
    vo, _ = o.detect(pb, 60, 50)
    assert (v == vo).all()
    keys, vers = o.dump_history()
    want = canon(keys, vers, 42, o.oldest_version)
    assert split_dump(cs.dump_history()) == want and len(want[1]) > 0
    # capacities
    n, nb, hdr = cs.export_history()
    assert (n, hdr) == (len(want[1]), want[0])
    kb, ko, vv = np.zeros(max(nb, 1), np.uint8), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int64)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n - 1) == C.FDBCS_E_NOMEM
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb - 1, vp(ko), vp(vv), n) == C.FDBCS_E_NOMEM
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n) == C.FDBCS_OK
    assert split_dump((kb[:nb], ko, vv[:n], hdr)) == want
    # read once: released
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n) == C.FDBCS_E_STATE
    # a detect between export and read invalidates the result
    cs.export_history()
    b = C.ConflictBatch(cs, None)
    b.add_packed(pb)
    b.detect_conflicts(70, 55)
    b.close()
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n) == C.FDBCS_E_STATE
    # so do a load and a clear
    cs.export_history()
    cs.load_history(kb[:nb], ko, vv[:n], hdr)
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n) == C.FDBCS_E_STATE
    cs.export_history()
    cs.clear(9)
    assert L.fdbcs_history_export_read(cs.handle, vp(kb), nb, vp(ko), vp(vv), n) == C.FDBCS_E_STATE
    cs.close()
