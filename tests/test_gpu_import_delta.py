"""GPU tests of the history import into the delta tier (ConflictSet.merge_history /
merge_pending_export with into="delta"): the same definition as the fold path, checked the same way
(the receiver's exported state equals merge_max over the oracles' canonical forms, the batches that
follow resolve exactly), plus what only this path has: it leaves the base alone and runs no
compaction, keeps the delta invariant where a base boundary inside the range holds a greater
version than the import, and falls back to the fold when the delta could pass its bound."""
import numpy as np
import pytest

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests.export_helpers import Pair, split_dump
from tests.helpers import EngineDriver
from tests.import_helpers import merge_max, merge_max_fast, pack, shifted
from tests.test_gpu_export import P14, c2_pair, prefix_sequence
from tests.test_gpu_import import (_long_pair, _prefix_pair, _routed_batch, adopt, c2_sender, clamp, dumped, expected,
                                   raises)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


def merge_checked(recv, imp, lo=None, hi=None, what=None):
    """Import `imp` (a state) into the pair's delta tier, compare with merge_max, require that the
    delta path ran and left the base and the compaction count alone, reload the oracle."""
    want = expected(recv, imp, lo, hi)
    size, comp = recv.cs.history_size(), recv.cs.stats()["compactions"]
    kb, ko, vv, hdr = pack(imp)
    n = recv.cs.merge_history(kb, ko, vv, hdr, lo=lo, hi=hi, into="delta")
    got = dumped(recv.cs)
    if got != want:
        m = min(len(got[1]), len(want[1]))
        d = next((i for i in range(m) if got[1][i] != want[1][i] or got[2][i] != want[2][i]), m)
        raise AssertionError((what, lo, hi, "header", got[0], want[0], "first difference at", d, len(got[1]),
                              len(want[1]), got[1][d:d + 2], got[2][d:d + 2], want[1][d:d + 2], want[2][d:d + 2]))
    assert n == recv.cs.history_size(), what
    info = recv.cs.import_info()
    assert info["path"] == 1, (what, info)
    assert info["base_boundaries"] == size - info["delta_before"], (what, info, size)  # the base is as it was
    assert info["base_boundaries"] + info["delta_after"] == n, (what, info, n)
    assert recv.cs.stats()["compactions"] == comp, what
    adopt(recv, want)
    recv.check(what=(what, "adopted"))
    return want


# ---- 1

@pytest.mark.parametrize("gc_interval", [0, 3])
def test_three_streams_multi_tile(engine, oracle_mod, gc_interval):
    r, seq = c2_pair(engine, oracle_mod, gc_interval)
    s, sseq = c2_sender(engine, oracle_mod)
    for pb, now, no in seq[:4]:
        r.detect(pb, now, no)
    for pb, now, no in sseq[:2]:
        s.detect(pb, now, no)
    assert r.cs.history_size() > 8000  # a loaded base under a delta
    # a clipped range: bounds between boundaries, about the middle half of the key space
    lo, hi = b"\x40" + b"\x00" * 20, b"\xc0\x01"
    imp = s.reference(lo, hi)
    assert split_dump(s.cs.dump_history(lo, hi)) == imp and len(imp[1]) > 2 * 1024
    want = merge_checked(r, imp, lo, hi, what="clipped")
    assert len(want[1]) > 2 * 1024  # several scan tiles: look-back and tile edges
    assert r.cs.import_info()["delta_after"] > 2 * 1024
    # an overlapping range straight away: the delta already holds the first import
    lo2, hi2 = b"\x80\x00\x01", b"\xe0" + b"\x00" * 17 + b"\x05"
    imp2 = s.reference(lo2, hi2)
    assert len(imp2[1]) > 2 * 1024
    before = r.cs.import_info()["delta_after"]
    merge_checked(r, imp2, lo2, hi2, what="overlapping")
    assert r.cs.import_info()["delta_before"] == before
    # the receiver goes on: verdicts and state exact after every batch; with a cadence the ordinary
    # compaction folds the imported delta into the base, and a GC runs
    st0 = r.cs.stats()
    for i, (pb, now, no) in enumerate(seq[4:]):
        r.detect(pb, now, no)
        r.check(what=("after", i))
    if gc_interval:
        st1 = r.cs.stats()
        assert st1["compactions"] > st0["compactions"] and st1["gc_runs"] > st0["gc_runs"]


# ---- 2

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ties_across_all_three_streams(engine, oracle_mod, seed, monkeypatch):
    monkeypatch.setenv("FDBCS_VALIDATE", "1")
    seq, sseq = prefix_sequence(seed), prefix_sequence(seed + 100)

    def pairs():
        r = Pair(engine, oracle_mod, gc_interval=3)  # compacts at the third batch: base and delta both hold keys
        s = Pair(engine, oracle_mod, gc_interval=0)
        for pb, now, no in seq[:5]:
            r.detect(pb, now, no)
        for pb, now, no in (seq[0], sseq[1], seq[2], sseq[3], seq[4]):  # partly the receiver's own batches
            s.detect(pb, now, no)
        return r, s

    r, s = pairs()
    own, imp = r.reference(), s.reference()
    both = sorted(set(own[1]) & set(imp[1]))
    assert len(both) >= 4  # the same keys in the receiver and the import
    present = set(own[1]) | set(imp[1])
    after = [k + b"\x00" for k in both if k + b"\x00" not in present]
    absent = [P14 + b"\x00\x02", P14 + b"\x02\x02\x02\x02\x02\x02", P14 + b"\xfe"]
    assert not present & set(absent) and len(after) >= 2
    cases = [(None, None), (both[0], both[-1]), (both[1], both[1] + b"\x00"), (after[0], after[-1]),
             (absent[0], absent[1]), (absent[1], absent[2]), (both[1], None), (None, after[0]),
             tuple(sorted((absent[1], both[-1])))]
    for c, (lo, hi) in enumerate(cases):
        if c:
            r, s = pairs()
        full = c % 2 == 1  # the whole history clipped by the import, or the export of the range itself
        merge_checked(r, s.reference() if full else s.reference(lo, hi), lo, hi, what=(seed, c))
        for i, (pb, now, no) in enumerate(seq[5:8]):
            r.detect(pb, now, no)
            r.check(what=(seed, c, "after", i))


# ---- 3

def test_long_keys_every_source_alignment(engine, oracle_mod):
    prefix = bytes(np.random.default_rng(3).integers(0, 256, 60, dtype=np.uint8))
    r, seq = _long_pair(engine, oracle_mod, prefix, 81, 3, 12)
    s, sseq = _long_pair(engine, oracle_mod, prefix, 82, 0, 8)
    for pb, now, no in seq[:8]:
        r.detect(pb, now, no)
    for pb, now, no in sseq:
        s.detect(pb, now, no)
    imp = s.reference()
    own = r.reference()
    assert imp[1][0] == b"" and sum(len(k) > 24 for k in imp[1]) > 20 and len(own[1]) > 20
    lo, hi = prefix + b"\x00\x01", prefix + b"\x02\x01\x01\x01\x01\x00"
    bounds = [(None, None), (lo, hi), (prefix[:20], None), (None, prefix + b"\x01"), (b"", prefix[:17]),
              (prefix + b"\x01\x00", prefix + b"\x01\x00\x00\x00"), (lo, None), (None, hi)]
    rd = r.cs.dump_history()
    for shift in range(1, 9):  # the imported keys' addresses in the byte array at every alignment modulo 8
        cs = engine.ConflictSet()
        cs.load_history(*rd)
        cs.set_oldest_version(r.cs.oldest_version)
        blo, bhi = bounds[shift - 1]
        imp_s = shifted(imp, shift, 1000 + shift)
        assert cs.merge_history(*pack(imp_s), lo=blo, hi=bhi, into="delta") == cs.history_size()
        assert cs.import_info()["path"] == 1
        want = clamp(merge_max_fast(own, imp_s, blo, bhi), r.o.oldest_version)
        assert dumped(cs) == want, (shift, blo, bhi)
        cs.close()
    # keys of 17 - 25 bytes, one with a tail of exactly 8 bytes, and bounds as long
    mid = (5, [prefix[:17], prefix[:20], prefix[:24], prefix[:24] + b"\x00"], [140, 101, 141, 102])
    merge_checked(r, mid, prefix[:16], prefix[:24] + b"\x00\x00", what="17-25 bytes")
    merge_checked(r, imp, lo, hi, what="long")
    # the receiver goes on (later versions: the import's are behind it); the tails the import
    # appended survive the GC that repacks the arena
    for i, (pb, now, no) in enumerate(seq[8:]):
        r.detect(pb, now + 100, no)
        r.check(what=("after", i))
    assert r.cs.stats()["gc_runs"] > 0


# ---- 4

def _probe(p, key, snap, now):
    """Verdict of one read of [key, key + 0) at `snap`, the engine's and the oracle's agreeing."""
    pb = PackedBatch.from_transactions([CommitTransaction([KeyRange(key, key + b"\x00")], [], snap, False)])
    return int(p.detect(pb, now, 0)[0])


@pytest.mark.parametrize("hole", [False, True])
def test_invariant_known_answer(engine, oracle_mod, hole):
    """A base boundary inside the range holds more (b: 50) than the import (30): the delta entry of
    the import must not span it.  hole: the receiver's delta holds a hole run across b, the closing
    boundary of a committed write [a, a + 0) (whose version, 60, is necessarily above the base's, so
    the imported 30 then starts at a + 0)."""
    COMMITTED, CONFLICT = 2, 0
    a, b, c, d = b"a", b"b", b"c", b"d"
    own = (0, [a, b, c, d], [10, 50, 10, 10])
    p = Pair(engine, oracle_mod, gc_interval=0)
    p.load_history(*pack(own))
    p.set_oldest_version(0)
    now, low = 60, a  # low: where the imported 30 shows
    if hole:
        wr = PackedBatch.from_transactions([CommitTransaction([], [KeyRange(a, a + b"\x00")], 55, False)])
        assert int(p.detect(wr, now, 0)[0]) == COMMITTED
        own = (0, [a, a + b"\x00", b, c], [60, 10, 50, 10])  # canonical: d repeats c's 10
        assert dumped(p.cs) == own
        now, low = now + 1, a + b"\x00"
    imp = (0, [a, d], [30, 0])  # the single segment [a, d) at 30
    kat = (0, [a, a + b"\x00", b, c, d], [60, 30, 50, 30, 10]) if hole else (0, [a, b, c, d], [30, 50, 30, 10])
    assert merge_max(own, imp, a, d) == kat  # not taken from the engine
    merge_checked(p, imp, a, d, what=("known answer", hole))
    assert dumped(p.cs) == kat

    def probes():
        nonlocal now
        assert _probe(p, b, 40, now) == CONFLICT        # the base's 50 shows through
        assert _probe(p, low, 35, now + 1) == COMMITTED
        assert _probe(p, low, 25, now + 2) == CONFLICT  # the imported 30
        assert _probe(p, c, 25, now + 3) == CONFLICT
        assert _probe(p, d, 25, now + 4) == COMMITTED   # outside the range
        now += 5

    probes()
    # the ordinary compaction folds the delta into the base: a delta entry that wrongly covered the
    # base's 50 would overwrite it here
    comp = p.cs.stats()["compactions"]
    p.cs.set_gc_interval(1)
    assert _probe(p, d, 25, now) == COMMITTED  # a batch without writes
    now += 1
    assert p.cs.stats()["compactions"] > comp
    assert dumped(p.cs) == kat
    probes()
    p.check(what="after the compaction")


# ---- 5

def test_edges(engine, oracle_mod):
    r = _prefix_pair(engine, oracle_mod, 5, 3)
    s = _prefix_pair(engine, oracle_mod, 6, 0)
    own = r.reference()
    top = max(own[2]) + 5
    # no boundaries, only a header: raises the range, and the set's header only without a lower bound
    merge_checked(r, (top - 3, [], []), own[1][2], own[1][5], what="n = 0 over a range")
    assert r.reference()[0] == own[0]
    merge_checked(r, (top, [], []), None, own[1][1], what="n = 0 from below")
    assert r.reference()[0] == top and r.reference()[1][0] == own[1][1]
    imp = s.reference()
    # lo == hi: nothing changes, the path is reported (a fold of the own dump first, so that it shows)
    r.cs.merge_history(*r.cs.dump_history())
    assert r.cs.import_info()["path"] == 0 and r.cs.import_info()["delta_after"] == 0
    before, size = dumped(r.cs), r.cs.history_size()
    swapped = list(imp[1])
    swapped[2], swapped[3] = swapped[3], swapped[2]
    for k in (own[1][3], own[1][3] + b"\x00", b"", P14 + b"\x03"):
        assert r.cs.merge_history(*pack(imp), lo=k, hi=k, into="delta") == size
        assert dumped(r.cs) == before and r.cs.history_size() == size
        info = r.cs.import_info()
        assert info["path"] == 1 and info["delta_before"] == info["delta_after"] == 0
        raises(engine, engine.FDBCS_E_INVALID, r.cs.merge_history, *pack((imp[0], swapped, imp[2])), lo=k, hi=k,
               into="delta")  # still validated
        r.cs.merge_history(*r.cs.dump_history())
        assert r.cs.import_info()["path"] == 0
    merge_checked(r, imp, b"\x01", b"\x02", what="below every key")
    merge_checked(r, imp, b"\x09", b"\x0a", what="above every key")
    merge_checked(r, imp, imp[1][3], None, what="hi none")
    merge_checked(r, s.reference(None, imp[1][2]), None, imp[1][2], what="lo none")
    merge_checked(r, imp, what="everything")
    # idempotent: the own dump changes nothing
    before = dumped(r.cs)
    r.cs.merge_history(*r.cs.dump_history(), into="delta")
    assert dumped(r.cs) == before and r.cs.import_info()["path"] == 1
    r.cs.merge_history(*pack(imp), into="delta")
    assert dumped(r.cs) == before
    r.check(what="after the idempotent imports")
    # commutative: A into B and B into A
    a, b = _prefix_pair(engine, oracle_mod, 7, 3), _prefix_pair(engine, oracle_mod, 8, 1)
    da, db = a.cs.dump_history(), b.cs.dump_history()
    a.cs.merge_history(*db, into="delta")
    b.cs.merge_history(*da, into="delta")
    assert a.cs.import_info()["path"] == b.cs.import_info()["path"] == 1
    assert dumped(a.cs) == dumped(b.cs) == clamp(merge_max(split_dump(da), split_dump(db)), a.cs.oldest_version)


# ---- 6

@pytest.mark.parametrize("n,path", [(5000, 1), (70_000, 0)])
def test_fallback_past_the_delta_bound(engine, n, path):
    """70 000 boundaries pass a new set's delta bound of 65 536: the fold takes the import."""
    rng = np.random.default_rng(n)
    keys = np.unique(rng.integers(0, 256, size=(n, 16), dtype=np.uint8), axis=0)
    n = len(keys)
    assert n > 65536 or path == 1
    vers = rng.integers(1, 50, size=n, dtype=np.int64) * 2 + (np.arange(n) & 1)  # neighbours differ
    ko = np.arange(n + 1, dtype=np.int64) * 16
    cs = engine.ConflictSet()
    assert cs.merge_history(keys.reshape(-1), ko, vers, 3, into="delta") == n == cs.history_size()
    info = cs.import_info()
    assert info["path"] == path and info["delta_before"] == 0, info
    assert (info["base_boundaries"], info["delta_after"]) == ((0, n) if path else (n, 0)), info
    kb2, ko2, vv2, hdr = cs.dump_history()
    assert hdr == 3 and (ko2 == ko).all() and (vv2 == vers).all() and (kb2 == keys.reshape(-1)).all()
    cs.close()


def test_fallback_under_a_set_delta_limit(engine, oracle_mod):
    r = Pair(engine, oracle_mod, gc_interval=0, delta_limit=64)
    for pb, now, no in prefix_sequence(13)[:4]:
        r.detect(pb, now, no)
    keys = [P14 + bytes([x, y]) for x in range(1, 21) for y in range(10)]
    imp = (0, keys, [200 + (i % 7) for i in range(len(keys))])
    want = expected(r, imp, keys[3], keys[-3])
    n = r.cs.merge_history(*pack(imp), lo=keys[3], hi=keys[-3], into="delta")
    info = r.cs.import_info()
    assert info["path"] == 0 and info["delta_after"] == 0 and info["base_boundaries"] == n == r.cs.history_size()
    assert dumped(r.cs) == want
    adopt(r, want)
    pb, _, no = prefix_sequence(13)[4]
    r.detect(pb, 300, no)
    r.check(what="after the fallback")
    # a few boundaries still go to the delta
    merge_checked(r, (0, keys[:5], [400, 401, 402, 403, 404]), keys[0], keys[4], what="under the limit")


def test_fallback_with_overlay_tails_grows_the_arena(engine, oracle_mod):
    """A fallback whose overlay holds tails, on a set whose tail arena must grow for the fold: the
    fold goes on from the overlay the delta import's first phase built, after the receiver's
    buffers moved.  No call reports the arena's capacity, so the count relies on a new set's arena
    of 1.5 * 64 KiB: 2400 keys of 40 bytes take 8 * (12 000 + 2400) bytes of overlay tails, which
    the fold may all have to pack behind the receiver's own."""
    r = Pair(engine, oracle_mod, gc_interval=0, delta_limit=64)
    for pb, now, no in prefix_sequence(13)[:4]:
        r.detect(pb, now, no)
    assert any(len(k) > 16 for k in r.reference()[1])  # tails of its own, which move with the arena
    # 24-byte tails behind 240 prefix words: the first and the last tail word decide among ten each
    tails = [bytes([t // 4]) * 8 + b"\x01" * 8 + b"\x00" * 7 + bytes([t]) for t in range(10)]
    keys = [P14 + bytes([x, y]) + t for x in (0, 1, 2, 3, 128, 255) for y in range(40) for t in tails]
    assert keys == sorted(set(keys)) and all(len(k) == 40 for k in keys)
    imp = (0, keys, [90 + (i * 7) % 41 for i in range(len(keys))])  # below and above the receiver's versions
    kb, ko, vv, hdr = pack(imp)
    assert 8 * ((len(kb) + 7) // 8 + len(keys)) > 3 * (1 << 16) // 2
    lo, hi = keys[37], keys[-40][:-1] + b"\xfe"  # one of the keys, and one between two of them
    assert len(lo) == len(hi) == 40 and keys[0] < lo < hi < keys[-1] and hi not in keys
    want = expected(r, imp, lo, hi)
    n = r.cs.merge_history(kb, ko, vv, hdr, lo=lo, hi=hi, into="delta")
    info = r.cs.import_info()
    assert info["path"] == 0 and info["delta_after"] == 0 and info["base_boundaries"] == n == r.cs.history_size()
    assert dumped(r.cs) == want
    adopt(r, want)
    pb, _, no = prefix_sequence(13)[4]
    r.detect(pb, 300, no)
    r.check(what="after the fallback")
    # the same import with invalid arrays: refused by the shared first phase, the set as it was
    before, info = r.cs.dump_history(), r.cs.import_info()
    bad = ko.copy()
    bad[len(keys) // 2] = ko[len(keys) // 2 - 1] - 1  # the key before it has length -1
    swapped = list(keys)
    swapped[1000], swapped[1001] = swapped[1001], swapped[1000]
    for arrays in ((kb, bad, vv, hdr), pack((0, swapped, imp[2]))):
        raises(engine, engine.FDBCS_E_INVALID, r.cs.merge_history, *arrays, lo=lo, hi=hi, into="delta")
        assert all(np.array_equal(x, y) for x, y in zip(r.cs.dump_history(), before)) and r.cs.import_info() == info
    r.check(what="after the refused imports")


# ---- 7

def test_atomicity_and_state_rules(engine, oracle_mod):
    C = engine
    r = _prefix_pair(engine, oracle_mod, 9, 3)
    s = _prefix_pair(engine, oracle_mod, 10, 0)
    imp = s.reference()
    kb, ko, vv, hdr = pack(imp)
    merge_checked(r, imp, imp[1][0], imp[1][1], what="a first import")  # import_info holds a delta import
    before, size, info = dumped(r.cs), r.cs.history_size(), r.cs.import_info()
    assert len(imp[1]) >= 6 and r.cs.history_size() > 0 and info["delta_after"] > 0
    merge = lambda *a, **k: r.cs.merge_history(*a, into="delta", **k)

    def untouched():
        assert dumped(r.cs) == before and r.cs.history_size() == size
        assert r.cs.import_info() == info
        r.check(what="untouched")

    swapped = list(imp[1])
    swapped[2], swapped[3] = swapped[3], swapped[2]
    raises(C, C.FDBCS_E_INVALID, merge, *pack((hdr, swapped, imp[2])))
    untouched()
    equal = list(imp[1])
    equal[-1] = equal[-2]
    raises(C, C.FDBCS_E_INVALID, merge, *pack((hdr, equal, imp[2])))
    untouched()
    neg = ko.copy()
    neg[2] = ko[1] - 1  # key 1's length is -1 (and key 2 longer by as much)
    raises(C, C.FDBCS_E_INVALID, merge, kb, neg, vv, hdr)
    untouched()
    off0 = ko.copy()
    off0[0] = 1
    raises(C, C.FDBCS_E_INVALID, merge, kb, off0, vv, hdr)
    untouched()
    # invalid input is refused even where the range is empty
    raises(C, C.FDBCS_E_INVALID, merge, *pack((hdr, swapped, imp[2])), lo=b"k", hi=b"k")
    untouched()
    raises(C, C.FDBCS_E_INVALID, merge, kb, ko, vv, hdr, lo=imp[1][4], hi=imp[1][1])
    untouched()
    # a pending export of the receiver is dropped by an import
    n, nb, _ = r.cs.export_history()
    merge_checked(r, imp, imp[1][1], imp[1][4], what="valid")
    raises(C, C.FDBCS_E_STATE, r.cs.read_export, n, nb)
    # versions: the greatest one the import left in the delta bounds the next `now`
    now = 100 + 5 * 6
    big = now + 1000
    out_of_range = (0, [P14 + b"\x00", P14 + b"\x01", P14 + b"\x02"], [1, big, 1])
    merge_checked(r, out_of_range, P14 + b"\x02", None, what="the great version outside the range")
    pb, _, no = prefix_sequence(9)[6]
    r.detect(pb, now, no)
    merge_checked(r, out_of_range, P14 + b"\x01", P14 + b"\x01\x00", what="the great version inside")
    b = C.ConflictBatch(r.cs, None)
    b.add_packed(pb)
    raises(C, C.FDBCS_E_VERSION, b.detect_conflicts, big - 1, no)
    b.close()
    r.detect(pb, big + 1, no)
    r.check(what="after the great version")
    assert r.cs.oldest_version == r.o.oldest_version == no  # the import moved no oldest version
    # an import while a batch is in flight: refused, the batch and the set unharmed
    pb2, _, _ = prefix_sequence(9)[7]
    b = C.ConflictBatch(r.cs, None)
    b.add_packed(pb2)
    b.detect_async(big + 5, no)
    raises(C, C.FDBCS_E_STATE, merge, kb, ko, vv, hdr)
    v = b.wait()
    b.close()
    vo, _ = r.o.detect(pb2, big + 5, no)
    assert (v == vo).all()
    r.check(what="after the refused import")


# ---- 8

def test_pending_export_path(engine, oracle_mod):
    C = engine
    r = _prefix_pair(engine, oracle_mod, 11, 3)
    s = _prefix_pair(engine, oracle_mod, 12, 2)
    own, full = r.reference(), s.reference()
    rd = r.cs.dump_history()
    for lo, hi in [(None, None), (full[1][2], full[1][-2]), (P14 + b"\x00\x02", None), (None, full[1][3] + b"\x00")]:
        d1, d2 = engine.ConflictSet(), engine.ConflictSet()
        for d in (d1, d2):
            d.load_history(*rd)
            d.set_oldest_version(r.cs.oldest_version)
        n, nb, hdr = s.cs.export_history(lo, hi)
        n1 = d1.merge_pending_export(s.cs, lo, hi, into="delta")
        kb, ko, vv = s.cs.read_export(n, nb)  # still pending and readable
        assert split_dump((kb, ko, vv, hdr)) == s.reference(lo, hi)
        assert d2.merge_history(kb, ko, vv, hdr, lo=lo, hi=hi, into="delta") == n1 == d1.history_size()
        assert d1.import_info() == d2.import_info() and d1.import_info()["path"] == 1
        want = clamp(merge_max(own, s.reference(lo, hi), lo, hi), r.o.oldest_version)
        assert dumped(d1) == dumped(d2) == want, (lo, hi)
        # the read released the result
        raises(C, C.FDBCS_E_STATE, d1.merge_pending_export, s.cs, lo, hi, into="delta")
        assert dumped(d1) == want
        d1.close()
        d2.close()
    s.cs.export_history()
    raises(C, C.FDBCS_E_INVALID, s.cs.merge_pending_export, s.cs, into="delta")
    raises(C, C.FDBCS_E_INVALID, r.cs.merge_pending_export, s.cs, b"b", b"a", into="delta")
    s.check(what="the sender is untouched")


# ---- 9

def test_range_hand_over_end_to_end(engine, oracle_mod):
    """B owns the keys below s = 0x80, A those from s on; [s, t) moves from A to B through B's delta."""
    C = engine
    rng = np.random.default_rng(21)
    s_key, t_key = b"\x80", b"\xc0"
    fa, fb = [0x80, 0x90, 0xa0, 0xb0, 0xd0, 0xf0], [0x10, 0x30, 0x50, 0x70]
    a = Pair(engine, oracle_mod, gc_interval=3)
    b = Pair(engine, oracle_mod, gc_interval=2)
    now, nows = 100, []
    for _ in range(8):
        a.detect(_routed_batch(rng, fa, now), now, now - 60)
        b.detect(_routed_batch(rng, fb, now), now, now - 60)
        nows.append(now)
        now += 5
    control = EngineDriver(engine, gc_interval=2)  # B without the hand-over
    control.cs.load_history(*b.cs.dump_history())
    control.cs.set_oldest_version(b.cs.oldest_version)
    moved = a.reference(s_key, t_key)
    assert len(moved[1]) >= 8
    want = expected(b, moved, s_key, t_key)
    got = b.cs.merge_history(*a.cs.dump_history(s_key, t_key), lo=s_key, hi=t_key, into="delta")
    assert got == b.cs.history_size() and b.cs.import_info()["path"] == 1
    assert dumped(b.cs) == want
    # reads in [s, t), now sent to B: snapshots straddle the versions A accepted writes at there
    keys = [bytes([f, x]) for f in (0x80, 0x90, 0xa0, 0xb0) for x in range(4)]
    probe = PackedBatch.from_transactions([
        CommitTransaction([KeyRange(k, k + b"\x00")], [], int(snap), False)
        for k in keys for snap in (nows[1], nows[4], nows[-1])])
    va, _ = a.o.detect(probe, now, now - 60)   # what the old owner would have said
    vb, _ = b.e.detect(probe, now, now - 60)
    vc, _ = control.detect(probe, now, now - 60)
    assert (vb == va).all()
    assert (va == 0).any() and (va == 2).any()  # some reads abort, some commit
    assert ((vc == 2) & (va == 0)).any()        # without the import B commits reads that must abort
    # B resolves on over its old and its new keys, two batches in flight
    adopt(b, want)
    b.o.detect(probe, now, now - 60)
    flying = []

    def land():
        bt, pb, at = flying.pop(0)
        v = bt.wait()
        bt.close()
        vo, _ = b.o.detect(pb, at, at - 60)
        assert (v == vo).all(), at

    for _ in range(4):
        now += 5
        pb = _routed_batch(rng, fb + [0x80, 0x90, 0xa0, 0xb0], now)
        bt = C.ConflictBatch(b.cs, None)
        bt.add_packed(pb)
        bt.detect_async(now, now - 60)
        flying.append((bt, pb, now))
        if len(flying) == 2:
            land()
    while flying:
        land()
    b.check(what="after the hand-over")
