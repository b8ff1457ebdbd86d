"""GPU tests of the read-version query (ConflictBatch.read_versions, ConflictSet.read_versions and
version_at).  Every case compares the device's answer with the plain-Python model
(tests/read_versions_model.py, pinned to the oracle by tests/test_read_versions_cpu.py) evaluated on
the set's own dump_history(floor=...), and, where the semantic oracle runs beside the set
(tests/export_helpers.Pair), with the model on the oracle's dump as well.  Lengths are asserted
equal, so no read drops out of a comparison."""
import ctypes

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests import keyspace_model as K
from tests import read_versions_model as M
from tests.device_add_helpers import Staged, keys_of, repack
from tests.export_helpers import NO_FLOOR, Pair
from tests.helpers import EngineDriver
from tests.test_gpu_export import c2_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_mod(oracle_built):
    return oracle_built


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch

    return torch


def check(cs, ranges, floor=None, pair=None, what=None):
    """cs.read_versions(ranges, floor) against the model on the set's own dump at that floor (and on
    the oracle's dump); returns it as a list."""
    got = cs.read_versions(ranges, floor)
    assert got.dtype == np.int64
    want = M.of_dump(cs.dump_history(floor=floor), ranges)
    assert len(got) == len(want) == len(ranges), what
    got = got.tolist()
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, (what, floor, len(bad), "of", len(got), [(ranges[i], got[i], want[i]) for i in bad[:5]])
    if pair is not None:
        keys, vers = pair.o.dump_history()
        f = pair.o.oldest_version if floor is None else floor
        want = M.read_versions(keys, vers.tolist(), pair.header, ranges, f)
        bad = [i for i in range(len(got)) if got[i] != want[i]]
        assert len(want) == len(got) and not bad, (what, "oracle", [(ranges[i], got[i], want[i]) for i in bad[:5]])
    return got


def write_batch(ranges, now):
    """One transaction that writes `ranges` and reads nothing: it always commits."""
    return PackedBatch.from_transactions([CommitTransaction([], [KeyRange(a, b) for a, b in ranges], now, False)])


def arrays(keys, vers):
    ko = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=ko[1:])
    return np.frombuffer(b"".join(keys), np.uint8), ko, np.asarray(vers, np.int64)


def all_pairs(probes):
    probes = sorted(set(probes))
    return [(a, b) for i, a in enumerate(probes) for b in probes[i:]]


# ---- 1. empty sets

@pytest.mark.parametrize("R", [0, 1, 15, 17, 4097])
def test_empty_sets(engine, R):
    rng = np.random.default_rng(R)
    ranges = []
    for _ in range(R):
        a, b = sorted(bytes(rng.integers(0, 4, size=int(rng.integers(0, 30))).astype(np.uint8)) for _ in range(2))
        ranges.append((a, b if rng.random() < 0.8 else a))
    cs = engine.ConflictSet()  # never loaded, never cleared
    got = cs.read_versions(ranges)
    assert got.dtype == np.int64 and got.tolist() == [0] * R
    if R:
        assert cs.version_at(b"") == 0 and cs.version_at(b"k" * 30, floor=NO_FLOOR) == 0
    cs.clear(42)
    assert cs.read_versions(ranges).tolist() == [42] * R
    assert cs.read_versions(ranges, floor=100).tolist() == [99] * R  # the header is clamped as the export's
    assert cs.read_versions(ranges, floor=NO_FLOOR).tolist() == [42] * R
    check(cs, ranges, what="cleared")
    # the batch form, R == 0 included: a batch without reads writes nothing
    b = engine.ConflictBatch(cs)
    b.add_packed(PackedBatch.from_transactions([CommitTransaction([KeyRange(a, e) for a, e in ranges],
                                                                  [KeyRange(b"w", b"x")], 50, False)]))
    out = b.read_versions()
    assert out.dtype == np.int64 and out.tolist() == [42] * R
    if R:
        kern, host = b.read_versions_timing()
        assert kern > 0 and host >= kern
    b.close()
    cs.close()


# ---- 2. and 3. both tiers with holes: every kind of span and every degenerate read

def K5(i):
    return b"k%05d" % i


def build_two_tiers(engine, oracle_mod, header):
    """A base of 60 boundaries at K5(10 i) (versions 1000 .. 2000, the base's greatest, 2900, at K5(300))
    under a delta of three write batches, whose ends leave holes; the greatest version of all, 3020,
    stands at K5(350)."""
    p = Pair(engine, oracle_mod, gc_interval=0, delta_limit=1 << 20)
    rng = np.random.default_rng(2)
    keys = [K5(10 * i) for i in range(1, 61)]
    vers = rng.integers(1000, 2000, size=60)
    vers[29] = 2900  # K5(300)
    p.load_history(*arrays(keys, vers), header)
    p.set_oldest_version(10)
    for now, ranges in ((3000, [(K5(105), K5(125)), (K5(200), K5(200) + b"\x00"), (K5(455), K5(458))]),
                        (3010, [(K5(5), K5(7)), (K5(650), K5(660)), (K5(210), K5(220))]),
                        (3020, [(K5(350), K5(400))])):
        p.detect(write_batch(ranges, now), now, 10)
    assert p.cs.history_size() > 60 + 8  # the delta holds boundaries of its own: nothing was compacted
    p.loaded = dict(zip(keys, vers.tolist()))  # the base's versions as loaded
    return p


@pytest.fixture(scope="module")
def two_tiers(engine, oracle_mod):
    ps = {h: build_two_tiers(engine, oracle_mod, h) for h in (50, 2950)}
    yield ps
    for p in ps.values():
        p.cs.close()


PROBES = [b"", b"\x00", b"k", b"l", b"zz", K5(7)] + [K5(j) for j in range(0, 700, 5)] + \
         [K5(j) + b"\x00" for j in (5, 7, 10, 105, 125, 200, 300, 350, 400, 600, 660)]


@pytest.mark.parametrize("header", [50, 2950])
def test_both_tiers_every_span(two_tiers, header):
    """All pairs of the probe keys (boundaries of either tier, keys strictly inside segments, keys
    below the first and past the last boundary): reads in the base only, in the delta only and across
    both, beginning and ending at and between boundaries."""
    p = two_tiers[header]
    ranges = [r for r in all_pairs(PROBES) if r[0] < r[1]]
    assert len(ranges) > 10000
    got = dict(zip(ranges, check(p.cs, ranges, pair=p, what=header)))
    assert got == dict(zip(ranges, check(p.cs, ranges, floor=NO_FLOOR, pair=p)))  # nothing lies below the floor
    # a boundary at e does not count: the greatest version of all starts at K5(350), the base's at K5(300)
    assert got[(K5(340), K5(350))] < 2900 and got[(K5(340), K5(350) + b"\x00")] == 3020
    assert got[(K5(290), K5(300))] < 2900 and got[(K5(290), K5(300) + b"\x00")] == 2900
    assert got[(K5(345), K5(350))] == got[(K5(340), K5(345))]  # begin strictly inside the same segment
    # the maximum in the first and in the last counted segment, and just outside either end
    assert got[(K5(300), K5(340))] == 2900 and got[(K5(305), K5(340))] == 2900 and got[(K5(310), K5(340))] < 2900
    assert got[(K5(395), K5(450))] == 3020 and got[(K5(400), K5(450))] < 2900
    # below the first boundary the header counts (once it is the maximum of the span)
    assert got[(b"", K5(0))] == header and got[(b"k", K5(5))] == header
    assert got[(b"", K5(100))] == max(header, 3010)
    assert (got[(b"", K5(5) + b"\x00")] == 3010) and (got[(K5(7), K5(10))] == header)  # the hole shows the header
    # past the last boundary of the base, around the delta's
    assert got[(K5(650), K5(655))] == 3010 and got[(K5(660), K5(695))] == got[(K5(600), K5(605))] < 2000
    assert got[(K5(695), b"zz")] == got[(K5(660), K5(665))]
    # the delta only / the base only / across both
    assert got[(K5(110), K5(120))] == 3000 and got[(K5(130), K5(190))] < 2000 and got[(K5(100), K5(130))] == 3000
    assert p.cs.version_at(K5(350)) == 3020 and p.cs.version_at(K5(349)) == got[(K5(345), K5(350))]


@pytest.mark.parametrize("header", [50, 2950])
def test_degenerate_reads(two_tiers, header):
    p = two_tiers[header]
    ranges = [(k, k) for k in sorted(set(PROBES))]
    got = dict(zip([r[0] for r in ranges], check(p.cs, ranges, pair=p, what=header)))
    base = p.loaded
    assert got[b""] == header and got[b"\x00"] == header and got[K5(0)] == header
    assert got[K5(5)] == header          # the first boundary (the delta's): the header
    assert got[K5(7)] == 3010            # at the boundary that ends the write: the write's segment lies below
    assert got[K5(10)] == header         # the first base boundary: the delta's hole below it shows the header
    assert got[K5(350)] == base[K5(340)]  # at a boundary only the delta has: the base segment below
    assert got[K5(355)] == 3020           # between boundaries, inside the delta's segment
    assert got[K5(110)] == 3000           # at a boundary only the base has, under the delta's segment
    assert got[K5(130)] == base[K5(120)] and got[K5(125)] == 3000  # the delta's segment below b is a hole / is not
    assert got[K5(300)] == base[K5(290)] and got[K5(305)] == 2900
    assert got[b"zz"] == base[K5(600)]
    # mixed with ordinary reads in one batch, a ragged last quad
    mixed = [(K5(350), K5(350)), (K5(340), K5(360)), (b"", b""), (K5(125), K5(125)), (K5(10), K5(10) + b"\x00")]
    assert check(p.cs, mixed, pair=p) == [base[K5(340)], 3020, header, 3000, base[K5(10)]]


# ---- 4. key lengths: both lookup forms

S16 = b"s" * 16
P20 = b"p" * 20
Q30 = b"q" * 30


def length_keys():
    short = [b"", b"\x00", b"a", b"a\x00", b"ab", b"m" * 15, b"m" * 15 + b"\x00", S16]
    mid = [S16 + b"\x00", S16 + b"x", P20, P20 + b"\x00", P20 + b"ab", P20 + b"abc\x00", P20 + b"abcd", P20 + b"b"]
    long = [P20 + b"abcd\x00", P20 + b"abcde", Q30, Q30 + b"\x00", Q30 + b"\x00\x00", Q30 + b"a" * 10,
            Q30 + b"a" * 70 + b"x", Q30 + b"a" * 70 + b"x\x00", Q30 + b"a" * 70 + b"y" * 8, Q30 + b"b"]
    assert max(map(len, short)) == 16 and 16 < min(map(len, mid)) and max(map(len, mid)) == 24
    assert min(map(len, long)) == 25 and max(map(len, long)) == 108
    return short, mid, long


def launches(cs):
    """Launches of the query's two kernels so far, as the engine's kernel profile reports them."""
    prof = cs.kernel_profile()
    return tuple(prof.get(f"k_read_versions<{x}>", {"launches": 0})["launches"] for x in ("false", "true"))


@pytest.mark.parametrize("gc_interval", [0, 1])
def test_key_lengths(engine, oracle_mod, torch_mod, gc_interval):
    """Keys of 0 to 16, 17 to 24 and 25 to 108 bytes in both tiers, shared prefixes of more than 16
    and more than 24 bytes, k beside k + b'\\0'.  A batch whose longest key has at most 24 bytes takes
    the short-key lookup, a longer one the long-key lookup (the read check's rule): the engine's kernel
    profile says which kernel ran, for host-added and for device-added batches (whose longest key the
    add kernels report in classes)."""
    short, mid, long = length_keys()
    every = sorted(set(short + mid + long))
    p = Pair(engine, oracle_mod, gc_interval=gc_interval, delta_limit=1 << 20)
    loaded = every[1::2]
    p.load_history(*arrays(loaded, [100 + 7 * i for i in range(len(loaded))]), 33)
    p.set_oldest_version(10)
    now = 1000
    for ks in (every[0::4], every[2::4]):  # keys the base has not, k + b'\0' ends beside loaded keys
        p.detect(write_batch([(k, k + b"\x00") for k in ks] + [(P20 + b"a", P20 + b"abc")], now), now, 10)
        now += 10
    for name, probes, is_long in (("short", short, False), ("mid", short[:3] + mid, False), ("long", long, True),
                                  ("mixed", every, True)):
        ranges = all_pairs(probes + [k + b"\x00" for k in probes if len(k) < (16 if name == "short" else 24
                                                                             if name == "mid" else 107)])
        longest = max(len(k) for r in ranges for k in r)
        assert (longest > 24) == is_long and (name != "short" or longest <= 16), (name, longest)
        before = launches(p.cs)
        got = check(p.cs, ranges, pair=p, what=name)
        assert len(set(got)) >= 4, name
        assert launches(p.cs) == (before[0] + (not is_long), before[1] + is_long), name  # one launch, of that form
        # the same reads from device memory
        pb = PackedBatch.from_transactions([CommitTransaction([KeyRange(a, e) for a, e in ranges], [], 2000, False)])
        st = Staged(torch_mod, pb)
        b = engine.ConflictBatch(p.cs)
        b.add_packed_device(st.dpb)
        assert b.read_versions().tolist() == got, name
        assert launches(p.cs) == (before[0] + 2 * (not is_long), before[1] + 2 * is_long), name
        b.close()
    p.cs.close()


# ---- 5. every range-max level, against the dense model

D = 10 ** 14 + 7
L2, L3 = 64 * 64, 64 * 64 * 64  # boundaries under one level-2 / level-3 entry
H_BIG = 3 * L3 + 3000
# the highest versions of all, deep inside the three whole level-3 blocks (the first the highest),
# then in the middle of level-2 blocks: a wide read finds them in upper-level entries alone
DEEP = (L3 + 100000, 2 * L3 + 150000, 100000, L3 + L2 * 5 + 2048, L3 + L2 * 40 + 2048, 2 * L3 + L2 * 55 + 2048)


@pytest.fixture(scope="module")
def dense(engine):
    """A base of 3*64*4096 + 3000 boundaries (three whole level-3 blocks, 192 whole level-2 blocks and
    a tail: a read over more than 128 whole level-2 blocks climbs to level 3), every version offset
    by D, isolated spikes at the block edges of every level and the highest versions deep inside
    blocks: (set, model, boundary universe indices, spike universe indices, versions by rank)."""
    rng = np.random.default_rng(5)
    hist_idx = K.FIRST_BOUNDARY + 2 * np.arange(H_BIG)  # a non-boundary key inside every segment
    U = int(hist_idx[-1]) + 3
    model = K.KeyspaceModel(K.make_universe(rng, U, "random16"), D + 1234)
    vers = D + 1000 + np.cumsum(rng.integers(1, 1000, size=H_BIG)) % 1000
    spikes = np.unique(np.concatenate([K.spike_positions(rng, H_BIG, 24), [2 * L3 - 1, 2 * L3, 3 * L3 - 1, 3 * L3]]))
    assert {63, 64, L2 - 1, L2, L3 - 1, L3} <= set(spikes.tolist()) and not set(DEEP) & set(spikes.tolist())
    vers[spikes] = D + 10 ** 6 + rng.permutation(len(spikes))
    vers[list(DEEP)] = D + 1_500_000 + np.arange(len(DEEP))[::-1]
    model.load(hist_idx, vers)
    cs = engine.ConflictSet()
    cs.set_gc_interval(0)
    cs.set_delta_limit(1 << 22)
    cs.load_history(*model.pack_keys(hist_idx), vers, model.header)
    cs.set_oldest_version(D + 500)
    assert cs.history_size() == H_BIG
    yield cs, model, hist_idx, hist_idx[spikes], vers
    cs.close()


def dense_spans(bnd, spike_u):
    nb = len(bnd)
    spans = [K.directed_spans(bnd), K.spike_spans(bnd, spike_u)]
    # widths just under and over 128, 128 * 64 and 128 * 4096 boundaries, and over 129 to 192 whole
    # level-2 blocks (what reaches level 3), from starts at, one before and one after the block edges
    # of every level
    extra = []
    wide = [w * L2 + e for w in (129, 130, 131, 150, 191, 192) for e in (-1, 0, 1, 64, L2 - 1)]
    for lo in K.STARTS + (2, 62, 66, L2 - 2, L2 + 2, L3 - 2, L3 + 2, L3 + L2 - 1, L3 + L2, L3 + L2 + 1):
        for ln in [126, 127, 128, 129, 130, 8190, 8191, 8192, 8193, 8194, 524286, 524287, 524288, 524289, 524290] + wide:
            if lo + ln < nb:
                extra.append((bnd[lo], bnd[lo + ln]))
                extra.append((bnd[lo] - 1, bnd[lo + ln] - 1))  # begin and end strictly inside segments
    extra += [(0, bnd[nb - 1]), (bnd[0], bnd[nb - 1] + 1), (bnd[1] - 1, bnd[3 * L3])]
    spans.append(np.array(extra, np.int64))
    k = np.concatenate([bnd[[0, 1, 63, 64, 65, L2, L3, 2 * L3, nb - 1]], bnd[[64, L2, L3]] - 1, [0, 1]])
    spans.append(np.stack([k, k], 1))  # degenerate reads at the edges
    return np.unique(np.concatenate(spans), axis=0)


def spans_by_level(bnd, spans, vers):
    """How many non-degenerate spans take their maximum from an entry of level 1, 2, 3 alone: the
    climb of the range maximum replayed (keyspace_model.climb_level) over the ranks the span counts,
    [the segment containing its begin, the boundaries below its end), with the ranks that hold the
    span's greatest version."""
    counts = {1: 0, 2: 0, 3: 0}
    lo_r = np.maximum(np.searchsorted(bnd, spans[:, 0], "right") - 1, 0)
    hi_r = np.searchsorted(bnd, spans[:, 1], "left")
    order = np.argsort(-vers, kind="stable")[:400]  # the ranks of the highest versions: deep ones, then spikes
    for lo, hi in zip(lo_r.tolist(), hi_r.tolist()):
        if hi - lo <= 128:
            continue
        inside = order[(order >= lo) & (order < hi)]
        if not len(inside):
            continue
        level = K.climb_level(lo, hi, inside[:1])  # versions are distinct among these: one holder
        if level in counts:
            counts[level] += 1
    return counts


def model_check(cs, model, spans, floor=None, what=None):
    a, b = spans[:, 0], spans[:, 1]
    want = model.read_max(a, b)
    model.check_table(a, b, np.random.default_rng(1))
    kb, ko = model.pack_keys(spans.ravel())
    raw, ko = kb.tobytes(), ko.tolist()
    keys = [raw[x:y] for x, y in zip(ko, ko[1:])]
    got = cs.read_versions(list(zip(keys[0::2], keys[1::2])), floor)
    assert len(got) == len(want) == len(spans)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, "of", len(want), spans[bad[:5]].tolist(), got[bad[:5]], want[bad[:5]])
    return got


def test_every_range_max_level(engine, dense):
    cs, model, bnd, spike_u, vers = dense
    spans = dense_spans(bnd, spike_u)
    width = np.searchsorted(bnd, spans[:, 1]) - np.searchsorted(bnd, spans[:, 0])
    assert (width > 128 * 4096).sum() >= 40 and ((width > 128 * 64) & (width <= 128 * 4096)).sum() >= 200
    assert ((width > 128) & (width <= 128 * 64)).sum() >= 200 and len(spans) >= 3000
    # spans whose greatest version only an entry of that level holds: a stale or missed entry of any
    # level, the top level's replicas included, is a wrong number
    reached = spans_by_level(bnd, spans, vers)
    assert reached[3] >= 100 and reached[2] >= 100 and reached[1] >= 100, reached
    got = model_check(cs, model, spans, floor=NO_FLOOR, what="base")
    assert (got >= D).all()  # versions far past 32 bits
    K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), model.rle(), "base")
    # a delta over it: writes at keys that were no boundaries, one beside every level-3 edge
    rng = np.random.default_rng(6)
    wa = np.concatenate([rng.integers(0, model.U - 4, size=600), bnd[[L3 - 1, L3, 2 * L3, L2, 64]] - 1])
    wb = wa + 1
    now = D + 2_000_000
    pb = model.batch(np.ones(len(wa), bool), wa, wb, np.full(len(wa), now))
    b = engine.ConflictBatch(cs)
    b.add_packed(pb)
    assert (b.detect_conflicts(now, D + 500) == K.COMMITTED).all()
    b.close()
    model.write(wa, wb, now)
    assert cs.history_size() > H_BIG + 300  # the delta holds the writes' boundaries: nothing was compacted
    got = model_check(cs, model, spans, what="base + delta")
    assert (got == now).sum() > 100 and (got < now).sum() > 100
    K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), model.rle(), "base + delta")


# ---- 6. floor and GC invariance

def c2_ranges(seq, dump):
    """The sequence's own reads, and reads between every 37th boundary of a dump."""
    raw, off = dump[0].tobytes(), dump[1].tolist()
    ks = [raw[off[i]:off[i + 1]] for i in range(0, len(off) - 1, 37)]
    out = [(a, b) for a, b in zip(ks, ks[1:])] + [(a, b) for a, b in zip(ks, ks[5:])] + [(k, k) for k in ks[::3]]
    for pb, _, _ in seq[:3]:
        out += [(r.begin, r.end) for t in pb.to_transactions()[:150] for r in t.read_conflict_ranges]
    return out


def test_floor_and_gc_invariance(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    twins = []
    for gc, limit in ((1, 0), (0, 1 << 20)):
        d = EngineDriver(C, gc_interval=gc, delta_limit=limit)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        twins.append(d)
    a, b = twins
    ranges = c2_ranges(seq, a.cs.dump_history(floor=NO_FLOOR))
    assert len(ranges) > 800
    # before the oldest version moves: as stored
    for d in twins:
        check(d.cs, ranges, floor=NO_FLOOR, what="loaded")
    for i, (pb, now, no) in enumerate(seq[:5]):
        va, ca = a.detect(pb, now, no)
        vb, cb = b.detect(pb, now, no)
        assert (va == vb).all() and ca == cb
        ga = check(a.cs, ranges, what=("gc every batch", i))
        gb = check(b.cs, ranges, what=("no gc", i))
        assert ga == gb, i  # the default floor: the oldest version
        oldest = a.cs.oldest_version
        assert oldest == b.cs.oldest_version == no
        hi = check(a.cs, ranges, floor=oldest + 2000, what=("floor above", i))
        assert hi == check(b.cs, ranges, floor=oldest + 2000) and min(hi) == oldest + 1999 < max(hi)
        check(b.cs, ranges, floor=NO_FLOOR, what=("as stored", i))
    assert a.cs.history_size() != b.cs.history_size()  # the tiers differ, the answers do not
    for d in twins:
        d.cs.close()


# ---- 7. after maintenance

def test_after_maintenance_and_hand_over(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    p = Pair(C, oracle_mod, gc_interval=0, delta_limit=1 << 20)
    p.load_history(kb, ko, vers, 7)
    p.set_oldest_version(95000)
    for pb, now, no in seq[:3]:
        p.detect(pb, now, no)
    ranges = c2_ranges(seq, p.cs.dump_history())
    before = check(p.cs, ranges, pair=p, what="two tiers")
    compactions = p.cs.stats()["compactions"]
    p.cs.set_gc_interval(1)  # the next batch compacts
    p.detect(*seq[3])
    assert p.cs.stats()["compactions"] == compactions + 1
    after = check(p.cs, ranges, pair=p, what="compacted")
    assert after != before
    p.cs.set_gc_interval(0)
    p.detect(*seq[4])
    check(p.cs, ranges, pair=p, what="a delta over the compacted base")
    # imports into either tier of a set with a history of its own
    dump = p.cs.dump_history()
    raw, off = dump[0].tobytes(), dump[1]
    n = len(dump[2])
    lo, hi = raw[off[n // 4]:off[n // 4 + 1]], raw[off[3 * n // 4]:off[3 * n // 4 + 1]]
    inside = [r for r in ranges if lo <= r[0] and r[1] <= hi and r[0] < r[1]]
    assert len(inside) > 100
    want_inside = p.cs.read_versions(inside).tolist()
    for into in ("delta", "base"):
        r = EngineDriver(C, gc_interval=0, delta_limit=1 << 20)
        r.load_history(kb, ko, vers, 7)
        r.cs.set_oldest_version(95000)
        r.detect(*seq[0])
        r.cs.set_oldest_version(p.cs.oldest_version)
        r.cs.merge_history(*p.cs.dump_history(lo, hi), lo=lo, hi=hi, into=into)
        assert r.cs.import_info()["path"] == (1 if into == "delta" else 0)
        got = check(r.cs, ranges, what=("imported into", into))
        check(r.cs, ranges, floor=NO_FLOOR, what=("imported into, as stored", into))
        # (everything below the oldest version reads as one value, every batch wrote one version)
        assert len(set(got)) >= 4
        r.cs.close()
    # a range hand-over to an empty set: inside [lo, hi) the receiver answers as the giver
    m = C.ConflictSet()
    m.clear(0)
    m.set_oldest_version(p.cs.oldest_version)
    m.merge_history(*p.cs.dump_history(lo, hi), lo=lo, hi=hi)
    assert m.read_versions(inside).tolist() == want_inside == p.cs.read_versions(inside).tolist()
    check(m, ranges, what="receiver")
    m.close()
    p.cs.close()


# ---- 8. the verdict property on the engine

def test_verdict_property_and_the_batch_is_unharmed(engine, oracle_mod):
    C = engine
    (kb, ko, vers), seq = c2_sequence()
    twins = []
    for _ in range(2):
        d = EngineDriver(C, gc_interval=0, delta_limit=1 << 20)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        for pb, now, no in seq[:3]:
            d.detect(pb, now, no)
        twins.append(d)
    a, twin = twins  # twin is never queried
    oldest = a.cs.oldest_version
    ranges = c2_ranges(seq, a.cs.dump_history())[:900]
    V = np.array(check(a.cs, ranges, what="V"))
    # three reads per transaction; its snapshot is the greatest V of them, or one less (never TooOld)
    T = len(ranges) // 3
    snap = np.maximum(V[:3 * T].reshape(T, 3).max(axis=1) - (np.arange(T) % 2), oldest)
    txns = [CommitTransaction([KeyRange(*ranges[3 * t + j]) for j in range(3)], [], int(snap[t]), True)
            for t in range(T)]
    pb = PackedBatch.from_transactions(txns)
    want = {t: [j for j in range(3) if V[3 * t + j] > snap[t]] for t in range(T)}
    now = seq[2][1] + 500
    results = []
    for d, query in ((a, True), (twin, False)):
        m = {}
        b = C.ConflictBatch(d.cs, m)
        b.add_packed(pb)
        if query:
            assert b.read_versions().tolist() == V.tolist()  # the batch's own reads, in read order
            assert b.read_versions(floor=NO_FLOOR).tolist() == check(d.cs, ranges[:3 * T], floor=NO_FLOOR)
        v = b.detect_conflicts(now, oldest)
        results.append((v.tolist(), {t: sorted(x) for t, x in m.items()}))
        b.close()
    v, m = results[0]
    assert len(v) == T and m == want  # conflicting reads are exactly {r : V_r > snapshot}
    assert v == [C.TransactionConflict if want[t] else C.TransactionCommitted for t in range(T)]
    assert 0.3 <= np.mean([bool(want[t]) for t in range(T)]) <= 0.7  # both outcomes, neither vacuous
    assert results[1] == results[0]
    # and the next writing batch
    va, ca = a.detect(*seq[3])
    vt, ct = twin.detect(*seq[3])
    assert (va == vt).all() and ca == ct and a.cs.history_size() == twin.cs.history_size()
    da, dt = a.cs.dump_history(), twin.cs.dump_history()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(da[:3], dt[:3])) and da[3] == dt[3]
    for d in twins:
        d.cs.close()


def test_reads_of_too_old_transactions_have_no_entry(engine, oracle_mod):
    """A transaction that is TooOld when the host adds it carries no ranges: the batch holds the other
    transactions' reads, in order, and the result has exactly their entries, through add_packed and
    through add_transaction; detect afterwards judges the batch as the oracle does."""
    C = engine
    p = Pair(C, oracle_mod, gc_interval=0, delta_limit=1 << 20)
    p.clear(40)
    p.detect(write_batch([(b"b", b"d"), (b"k", b"k\x00")], 100), 100, 90)  # the oldest version is 90 now
    reads = [[(b"a", b"c")], [(b"b", b"b"), (b"c", b"z")], [], [(b"k", b"l"), (b"", b"b")], [(b"d", b"e")]]
    snaps = [95, 50, 10, 89, 100]  # transactions 1 and 3 are TooOld; 2 has no reads, so it is not
    txns = [CommitTransaction([KeyRange(a, e) for a, e in r], [], s, True) for r, s in zip(reads, snaps)]
    held = [r for t in (0, 4) for r in reads[t]]
    want = check(p.cs, held, pair=p)
    assert want == [100, 89]
    for packed in (True, False):
        m = {}
        b = C.ConflictBatch(p.cs, m)
        if packed:
            b.add_packed(PackedBatch.from_transactions(txns))
        else:
            for t in txns:
                b.add_transaction(t)
        too_old = []
        b.get_too_old_transactions(too_old)
        assert too_old == [1, 3]
        got = b.read_versions()
        assert len(got) == len(held) == 2 and got.tolist() == want
        v = b.detect_conflicts(100, 90)
        vo, co = p.o.detect(PackedBatch.from_transactions(txns), 100, 90)
        assert v.tolist() == vo.tolist() == [C.TransactionConflict, C.TransactionTooOld, C.TransactionCommitted,
                                             C.TransactionTooOld, C.TransactionCommitted]
        assert {t: sorted(x) for t, x in m.items()} == co
        b.close()
    p.cs.close()


# ---- 9. device paths

def test_device_paths_and_pending_export(engine, oracle_mod, torch_mod):
    C, torch = engine, torch_mod
    (kb, ko, vers), seq = c2_sequence()
    twins = []
    for _ in range(2):
        d = EngineDriver(C, gc_interval=0, delta_limit=1 << 20)
        d.load_history(kb, ko, vers, 7)
        d.cs.set_oldest_version(95000)
        for pb, now, no in seq[:2]:
            d.detect(pb, now, no)
        twins.append(d)
    a, twin = twins
    pb, now, no = seq[2]
    ranges = [(pb.read_range(r).begin, pb.read_range(r).end) for r in range(pb.n_reads)]
    want = check(twin.cs, ranges, what="host form")
    dump = twin.cs.dump_history()
    raw, off = dump[0].tobytes(), dump[1]
    n = len(dump[2])
    k1, k2 = raw[off[n // 4]:off[n // 4 + 1]], raw[off[n // 2]:off[n // 2 + 1]]
    want_export = twin.cs.dump_history(k1, k2)
    na, nba, hdra = a.cs.export_history(k1, k2)  # pending while the queries run
    # the same arrays through add_packed and add_packed_device
    bh = C.ConflictBatch(a.cs)
    bh.add_packed(pb)
    host = bh.read_versions()
    st = Staged(torch, pb)
    bd = C.ConflictBatch(a.cs)
    bd.add_packed_device(st.dpb)
    dev_added = bd.read_versions()
    assert host.tolist() == dev_added.tolist() == want and st.intact(torch)
    # into a torch tensor, poisoned around the result
    out = torch.full((pb.n_reads + 16,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bd.read_versions_device(out.data_ptr() + 64, pb.n_reads)
    got = out.cpu().numpy()
    assert got[8:8 + pb.n_reads].tolist() == want and (got[:8] == -7).all() and (got[8 + pb.n_reads:] == -7).all()
    bh.read_versions_device(out.data_ptr(), pb.n_reads + 16, floor=NO_FLOOR)
    assert out.cpu().numpy()[:pb.n_reads].tolist() == check(twin.cs, ranges, floor=NO_FLOOR)
    bh.close()
    # the pending export reads back unchanged
    got = a.cs.read_export(na, nba)
    assert hdra == want_export[3] and all((x == y).all() for x, y in zip(got, want_export[:3]))
    # the queried device-added batch detects as its host-added twin
    v = bd.detect_conflicts(now, no)
    vt, _ = twin.detect(pb, now, no)
    assert (v == vt).all()
    bd.close()
    for d in twins:
        d.cs.close()


# ---- 10. statuses

def test_statuses(engine, oracle_mod, torch_mod):
    C, torch = engine, torch_mod
    L = C.load_library()
    out = np.full(64, -7, np.int64)
    po = out.ctypes.data

    def rv(b, cap=64, ptr=po):
        return L.fdbcs_batch_read_versions(b._h, C.NO_FLOOR, ptr, cap)

    cs = C.ConflictSet()
    cs.clear(42)
    rng = np.random.default_rng(8)
    pb = W.random_small_batch(rng, 12, alphabet=3, max_len=3, now=60, staleness=5)
    assert 0 < pb.n_reads <= 64
    # batches in flight on the set; the batch is submitted; the batch is done
    other = C.ConflictBatch(cs)
    other.add_packed(pb)
    b = C.ConflictBatch(cs)
    b.add_packed(pb)
    other.detect_async(60, 50)
    assert rv(b) == C.FDBCS_E_STATE
    assert rv(other) == C.FDBCS_E_STATE
    with pytest.raises(C.FdbcsError) as ei:
        cs.read_versions([(b"a", b"b")])
    assert ei.value.status == C.FDBCS_E_STATE
    other.wait()
    assert rv(other) == C.FDBCS_E_STATE
    other.close()
    # capacity and NULL output; a batch without reads takes both
    assert rv(b, cap=pb.n_reads - 1) == C.FDBCS_E_NOMEM
    assert rv(b, ptr=None) == C.FDBCS_E_INVALID
    assert L.fdbcs_batch_read_versions_device(b._h, 0, None, 64) == C.FDBCS_E_INVALID
    assert (out == -7).all()
    empty = C.ConflictBatch(cs)
    assert rv(empty, cap=0, ptr=None) == C.FDBCS_OK
    empty.close()
    # the refusals left the batch whole: it is queried, then detected, as the oracle says
    assert rv(b) == C.FDBCS_OK and (out[pb.n_reads:] == -7).all()
    o = oracle_mod.OracleConflictSet()
    o.clear(42)
    vo, _ = o.detect(pb, 60, 50)
    vo2, _ = o.detect(pb, 60, 50)
    assert (b.detect_conflicts(60, 50) == vo2).all()
    b.close()
    # a batch that packed a share, and a routed batch
    st = Staged(torch, pb)
    sp = C.ConflictBatch(cs)
    cap = C.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, len(pb.key_bytes))
    buf = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp.share_pack_device(st.dpb, buf.data_ptr(), cap)
    assert rv(sp) == C.FDBCS_E_STATE
    sp.share_pack_info()
    assert rv(sp) == C.FDBCS_E_STATE
    sp.close()
    share = C.share_pack(pb)
    stride = (len(share) + 255) // 256 * 256
    host = np.zeros(stride, np.uint8)
    host[:len(share)] = share
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    rt = C.ConflictBatch(cs)
    rt.add_routed(dev.data_ptr(), stride, 1, pb.n_txn, None, None, (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes))
    assert rv(rt) == C.FDBCS_E_STATE
    rt.routed_info()
    assert rv(rt) == C.FDBCS_E_STATE
    rt.close()
    # a malformed device-added batch: FDBCS_E_INVALID, and the batch is empty again, as after a failed detect
    k = keys_of(pb)
    r = next(i for i in range(pb.n_reads) if k[2 * i] < k[2 * i + 1])
    k[2 * r], k[2 * r + 1] = k[2 * r + 1], k[2 * r]
    bad = Staged(torch, repack(pb, keys=k))
    mb = C.ConflictBatch(cs)
    mb.add_packed_device(bad.dpb)
    assert rv(mb) == C.FDBCS_E_INVALID
    mb.add_packed_device(st.dpb)  # the same object takes a valid add and answers
    assert mb.read_versions().tolist() == cs.read_versions([(pb.read_range(i).begin, pb.read_range(i).end)
                                                            for i in range(pb.n_reads)]).tolist()
    mb2 = C.ConflictBatch(cs)
    mb2.add_packed_device(bad.dpb)
    with pytest.raises(C.FdbcsError) as ei:
        mb2.read_versions()
    assert ei.value.status == C.FDBCS_E_INVALID and mb2.transaction_count == 0
    mb2.close()
    # the batch's set is gone
    mb.cs = None
    cs.close()
    assert rv(mb) == C.FDBCS_E_STATE
    a, c = ctypes.c_double(), ctypes.c_double()
    assert L.fdbcs_batch_read_versions_timing(mb._h, ctypes.byref(a), ctypes.byref(c)) == C.FDBCS_E_STATE
    mb.close()
