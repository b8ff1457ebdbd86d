"""GPU tests of ConflictSet.verify (fdbcs_history_verify): clean reports with the examined counts the
sizes imply in every state the engine's builders leave (load, merges into both delta buffers,
compaction, GC, both imports, clear, the directory knobs), and, through the what-if override, that
every check class bites: the device report equals tests/verify_model.py's, field for field, in every
class but DIR and EDIR, for overrides at the first, last and block-edge elements of every array.
Nothing here writes into a set's arrays."""
import numpy as np
import pytest

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from tests import verify_model as M
from tests.tier_model import TierSim, union_segments

pytestmark = pytest.mark.gpu

HDR = 7
BIG_N = 262144 + 4096 + 64 + 9  # two level-3 entries and a partial block at every level
SIGN = 1 << 63
CI = M.CLASSES.index


def arrays(keys):
    ko = np.zeros(len(keys) + 1, np.int64)
    ko[1:] = np.cumsum([len(k) for k in keys])
    return np.frombuffer(b"".join(keys) + b"\0", np.uint8), ko  # (a spare byte: the empty key alone has no bytes to point at)


def loaded(C, keys, vers, header=HDR):
    cs = C.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(1 << 22)
    cs.load_history(*arrays(keys), np.asarray(vers, np.int64), header)
    return cs


def write_batch(cs, C, ranges, now, oldest=0):
    """One transaction that writes `ranges` and reads nothing: it always commits."""
    b = C.ConflictBatch(cs)
    b.add_packed(PackedBatch.from_transactions([CommitTransaction([], [KeyRange(a, e) for a, e in ranges], now, False)]))
    v = b.detect_conflicts(now, oldest)
    b.close()
    assert list(v) == [C.TransactionCommitted]


def modelled(rep):
    return [[rep.rows[t][CI(c)] for c in M.MODELLED] for t in range(2)]


def of_model(rows):
    return [[rows[t][CI(c)] for c in M.MODELLED] for t in range(2)]


def assert_clean(rep, n_long=None, what=None):
    """No violation anywhere, and per tier the examined counts its size implies."""
    assert rep.ok, (what, rep)
    for tier in range(2):
        n = rep.sizes[tier]
        want = M.expected_examined(n, rep.examined(tier, "tails") if n_long is None else n_long[tier], tier)
        got = {k: rep.examined(tier, k) for k in want}
        assert got == want, (what, tier)
        assert all(rep.first(tier, c) == -1 for c in range(len(M.CLASSES)))
    assert rep.examined(1, "edir") == rep.edir_trusted


# ---- clean states over every size around a block edge

@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097])
def test_clean_after_load_and_a_batch(engine, n):
    C = engine
    rng = np.random.default_rng(n)
    keys = M.make_keys(rng, n + 40)
    extra = set(int(x) for x in rng.choice(len(keys), size=40, replace=False)) - {0}
    base = [k for i, k in enumerate(keys) if i not in extra][:n]
    cs = loaded(C, base, rng.integers(10, 1000, size=n))
    n_long = sum(len(k) > 16 for k in base)
    rep = cs.verify()
    assert rep.sizes == (n, 0)
    assert_clean(rep, (n_long, 0), n)
    assert rep.examined(0, "dir") >= 3 if n else rep.examined(0, "dir") == 0
    assert rep.examined(1, "dominance") == 0 and rep.edir_trusted == 0
    ms_kernels, ms_host = cs.verify_timing()
    assert ms_host >= ms_kernels >= 0
    # a delta with holes over it: ranges between keys the base does not hold
    ex = sorted(extra)
    ranges = [(keys[a], keys[a] + b"\xff") for a in ex[::2]]
    write_batch(cs, C, ranges, 5000)
    rep = cs.verify()
    assert rep.sizes[0] == n and rep.sizes[1] == cs.history_size() - n > 0
    assert_clean(rep, None, (n, "delta"))
    assert rep.examined(1, "dominance") > 0
    cs.clear(99)
    rep = cs.verify()
    assert rep.sizes == (0, 0) and rep.ok and rep.as_dict()["tiers"][0]["order"] == dict(examined=0, violations=0, first=-1)
    assert all(r == (0, 0, -1) for t in rep.rows for r in t) and rep.edir_trusted == 0
    cs.close()


# ---- the state sequence on a small set, the delta predicted by TierSim

class Small:
    """5000 loaded boundaries out of a universe of 6000 keys, and two write batches that leave a delta
    with holes (both delta buffers have been current), stored as TierSim says."""

    def __init__(self, C):
        rng = np.random.default_rng(11)
        self.U = U = M.make_keys(rng, 6000)
        out = set(int(x) for x in rng.choice(len(U), size=1000, replace=False)) - {0}
        self.bidx = [i for i in range(len(U)) if i not in out]
        self.bvers = rng.integers(100, 1000, size=len(self.bidx))
        self.sim = TierSim(HDR)
        self.sim.load(self.bidx, self.bvers, HDR)
        self.cs = loaded(C, [U[i] for i in self.bidx], self.bvers)
        self.C, self.rng, self.now = C, rng, 5000

    def batch(self, n_ranges, oldest=0):
        starts = np.sort(self.rng.choice(len(self.U) - 8, size=n_ranges, replace=False))
        writes = [(int(a), int(a) + int(self.rng.integers(1, 7))) for a in starts]
        self.now += 1
        write_batch(self.cs, self.C, [(self.U[a], self.U[b]) for a, b in writes], self.now, oldest)
        self.sim.merge(union_segments(writes), self.now)

    def model(self):
        dv = [M.HOLE if v is None else v for v in self.sim.dv]
        return M.build([self.U[i] for i in self.sim.bk], self.sim.bv, [self.U[i] for i in self.sim.dk], dv, HDR)


@pytest.fixture(scope="module")
def small(engine):
    s = Small(engine)
    s.batch(300)
    s.batch(200)
    s.state = s.model()
    s.clean_rows = M.verify(s.state)
    yield s
    s.cs.close()


def test_delta_with_holes_is_clean_and_equals_the_model(small):
    rep = small.cs.verify()
    st = small.state
    assert rep.sizes == (st.tiers[0].n, st.tiers[1].n)
    assert (st.tiers[1].ver == M.HOLE).sum() > 50 and (st.tiers[1].ver != M.HOLE).sum() > 300
    assert M.clean(small.clean_rows)
    assert_clean(rep, None, "delta")
    assert modelled(rep) == of_model(small.clean_rows)
    assert rep.edir_trusted > 0 and rep.examined(0, "dir") > 3
    # a subset of classes examines only those
    part = small.cs.verify(checks=("lvl1", "dominance"))
    assert [c for c in M.CLASSES if part.examined(1, c)] == ["dominance", "lvl1"]
    assert small.cs.verify(checks=1 << CI("order")).examined(0, "order") == st.tiers[0].n - 1


def delta_overrides(st):
    d = st.tiers[1]
    yield "lvl1", 0, 4, 0, 0
    yield "lvl1", len(d.lvl1) - 1, 4, 0, 0
    yield "lvl2", 0, 1 << 20, 0, 0
    yield "skey8", len(d.skey8[0]) - 1, 0, 1, 0
    yield "skey", len(d.skey[0][0]) - 1, 1, 0, 0
    yield "skey", 0, 1, 0, 3


def test_every_class_bites_on_the_delta(small):
    C, cs, st = small.C, small.cs, small.state
    for what, idx, lo, hi, level in delta_overrides(st):
        rep = cs.verify(override=C.VerifyOverride(what, 1, idx, lo, hi, level))
        want_first = idx if what != "skey" else level << 48 | idx
        bad = [(t, M.CLASSES[c], r[1], r[2]) for t in range(2) for c, r in enumerate(rep.rows[t]) if r[1]]
        assert bad == [(1, what, 1, want_first)], (what, idx, bad)
        assert modelled(rep) == of_model(M.verify(st, (what, 1, idx, lo, hi, level), order_clean=True))
    # a level-3 replica: of the two masks one raises it above every version (test_lvl3_replica_overrides)
    flags = [cs.verify(override=C.VerifyOverride("lvl3", 1, 0, m)) for m in (1 << 62, 3 << 62)]
    assert sum(not r.ok for r in flags) >= 1
    for r in flags:
        assert r.ok or [(t, c) for t in range(2) for c, x in enumerate(r.rows[t]) if x[1]] == [(1, CI("lvl3"))]
    # a versioned boundary lowered below the base version it covers
    d = st.tiers[1]
    j = next(k for k in range(10, d.n) if int(d.ver[k]) != M.HOLE)
    ov = ("version", 1, j, int(d.ver[j]) ^ 1, 0)  # -> 1, below every loaded version
    rep = cs.verify(override=C.VerifyOverride(*ov))
    assert rep.violations(1, "dominance") >= 1 and rep.first(1, "dominance") == j
    assert modelled(rep) == of_model(M.verify(st, ov, order_clean=True))
    # delta directory: a trusted entry flags exactly its slot, an untrusted one nothing
    clean = cs.verify(checks=("edir",))
    assert clean.ok and clean.examined(1, "edir") == clean.edir_trusted > 0
    rep = cs.verify(checks=("edir",), override=C.VerifyOverride("edir", 1, 0, 1))
    assert (rep.violations(1, "edir"), rep.first(1, "edir")) == (1, 0)  # slot 0 is always written by the first start
    # flipping a tag bit makes the entry another epoch's: one trusted entry fewer, nothing flagged
    rep = cs.verify(checks=("edir",), override=C.VerifyOverride("edir", 1, 0, 1 << 32))
    assert rep.ok and rep.edir_trusted == clean.edir_trusted - 1


def test_clean_through_compaction_gc_imports_and_clear(engine):
    C = engine
    s = Small(C)
    s.batch(300)
    s.batch(200)
    before = s.cs.stats()
    s.cs.set_gc_interval(1)  # every batch compacts, and collects garbage once the oldest version moved
    s.batch(100, oldest=600)
    after = s.cs.stats()
    assert after["compactions"] > before["compactions"] and after["gc_runs"] > before["gc_runs"]
    rep = s.cs.verify()
    assert rep.sizes[1] == 0 and 0 < rep.sizes[0] == s.cs.history_size()
    assert rep.examined(0, "tails") > 100  # long keys survived the repack
    assert_clean(rep, None, "compaction + gc")
    s.cs.set_gc_interval(0)
    s.batch(150, oldest=600)
    assert_clean(s.cs.verify(), None, "delta over the compacted base")
    # the two imports, from a set with other versions over the same keys
    src = loaded(C, [s.U[i] for i in s.bidx], s.bvers + 3000)  # above the loaded versions, below every batch's
    dump = src.dump_history(s.U[1000], s.U[3000], M.HOLE)
    s.cs.merge_history(*dump, lo=s.U[1000], hi=s.U[3000])
    assert s.cs.import_info()["path"] == 0
    assert_clean(s.cs.verify(), None, "fold")
    s.batch(120, oldest=600)
    dump = src.dump_history(s.U[3500], s.U[5000], M.HOLE)
    s.cs.merge_history(*dump, lo=s.U[3500], hi=s.U[5000], into="delta")
    assert s.cs.import_info()["path"] == 1
    rep = s.cs.verify()
    assert rep.sizes[1] > 100
    assert_clean(rep, None, "delta import")
    src.close()
    s.cs.clear(1)
    assert s.cs.verify().ok
    s.cs.close()


@pytest.mark.parametrize("knobs", [{"FDBCS_DIR_BITS": "8"}, {"FDBCS_DIR_BITS": "20"}, {"FDBCS_DIRECTORY": "0"}],
                         ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_directory_knobs(engine, monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    s = Small(engine)
    s.batch(300)
    s.batch(200)
    rep = s.cs.verify()
    assert_clean(rep, None, knobs)
    if "FDBCS_DIRECTORY" in knobs:
        assert rep.examined(0, "dir") == 0
    else:
        assert 3 <= rep.examined(0, "dir") <= (1 << int(knobs["FDBCS_DIR_BITS"])) + 4
        rep = s.cs.verify(checks=("dir",), override=engine.VerifyOverride("dir", 0, 2, 1))
        assert (rep.violations(0, "dir"), rep.first(0, "dir")) == (1, 2)
    s.cs.close()


# ---- every class bites on the base: 266313 boundaries right after the load

@pytest.fixture(scope="module")
def big(engine):
    rng = np.random.default_rng(266313)
    keys = M.make_keys(rng, BIG_N)
    vers = rng.integers(1000, 10 ** 6, size=BIG_N)
    vers[264000] = 10 ** 9  # the only maximum of the second level-3 entry, deep inside it
    cs = loaded(engine, keys, vers)
    st = M.build(keys, vers, header=HDR)
    assert M.clean(M.verify(st))
    yield engine, cs, st
    cs.close()


EDGES = [0, 63, 64, 4095, 4096, 262143, 262144, BIG_N - 1]


def test_big_set_is_clean(big):
    C, cs, st = big
    rep = cs.verify()
    assert rep.sizes == (BIG_N, 0)
    assert_clean(rep, (int((st.tiers[0].ln > 16).sum()), 0), "big")
    assert rep.examined(0, "lvl3") == 2 and rep.examined(0, "lvl2") == 66
    assert modelled(rep) == of_model(M.verify(st))


def same(big, ov, skip=()):
    """The device report under override `ov` equals the model's in every modelled class."""
    C, cs, st = big
    rep = cs.verify(override=C.VerifyOverride(*ov))
    rows = M.verify(st, ov, order_clean=True)
    for t in range(2):
        for c in M.MODELLED:
            if c not in skip:
                assert rep.rows[t][CI(c)] == rows[t][CI(c)], (ov, t, c)
    return rep


def test_key_and_len_tail_overrides(big):
    C, cs, st = big
    base = st.tiers[0]
    for e in EDGES:
        group_start = e % 8 == 0
        for lo, hi in ((1, 0), (0, 1 << 40), (1 << 63, 1 << 63)):
            rep = same(big, ("key", 0, e, lo, hi))
            assert group_start == (rep.violations(0, "skey8") == 1)
        i = e + 1 if group_start and e + 1 < BIG_N else e  # and beside it, where no sample reads the key
        rep = same(big, ("key", 0, i, 0, 1 << 40))
        assert i % 8 == 0 or rep.violations(0, "skey8") + rep.violations(0, "skey") + rep.violations(0, "dir") == 0
        same(big, ("len_tail", 0, e, 1, 0))
        same(big, ("len_tail", 0, e, 32, 0))
    # a tail sent past tail_used: TAILS at that key, the pair's order not judged; the call returns
    i = next(k for k in range(1000, BIG_N) if int(base.ln[k]) == 113)
    far = (st.tail_used // 8) ^ int(base.tu[i])
    rep = same(big, ("len_tail", 0, i, 0, far))
    assert (rep.violations(0, "tails"), rep.first(0, "tails")) == (1, i)
    rep = same(big, ("len_tail", 0, i, 0, 0xFFFFFFFF ^ int(base.tu[i])))  # the largest unit there is
    assert (rep.violations(0, "tails"), rep.first(0, "tails")) == (1, i)
    # tail words: the first and last of the arena, and the first word of a tail that decides an order
    words = st.tail_used // 8
    tie = np.flatnonzero((base.hi[:-1] == base.hi[1:]) & (base.lo[:-1] == base.lo[1:]) & (base.ln[:-1] > 16)
                         & (base.ln[1:] > 16))
    w = int(base.tu[int(tie[len(tie) // 2]) + 1])
    for word, mask in ((0, 0xFF), (words - 1, 0xFF), (w, int(st.arena[w]) & 0xFF)):
        same(big, ("tail_word", 0, word, mask))
    assert not same(big, ("tail_word", 0, w, int(st.arena[w]) & 0xFF)).ok


def test_version_overrides(big):
    C, cs, st = big
    base = st.tiers[0]
    for e in EDGES:
        # the new maximum of everything above it: exactly one entry of each level
        rep = same(big, ("version", 0, e, 1 << 40))
        assert [(rep.violations(0, c), rep.first(0, c)) for c in ("lvl1", "lvl2", "lvl3")] == \
            [(1, e // 64), (1, e // 4096), (1, e // 262144)]
        # lowered: the model decides whether the element was its block's only maximum
        v = int(base.ver[e])
        same(big, ("version", 0, e, v ^ (v >> 1)))
        rep = same(big, ("version", 0, e, v ^ SIGN))  # a hole in the base
        assert (rep.violations(0, "versions"), rep.first(0, "versions")) == (1, e)
    blk = base.ver[:64]
    low = int(np.argmin(blk))
    assert same(big, ("version", 0, low, int(blk[low]) ^ 1)).ok  # a non-maximum lowered to 1: nothing
    rep = same(big, ("version", 0, 264000, 10 ** 9 ^ 1000))  # the second level-3 entry's only maximum lowered to 1000
    assert [(rep.violations(0, c), rep.first(0, c)) for c in ("lvl1", "lvl2", "lvl3")] == \
        [(1, 264000 // 64), (1, 264000 // 4096), (1, 1)]


def test_level_and_sample_overrides(big):
    C, cs, st = big
    for e in EDGES:
        for what, span in (("lvl1", 64), ("lvl2", 4096), ("skey8", 8)):
            rep = same(big, (what, 0, e // span, 2, 0))
            assert (rep.violations(0, what), rep.first(0, what)) == (1, e // span)
        for L in (0, 1, 4, 11):
            d = e // (64 * 8 ** L)
            rep = same(big, ("skey", 0, d, 0, 1 << 50, L))
            assert (rep.violations(0, "skey"), rep.first(0, "skey")) == (1, L << 48 | d)


def test_lvl3_replica_overrides(big):
    """Which replica the epilogue's workgroups wrote is theirs to choose, so the replicas are probed
    by what-ifs alone.  M1 raises a replica that holds a version (below 2^62) above every version and
    lowers an empty one (INT64_MIN) further below; M2 does the opposite.  So for every replica exactly
    one of the two raises it above the maximum, which must flag the entry, and the other lowers it,
    which flags the entry iff the replica is the only one that holds the maximum."""
    C, cs, st = big
    M1, M2 = 1 << 62, 3 << 62
    for j in range(2):
        sole = 0
        for r in range(8):
            flags = []
            for mask in (M1, M2):
                rep = cs.verify(checks=("lvl3",), override=C.VerifyOverride("lvl3", 0, 8 * j + r, mask))
                assert rep.violations(0, "lvl3") in (0, 1) and rep.first(0, "lvl3") in (-1, j)
                flags.append(rep.violations(0, "lvl3"))
            assert sum(flags) >= 1, (j, r)
            sole += sum(flags) == 2
        assert sole <= 1


def test_dir_overrides(big):
    C, cs, st = big
    clean = cs.verify(checks=("dir",))
    slots = clean.examined(0, "dir")
    assert clean.ok and slots > 1000  # the family's digits spread over many slots
    for v in (0, 1, slots // 2, slots - 1):
        rep = cs.verify(checks=("dir",), override=C.VerifyOverride("dir", 0, v, 1))
        assert (rep.violations(0, "dir"), rep.first(0, "dir")) == (1, v)
    rep = cs.verify(checks=("dir",), override=C.VerifyOverride("dir", 0, slots // 2, SIGN >> 32))  # a negative count
    assert (rep.violations(0, "dir"), rep.first(0, "dir")) == (1, slots // 2)


# ---- errors and side effects

def test_errors_and_side_effects(engine):
    C = engine
    base = C.live_resources()
    s = Small(C)
    cs = s.cs
    # a pending export stays readable
    n, nb, hdr = cs.export_history()
    rep = cs.verify()
    assert rep.ok
    kb, ko, vv = cs.read_export(n, nb)
    assert 0 < len(vv) == n <= len(s.bidx)
    # overrides outside the arrays
    for ov in (("key", 0, len(s.bidx), 1), ("key", 1, 0, 1), ("lvl3", 0, 8, 1), ("skey", 0, 1, 1, 0, 12),
               ("edir", 0, 0, 1), ("dir", 1, 0, 1), ("tail_word", 0, 1 << 40, 1), ("version", 2, 0, 1), ("key", 0, -1, 1)):
        with pytest.raises(C.FdbcsError) as e:
            cs.verify(override=C.VerifyOverride(*ov))
        assert e.value.status == C.FDBCS_E_INVALID, ov
    with pytest.raises(C.FdbcsError) as e:
        cs.verify(checks=1 << 12)
    assert e.value.status == C.FDBCS_E_INVALID
    # a batch in flight
    b = C.ConflictBatch(cs)
    b.add_packed(PackedBatch.from_transactions([CommitTransaction([KeyRange(s.U[5], s.U[9])], [KeyRange(s.U[5], s.U[6])],
                                                                  10 ** 6, False)]))
    b.detect_async(6000, 0)
    with pytest.raises(C.FdbcsError) as e:
        cs.verify()
    assert e.value.status == C.FDBCS_E_STATE
    assert list(b.wait()) == [C.TransactionCommitted]
    b.close()
    assert cs.verify().ok
    cs.close()
    assert C.live_resources() == base


def test_verdicts_after_a_verify_equal_those_without(engine):
    C = engine
    got = []
    for with_verify in (False, True):
        s = Small(C)
        s.batch(300)
        if with_verify:
            assert s.cs.verify().ok
            assert not s.cs.verify(override=C.VerifyOverride("version", 0, 5, 1 << 40)).ok
        rng = np.random.default_rng(5)
        txns = []
        for _ in range(400):
            a = int(rng.integers(0, len(s.U) - 10))
            txns.append(CommitTransaction([KeyRange(s.U[a], s.U[a + 3])], [KeyRange(s.U[a + 1], s.U[a + 2])],
                                          int(rng.integers(0, 6000)), False))
        b = C.ConflictBatch(s.cs)
        b.add_packed(PackedBatch.from_transactions(txns))
        got.append(b.detect_conflicts(7000, 0).copy())
        b.close()
        assert s.cs.verify().ok
        s.cs.close()
    assert 0 < (got[0] == C.TransactionCommitted).sum() < len(got[0])
    assert (got[0] == got[1]).all()
