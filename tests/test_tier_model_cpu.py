"""tests/tier_model.TierSim held against things it shares nothing with, and the coverage and the
sensitivity of the directed plan of tests/merge_plan.py (no GPU: the engine is never consulted).

  raw boundary set   the folded tiers against the semantic oracle's dump, boundary for boundary (not
                     canonical), after every batch of random multi-range batches under delta limits that
                     compact every 1, 3 and 7 batches or so, and after every plan step until a GC drops
                     something;
  with GC            against the oracle's full removeBefore pass.  The oracle starts wasAbove = true, as
                     SkipList.cpp:546 does, so it keeps the first boundary whatever its version; the
                     engine's gc_keep (and TierSim) compares boundary 0 with the header version and
                     drops it when both are below the floor.  Raw sizes are held where the two agree,
                     and up to that one boundary elsewhere; the canonical form everywhere;
  canonical form     TierSim's step function, run-length encoded and clamped, against KeyspaceModel after
                     every batch (merge_plan.Plan.step asserts it for every plan step);
  a wrong merge      fifteen mutants of TierSim, one rule off each: wherever a family reaches a mutant's
  cannot pass        rule, some quantity the GPU test asserts differs from the true model's."""
import os
import re

import numpy as np
import pytest

from tests import keyspace_model as K
from tests import merge_plan as MP
from tests import tier_model as TM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foundationdb_amd", "csrc")


def rand_batch(rng, U, now, n):
    """Multi-range transactions over a tiny universe: touching, nested and empty ranges, snapshots that
    straddle the oldest version (TooOld) and the recent writes (aborted writers)."""
    tb = K.TxnBatch()

    def rg():
        a = int(rng.integers(0, U))
        if rng.random() < 0.15:
            return a, a
        return a, min(U - 1, a + int(rng.integers(1, 5)))

    for _ in range(n):
        tb.add(reads=[rg() for _ in range(int(rng.integers(0, 3)))], writes=[rg() for _ in range(int(rng.integers(0, 4)))],
               snap=int(now - rng.integers(1, 14)))
    return tb


def tiny_universe(rng, U):
    keys = set()
    while len(keys) < U:
        keys.add(bytes(rng.integers(0, 3, size=int(rng.integers(0, 5))).astype(np.uint8)))
    return K.KeyspaceModel(K.var_universe(keys), 0)


def raw_of(model, sim):
    ks = K.split_keys(model.kb, model.ko)
    bk, bv = sim.folded()
    return [ks[j] for j in bk], [int(v) for v in bv]


@pytest.mark.parametrize("U,limit", [(6, 1), (17, 12), (40, 40)])
def test_raw_boundaries_random(oracle_built, U, limit):
    """100 random batches per delta limit (compactions every 1, 2-3 and 6-7 batches), no GC: TierSim's
    folded tiers equal the oracle's raw boundaries under the reference's sweep (empty writes split a
    span), and the engine's sweep (they do not) differs from it by boundaries that repeat the version
    before them and by nothing else."""
    rng = np.random.default_rng(U)
    model = tiny_universe(rng, U)
    sim, eng = TM.TierSim(0, limit), TM.TierSim(0, limit)
    orc = oracle_built.OracleConflictSet()
    now, extra = 20, 0
    for i in range(100):
        tb = rand_batch(rng, U, now, int(rng.integers(1, 12)))
        other = K.KeyspaceModel((model.kb, model.ko), 0)
        other.ver = model.ver.copy()
        res, f = TM.run_batch(model, sim, tb, now, 0, empty_splits=True)
        TM.run_batch(other, eng, tb, now, 0)
        v, _ = orc.detect(tb.pack(model), now, 0, gc=False)
        assert (v == res.verdicts).all(), i
        ok, ov = orc.dump_history()
        assert raw_of(model, sim) == (ok, ov.tolist()), i
        for a, b in zip(sim.canonical(U), eng.canonical(U)):
            assert np.array_equal(a, b)
        hdr, s, vv = sim.canonical(U)
        assert np.array_equal(s, model.boundaries()) and np.array_equal(vv, model.ver[s])
        ek, ev = raw_of(model, eng)
        assert set(ek) <= set(ok)
        extra += len(ok) - len(ek)
        now += 3
    st = sim.stats
    assert st["compactions"] >= 100 // (limit // 5 + 1) - 5 and st["gc_runs"] == 0, st
    assert extra > 0  # (the empty-write split is reached)


def test_gc_first_boundary(oracle_built):
    """The one place gc_keep and the reference differ: a first boundary below the floor under a header
    below the floor.  SkipList.cpp:546 starts every removeBefore pass with wasAbove = true, so the
    reference (and the oracle) keeps the first node it meets; gc_keep compares boundary 0 with the
    header version and drops it.  Both read floor - 1 there: the canonical forms agree."""
    model = K.KeyspaceModel(K.var_universe({b"a", b"b", b"c", b"d"}), 10)
    idx, vers = np.array([0, 1, 3]), np.array([50, 200, 60])
    kb, ko = model.pack_keys(idx)
    orc = oracle_built.OracleConflictSet()
    orc.load_history(kb, ko, vers, 10)
    sim = TM.TierSim(10, 0, 1)
    sim.load(idx, vers, 10)
    model.load(idx, vers)
    tb = K.TxnBatch()
    tb.add(reads=[(0, 1)], snap=300)
    orc.detect(tb.pack(model), 400, 100, gc=True)
    f = sim.batch(0, [], 400, 100)
    assert f.gc.dropped == [0]
    keys, ov = orc.dump_history()
    assert keys == [b"a", b"b", b"d"] and ov.tolist() == [50, 200, 60]  # the reference's behaviour
    assert raw_of(model, sim) == ([b"b", b"d"], [200, 60])  # gc_keep's
    assert [x.tolist() if hasattr(x, "tolist") else x for x in sim.canonical(4, 100)] == [99, [1, 3], [200, 99]]


def test_raw_boundaries_random_gc(oracle_built):
    """Random batches with the oldest version following ten versions behind and a compaction with GC
    at every batch, against the oracle's full pass: equal, or equal up to the oracle's first boundary
    where that one is below the floor under a header below the floor (and up to the version, below the
    floor either way, that a later end boundary inherits from there)."""
    U = 23
    rng = np.random.default_rng(3)
    model = tiny_universe(rng, U)
    sim = TM.TierSim(0, 0, 1)
    orc = oracle_built.OracleConflictSet()
    now, agree, differ = 20, 0, 0
    for i in range(100):
        tb = rand_batch(rng, U, now, int(rng.integers(1, 12)))
        res, f = TM.run_batch(model, sim, tb, now, now - 10, empty_splits=True)
        v, _ = orc.detect(tb.pack(model), now, now - 10, gc=True)
        assert (v == res.verdicts).all(), i
        ok, ov = orc.dump_history()
        mine, theirs = raw_of(model, sim), (ok, ov.tolist())
        if mine == theirs:
            agree += 1
        else:  # the oracle's first boundary alone, and what later ends inherited from it: all below the floor
            cl = lambda vs: [v if v >= sim.oldest else sim.oldest - 1 for v in vs]
            if len(theirs[0]) > len(mine[0]):
                assert theirs[1][0] < sim.oldest and sim.header < sim.oldest, i
                theirs = theirs[0][1:], theirs[1][1:]
            assert mine[0] == theirs[0] and cl(mine[1]) == cl(theirs[1]), i
            differ += 1
        hdr, s, vv = sim.canonical(U, sim.oldest)
        ver = np.where(model.ver >= sim.oldest, model.ver, sim.oldest - 1)
        b = np.flatnonzero(ver != np.concatenate([[sim.oldest - 1], ver[:-1]]))
        assert hdr == sim.oldest - 1 and np.array_equal(s, b) and np.array_equal(vv, ver[b]), i
        now += 3
    assert agree >= 5 and differ >= 5 and sim.stats["gc_runs"] == 100, (agree, differ)


# ---------------------------------------------------------------------------------- the plans


def oracle_replay(oracle, plan):
    """The plan's batches through the semantic oracle: its verdicts against the plan's expected ones,
    and TierSim's folded tiers against its raw dump after every step until a GC drops something."""
    orc = oracle.OracleConflictSet()
    if plan.loaded is not None:
        orc.load_history(*plan.loaded)
    else:
        orc.clear(plan.header0)
    orc.set_oldest_version(plan.first_oldest)
    cleared, keys = dict(plan.cleared), plan.uni.keys
    skip = {keys[k] for k in plan.empty_writes}
    raw_steps = 0
    dropped = False
    for i, st in enumerate(plan.steps):
        if i in cleared:
            orc.clear(cleared[i])
            dropped = False
        v, _ = orc.detect(st.pb, st.now, st.new_oldest, gc=False)
        assert (v == st.want).all(), (plan.name, st.name, np.flatnonzero(v != st.want)[:5])
        dropped |= st.gc_dropped > 0
        if dropped:
            continue
        ok, ov = orc.dump_history()
        bk, bv = st.raw
        mine = {keys[j] for j in bk.tolist()} if skip else ()
        keep = [j for j, k in enumerate(ok) if k not in skip or k in mine]  # (the split at an empty write alone)
        assert [ok[j] for j in keep] == [keys[j] for j in bk.tolist()], (plan.name, st.name)
        assert ov[keep].tolist() == bv.tolist(), (plan.name, st.name)
        raw_steps += 1
    return raw_steps


@pytest.mark.parametrize("layout", MP.LAYOUTS)
def test_plans_against_oracle(oracle_built, layout):
    """Every family under every layout: building it asserts its coverage (merge_plan); the oracle confirms
    every expected verdict and every raw boundary set.  (The wide layout: the families whose batches are
    few.)"""
    fams = MP.ALL_FAMILIES + (("tails", "clear-reuse") if layout == "long" else ("clear-reuse",))
    if layout == "wide":
        fams = ("segment-tiles", "glue-exact", "compaction", "gc", "single-rider")
    total = 0
    for fam in fams:
        for plan in MP.build(fam, layout):
            total += oracle_replay(oracle_built, plan)
    assert total >= 50


def test_plan_coverage():
    """What the plan reaches, layout by layout (each family's own assertions ran when it was built)."""
    for layout in MP.LAYOUTS:
        sp = MP.SEG_PER[layout]
        for fam in MP.ALL_FAMILIES:
            plans = MP.build(fam, layout)
            for p in plans:
                reads = [s for s in p.steps if s.kind == "read"]
                assert reads and all((s.want == K.CONFLICT).mean() >= 0.3 and (s.want == K.COMMITTED).mean() >= 0.3 for s in reads)
                longest = max(int(np.diff(s.pb.key_offsets).max()) for s in p.steps)
                assert (longest > 24) == (layout == "long")
                assert all((s.pb.n_writes >= MP.N_RIDER) == (layout == "wide") for s in p.steps if s.kind == "write")
        us = MP.build("segment-tiles", layout)[0].coverage["segment-tiles"]["U"]
        assert {sp - 1, sp, sp + 1, 2 * sp - 1, 2 * sp, 2 * sp + 1} <= set(us)
        assert layout == "wide" or {0, 1, 3 * sp} <= set(us)
        assert MP.build("epilogue-delta", layout)[0].coverage["epilogue-delta"]["sizes"] == list(MP.EPI_SIZES)
    headers = {p.coverage["compaction"]["header"] for lay in MP.LAYOUTS for p in MP.build("compaction", lay)}
    assert len(headers) == 2  # holes below the first base boundary under two header versions


def test_constants_match_the_sources():
    """The constants the models restate, read out of the sources: a changed tile, threshold or cadence
    fails here, and the plan's sizes are then placed anew."""
    def const(path, name):
        src = open(os.path.join(CSRC, path)).read()
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert m, (path, name)
        return int(m.group(1))

    assert MP.SCAN_TILE == const("scan.h", "kScanThreads") * const("scan.h", "kScanPer")
    assert re.search(r"constexpr int kScanTile = kScanThreads \* kScanPer;", open(os.path.join(CSRC, "scan.h")).read())
    assert TM.GC_EVERY == const("engine_impl.h", "kGcEveryCompactions")
    assert TM.DELTA_TILE == const("kernels.hip", "kDeltaTile") and TM.SEG_LDS == const("kernels.hip", "kSegLds")
    assert MP.N_RIDER == const("kernels.hip", "kSegWideMinW")
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    m = re.search(r"seg_per\(bool long_keys, bool wide\) \{ return long_keys \|\| !wide \? (\d+) : (\d+); \}", kernels)
    assert m and (int(m.group(1)), int(m.group(2))) == (MP.SEG_PER["narrow"], MP.SEG_PER["wide"])
    assert MP.SEG_PER["long"] == int(m.group(1))
    engine = open(os.path.join(CSRC, "engine.cpp")).read()
    m = re.search(r"cs->n_ub <= \(16 << 20\) \? (\d+) : 4096", engine)  # the compaction's copy tile of a small base
    assert m and int(m.group(1)) == TM.BASE_TILE
    m = re.search(r"std::max<int64_t>\(\{\(int64_t\)1 << (\d+), n_base / 16", engine)  # delta_limit_for()
    assert m and 1 << int(m.group(1)) == TM.DEFAULT_DELTA_LIMIT


# ---------------------------------------------------------------------------------- mutants


def replay_mutant(plan, mutant):
    """The plan's batches through a TierSim with one rule off.  Returns (times the rule was reached, steps
    at which a size or a counter differs from the true model's, steps at which a read verdict or a
    canonical dump at either floor differs)."""
    sim = TM.TierSim(plan.header0, plan.delta_limit, 0, mutant)
    sim.oldest = plan.first_oldest
    if plan.loaded_idx is not None:
        sim.load(plan.loaded_idx, plan.loaded[2], plan.loaded[3])
    cleared, U = dict(plan.cleared), plan.uni.U
    sizes = seen = 0
    for i, st in enumerate(plan.steps):
        if i in cleared:
            sim.clear(cleared[i])
        if st.gc_interval is not None:
            sim.gc_interval = st.gc_interval
        if st.kind == "read" and st.dump is not None:  # the check reads the state before the batch's own Y half
            m = K.KeyspaceModel((plan.uni.kb, plan.uni.ko), sim.header)
            m.ver = sim.versions(U)
            a, b, snap = st.reads
            got = np.where(m.read_max(a, b) > snap, K.CONFLICT, K.COMMITTED)
            seen += int((got != st.want).any())
        f = sim.batch(st.replay[0], st.replay[1], st.now, st.new_oldest)
        sizes += plan.expect(f) != st.expect
        if st.dump is not None:
            for floor, want in zip((sim.oldest, None), st.dump):
                hdr, s, vv = sim.canonical(U, floor)
                same = hdr == want[0] and np.array_equal(vv, want[3]) and np.array_equal(plan.model.pack_keys(s)[1], want[2])
                seen += int(not same)
    return sim.reached, sizes, seen


def test_mutants_cannot_pass():
    """Wherever a family of the narrow layout reaches a mutant's rule, a size, a counter, a verdict or a
    dump differs at one step at least; every mutant is reached by some family; the mutants that store
    one boundary too many at a version that changes nothing (SIZE_ONLY) show in sizes and nowhere else.
    (No count is asked of a family that never reaches the rule: a GC mutant has nothing to change in a
    family without a GC, a glue mutant nothing in one without touching segments.)"""
    table, plans = {}, {}
    for fam in MP.ALL_FAMILIES + ("tails",):
        if fam.startswith("epilogue-"):  # (the sizes up to 1025: the replay is plain Python)
            plans[fam] = [MP.epilogue("narrow", fam[9:], MP.EPI_SIZES[:9])]
        else:
            plans[fam] = MP.build(fam, "long" if fam == "tails" else "narrow")
    for mu in TM.MUTANTS:
        for fam, ps in plans.items():
            for plan in ps:
                reached, sizes, seen = replay_mutant(plan, mu)
                r = table.setdefault((mu, fam), [0, 0, 0])
                r[0], r[1], r[2] = r[0] + reached, r[1] + sizes, r[2] + seen
    for (mu, fam), (reached, sizes, seen) in table.items():
        if reached:
            assert sizes + seen >= 1, (mu, TM.MUTANTS[mu], fam, reached)
        else:
            assert sizes + seen == 0, (mu, fam)
        # (where a GC drops boundaries, one boundary too many changes what it keeps below the floor,
        # which the dump without a floor shows)
        if mu in TM.SIZE_ONLY and not any(st.gc_dropped for p in plans[fam] for st in p.steps):
            assert seen == 0 and (sizes >= 1) == (reached > 0), (mu, fam, reached, sizes, seen)
    for mu in TM.MUTANTS:
        fams = [fam for (m, fam), r in table.items() if m == mu and r[0]]
        if mu == 10:
            # An equivalent mutant: if boundary i - 1 was dropped, it and i - 2 are below the floor, and so
            # on back to the last kept boundary, which is below the floor too (else i - 1 had been kept
            # or the run is empty): the kept predecessor is below the floor exactly when the source one is.
            assert not fams
            continue
        assert len(fams) >= 2, (mu, TM.MUTANTS[mu], fams)
