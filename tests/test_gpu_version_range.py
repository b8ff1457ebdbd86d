"""Nothing depends on where the version axis starts.

Every other test keeps its versions under 2**31 (the largest is about 1.1e7); a production
cluster's are around 1e13 to 1e14.  Versions travel through 64-bit wave shuffles, 64-bit atomicMax,
the hole sentinel INT64_MIN, the export's floor - 1 clamp, the import's pointwise max, the routed
share layout and the add-time TooOld test.  Here each sequence runs on the engine as it is and with
every version moved by D -- snapshots, now, new_oldest, clear versions, loaded versions, header and
the initial oldest version -- for D just below 2**31, just above 2**32, at 1e14 and at 2**62.  Then

  * verdicts and conflicting-key reports are identical to the unshifted run's,
  * both runs equal the semantic oracle fed the same (shifted) input, state included, and
  * the shifted dump is the unshifted one with D added to the header and to every version, at the
    default floor and with no floor (what is stored below the floor depends on when the engine
    collected garbage, so there the two engine runs are compared with each other only).
"""
import bisect

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import PackedBatch
from tests.export_helpers import NO_FLOOR, Pair, canon, split_dump
from tests.helpers import load_json, nonempty, scenario_batches, shift_batch
from tests.import_helpers import merge_max_fast

pytestmark = pytest.mark.gpu

SHIFTS = [2 ** 31 - 3, 2 ** 32 + 5, 10 ** 14 + 7, 2 ** 62]



def run_steps(engine, oracle_mod, steps, D, gc_interval=1, delta_limit=0, early_add=False, baseline=False):
    """Steps ("clear", v) / ("load", kb, ko, vers, header) / ("batch", pb, now, new_oldest), every
    version moved by D.  Engine and semantic oracle side by side (state compared after every
    batch); early_add: each batch is added before the previous batch's detect, so its TooOld test
    reads the oldest version of one batch earlier (SkipList.cpp:770); baseline: verdicts also equal
    the skip-list restatement's.  Returns the per-batch (verdicts, reports) and both dumps."""
    pair = Pair(engine, oracle_mod, gc_interval=gc_interval, delta_limit=delta_limit)
    pair.set_oldest_version(D)  # the axis' origin: a fresh set's oldest version is 0
    sl = oracle_mod.SkipListBaseline() if baseline else None
    if sl:
        sl.set_oldest_version(D)
    out = []
    batches = [i for i, st in enumerate(steps) if st[0] == "batch"]
    objs = {}

    def add(i):
        m = {}
        b = engine.ConflictBatch(pair.cs, m)
        objs[i] = (b, m, pair.cs.oldest_version)
        b.add_packed(shift_batch(steps[i][1], D))

    for i, st in enumerate(steps):
        if st[0] == "clear":
            assert not objs
            pair.clear(st[1] + D)
            if sl:
                sl.clear(st[1] + D)
            continue
        if st[0] == "load":
            _, kb, ko, vers, header = st
            pair.load_history(kb, ko, vers + np.int64(D), header + D)
            pair.set_oldest_version(D)
            if sl:
                sl.load_history(kb, ko, vers + np.int64(D), header + D)
                sl.set_oldest_version(D)
            continue
        _, pb, now, new_oldest = st
        if i not in objs:
            add(i)
        nxt = batches.index(i) + 1
        if early_add and nxt < len(batches) and steps[batches[nxt] - 1][0] == "batch":
            add(batches[nxt])
        b, m, add_oldest = objs.pop(i)
        v = b.detect_conflicts(now + D, new_oldest + D)
        b.close()
        rep = {t: sorted(x) for t, x in m.items()}
        vo, co = pair.o.detect(shift_batch(pb, D), now + D, new_oldest + D, add_oldest=add_oldest)
        assert (v == vo).all(), (i, D, np.flatnonzero(v != vo)[:10])
        assert rep == co, (i, D)
        if sl:
            vs, _ = sl.detect(shift_batch(pb, D), now + D, new_oldest + D, add_oldest=add_oldest)
            assert (v == vs).all(), (i, D, np.flatnonzero(v != vs)[:10])
        if not objs:  # an export refuses while a batch is added and undetected
            pair.check(what=(i, D))
        out.append((v, rep))
    dumps = (split_dump(pair.cs.dump_history()), split_dump(pair.cs.dump_history(floor=NO_FLOOR)))
    pair.cs.close()
    return out, dumps


def assert_moved_by(base, shifted, D, what=None):
    (rb, db), (rs, ds) = base, shifted
    assert len(rb) == len(rs)
    for i, ((vb, cb), (vs, cs)) in enumerate(zip(rb, rs)):
        assert (vb == vs).all(), (what, i, np.flatnonzero(vb != vs)[:10])
        assert cb == cs, (what, i)
    for (hb, kb, vb), (hs, ks, vs) in zip(db, ds):
        assert hs == hb + D, (what, "header", hs, hb)
        assert ks == kb, what
        assert vs == [x + D for x in vb], what


# The unshifted run of each sequence is a module-scoped fixture: computed once, shared by its shifted
# cases, and a failure in it is reported as that fixture's, not under a shifted case's id.


# ---- (a) the known-answer scenarios, clears included


def kat_steps():
    out = []
    for scn in load_json("kat_scenarios.json"):
        steps, expect = [("clear", 0)], []
        for i, (pb, now, new_oldest, exp, conf) in enumerate(scenario_batches(scn)):
            if scn.get("clear_before") == i:
                steps.append(("clear", scn["clear_version"]))
            steps.append(("batch", pb, now, new_oldest))
            expect.append((exp, conf))
        out.append((scn["name"], steps, expect))
    assert len(out) == 13
    return out


@pytest.fixture(scope="module")
def kat_base(engine, oracle_built):
    base = {}
    for name, steps, expect in kat_steps():
        base[name] = run_steps(engine, oracle_built, steps, 0)
        for (v, rep), (exp, conf) in zip(base[name][0], expect):  # the unshifted run is the known answer
            assert v.tolist() == exp, name
            if conf:
                assert nonempty(rep) == conf, name
    return base


@pytest.mark.parametrize("D", SHIFTS)
def test_kat_scenarios_shifted(engine, oracle_built, kat_base, D):
    for name, steps, _ in kat_steps():
        assert_moved_by(kat_base[name], run_steps(engine, oracle_built, steps, D), D, name)


# ---- (b) random batches whose snapshots straddle the oldest version


def random_steps():
    rng = np.random.default_rng(2031)
    steps, now = [("clear", 5)], 10
    for _ in range(12):
        pb = W.random_small_batch(rng, int(rng.integers(20, 80)), alphabet=3, max_len=3, now=now, staleness=15)
        steps.append(("batch", pb, now, now - int(rng.integers(0, 12))))
        now += int(rng.integers(1, 6))
    return steps


RANDOM_CONFIGS = [(1, 0), (0, 0), (0, 25)]


@pytest.fixture(scope="module")
def random_base(engine, oracle_built):
    steps = random_steps()
    return {(gc, dl, early): run_steps(engine, oracle_built, steps, 0, gc_interval=gc, delta_limit=dl, early_add=early)
            for gc, dl in RANDOM_CONFIGS for early in (False, True)}


@pytest.mark.parametrize("D", SHIFTS)
@pytest.mark.parametrize("early_add", [False, True], ids=["add_at_detect", "add_one_batch_early"])
@pytest.mark.parametrize("gc_interval,delta_limit", RANDOM_CONFIGS)
def test_random_batches_shifted(engine, oracle_built, random_base, gc_interval, delta_limit, early_add, D):
    """TooOld is decided right at the shifted boundary, at add time and one batch early."""
    base = random_base[gc_interval, delta_limit, early_add]
    got = run_steps(engine, oracle_built, random_steps(), D, gc_interval=gc_interval, delta_limit=delta_limit,
                    early_add=early_add)
    assert_moved_by(base, got, D, "random")
    seen = np.concatenate([v for v, _ in base[0]])
    assert {0, 1, 2} <= set(seen.tolist())  # conflicts, TooOld and commits all occur


# ---- (c) C4's shape, the window sliding every batch


def c4_steps():
    p = W.C4Params(txns=500, users=1000, items=200, history=20_000, window=12_000, staleness=4_000)
    kb, ko, vers = W.c4_history(p, seed=4, start_version=100_000)
    rng = np.random.default_rng(5)
    steps, now = [("load", kb, ko, vers, 7)], 100_000
    for _ in range(6):
        now += p.version_step
        steps.append(("batch", W.c4_batch(p, rng, now), now, now - p.window))
    return steps


@pytest.fixture(scope="module")
def c4_base(engine, oracle_built):
    steps = c4_steps()
    return steps, run_steps(engine, oracle_built, steps, 0, baseline=True)


@pytest.mark.parametrize("D", SHIFTS)
def test_c4_window_shifted(engine, oracle_built, c4_base, D):
    steps, base = c4_base
    assert_moved_by(base, run_steps(engine, oracle_built, steps, D, baseline=True), D, "c4")
    assert {0, 2} <= set(np.concatenate([v for v, _ in base[0]]).tolist())


# ---- (d) the range hand-over


def _value_at(state, key):
    hdr, ks, vs = state
    i = bisect.bisect_right(ks, key)
    return vs[i - 1] if i else hdr


def _point_batch(rng, now, txns=30):
    """Point reads and writes over 32 two-byte keys, so that the history stays finely divided."""
    from foundationdb_amd.packing import CommitTransaction, KeyRange

    key = lambda: bytes([int(rng.integers(0, 8)) * 0x10 + 0x10, int(rng.integers(0, 4))])
    pt = lambda k: KeyRange(k, k + b"\x00")
    return PackedBatch.from_transactions([
        CommitTransaction([pt(key()) for _ in range(int(rng.integers(0, 3)))],
                          [pt(key()) for _ in range(int(rng.integers(0, 2)))], int(now - rng.integers(0, 6)), False)
        for _ in range(txns)])


def hand_over(engine, oracle_mod, D):
    """Two sets over the same keys, batches at alternating versions, then [lo, hi) handed from a to
    fresh copies of b by merge_history and by merge_pending_export.  Returns the merged state."""
    rng = np.random.default_rng(77)
    a = Pair(engine, oracle_mod, gc_interval=3)
    b = Pair(engine, oracle_mod, gc_interval=2)
    now = 100
    for p in (a, b):
        p.clear(D + 90)
        p.set_oldest_version(D)
    for i in range(8):
        for j, p in enumerate((a, b)):
            p.detect(shift_batch(_point_batch(rng, now + j), D), now + j + D, now - 30 + D)
        now += 5
    lo, hi = b"\x20", b"\x70"
    own, moved = b.reference(), a.reference(lo, hi)
    pts = [k for k in sorted(set(own[1]) | set(moved[1])) if lo <= k < hi]
    diff = [_value_at(own, k) - _value_at(moved, k) for k in pts]
    assert min(diff) < 0 < max(diff)  # each side holds the greater version somewhere in the range
    merged = merge_max_fast(own, moved, lo, hi)
    want = canon(merged[1], merged[2], merged[0], b.o.oldest_version)
    bd = b.cs.dump_history()
    for how in ("host arrays", "pending export"):
        d = engine.ConflictSet()
        d.load_history(*bd)
        d.set_oldest_version(b.cs.oldest_version)
        if how == "host arrays":
            n = d.merge_history(*a.cs.dump_history(lo, hi), lo=lo, hi=hi)
        else:
            a.cs.export_history(lo, hi)
            n = d.merge_pending_export(a.cs, lo, hi)
        assert n == d.history_size()
        assert split_dump(d.dump_history()) == want, (how, D)
        if how == "host arrays":
            raw = split_dump(d.dump_history(floor=NO_FLOOR))
        d.close()
    a.cs.close()
    b.cs.close()
    return [], (want, raw)


@pytest.fixture(scope="module")
def hand_over_base(engine, oracle_built):
    return hand_over(engine, oracle_built, 0)


@pytest.mark.parametrize("D", SHIFTS)
def test_range_hand_over_shifted(engine, oracle_built, hand_over_base, D):
    assert_moved_by(hand_over_base, hand_over(engine, oracle_built, D), D, "hand_over")


# ---- (e) the routed path


def routed(engine, oracle_mod, D):
    """Two plain batches, then one batch whose two proxy shares are routed on the device to a
    resolver owning every key; its verdicts against the unrouted batch on a twin set."""
    import torch

    from foundationdb_amd.sharding import KeyRangeSharding

    rng = np.random.default_rng(404)
    sets = [engine.ConflictSet(0) for _ in range(2)]
    ora = oracle_mod.OracleConflictSet()
    for s in sets + [ora]:
        s.clear(D + 3)
        s.set_oldest_version(D)
    now = 10
    for _ in range(2):
        pb = shift_batch(W.random_small_batch(rng, 150, alphabet=5, max_len=3, now=now, staleness=12), D)
        want, _ = ora.detect(pb, now + D, now - 9 + D)
        for cs in sets:
            b = engine.ConflictBatch(cs)
            b.add_packed(pb)
            assert (b.detect_conflicts(now + D, now - 9 + D) == want).all()
            b.close()
        now += 4
    G, Tshare = 2, 120
    pb = shift_batch(W.random_small_batch(rng, G * Tshare, alphabet=5, max_len=3, now=now, staleness=20), D)
    shares = [engine.share_pack(pb.slice_txns(g * Tshare, (g + 1) * Tshare)) for g in range(G)]
    stride = (max(len(x) for x in shares) + 255) // 256 * 256
    host = np.zeros(G * stride, np.uint8)
    for g, x in enumerate(shares):
        host[g * stride: g * stride + len(x)] = x
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    route = KeyRangeSharding([]).route(pb)[0]  # the transactions that carry ranges
    sub = route.batch
    out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
    b = engine.ConflictBatch(sets[0])
    b.add_routed(dev.data_ptr(), stride, G, Tshare, None, None, (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes),
                 out.data_ptr(), pb.n_txn)
    b.detect_async(now + D, now - 9 + D)
    got = b.wait()
    b.close()
    u = engine.ConflictBatch(sets[1])
    u.add_packed(sub)
    plain = u.detect_conflicts(now + D, now - 9 + D)
    u.close()
    want, _ = ora.detect(sub, now + D, now - 9 + D)
    np.testing.assert_array_equal(got, plain)
    np.testing.assert_array_equal(got, want)
    conflict_bytes = np.zeros(pb.n_txn, np.uint8)
    conflict_bytes[route.txn_ids] = 2 - want.astype(np.uint8)
    np.testing.assert_array_equal(out.cpu().numpy(), conflict_bytes)
    assert {0, 1, 2} <= set(got.tolist())
    dumps = tuple(split_dump(sets[0].dump_history(floor=f)) for f in (None, NO_FLOOR))
    assert dumps == tuple(split_dump(sets[1].dump_history(floor=f)) for f in (None, NO_FLOOR))
    for cs in sets:
        cs.close()
    return [(got, {})], dumps


@pytest.fixture(scope="module")
def routed_base(engine, oracle_built):
    return routed(engine, oracle_built, 0)


@pytest.mark.parametrize("D", SHIFTS)
def test_routed_batch_shifted(engine, oracle_built, routed_base, D):
    assert_moved_by(routed_base, routed(engine, oracle_built, D), D, "routed")


# ---- (f) the resolver's host logic over the engine


def resolved(engine, oracle_mod, D):
    from foundationdb_amd.resolver import Resolver, ResolveTransactionBatchRequest as Req
    from tests.test_resolver import OracleBatch

    cs, ref_cs = engine.new_conflict_set(), oracle_mod.OracleConflictSet()
    for s in (cs, ref_cs):
        s.clear(D + 900)
        s.set_oldest_version(D)
    gpu = Resolver(conflict_set=cs, batch_factory=engine.ConflictBatch, max_write_transaction_life_versions=3000)
    ref = Resolver(conflict_set=ref_cs, batch_factory=OracleBatch, max_write_transaction_life_versions=3000)
    rng = np.random.default_rng(11)
    prev, v = -1, D + 4000
    out = []
    for i in range(5):
        pb = shift_batch(W.random_small_batch(rng, 200, alphabet=6, max_len=5, now=v - D, staleness=4500), D)
        txns = pb.to_transactions()
        for t in txns[::7]:
            t.report_conflicting_keys = True
        req = Req(prev, v, prev, txns, proxy=None if prev < 0 else "p0")
        (_, ra), = gpu.submit(req)
        (_, rb), = ref.submit(req)
        assert ra.committed == rb.committed
        rep = {t: sorted(x) for t, x in ra.conflicting_key_range_map.items()}
        assert rep == {t: sorted(x) for t, x in rb.conflicting_key_range_map.items()}
        out.append((np.array(ra.committed, np.uint8), rep))
        prev, v = v, v + 1000
    dumps = tuple(split_dump(cs.dump_history(floor=f)) for f in (None, NO_FLOOR))
    cs.close()
    return out, dumps


@pytest.fixture(scope="module")
def resolver_base(engine, oracle_built):
    return resolved(engine, oracle_built, 0)


@pytest.mark.parametrize("D", SHIFTS)
def test_resolver_chain_shifted(engine, oracle_built, resolver_base, D):
    res = resolved(engine, oracle_built, D)
    assert_moved_by(resolver_base, res, D, "resolver")
    assert {0, 1, 2} <= set(np.concatenate([v for v, _ in res[0]]).tolist())
