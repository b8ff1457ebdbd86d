"""Device routing under a keyResolvers ownership history (fdbcs_batch_add_routed_map,
CommitProxyServer.actor.cpp:147-174): G resolvers on one GPU, each routing the same gathered shares
as one resolver of the map, against the host routing (sharding.KeyResolvers.route) and an oracle
per resolver fed that routing -- the checks of test_device_routing_matches_host_routing plus the
read-id view and the MAX of the conflict bytes."""
import copy

import numpy as np
import pytest

from foundationdb_amd.packing import PackedBatch
from foundationdb_amd.sharding import KeyRangeSharding, KeyResolvers
from tests.route_map_helpers import MapRouted, history_floors, large_map, moves_recipe, random_move, tx
from tests.routed_report_helpers import Floors, bytes_as_sets, make_splits, proxy_sets, sorted_map

pytestmark = pytest.mark.gpu

MOVE_CASES = [(2, 6, 3, False), (3, 200, 3, False), (4, 5, 24, True)]


def _sets(engine, oracle_built, G):
    return [engine.ConflictSet(0) for _ in range(G)], [oracle_built.OracleConflictSet() for _ in range(G)]


def _run(engine, oras, rt, now, oldest):
    rt.check_sizes(engine)
    rt.detect(now, oldest)
    return rt.check_verdicts(oras, rt.wait(), now, oldest)


def test_static_map_equals_static_bounds(engine, oracle_built):
    """A map with one history entry per range routes exactly as add_routed with the matching
    [lo, hi): sizes, verdicts, conflict bytes and read ids, G = 3, two batches."""
    import torch

    from foundationdb_amd import workloads as W

    G, Tshare = 3, 120
    rng = np.random.default_rng(31)
    splits = make_splits(rng, G, 6, False)
    kr = KeyResolvers.from_sharding(KeyRangeSharding(splits))
    sets_m, oras = _sets(engine, oracle_built, G)
    sets_s = [engine.ConflictSet(0) for _ in range(G)]
    now = 10
    for _ in range(2):
        pb = W.random_small_batch(rng, G * Tshare, alphabet=6, max_len=3, now=now, staleness=12)
        a = MapRouted(engine, torch, sets_m, kr, pb, Tshare)
        b = MapRouted(engine, torch, sets_s, kr, pb, Tshare, static_splits=splits)
        a.check_sizes(engine)
        b.check_sizes(engine)
        a.detect(now, now - 9)
        b.detect(now, now - 9)
        got_a, got_b = a.wait(), b.wait()
        for g in range(G):
            np.testing.assert_array_equal(got_a[g], got_b[g])
            np.testing.assert_array_equal(a.conf[g], b.conf[g])
            np.testing.assert_array_equal(a.read_ids[g], b.read_ids[g])
        a.check_verdicts(oras, got_a, now, now - 9)
        now += 4
    for cs in sets_m + sets_s:
        cs.close()


@pytest.mark.parametrize("G,alphabet,max_len,long_split", MOVE_CASES)
def test_moves(engine, oracle_built, G, alphabet, max_len, long_split):
    """The multi-resolver parameter sets of test_device_routing_matches_host_routing under
    resharding: 12 batches of 120 transactions per share, a random subrange moved to a random
    resolver at batches 2, 4, 6, 8, 10 at that batch's version, a coalesce at batch 9.  The floors
    are counted from the host routing before any GPU call: without them the test could pass on
    code that ignores the history or the snapshot."""
    import torch

    from foundationdb_amd import workloads as W

    rng = np.random.default_rng(100 + G + alphabet)
    splits = make_splits(rng, G, alphabet, long_split)
    steps = list(moves_recipe(W, rng, splits, G, alphabet, max_len))
    first = sum(history_floors(kr, pb)[0] for pb, _, kr in steps)
    second = sum(history_floors(kr, pb)[1] for pb, _, kr in steps)
    print(f"floors G={G}: not-an-owner reads {first}, snapshot-excluded former owners {second}")
    assert first >= 50 and second >= 50, (first, second)
    assert not long_split or any(len(b) == 20 for b in steps[-1][2].bounds + steps[0][2].bounds)
    sets, oras = _sets(engine, oracle_built, G)
    for pb, now, kr in steps:
        _run(engine, oras, MapRouted(engine, torch, sets, kr, pb, 120), now, now - 9)
    for cs in sets:
        cs.close()


@pytest.mark.parametrize("off", [0, 10 ** 14 + 7])
def test_snapshot_at_the_move_version(engine, oracle_built, off):
    """[0x50, 0x60) moved 1 -> 0 at version v after a write there at v: of the reads at snapshots
    v - 1, v, v + 1 the former owner receives the first two, and only it sees the first one's
    conflict.  With an empty read at a bound key, reads ending exactly at a bound and a write
    spanning the moved range; again with every version offset past 2^32."""
    import torch

    v = 100 + off
    before = KeyResolvers(2, [b"\x50"])
    after = KeyResolvers(2, [b"\x50"])
    after.apply_changes([(b"\x50", b"\x60", 0)], v)
    sets, oras = _sets(engine, oracle_built, 2)
    pa = PackedBatch.from_transactions([tx([], [(b"\x52", b"\x54")], v - 3), tx([], [(b"\x10", b"\x11")], v - 3)])
    ra = MapRouted(engine, torch, sets, before, pa, 1)
    _run(engine, oras, ra, v, v - 50)
    assert [r.batch.n_txn for r in ra.routes] == [1, 1]
    rd = (b"\x52", b"\x54")
    pb = PackedBatch.from_transactions([
        tx([rd], [], v - 1), tx([rd], [], v), tx([rd], [], v + 1),
        tx([(b"\x50", b"\x50")], [], v + 1),   # empty, at a bound key: rangeContaining -> the moved range
        tx([(b"\x55", b"\x60")], [], v + 1),   # ends exactly at a bound: the range after it is not met
        tx([(b"\x40", b"\x50")], [(b"\x40", b"\x70")], v + 1),  # a write over all three map ranges
    ])
    rb = MapRouted(engine, torch, sets, after, pb, 3)
    rb.check_sizes(engine)
    # resolver 0 (the new owner) gets everything; resolver 1 the two old-enough reads and the write
    assert rb.routes[0].txn_ids.tolist() == [0, 1, 2, 3, 4, 5]
    assert rb.routes[1].txn_ids.tolist() == [0, 1, 5]
    assert (rb.routes[1].batch.n_reads, rb.routes[1].batch.n_writes) == (2, 1)
    rb.detect(v + 5, v - 50)
    vs, _ = rb.check_verdicts(oras, rb.wait(), v + 5, v - 50)
    assert rb.combined.tolist() == [0, 2, 2, 2, 2, 2]
    assert vs[0].tolist() == [2] * 6 and vs[1].tolist() == [0, 2, 2]
    for cs in sets:
        cs.close()


def test_large_map_in_global_memory(engine, oracle_built):
    """300 ranges with two-byte bounds (past the kernel's LDS staging limit of 256), histories 1-3
    deep over 4 resolvers: reads and writes from the empty key to 0xff 0xff 0xff (the summary
    walk), ranges that begin and end on bounds, and random ones, at snapshots around the moves."""
    import torch

    G, Tshare = 4, 100
    rng = np.random.default_rng(300)
    kr = large_map(rng)
    assert len(kr.bounds) == 300 and {len(h) for h in kr.hist} == {1, 2, 3}
    bnd = kr.bounds

    def key():
        return bytes(int(x) for x in rng.integers(0, 256, size=int(rng.integers(0, 4))))

    def rnd():
        k = int(rng.integers(0, 12))
        i = int(rng.integers(0, 300))
        if k == 0:
            return (b"", b"\xff\xff\xff")
        if k == 1:  # begins and ends on bounds, any distance apart
            i, j = sorted(int(x) for x in rng.integers(0, 300, size=2))
            return (bnd[i], bnd[j])
        if k == 2:  # begins on a bound, ends inside a range some blocks later
            return (bnd[i], max(bnd[i], bnd[min(299, i + int(rng.integers(0, 200)))] + b"\x01"))
        if k == 3:
            return tuple(sorted([key(), key()]))
        if k < 8:  # on bounds, zero to two map ranges
            return (bnd[i], bnd[min(299, i + int(rng.integers(0, 3)))])
        return (bnd[i] + b"\x00", bnd[i] + bytes([int(rng.integers(0, 3))]))  # inside one map range

    txns = [tx([rnd() for _ in range(int(rng.integers(0, 4)))], [rnd() for _ in range(int(rng.integers(0, 3)))],
               int(rng.integers(15, 65))) for _ in range(G * Tshare)]
    pb = PackedBatch.from_transactions(txns)
    first, second = history_floors(kr, pb)
    assert first >= 50 and second >= 50, (first, second)
    sets, oras = _sets(engine, oracle_built, G)
    _run(engine, oras, MapRouted(engine, torch, sets, kr, pb, Tshare), 70, 10)
    for cs in sets:
        cs.close()


@pytest.mark.parametrize("submit_thread", ["1", "0"])
def test_pipelined_maps(engine, oracle_built, monkeypatch, submit_thread):
    """Three batches in flight on every resolver, each routed under its own map with a move between
    consecutive batches, all routed before the first detect and waited in order: every batch keeps
    the map of its own slot, and a new map needs no drain."""
    import torch

    from foundationdb_amd import workloads as W

    monkeypatch.setenv("FDBCS_SUBMIT_THREAD", submit_thread)
    G, alphabet, max_len, _ = MOVE_CASES[0]
    rng = np.random.default_rng(515)
    splits = make_splits(rng, G, alphabet, False)
    kr = KeyResolvers(G, splits)
    sets, oras = _sets(engine, oracle_built, G)
    now = 10
    floors = np.zeros(2, np.int64)
    for _ in range(2):  # the second round reuses the first one's slots
        group = []
        for _ in range(3):
            random_move(rng, kr, alphabet, max_len, now)
            pb = W.random_small_batch(rng, G * 120, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
            group.append((pb, now, copy.deepcopy(kr)))
            floors += history_floors(kr, pb)
            now += 4
        rts = [MapRouted(engine, torch, sets, m, pb, 120) for pb, _, m in group]
        for rt, (_, now, _) in zip(rts, group):
            rt.detect(now, now - 9)
        for rt, (_, now, _) in zip(rts, group):
            got = rt.wait()
            rt.check_verdicts(oras, got, now, now - 9)
    assert floors.min() > 0, floors
    for cs in sets:
        cs.close()


def test_reports(engine, oracle_built):
    """Conflicting-key reports of batches routed under a map with moves: each resolver's
    conflictingKeyRangeMap and report bytes against its oracle, the MAX of the bytes against the
    proxy's lists."""
    import torch

    from foundationdb_amd import sharding
    from foundationdb_amd import workloads as W

    G, alphabet, max_len, _ = MOVE_CASES[0]
    rng = np.random.default_rng(617)
    splits = make_splits(rng, G, alphabet, False)
    steps = list(moves_recipe(W, rng, splits, G, alphabet, max_len, batches=8))
    assert min(sum(history_floors(kr, pb)[i] for pb, _, kr in steps) for i in (0, 1)) >= 50
    sets, oras = _sets(engine, oracle_built, G)
    fl = Floors()
    for pb, now, kr in steps:
        rt = MapRouted(engine, torch, sets, kr, pb, 120, reports=True)
        rt.check_sizes(engine)
        rt.detect(now, now - 9)
        got = rt.wait()
        vs, ms = rt.check_verdicts(oras, got, now, now - 9)
        mx = np.zeros(pb.n_reads, np.uint8)
        for g in range(G):
            assert sorted_map(rt.maps[g]) == sorted_map(ms[g]), f"resolver {g}"
            dev = rt.reps[g].cpu().numpy()[: pb.n_reads]
            np.testing.assert_array_equal(dev, sharding.report_bytes(pb, rt.routes[g], ms[g]), err_msg=f"resolver {g}")
            mx = np.maximum(mx, dev)
        lists, want = proxy_sets(pb, rt.routes, ms, rt.combined)
        assert bytes_as_sets(pb, mx) == want
        fl.add(lists)
    assert fl.reported > 0 and fl.multi > 0 and fl.dup > 0
    for cs in sets:
        cs.close()


def test_errors_leave_the_batch_usable(engine, oracle_built):
    """An invalid map is FDBCS_E_INVALID at the call and the batch stays usable; capacities too
    small are FDBCS_E_NOMEM at detect, and the batch is routed again with larger ones and the same
    map."""
    import torch

    from foundationdb_amd import workloads as W
    from tests.route_map_helpers import gather

    rng = np.random.default_rng(717)
    kr = KeyResolvers(2, [b"\x02"])
    kr.apply_changes([(b"\x01", b"\x03", 1)], 5)
    pb = W.random_small_batch(rng, 200, alphabet=6, max_len=3, now=10, staleness=12)
    route = kr.route(pb)[1]
    dev, stride = gather(engine, torch, pb, 2, 100)
    cs = engine.ConflictSet(0)
    out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
    caps = (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
    b = engine.ConflictBatch(cs)
    bad = kr.flat()
    bad["hist_versions"] = bad["hist_versions"][::-1].copy()
    assert np.any(np.diff(bad["hist_versions"]) < 0)
    with pytest.raises(engine.FdbcsError) as e:
        b.add_routed_map(dev.data_ptr(), stride, 2, 100, bad, 1, caps, out.data_ptr(), pb.n_txn)
    assert e.value.status == engine.FDBCS_E_INVALID
    with pytest.raises(engine.FdbcsError) as e:
        b.add_routed_map(dev.data_ptr(), stride, 2, 100, kr, -1, caps, out.data_ptr(), pb.n_txn)
    assert e.value.status == engine.FDBCS_E_INVALID
    assert route.batch.n_reads > 4
    b.add_routed_map(dev.data_ptr(), stride, 2, 100, kr, 1, (pb.n_txn, 4, pb.n_writes, pb.tail_bytes), out.data_ptr(),
                     pb.n_txn)
    with pytest.raises(engine.FdbcsError) as e:
        b.detect_async(10, 1)
    assert e.value.status == engine.FDBCS_E_NOMEM
    b.add_routed_map(dev.data_ptr(), stride, 2, 100, kr, 1, caps, out.data_ptr(), pb.n_txn)
    T, R, Wn, _, _ = b.routed_info()
    assert (T, R, Wn) == (route.batch.n_txn, route.batch.n_reads, route.batch.n_writes)
    b.detect_async(10, 1)
    got = b.wait()
    b.close()
    want, _ = oracle_built.OracleConflictSet().detect(route.batch, 10, 1)
    np.testing.assert_array_equal(got, want)
    from foundationdb_amd import sharding

    np.testing.assert_array_equal(out.cpu().numpy(), sharding.conflict_bytes(pb.n_txn, route, want))
    cs.close()
