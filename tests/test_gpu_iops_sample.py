"""The resolver's iops sample of device-routed batches (fdbcs_batch_set_iops_sample), taken on the
GPU: every output (keys, key offsets, metrics, range indices) against balancing.iops_sample_of of
the host routing's sub-batch, which restates the roll in integers, so equality is exact."""
import copy
import ctypes

import numpy as np
import pytest

from foundationdb_amd import balancing as B
from foundationdb_amd import workloads as W
from foundationdb_amd.packing import PackedBatch
from foundationdb_amd.sharding import KeyRangeSharding, KeyResolvers
from tests.route_map_helpers import MapRouted, gather, moves_recipe, tx

pytestmark = pytest.mark.gpu

TILE = 256  # transfer.h kIopsTile: ranges per workgroup of the sample's scan (one per thread)


def want_of(sub, units, seed):
    keys, metrics, index = B.iops_sample_of(sub, units, seed)
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in keys], dtype=np.int64)]).astype(np.int64)
    return b"".join(keys), offsets, metrics, index


def check_sample(b, sub, units, seed, what=""):
    """All four outputs of the device sample of batch b against the restatement; returns them."""
    kb, ko, met, idx = b.iops_sample_raw()
    wb, wo, wm, wi = want_of(sub, units, seed)
    np.testing.assert_array_equal(idx, wi, err_msg=what)
    np.testing.assert_array_equal(met, wm, err_msg=what)
    np.testing.assert_array_equal(ko, wo, err_msg=what)
    assert kb.tobytes() == wb, what
    return kb, ko, met, idx


class Single:
    """A batch routed whole to one resolver (no bounds): the sub-batch is the host routing's."""

    def __init__(self, engine, cs, pb, caps=None, lo=None, hi=None):
        import torch

        self.sub = KeyResolvers(1).route(pb)[0].batch if lo is None and hi is None else None
        self.dev, stride = gather(engine, torch, pb, 1, max(pb.n_txn, 1))
        self.out = torch.full((max(pb.n_txn, 1),), 7, dtype=torch.uint8, device="cuda")
        self.args = (self.dev.data_ptr(), stride, 1, max(pb.n_txn, 1), lo, hi)
        self.tail = (self.out.data_ptr(), pb.n_txn)
        self.caps = caps or (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
        self.b = engine.ConflictBatch(cs)
        self.b.add_routed(*self.args, self.caps, *self.tail)


@pytest.fixture(scope="module")
def cs1(engine):
    cs = engine.ConflictSet(0)
    yield cs
    cs.close()


def random_key(rng, n):
    k = rng.integers(0, 256, size=n, dtype=np.uint8)
    r = rng.random(n)
    k[r < 0.25] = 0
    k[r > 0.75] = 255
    return k.tobytes()


LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 63, 64, 65, 200, 4101]


def test_every_range_kept_every_length_and_alignment(engine, cs1):
    """units = 1 keeps every range: the output is every begin key in range order, byte-exact, at
    every alignment of the destination."""
    rng = np.random.default_rng(21)
    for attempt in range(400):  # an order whose output offsets cover the residues, found on the CPU
        rk = [random_key(rng, n) for n in rng.permutation(LENGTHS * 2)]
        wk = [random_key(rng, n) for n in rng.permutation(LENGTHS * 2)]
        lens = np.array([len(k) for k in rk + wk])
        offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
        after_long = {int(o) % 8 for o, prev in zip(offs[1:], lens[:-1]) if prev > 16}
        of_long = {int(o) % 8 for o, n in zip(offs, lens) if n > 16}
        if len(after_long) == 8 and len(of_long) == 8:
            break
    assert len(after_long) == 8 and len(of_long) == 8
    assert any(0 in k and 255 in k for k in rk) and sorted(set(lens.tolist())) == LENGTHS
    txns = [tx([(a, a + b"\xff")], [(c, c + b"\xff")], 5) for a, c in zip(rk, wk)]
    pb = PackedBatch.from_transactions(txns)
    s = Single(engine, cs1, pb)
    s.b.set_iops_sample(1, 77)
    assert (s.sub.n_reads, s.sub.n_writes) == (len(rk), len(wk))
    kb, ko, met, idx = check_sample(s.b, s.sub, 1, 77)
    raw = kb.tobytes()
    assert [raw[ko[i]:ko[i + 1]] for i in range(len(met))] == rk + wk
    np.testing.assert_array_equal(met, 100 + lens)
    np.testing.assert_array_equal(idx, np.arange(len(lens)))
    s.b.close()


@pytest.mark.parametrize("shape", ["reads", "seam"])
@pytest.mark.parametrize("n", [1, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_tile_edges_of_the_scan(engine, cs1, n, shape):
    """R + W around the scan's tile, all reads and one read followed by writes (index R + w)."""
    rng = np.random.default_rng(n)
    keys = [bytes(int(x) for x in rng.integers(0, 256, size=3)) for _ in range(n)]
    if shape == "reads":
        txns = [tx([(k, k + b"\x00")], [], 5) for k in keys]
    else:
        txns = [tx([(keys[0], keys[0] + b"\x00")], [], 5)] + [tx([], [(k, k + b"\x00")], 5) for k in keys[1:]]
    pb = PackedBatch.from_transactions(txns)
    s = Single(engine, cs1, pb)
    s.b.set_iops_sample(1, n)
    assert (s.sub.n_reads, s.sub.n_writes) == ((n, 0) if shape == "reads" else (1, n - 1))
    kb, ko, met, idx = check_sample(s.b, s.sub, 1, n)
    assert len(met) == n and kb.tobytes() == b"".join(keys)
    s.b.close()


def test_threshold(engine, cs1):
    """units = 110: metrics 110 and 111 (10- and 11-byte keys) always count, as themselves; metric
    109 is rolled at odds 109 / 110 and counts as 110."""
    rng = np.random.default_rng(3)
    keys = [bytes(int(x) for x in rng.integers(0, 256, size=9 + i % 3)) for i in range(3000)]
    txns = [tx([(keys[t], keys[t] + b"\x00")], [(keys[1500 + t], keys[1500 + t] + b"\x00")], 5) for t in range(1500)]
    pb = PackedBatch.from_transactions(txns)
    s = Single(engine, cs1, pb)
    s.b.set_iops_sample(110, 3)
    kb, ko, met, idx = check_sample(s.b, s.sub, 110, 3)
    lens = np.diff(ko)
    assert int((lens == 10).sum()) == 1000 and set(met[lens == 10].tolist()) == {110}
    assert int((lens == 11).sum()) == 1000 and set(met[lens == 11].tolist()) == {111}
    assert 0 < int((lens == 9).sum()) < 1000 and set(met[lens == 9].tolist()) == {110}
    s.b.close()


def _owners(sub):
    """Transaction of every range of a sub-batch, reads then writes."""
    t = np.arange(sub.n_txn)
    return np.concatenate([np.repeat(t, np.diff(sub.read_offsets)), np.repeat(t, np.diff(sub.write_offsets))])


def test_sparse_sample_under_static_splits_and_a_moving_map(engine, oracle_built):
    """The moves recipe (12 batches of 4 x 120 transactions, moves and a coalesce between them),
    units = 300, routed under the moving map and again under the static splits; every batch is
    detected with oldest = now - 6 and held against the oracles, so the sample is shown not to
    disturb the batch.  The floors are what makes the comparison mean something: sampled ranges
    that begin in a map range another resolver owns now, and sampled ranges of TooOld
    sub-transactions (counted from the verdict bytes)."""
    import torch

    G, Tshare, units = 4, 120, 300
    splits = [b"\x01", b"\x02", b"\x03"]
    steps = list(moves_recipe(W, np.random.default_rng(11), splits, G, alphabet=4, max_len=3))
    assert len(steps) == 12
    for static in (False, True):
        sets = [engine.ConflictSet(0) for _ in range(G)]
        oras = [oracle_built.OracleConflictSet() for _ in range(G)]
        routed = sampled = foreign = too_old = 0
        for n, (pb, now, kr_moving) in enumerate(steps, 1):
            kr = KeyResolvers(G, splits) if static else kr_moving
            rt = MapRouted(engine, torch, sets, kr, pb, Tshare, static_splits=splits if static else None)
            for g in range(G):
                rt.objs[g].set_iops_sample(units, 1000 * n + g)
            rt.check_sizes(engine)
            got_idx = []
            for g in range(G):
                sub = rt.routes[g].batch
                kb, ko, met, idx = check_sample(rt.objs[g], sub, units, 1000 * n + g, f"batch {n} resolver {g}")
                raw = kb.tobytes()
                routed += sub.n_reads + sub.n_writes
                sampled += len(idx)
                foreign += sum(1 for i in range(len(idx)) if kr.owner_of(raw[ko[i]:ko[i + 1]]) != g)
                got_idx.append(idx)
            rt.detect(now, now - 6)
            got = rt.wait()
            rt.check_verdicts(oras, got, now, now - 6)
            for g in range(G):
                own = _owners(rt.routes[g].batch)
                too_old += int((got[g][own[got_idx[g]]] == engine.TransactionTooOld).sum())
        print(f"static={static}: routed {routed}, sampled {sampled}, foreign begins {foreign}, TooOld {too_old}")
        if not static:
            assert sampled >= 8000 and foreign >= 2000 and too_old >= 500, (routed, sampled, foreign, too_old)
        assert 0 < sampled < routed
        for cs in sets:
            cs.close()


def test_pipelining_and_lifetime(engine, oracle_built):
    """Four routed batches in flight on one set, each with its own seed: the sample is readable
    before the batch's detect is issued and still the same after its wait; a second round reuses
    the first one's slots."""
    rng = np.random.default_rng(55)
    cs = engine.ConflictSet(0)
    ora = oracle_built.OracleConflictSet()
    now = 10
    for rnd in range(2):
        group = []
        for j in range(4):
            pb = W.random_small_batch(rng, 300, alphabet=5, max_len=20 if j == 3 else 3, now=now, staleness=12)
            s = Single(engine, cs, pb)
            seed = (1 << 63) + 17 * (4 * rnd + j)
            s.b.set_iops_sample(250, seed)
            group.append((s, seed, now))
            now += 4
        first = []
        for s, seed, at in group:
            first.append(check_sample(s.b, s.sub, 250, seed))
            s.b.detect_async(at, at - 9)
        for (s, seed, at), before in zip(group, first):
            got = s.b.wait()
            want, _ = ora.detect(s.sub, at, at - 9)
            np.testing.assert_array_equal(got, want)
            after = check_sample(s.b, s.sub, 250, seed)
            for x, y in zip(before, after):
                np.testing.assert_array_equal(x, y)
            assert 0 < len(after[2]) < s.sub.n_reads + s.sub.n_writes
            assert s.b.iops_sample_timing() > 0
            s.b.close()
    cs.close()


def test_an_empty_routed_batch_has_an_empty_sample(engine, cs1):
    rng = np.random.default_rng(56)
    pb = W.random_small_batch(rng, 100, alphabet=4, max_len=3, now=10, staleness=12)
    s = Single(engine, cs1, pb, lo=b"\xf0")  # every key is below the resolver's range
    s.b.set_iops_sample(1, 5)
    kb, ko, met, idx = s.b.iops_sample_raw()
    assert s.b.routed_info()[:3] == (0, 0, 0)
    assert len(kb) == 0 and ko.tolist() == [0] and len(met) == 0 and len(idx) == 0
    s.b.close()


def _status(engine, f, *a):
    with pytest.raises(engine.FdbcsError) as e:
        f(*a)
    return e.value.status


def test_errors(engine, cs1):
    rng = np.random.default_rng(57)
    lib = engine.load_library()
    pb = W.random_small_batch(rng, 200, alphabet=6, max_len=3, now=10, staleness=12)
    # a batch added on the host is not sampled on the device
    b = engine.ConflictBatch(cs1)
    b.add_packed(pb)
    assert _status(engine, b.set_iops_sample, 300, 1) == engine.FDBCS_E_STATE
    b.close()
    # no request, a bad unit, too small a capacity in the read
    s = Single(engine, cs1, pb)
    assert _status(engine, s.b.iops_sample_raw) == engine.FDBCS_E_STATE
    assert _status(engine, s.b.set_iops_sample, 0, 1) == engine.FDBCS_E_INVALID
    assert _status(engine, s.b.iops_sample_raw) == engine.FDBCS_E_STATE
    s.b.set_iops_sample(300, 1)
    s.b.set_iops_sample(300, 2)  # replaces the request
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    assert lib.fdbcs_batch_iops_sample(s.b._h, ctypes.byref(n), ctypes.byref(nb)) == 0
    assert n.value > 0 and nb.value > 0
    kb, ko = np.zeros(nb.value, np.uint8), np.zeros(n.value + 1, np.int64)
    met, idx = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    p = [ctypes.c_void_p(x.ctypes.data) for x in (kb, ko, met, idx)]
    assert lib.fdbcs_batch_iops_sample_read(s.b._h, p[0], nb.value, p[1], p[2], p[3], n.value - 1) == engine.FDBCS_E_NOMEM
    assert lib.fdbcs_batch_iops_sample_read(s.b._h, p[0], nb.value - 1, p[1], p[2], p[3], n.value) == engine.FDBCS_E_NOMEM
    assert lib.fdbcs_batch_iops_sample_read(s.b._h, p[0], nb.value, p[1], p[2], None, n.value) == 0
    wb, wo, wm, wi = want_of(s.sub, 300, 2)
    assert kb.tobytes() == wb and ko.tolist() == wo.tolist() and met.tolist() == wm.tolist()
    check_sample(s.b, s.sub, 300, 2)
    # after detect the request is refused; the sample taken before stays readable
    s.b.detect_async(10, 1)
    assert _status(engine, s.b.set_iops_sample, 300, 3) == engine.FDBCS_E_STATE
    s.b.wait()
    check_sample(s.b, s.sub, 300, 2)
    s.b.close()
    # capacities too small: the routing's error comes out of the sample call, and the batch can be
    # routed again with enough room
    assert pb.n_reads > 4
    s = Single(engine, cs1, pb, caps=(pb.n_txn, 4, pb.n_writes, pb.tail_bytes))
    s.b.set_iops_sample(300, 4)
    assert _status(engine, s.b.iops_sample_raw) == engine.FDBCS_E_NOMEM
    assert _status(engine, s.b.iops_sample_raw) == engine.FDBCS_E_STATE  # the request went with the batch
    s.b.add_routed(*s.args, (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes), *s.tail)
    s.b.set_iops_sample(300, 4)
    check_sample(s.b, s.sub, 300, 4)
    s.b.close()


def test_closed_loop_without_host_routing(engine, oracle_built):
    """add_routed_map -> device sample -> ResolverLoad -> ResolutionBalancer -> the next map: the
    same moves as BalancedRouting.route(pb, version, seed) makes on the host, and verdicts equal
    to the oracles fed the host routing."""
    import torch

    from tests.test_iops_sample_cpu import balancer_recipe, new_routing

    G, units = 2, 1_000
    host, loop = new_routing(G), new_routing(G)
    sets = [engine.ConflictSet(0) for _ in range(G)]
    oras = [oracle_built.OracleConflictSet() for _ in range(G)]
    for pb, version in balancer_recipe(G):
        host.route(pb, version, seed=version)
        kr = copy.deepcopy(loop.begin_batch(version))
        rt = MapRouted(engine, torch, sets, kr, pb, pb.n_txn // G)
        for g in range(G):
            rt.objs[g].set_iops_sample(units, B.seed_of(version, g))
        loop.end_batch(version, [rt.objs[g].iops_sample()[:2] for g in range(G)])
        assert loop.history == host.history
        rt.detect(version, version - 5_000_000)
        rt.check_verdicts(oras, rt.wait(), version, version - 5_000_000)
    assert host.balancer.moves_made > 0 and loop.balancer.moves_made == host.balancer.moves_made
    assert loop.kr.hist == host.kr.hist and loop.kr.bounds == host.kr.bounds
    for cs in sets:
        cs.close()
