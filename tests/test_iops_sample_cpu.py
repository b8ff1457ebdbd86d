"""The counter-based roll of the resolver's iops sample (balancing.iops_roll, the restatement the
device sample of fdbcs_batch_set_iops_sample is held against) and its plumbing through
ResolverLoad and BalancedRouting, on the CPU."""
import copy

import numpy as np
import pytest

from foundationdb_amd import balancing as B
from foundationdb_amd import workloads as W
from foundationdb_amd.sharding import KeyRangeSharding, KeyResolvers

M64 = (1 << 64) - 1


def mix_int(seed, i):
    """The mix in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_int(pb, units, seed):
    """iops_sample_of as a per-range loop over Python integers."""
    keys, metrics, index = [], [], []
    for i in range(pb.n_reads + pb.n_writes):
        k = pb.key(2 * i)
        metric = 100 + len(k)
        u = mix_int(seed, i) >> 32
        if metric >= units or u * units < (metric << 32):
            keys.append(k)
            metrics.append(metric if metric >= units else units)
            index.append(i)
    return keys, metrics, index


KNOWN_MIX = [
    (0, 0, 0xE220A8397B1DCDAF),
    (0, 1, 0x6E789E6AA1B965F4),
    (1, 0, 0x910A2DEC89025CC1),
    (0x0123456789ABCDEF, 12345, 0xF7527293C188657D),
    (2 ** 64 - 1, 2 ** 31 - 1, 0xE478654D2C0A5F3F),
]


@pytest.mark.parametrize("seed,i,z", KNOWN_MIX)
def test_known_answers_of_the_mix(seed, i, z):
    assert int(B.iops_mix(seed, i)) == z == mix_int(seed, i)
    hit, _ = B.iops_roll(seed, [i], [1], (1 << 31) - 1)
    assert bool(hit[0]) == ((z >> 32) * ((1 << 31) - 1) < (1 << 32))  # u is the top 32 bits of z


def test_known_counts_of_the_roll():
    i = np.arange(35000)
    got = [int(B.iops_roll(s, i, np.full(35000, 116), 20000)[0].sum()) for s in range(5)]
    assert got == [215, 199, 223, 188, 231]  # the expectation is 35000 * 116 / 20000 = 203
    i = np.arange(3000)
    for metric, n, value in [(109, 2971, 110), (110, 3000, 110), (111, 3000, 111)]:
        hit, val = B.iops_roll(3, i, np.full(3000, metric), 110)
        assert int(hit.sum()) == n
        assert set(val[hit].tolist()) == {value}


def test_units_out_of_range():
    for units in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            B.iops_roll(0, [0], [100], units)


@pytest.mark.parametrize("units", [1, 101, 103, 300, 20000])
def test_iops_sample_of_equals_the_integer_loop(units):
    rng = np.random.default_rng(units)
    empty_begins = 0
    for trial in range(4):
        pb = W.random_small_batch(rng, 60, alphabet=3, max_len=4, now=50, staleness=10)
        seed = int(rng.integers(0, 1 << 63)) * 2 + trial
        keys, metrics, index = B.iops_sample_of(pb, units, seed)
        wk, wm, wi = sample_int(pb, units, seed)
        assert keys == wk and metrics.tolist() == wm and index.tolist() == wi
        assert metrics.dtype == np.int32 and index.dtype == np.int32
        empty_begins += sum(1 for i in range(pb.n_reads + pb.n_writes) if len(pb.key(2 * i)) == 0)
    assert empty_begins > 0


def _state(load):
    return list(load.sample.keys), list(load.sample.vals), sorted(load.sample.queue)


def test_resolver_load_add_sampled():
    rng = np.random.default_rng(7)
    pb = W.random_small_batch(rng, 200, alphabet=4, max_len=3, now=50, staleness=10)
    keys, metrics, _ = B.iops_sample_of(pb, 300, 99)
    assert 20 < len(keys) < pb.n_reads + pb.n_writes
    a, b, c = (B.ResolverLoad(2, key_bytes_per_sample=300) for _ in range(3))
    a.add_batch(pb, 5.0, seed=99)
    b.add_sampled(keys, metrics, 5.0)
    assert _state(a) == _state(b)
    assert list(a.sample.queue) == list(b.sample.queue)
    assert sum(a.sample.vals) == int(metrics.sum())
    perm = rng.permutation(len(keys))
    c.add_sampled([keys[i] for i in perm], metrics[perm], 5.0)
    assert (c.sample.keys, c.sample.vals) == (a.sample.keys, a.sample.vals)
    a.poll(5.5)
    assert a.sample.keys
    a.poll(6.0)
    assert not a.sample.keys and not a.sample.vals and not a.sample.queue
    one = B.ResolverLoad(1, key_bytes_per_sample=300)  # a lone resolver keeps no sample (:178)
    one.add_sampled(keys, metrics, 5.0)
    one.add_batch(pb, 5.0, seed=99)
    assert not one.sample.keys and not one.sample.queue


def test_add_batch_without_a_seed_is_unchanged():
    """The generator-driven roll draws exactly what it drew before the seed existed."""
    rng = np.random.default_rng(8)
    pb = W.random_small_batch(rng, 100, alphabet=4, max_len=3, now=50, staleness=10)
    a = B.ResolverLoad(2, np.random.default_rng(1), key_bytes_per_sample=300)
    a.add_batch(pb, 1.0)
    n = pb.n_reads + pb.n_writes
    u = np.random.default_rng(1).random(n)
    order = []
    for t in range(pb.n_txn):
        order += [2 * (pb.n_reads + w) for w in range(pb.write_offsets[t], pb.write_offsets[t + 1])]
        order += [2 * r for r in range(pb.read_offsets[t], pb.read_offsets[t + 1])]
    want = {}
    for x, k in zip(u, order):
        key = pb.key(k)
        if x < (100 + len(key)) / 300:
            want[key] = want.get(key, 0) + 300
    assert dict(zip(a.sample.keys, a.sample.vals)) == want


def balancer_recipe(G=2):
    """test_balancer_over_engines_on_hot_keys' recipe: 40 Zipf-skewed 400-transaction batches."""
    p = W.C2Params(txns=400)
    zipf = W.ZipfGenerator(100_000)
    rng = np.random.default_rng(5)
    version = 10_000_000
    for _ in range(40):
        yield W.c3_batch(p, rng, version, zipf), version
        version += 1000


def new_routing(G=2):
    return B.BalancedRouting(G, KeyResolvers.from_sharding(KeyRangeSharding.uniform(G)), seed=3,
                             min_balance_difference=5_000, balance_time=0.005, key_bytes_per_sample=1_000)


def test_begin_end_batch_equals_route():
    G = 2
    a, b = new_routing(G), new_routing(G)
    for pb, version in balancer_recipe(G):
        a.route(pb, version, seed=version)
        kr = b.begin_batch(version)
        assert kr is b.kr
        parts = copy.deepcopy(kr).route(pb)
        b.end_batch(version, [B.iops_sample_of(parts[g].batch, 1_000, B.seed_of(version, g))[:2] for g in range(G)])
        assert a.history == b.history
    assert a.balancer.moves_made > 0 and a.history
    assert a.balancer.moves_made == b.balancer.moves_made
    assert a.kr.hist == b.kr.hist and a.kr.bounds == b.kr.bounds
    assert B.seed_of(7, 0) != B.seed_of(7, 1)


def test_route_without_a_seed_is_unchanged():
    """route(pb, version) draws from each resolver's generator as before: the same moves as a
    driver written out by hand over the public pieces."""
    G = 2
    a, b = new_routing(G), new_routing(G)
    for pb, version in balancer_recipe(G):
        a.route(pb, version)
        if b.pending:
            b.kr.apply_changes(b.pending, version)
            b.history.append((version, b.pending))
            b.pending = []
        parts = b.kr.route(pb)
        now = version / B.VERSIONS_PER_SECOND
        for g in range(G):
            b.loads[g].poll(now)
            b.loads[g].add_batch(parts[g].batch, now)
        if b.next_balance is None:
            b.next_balance = now + b.balance_time
            b.next_coalesce = now + 1.0
        if now >= b.next_balance:
            b.next_balance = now + b.balance_time
            b.pending = b.balancer.step(lambda i: b.loads[i].metrics(),
                                        lambda i, lo, hi, off, fr: b.loads[i].split(lo, hi, off, fr))
        if now >= b.next_coalesce:
            b.next_coalesce = now + 1.0
            b.kr.coalesce(version)
    assert a.history == b.history and a.balancer.moves_made > 0
