"""Shared by the routed conflicting-key report tests (CPU and GPU): the known-answer case, the
split construction of test_device_routing_matches_host_routing, and the proxy-side comparisons."""
import numpy as np

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch
from foundationdb_amd.sharding import KeyRangeSharding, combine_conflicting_keys

# the four parameter sets of test_device_routing_matches_host_routing with the oracle's own counts
# on exactly those inputs: reported transactions, proxy lists with >= 2 distinct indices, proxy
# lists holding an index twice.  The tests require at least half of each.
RANDOM_CASES = [
    ((2, 6, 3, False), (844, 371, 450)),
    ((3, 200, 3, False), (1277, 578, 913)),
    ((4, 5, 24, True), (1677, 852, 1378)),
    ((1, 6, 3, False), (405, 151, 0)),
]


def _tx(reads, writes, snap, report):
    return CommitTransaction([KeyRange(a, b) for a, b in reads], [KeyRange(a, b) for a, b in writes], snap, report)


def known_answer():
    """Two resolvers split at b"m", shares of 2 transactions.  Per batch: (packed batch, now, new
    oldest, combined verdicts, local resolver maps, report bytes per resolver, proxy lists)."""
    b1 = PackedBatch.from_transactions([
        _tx([], [(b"a", b"b"), (b"x", b"y")], 9, False),
        _tx([(b"c", b"d"), (b"a", b"b"), (b"x", b"y")], [], 9, True),
        _tx([(b"k", b"p")], [(b"l", b"n")], 9, True),
        _tx([(b"a", b"a")], [], 9, True),
    ])
    b2 = PackedBatch.from_transactions([
        _tx([(b"e", b"f"), (b"k", b"p"), (b"a", b"b")], [], 5, True),
        _tx([(b"k", b"p")], [], 10, True),
        _tx([(b"q", b"r")], [(b"q", b"r")], 0, True),
        _tx([], [(b"z", b"zz")], 0, True),
    ])
    return [
        (b1, 10, 1, [2, 0, 2, 2], [{1: [1], 2: [], 3: []}, {1: [0], 2: []}],
         [[0, 1, 0, 0, 0], [0, 0, 1, 0, 0]], {1: [1, 2]}),
        (b2, 20, 2, [0, 2, 1, 2], [{0: [1, 2], 1: []}, {0: [0], 1: []}],
         [[0, 1, 1, 0, 0], [0, 1, 0, 0, 0]], {0: [1, 2, 1]}),
    ]


KNOWN_SPLITS = [b"m"]
KNOWN_TSHARE = 2


def make_splits(rng, G, alphabet, long_split):
    """The split keys of test_device_routing_matches_host_routing (same draws from `rng`)."""
    letters = sorted(set(int(x) for x in rng.integers(1, alphabet, size=3 * G)))[: G - 1]
    while len(letters) < G - 1:
        letters.append(letters[-1] + 1 if letters else 1)
    splits = [bytes([x]) for x in sorted(set(letters))][: G - 1]
    if long_split and G > 2:
        splits[1] = bytes([splits[1][0]] * 20)
        splits = sorted(set(splits))
    return splits


def sorted_map(m):
    return {int(t): sorted(int(i) for i in v) for t, v in m.items()}


def bytes_as_sets(pb, c):
    """Report bytes over the batch's reads -> {transaction: sorted read indices} of the ones."""
    out = {}
    owner = np.repeat(np.arange(pb.n_txn), np.diff(pb.read_offsets))
    for g in np.flatnonzero(np.asarray(c)).tolist():
        t = int(owner[g])
        out.setdefault(t, []).append(g - int(pb.read_offsets[t]))
    return out


def proxy_sets(pb, routes, maps, combined):
    """(the proxy's lists, {transaction: sorted set of its list} without the empty ones)."""
    lists = combine_conflicting_keys(pb, routes, maps, combined)
    return lists, {t: sorted(set(v)) for t, v in lists.items() if v}


class Floors:
    """Counts that keep the random tests from passing vacuously."""

    def __init__(self):
        self.reported = self.multi = self.dup = 0

    def add(self, lists):
        for v in lists.values():
            self.reported += 1
            self.multi += len(set(v)) >= 2
            self.dup += len(set(v)) < len(v)

    def check(self, G, want):
        assert self.reported >= want[0] / 2, (self.reported, want)
        assert self.multi >= want[1] / 2, (self.multi, want)
        if G > 1:
            assert self.dup >= want[2] / 2, (self.dup, want)
