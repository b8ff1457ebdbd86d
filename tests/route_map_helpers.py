"""Shared by the keyResolvers-map routing tests (CPU and GPU): the numpy restatement of the kernel's
"kept iff" over fdbcs_route_map_pack's arrays, the resharding recipe with its vacuity floors, and
the per-resolver checks of test_device_routing_matches_host_routing for batches routed with
fdbcs_batch_add_routed_map."""
import copy
import ctypes

import numpy as np

from foundationdb_amd import sharding
from foundationdb_amd.packing import CommitTransaction, KeyRange
from foundationdb_amd.sharding import KeyResolvers, _range_spans


def tx(reads, writes, snap, report=False):
    return CommitTransaction([KeyRange(a, b) for a, b in reads], [KeyRange(a, b) for a, b in writes], snap, report)


def spans(kr, pb):
    """(m0, m1) of every read, then of every write, over the map's ranges."""
    R, W = pb.n_reads, pb.n_writes
    r, w = np.arange(R), np.arange(W)
    return (_range_spans(pb, 2 * r, 2 * r + 1, kr.bounds), _range_spans(pb, 2 * (R + w), 2 * (R + w) + 1, kr.bounds))


def kept_from_pack(own, until, kr, pb):
    """The kernel's predicate from one resolver's own[] / until[]: (reads kept, writes kept)."""
    (rm0, rm1), (wm0, wm1) = spans(kr, pb)
    m = np.arange(len(kr.bounds))[None, :]
    snap = np.repeat(pb.read_snapshot, np.diff(pb.read_offsets))
    newest = (own & 1) != 0
    older = (own & 2) != 0
    rin = (rm0[:, None] <= m) & (m <= rm1[:, None])
    rkeep = (rin & (newest[None, :] | (older[None, :] & (until[None, :] >= snap[:, None])))).any(1)
    win = (wm0[:, None] <= m) & (m <= wm1[:, None])
    return rkeep, (win & newest[None, :]).any(1)


def history_floors(kr, pb):
    """(reads sent to a resolver that is not a current owner of anything they meet, reads that a
    former owner of a range they meet does not receive because of their snapshot), as (read,
    resolver) pairs of the host routing."""
    (rm0, rm1), _ = spans(kr, pb)
    rmask, _ = kr.masks(pb)
    m = np.arange(len(kr.bounds))[None, :]
    rin = (rm0[:, None] <= m) & (m <= rm1[:, None])
    first = second = 0
    for g in range(kr.G):
        cur = np.array([h[-1][1] == g for h in kr.hist])
        old = np.array([any(r == g for _, r in h[:-1]) for h in kr.hist])
        got = ((rmask >> g) & 1) != 0
        first += int((got & ~(rin & cur[None, :]).any(1)).sum())
        second += int(((rin & old[None, :]).any(1) & ~got).sum())
    return first, second


def random_key(rng, alphabet, max_len):
    return bytes(int(x) for x in rng.integers(0, alphabet, size=int(rng.integers(0, max_len + 1))))


def random_move(rng, kr, alphabet, max_len, version):
    """A random key subrange to a random resolver at `version` (the master's resolverChanges)."""
    while True:
        a, b = sorted([random_key(rng, alphabet, max_len), random_key(rng, alphabet, max_len)])
        if a < b:
            break
    kr.apply_changes([(a, b, int(rng.integers(0, kr.G)))], version)


def moves_recipe(W, rng, splits, G, alphabet, max_len, Tshare=120, batches=12):
    """The issue's recipe: `batches` global batches of G shares, now += 4 each, staleness 12; a
    random move at batches 2, 4, 6, 8, 10 at version now, coalesce(now, 9) at batch 9.  Yields
    (batch, now, the map the batch is routed under)."""
    kr = KeyResolvers(G, splits)
    now = 10
    for step in range(batches):
        if step in (2, 4, 6, 8, 10):
            random_move(rng, kr, alphabet, max_len, now)
        if step == 9:
            kr.coalesce(now, 9)
        pb = W.random_small_batch(rng, G * Tshare, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
        yield pb, now, copy.deepcopy(kr)
        now += 4


# ------------------------------------------------------------------ GPU side
def dev_read_i32(engine, ptr, n):
    """n int32 of the engine's device memory (the views of fdbcs_batch_routed_info), through the
    HIP runtime the engine's library is linked against."""
    out = np.zeros(n, np.int32)
    if n:
        f = engine.load_library().hipMemcpy
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert f(out.ctypes.data, ptr, 4 * n, 2) == 0  # hipMemcpyDeviceToHost
    return out


def gather(engine, torch, pb, G, Tshare):
    shares = [engine.share_pack(pb.slice_txns(g * Tshare, (g + 1) * Tshare)) for g in range(G)]
    stride = (max(len(x) for x in shares) + 255) // 256 * 256
    host = np.zeros(G * stride, np.uint8)
    for g, x in enumerate(shares):
        host[g * stride: g * stride + len(x)] = x
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return dev, stride


class MapRouted:
    """One global batch routed on every resolver of `kr` (one conflict set each, all on one GPU)
    with add_routed_map, or with add_routed under `static_splits`.  Outputs are prefilled with 7,
    so an unwritten byte shows."""

    def __init__(self, engine, torch, sets, kr, pb, Tshare, static_splits=None, reports=False, caps=None):
        G = len(sets)
        self.pb, self.kr = pb, kr
        self.routes = kr.route(pb)
        self.dev, stride = gather(engine, torch, pb, G, Tshare)
        self.args = (self.dev.data_ptr(), stride, G, Tshare)
        self.caps = caps or (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
        self.objs, self.maps, self.outs, self.reps = [], [], [], []
        for g in range(G):
            m = {} if reports else None
            out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
            rep = torch.full((max(pb.n_reads, 1),), 7, dtype=torch.uint8, device="cuda")
            b = engine.ConflictBatch(sets[g], m)
            if static_splits is None:
                b.add_routed_map(*self.args, kr, g, self.caps, out.data_ptr(), pb.n_txn)
            else:
                lo = static_splits[g - 1] if g > 0 else None
                hi = static_splits[g] if g < G - 1 else None
                b.add_routed(*self.args, lo, hi, self.caps, out.data_ptr(), pb.n_txn)
            if reports:
                b.set_report_output(rep.data_ptr(), pb.n_reads)
            self.objs.append(b)
            self.maps.append(m)
            self.outs.append(out)
            self.reps.append(rep)

    def check_sizes(self, engine):
        """routed_info against the host routing, the read-id view against ShardBatch.read_ids."""
        self.read_ids = []
        for g, b in enumerate(self.objs):
            sub = self.routes[g].batch
            T, R, Wn, _, rid = b.routed_info()
            assert (T, R, Wn) == (sub.n_txn, sub.n_reads, sub.n_writes), f"resolver {g}"
            ids = dev_read_i32(engine, rid, R)
            np.testing.assert_array_equal(ids, self.routes[g].read_ids, err_msg=f"resolver {g}")
            self.read_ids.append(ids)

    def detect(self, now, oldest):
        for b in self.objs:
            b.detect_async(now, oldest)

    def wait(self):
        got = [b.wait() for b in self.objs]
        self.conf = [o.cpu().numpy() for o in self.outs]
        for b in self.objs:
            b.close()
        return got

    def check_verdicts(self, oras, got, now, oldest):
        """Per resolver the verdicts against its oracle fed the host routing and the device
        conflict bytes against host-built ones; their MAX against sharding.combine.  Returns the
        oracles' verdicts and maps."""
        pb = self.pb
        mx = np.zeros(pb.n_txn, np.uint8)
        vs, ms = [], []
        for g in range(len(self.objs)):
            want, wmap = oras[g].detect(self.routes[g].batch, now, oldest)
            np.testing.assert_array_equal(got[g], want, err_msg=f"resolver {g}")
            np.testing.assert_array_equal(self.conf[g], sharding.conflict_bytes(pb.n_txn, self.routes[g], want),
                                          err_msg=f"resolver {g}")
            mx = np.maximum(mx, self.conf[g])
            vs.append(want)
            ms.append(wmap)
        self.combined = sharding.combine(pb.n_txn, self.routes, vs)
        np.testing.assert_array_equal(2 - mx, self.combined)
        return vs, ms


def large_map(rng, n_ranges=300, G=4):
    """n_ranges ranges with two-byte bounds, histories 1-3 deep over G resolvers, versions 20..59."""
    vals = sorted(int(x) for x in rng.choice(65536, size=n_ranges - 1, replace=False))
    kr = KeyResolvers(G, [bytes([v >> 8, v & 255]) for v in vals], owners=[0] * n_ranges)
    for m in range(n_ranges):
        d = int(rng.integers(1, 4))
        vs = sorted(int(x) for x in rng.integers(20, 60, size=d - 1))
        kr.hist[m] = [(0 if i == 0 else vs[i - 1], int(rng.integers(0, G))) for i in range(d)]
    return kr
