"""A proxy's share packed on the GPU from device-resident arrays (fdbcs_batch_share_pack_device)
against fdbcs_share_pack, byte for byte, and routed end to end from a gather buffer the device
packed.  The output sits between 64 bytes of 0xFF poison and is itself prefilled with 0xFF (an
unwritten gap byte shows as a mismatch with the host's zeroed buffer); the input arrays are staged
with their own poison (device_add_helpers.Staged)."""
import numpy as np
import pytest

from foundationdb_amd.packing import DevicePackedBatch, InvertedRange, PackedBatch
from foundationdb_amd.sharding import KeyRangeSharding, KeyResolvers
from tests.device_add_helpers import POISON, Staged, keys_of, repack
from tests.route_map_helpers import MapRouted, tx
from tests.routed_report_helpers import make_splits, sorted_map

pytestmark = pytest.mark.gpu

EMPTY = 320  # the empty share: header, roff[0], woff[0] and the tail slack


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch

    return torch


@pytest.fixture(scope="module")
def cs(engine):
    s = engine.ConflictSet(0)
    yield s
    s.close()


class Out:
    """cap bytes of device memory at a 64-byte aligned address, 0xFF all over, poison on both sides."""

    def __init__(self, torch, cap):
        self.torch, self.cap = torch, cap
        self.t = torch.full((POISON + cap + POISON,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() + POISON
        assert self.ptr % 64 == 0

    def host(self):
        self.torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def body(self):
        return self.host()[POISON: POISON + self.cap]

    def intact(self):
        h = self.host()
        return bool((h[:POISON] == 0xFF).all() and (h[-POISON:] == 0xFF).all())

    def untouched(self):
        return bool((self.host() == 0xFF).all())


def header(buf):
    """(bytes, T, R, W, tail_bytes) of a share's header: what share_pack_info returns."""
    T, R, Wn = (int(x) for x in np.frombuffer(buf[:12].tobytes(), np.int32))
    h = np.frombuffer(buf[:128].tobytes(), np.int64)
    return int(h[2]), T, R, Wn, int(h[9])


def empty_share(engine):
    e = engine.share_pack(PackedBatch.from_transactions([]))
    assert len(e) == EMPTY and header(e) == (EMPTY, 0, 0, 0, 0)
    return e


def bound_of(engine, pb):
    return engine.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, len(pb.key_bytes))


def status(engine, f, *a):
    with pytest.raises(engine.FdbcsError) as e:
        f(*a)
    return e.value.status


def check_pack(engine, torch, cs, pb, extra=0, report=False, **stage):
    """pb packed by the device into a fresh buffer of bound + extra bytes on a new batch: the share
    equals the host's, _info its header, and both poisons are intact.  Returns the host's share."""
    want = engine.share_pack(pb)
    st = Staged(torch, pb, **stage)
    cap = engine.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, st.dpb.key_bytes_len) + extra
    assert cap >= len(want)
    out = Out(torch, cap)
    b = engine.ConflictBatch(cs, {} if report else None)
    b.share_pack_device(st.dpb, out.ptr, cap)
    info = b.share_pack_info()
    got = out.body()[: info[0]]
    assert info == header(want) and info[0] == len(want)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert out.intact() and st.intact(torch)
    kern, host = b.share_pack_timing()
    assert kern > 0 and host > 0
    b.close()
    return want


# ---- 1. byte identity


def rng_key(rng, n, first=None):
    k = bytes(rng.integers(1, 250, size=n, dtype=np.uint8).tolist())
    return k if first is None or n == 0 else bytes([first]) + k[1:]


def ordered(a, b):
    return (a, b) if a <= b else (b, a)


LENGTHS = [0, 1, 15, 16, 17, 23, 24, 25, 31, 32, 33, 64, 65, 200]


def mixed_batch(seed=1):
    """Ranges over every key length of LENGTHS in shuffled order, several per transaction."""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.permutation(np.repeat(LENGTHS, 8))]
    rs = [ordered(rng_key(rng, lens[2 * i]), rng_key(rng, lens[2 * i + 1])) for i in range(len(lens) // 2)]
    txns, i = [], 0
    while i < len(rs):
        n = int(rng.integers(1, 5))
        part = rs[i: i + n]
        txns.append(tx(part[::2], part[1::2], int(rng.integers(1, 100)), bool(rng.integers(0, 2))))
        i += n
    return PackedBatch.from_transactions(txns)


def tail_residues(share):
    """Destination byte residues (mod 8) of the tails of a share's long keys, and the tail lengths
    in key order."""
    _, _, R, Wn, _ = header(share)
    h = np.frombuffer(share[:128].tobytes(), np.int64)
    off_keys, off_tail = int(h[3]), int(h[8])
    rec = np.frombuffer(share[off_keys: off_keys + 48 * (R + Wn)].tobytes(), np.uint32).reshape(-1, 6)
    long_ = rec[:, 4] > 16
    return set(((off_tail + rec[long_, 5]) % 8).tolist()), (rec[long_, 4] - 16).tolist()


def adjacent_tails_batch():
    """Keys whose tails of 1, 7, 8, 9 and 17 bytes lie next to each other, twice, the second time
    one byte further."""
    rng = np.random.default_rng(2)
    ks = [rng_key(rng, n, first=0x20 + i) for i, n in enumerate([17, 23, 24, 25, 33, 18, 17, 23, 24, 25, 33, 40])]
    return PackedBatch.from_transactions([tx([(ks[0], ks[1]), (ks[2], ks[3]), (ks[4], ks[5])], [], 7, True),
                                          tx([(ks[6], ks[7]), (ks[8], ks[9]), (ks[10], ks[11])], [], 8)])


def empty_runs_batch():
    rng = np.random.default_rng(3)

    def t(nr, nw):
        rr = lambda: (lambda a: (a, a + b"\x01"))(rng_key(rng, int(rng.integers(1, 30))))
        return tx([rr() for _ in range(nr)], [rr() for _ in range(nw)], int(rng.integers(1, 50)), bool(rng.integers(0, 2)))

    e = lambda n: [t(0, 0) for _ in range(n)]
    return PackedBatch.from_transactions(e(3) + [t(1, 1), t(0, 2)] + e(70) + [t(2, 0), t(0, 1)] + e(2) + [t(1, 0)] + e(4))


def big_txn_batch():
    rng = np.random.default_rng(4)
    rr = lambda: (lambda a: (a, a + b"\x00"))(rng_key(rng, int(rng.integers(10, 30))))
    return PackedBatch.from_transactions([tx([rr()], [rr()], 5), tx([rr() for _ in range(450)], [rr() for _ in range(150)], 6, True),
                                          tx([rr()], [rr()], 7)])


def one_sided_batch(reads):
    rng = np.random.default_rng(5 + reads)
    rr = lambda: (lambda a: (a, a + b"\x00"))(rng_key(rng, int(rng.integers(0, 40))))
    return PackedBatch.from_transactions([tx([rr(), rr()] if reads else [], [] if reads else [rr(), rr()], 5 + i, bool(i & 1))
                                          for i in range(9)])


def test_mixed_lengths_and_all_tail_residues(engine, torch_mod, cs):
    pb = mixed_batch()
    want = check_pack(engine, torch_mod, cs, pb)
    res, _ = tail_residues(want)
    assert res == set(range(8))
    assert set(np.diff(pb.key_offsets).tolist()) == set(LENGTHS)


def test_adjacent_short_tails(engine, torch_mod, cs):
    want = check_pack(engine, torch_mod, cs, adjacent_tails_batch())
    assert tail_residues(want)[1] == [1, 7, 8, 9, 17, 2, 1, 7, 8, 9, 17, 24]


@pytest.mark.parametrize("shift", range(8))
def test_arena_at_every_byte_alignment(engine, torch_mod, cs, shift):
    check_pack(engine, torch_mod, cs, mixed_batch(10 + shift), shift=shift, base=5 + shift)


@pytest.mark.parametrize("with_report", [True, False])
@pytest.mark.parametrize("collects", [True, False])
def test_report_flags_given_and_null(engine, torch_mod, cs, with_report, collects):
    """The flags are copied whether or not the batch collects reports; a NULL array packs zeros
    (the host's share of the same batch with no flag set)."""
    pb = mixed_batch(20)
    assert pb.report.any()
    if not with_report:
        want = engine.share_pack(repack(pb, report=np.zeros_like(pb.report)))
        st = Staged(torch_mod, pb, with_report=False)
        out = Out(torch_mod, bound_of(engine, pb))
        b = engine.ConflictBatch(cs, {} if collects else None)
        b.share_pack_device(st.dpb, out.ptr, out.cap)
        n = b.share_pack_info()[0]
        assert np.array_equal(out.body()[:n], want) and out.intact() and st.intact(torch_mod)
        b.close()
    else:
        check_pack(engine, torch_mod, cs, pb, report=collects)


@pytest.mark.parametrize("name,make", [("empty_runs", empty_runs_batch), ("txn_of_600_ranges", big_txn_batch),
                                       ("reads_only", lambda: one_sided_batch(True)),
                                       ("writes_only", lambda: one_sided_batch(False)),
                                       ("T0", lambda: PackedBatch.from_transactions([]))])
def test_shapes(engine, torch_mod, cs, name, make):
    pb = make()
    want = check_pack(engine, torch_mod, cs, pb, extra=192)
    if name == "T0":
        assert np.array_equal(want, empty_share(engine))
    if name == "empty_runs":  # the owner of a range after a run of empty transactions is the run's last + 1
        _, T, R, Wn, _ = header(want)
        assert T == pb.n_txn and (np.diff(pb.read_offsets) == 0).sum() > 70


@pytest.mark.parametrize("n_ranges", [127, 128, 129, 511, 512, 513])
def test_key_counts_around_the_scan_tile(engine, torch_mod, cs, n_ranges):
    """2 (R + W) = 254 | 256 | 258 and 1022 | 1024 | 1026 keys, straddling one and four 256-key scan
    tiles; then with one transaction more than keys, so that the scan's last elements are offset
    entries past the keys."""
    rng = np.random.default_rng(n_ranges)
    rs = [(lambda a: (a, a + b"\x00"))(rng_key(rng, int(rng.integers(14, 28)))) for _ in range(n_ranges)]
    txns = [tx([rs[0]], [], 5, True)] + [tx([r], [], 6) if i % 3 else tx([], [r], 5, True) for i, r in enumerate(rs[1:])]
    for pad in (0, 2 * n_ranges - len(txns) + 1):
        pb = PackedBatch.from_transactions(txns + [tx([], [], 5)] * pad)
        assert pad == 0 or pb.n_txn + 1 > 2 * n_ranges
        check_pack(engine, torch_mod, cs, pb)


# ---- 2. routing end to end


class DevPacked(MapRouted):
    """MapRouted over a gather buffer that each resolver's batch handle packed its own share into
    (device=True: share_pack_device at gather + g * stride, stride from share_bytes_bound; then
    the same handles are routed), or over the host-packed twin of that buffer."""

    def __init__(self, engine, torch, sets, kr, pb, Tshare, static_splits=None, device=True):
        G = len(sets)
        self.pb, self.kr = pb, kr
        self.routes = kr.route(pb)
        parts = [pb.slice_txns(g * Tshare, (g + 1) * Tshare) for g in range(G)]
        stride = max(bound_of(engine, p) for p in parts)
        assert stride % 64 == 0
        self.gbuf = Out(torch, G * stride)
        self.caps = (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
        self.maps = [{} for _ in range(G)]
        self.objs = [engine.ConflictBatch(sets[g], self.maps[g]) for g in range(G)]
        self.staged = []
        if device:
            for g, b in enumerate(self.objs):
                st = Staged(torch, parts[g], shift=g, base=3 * g)
                b.share_pack_device(st.dpb, self.gbuf.ptr + g * stride, stride)
                self.staged.append(st)
            for g, b in enumerate(self.objs):
                assert b.share_pack_info() == header(engine.share_pack(parts[g]))
        else:
            host = np.zeros(G * stride, np.uint8)
            for g, p in enumerate(parts):
                x = engine.share_pack(p)
                host[g * stride: g * stride + len(x)] = x
            self.gbuf.t[POISON: POISON + G * stride] = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
        self.args = (self.gbuf.ptr, stride, G, Tshare)
        self.outs, self.reps = [], []
        for g, b in enumerate(self.objs):
            out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
            rep = torch.full((max(pb.n_reads, 1),), 7, dtype=torch.uint8, device="cuda")
            if static_splits is None:
                b.add_routed_map(*self.args, kr, g, self.caps, out.data_ptr(), pb.n_txn)
            else:
                lo = static_splits[g - 1] if g > 0 else None
                hi = static_splits[g] if g < G - 1 else None
                b.add_routed(*self.args, lo, hi, self.caps, out.data_ptr(), pb.n_txn)
            b.set_report_output(rep.data_ptr(), pb.n_reads)
            self.outs.append(out)
            self.reps.append(rep)


@pytest.mark.parametrize("mapped", [False, True])
def test_routing_end_to_end_from_a_device_packed_gather_buffer(engine, oracle_built, torch_mod, mapped):
    from foundationdb_amd import sharding
    from foundationdb_amd import workloads as W

    torch = torch_mod
    G, Tshare, alphabet, max_len = 3, 120, 5, 24
    rng = np.random.default_rng(41 + mapped)
    splits = make_splits(rng, G, alphabet, False)
    kr = KeyResolvers.from_sharding(KeyRangeSharding(splits))
    if mapped:  # the start of resolver 1's range moved to resolver 0 at version 12: batches at now = 10, 14, 18
        kr.apply_changes([(splits[0], splits[0] + b"\x02", 0)], 12)
        assert [r for _, r in kr.hist[1]] == [1, 0] and len(kr.bounds) == G + 1
    sets_d = [engine.ConflictSet(0) for _ in range(G)]
    sets_h = [engine.ConflictSet(0) for _ in range(G)]
    oras = [oracle_built.OracleConflictSet() for _ in range(G)]
    seen, now = set(), 10
    reported = 0
    for _ in range(3):
        pb = W.random_small_batch(rng, G * Tshare, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
        assert int(np.diff(pb.key_offsets).max()) > 16
        st = None if mapped else splits
        d = DevPacked(engine, torch, sets_d, kr, pb, Tshare, static_splits=st, device=True)
        h = DevPacked(engine, torch, sets_h, kr, pb, Tshare, static_splits=st, device=False)
        body_d, body_h, stride = d.gbuf.body(), h.gbuf.body(), d.args[1]
        for g in range(G):
            n = header(body_h[g * stride:])[0]
            assert np.array_equal(body_d[g * stride: g * stride + n], body_h[g * stride: g * stride + n]), g
        d.check_sizes(engine)
        h.check_sizes(engine)
        d.detect(now, now - 9)
        h.detect(now, now - 9)
        got_d, got_h = d.wait(), h.wait()
        vs, ms = d.check_verdicts(oras, got_d, now, now - 9)
        mx = np.zeros(pb.n_reads, np.uint8)
        for g in range(G):
            np.testing.assert_array_equal(got_d[g], got_h[g])
            np.testing.assert_array_equal(d.conf[g], h.conf[g])
            np.testing.assert_array_equal(d.read_ids[g], h.read_ids[g])
            rep_d, rep_h = d.reps[g].cpu().numpy()[: pb.n_reads], h.reps[g].cpu().numpy()[: pb.n_reads]
            np.testing.assert_array_equal(rep_d, rep_h)
            np.testing.assert_array_equal(rep_d, sharding.report_bytes(pb, d.routes[g], ms[g]), err_msg=f"resolver {g}")
            assert sorted_map(d.maps[g]) == sorted_map(h.maps[g]) == sorted_map(ms[g])
            mx = np.maximum(mx, rep_d)
        reported += int(mx.sum())
        seen |= set(d.combined.tolist())
        assert d.gbuf.intact() and all(s.intact(torch) for s in d.staged)
        now += 4
    assert seen == {0, 1, 2} and reported > 0  # conflicts (history ones from batch 2 on), TooOld, commits
    for s in sets_d + sets_h:
        s.close()


# ---- 3. four in flight


def test_four_packs_in_flight_beside_detects(engine, oracle_built, torch_mod):
    """One resolver, one share per batch: the packs of batches i + 1 .. i + 3 are enqueued while
    batch i is detected, each into its own gather buffer; batch 2's arrays are still being copied
    by a torch stream when its pack is enqueued behind the ready flag that stream sets."""
    from foundationdb_amd import workloads as W

    torch = torch_mod
    rng = np.random.default_rng(6)
    seq = [(W.random_small_batch(rng, 150, alphabet=5, max_len=24, now=10 + 4 * i, staleness=12), 10 + 4 * i, 1 + 4 * i)
           for i in range(8)]
    caps = lambda pb: (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)

    def route(b, out, pb):
        b.add_routed(out.ptr, out.cap, 1, pb.n_txn, None, None, caps(pb))

    serial_set, ora = engine.ConflictSet(0), oracle_built.OracleConflictSet()
    want, shares = [], []
    for pb, now, oldest in seq:
        st, out = Staged(torch, pb), Out(torch, bound_of(engine, pb))
        b = engine.ConflictBatch(serial_set)
        b.share_pack_device(st.dpb, out.ptr, out.cap)
        n = b.share_pack_info()[0]
        shares.append(out.body()[:n].copy())
        route(b, out, pb)
        b.detect_async(now, oldest)  # (a routed batch's verdict count is known to wait())
        want.append(b.wait().tolist())
        b.close()
        # (a routed batch holds the transactions that have a range: the host routing's sub-batch)
        assert want[-1] == ora.detect(KeyResolvers(1).route(pb)[0].batch, now, oldest)[0].tolist()
    assert any(0 in w for w in want) and any(1 in w for w in want)

    pipe = engine.ConflictSet(0)
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bs = [engine.ConflictBatch(pipe) for _ in seq]
    outs = [Out(torch, bound_of(engine, pb)) for pb, _, _ in seq]
    # staged ahead (a staging's synchronize would drain the batches in flight), all but batch 2
    stg = [Staged(torch, pb, shift=i % 8) if i != 2 else None for i, (pb, _, _) in enumerate(seq)]

    def pack(i):
        if i == 2:
            stg[i] = Staged(torch, seq[i][0], shift=i % 8, sync=False)
            flag.fill_(9)  # on the stream of the copies, after them; no synchronize before the call
            bs[i].share_pack_device(stg[i].dpb, outs[i].ptr, outs[i].cap, flag.data_ptr(), 9)
        else:
            bs[i].share_pack_device(stg[i].dpb, outs[i].ptr, outs[i].cap)

    for i in range(min(4, len(seq))):
        pack(i)
    for i, (pb, now, oldest) in enumerate(seq):
        n = bs[i].share_pack_info()[0]
        route(bs[i], outs[i], pb)
        bs[i].detect_async(now, oldest)
        if i + 4 < len(seq):
            pack(i + 4)  # batches i + 1 .. i + 3 are packing or packed; this one joins while i is detected
        assert n == len(shares[i])
    got = [b.wait().tolist() for b in bs]
    assert got == want
    for i, b in enumerate(bs):
        assert np.array_equal(outs[i].body()[: len(shares[i])], shares[i]) and outs[i].intact() and stg[i].intact(torch)
        b.close()
    a, c = serial_set.dump_history(), pipe.dump_history()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], c[:3])) and a[3] == c[3]
    serial_set.close()
    pipe.close()


# ---- 4. rejections


def valid_batch():
    k16 = bytes(range(0x30, 0x40))
    k40 = bytes(range(0x50, 0x78))
    return PackedBatch.from_transactions([
        tx([(b"a", b"b")], [(b"c", b"d")], 100, True),
        tx([(k16, k16 + b"\x00"), (b"e", b"f")], [(k40, k40[:-1] + b"\x79")], 100),
        tx([(b"g", b"h")], [(b"i", b"j"), (b"k", b"l")], 3, True),  # TooOld once the oldest version is 50
        tx([], [(b"m", b"n")], 100),
    ])


def swapped(pb, r):
    k = keys_of(pb)
    k[2 * r], k[2 * r + 1] = k[2 * r + 1], k[2 * r]
    assert k[2 * r] > k[2 * r + 1]
    return repack(pb, keys=k)


def off(pb, name, i, v):
    a = getattr(pb, name).copy()
    a[i] = v
    return repack(pb, **{name: a})


def rejections():
    pb = valid_batch()
    ko = pb.key_offsets
    return {
        "first_write_offset_is_1": off(pb, "write_offsets", 0, 1),
        "first_read_offset_is_1": off(pb, "read_offsets", 0, 1),
        "read_offset_decreases": off(pb, "read_offsets", 2, 0),
        "last_read_offset_is_not_R": (off(pb, "read_offsets", 4, 5), (4, 5)),
        "last_write_offset_is_not_W": (off(pb, "write_offsets", 4, 4), (4, 5)),
        "key_offset_past_the_arena": off(pb, "key_offsets", len(ko) - 1, int(ko[-1]) + 8),
        "key_offset_decreases": off(pb, "key_offsets", 5, int(ko[4]) - 1),
        "inverted_in_the_prefix": swapped(pb, 0),
        "inverted_in_the_tail": swapped(pb, 4 + 1),
        "inverted_with_a_stale_snapshot": swapped(pb, 3),
    }


REJECT = rejections()


def assert_empty_share_only(engine, out):
    body = out.body()
    assert np.array_equal(body[:EMPTY], empty_share(engine))
    assert (body[EMPTY:] == 0xFF).all() and out.intact()


@pytest.mark.parametrize("name", list(REJECT))
def test_rejections(engine, oracle_built, torch_mod, name):
    torch = torch_mod
    bad, sizes = REJECT[name] if isinstance(REJECT[name], tuple) else (REJECT[name], None)
    good = valid_batch()
    cs, o = engine.ConflictSet(0), oracle_built.OracleConflictSet()
    for s in (cs, o):
        s.set_oldest_version(50)
    prefill = PackedBatch.from_transactions([tx([], [(b"a", b"c")], 60)])
    b0 = engine.ConflictBatch(cs)
    b0.add_packed(prefill)
    b0.detect_conflicts(105, 50)
    b0.close()
    o.detect(prefill, 105, 50)
    before = cs.dump_history()
    st = Staged(torch, bad, sizes=sizes)
    out = Out(torch, bound_of(engine, good) + 128)
    m = {}
    b = engine.ConflictBatch(cs, m)
    b.share_pack_device(st.dpb, out.ptr, out.cap)
    caps = (good.n_txn, good.n_reads, good.n_writes, good.tail_bytes)
    if name == "inverted_in_the_prefix":  # the routed add straight after the bad pack returns its error
        with pytest.raises(InvertedRange):  # (the binding's exception for FDBCS_E_INVALID from an add)
            b.add_routed(out.ptr, out.cap, 1, good.n_txn, None, None, caps)
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_INVALID
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_INVALID  # until the next pack
    assert_empty_share_only(engine, out)
    assert st.intact(torch)
    after = cs.dump_history()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[:3], after[:3])) and before[3] == after[3]
    # the same handle packs the valid batch and routes it
    st2 = Staged(torch, good)
    b.share_pack_device(st2.dpb, out.ptr, out.cap)
    want = engine.share_pack(good)
    assert b.share_pack_info() == header(want)
    assert np.array_equal(out.body()[: len(want)], want)
    b.add_routed(out.ptr, out.cap, 1, good.n_txn, None, None, caps)
    b.detect_async(120, 50)
    v = b.wait()
    wv, conf = o.detect(good, 120, 50)
    assert v.tolist() == wv.tolist() == [0, 2, 1, 2] and sorted_map(m) == sorted_map(conf) == {0: [0]}
    assert out.intact() and st2.intact(torch)
    b.close()
    cs.close()


def test_routed_add_after_a_reported_error_routes_the_empty_share(engine, torch_mod, cs):
    """The routed add returns a pack's error only while nobody has waited for the pack: once
    share_pack_info has reported it, the buffer holds the empty share and routes as no
    transactions."""
    good = valid_batch()
    st, out = Staged(torch_mod, REJECT["inverted_in_the_tail"]), Out(torch_mod, bound_of(engine, good))
    b = engine.ConflictBatch(cs)
    b.share_pack_device(st.dpb, out.ptr, out.cap)
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_INVALID
    b.add_routed(out.ptr, out.cap, 1, good.n_txn, None, None, (good.n_txn, good.n_reads, good.n_writes, good.tail_bytes))
    assert b.routed_info()[:3] == (0, 0, 0)
    assert_empty_share_only(engine, out)
    b.close()


def test_exact_size_one_step_over_cap(engine, torch_mod, cs):
    good = valid_batch()
    exact = len(engine.share_pack(good))
    cap = exact - 64
    assert cap >= engine.share_bytes_bound(good.n_txn, good.n_reads, good.n_writes, 0) and good.tail_bytes > 0
    st, out = Staged(torch_mod, good), Out(torch_mod, cap)
    b = engine.ConflictBatch(cs)
    b.share_pack_device(st.dpb, out.ptr, cap)
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_NOMEM
    assert_empty_share_only(engine, out)
    out2 = Out(torch_mod, exact)  # exactly enough
    b.share_pack_device(st.dpb, out2.ptr, exact)
    assert b.share_pack_info()[0] == exact and np.array_equal(out2.body(), engine.share_pack(good)) and out2.intact()
    b.close()


def test_ready_flag_never_set_times_out(engine, torch_mod, monkeypatch):
    monkeypatch.setenv("FDBCS_ROUTE_TIMEOUT_MS", "50")
    s = engine.ConflictSet(0)
    good = valid_batch()
    never = torch_mod.zeros(1, dtype=torch_mod.int32, device="cuda")
    st, out = Staged(torch_mod, good), Out(torch_mod, bound_of(engine, good))
    b = engine.ConflictBatch(s)
    b.share_pack_device(st.dpb, out.ptr, out.cap, never.data_ptr(), 1)
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_TIMEOUT
    assert_empty_share_only(engine, out)
    b.share_pack_device(st.dpb, out.ptr, out.cap, never.data_ptr(), 0)  # the flag's value now
    assert b.share_pack_info() == header(engine.share_pack(good))
    b.close()
    s.close()


# ---- 5. host refusals and state


def test_host_side_refusals_write_nothing(engine, torch_mod, cs):
    good = valid_batch()
    st = Staged(torch_mod, good)
    d = st.dpb
    floor = engine.share_bytes_bound(good.n_txn, good.n_reads, good.n_writes, 0)
    out = Out(torch_mod, bound_of(engine, good))
    b = engine.ConflictBatch(cs)
    assert status(engine, b.share_pack_device, d, 0, out.cap) == engine.FDBCS_E_INVALID
    assert status(engine, b.share_pack_device, d, out.ptr + 8, out.cap - 8) == engine.FDBCS_E_INVALID
    assert status(engine, b.share_pack_device, d, out.ptr + 32, out.cap - 32) == engine.FDBCS_E_INVALID
    assert status(engine, b.share_pack_device, d, out.ptr, floor - 64) == engine.FDBCS_E_NOMEM
    assert status(engine, b.share_pack_device, d, out.ptr, floor - 1) == engine.FDBCS_E_NOMEM
    bad = lambda **kw: DevicePackedBatch(**{**d.__dict__, **kw})
    assert status(engine, b.share_pack_device, bad(n_txn=0), out.ptr, EMPTY - 64) == engine.FDBCS_E_NOMEM
    for kw in ({"n_txn": -1}, {"n_reads": -1}, {"n_writes": -1}, {"key_bytes_len": -1}, {"read_offsets": 0},
               {"write_offsets": 0}, {"read_snapshot": 0}, {"key_offsets": 0}, {"key_bytes": 0}, {"n_txn": 49153}):
        assert status(engine, b.share_pack_device, bad(**kw), out.ptr, 1 << 24) == engine.FDBCS_E_INVALID, kw
    assert status(engine, b.share_pack_device, bad(key_bytes_len=1 << 32), out.ptr, 1 << 40) == engine.FDBCS_E_NOMEM
    assert status(engine, b.share_pack_device, bad(n_reads=1 << 27, n_writes=1 << 27), out.ptr, 1 << 40) == engine.FDBCS_E_NOMEM
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_STATE  # never packed
    assert status(engine, b.share_pack_timing) == engine.FDBCS_E_STATE
    cs.sync()
    assert out.untouched() and st.intact(torch_mod)
    b.close()


def test_states(engine, torch_mod, cs):
    good = valid_batch()
    st = Staged(torch_mod, good)
    d = st.dpb
    out = Out(torch_mod, bound_of(engine, good))
    caps = (good.n_txn, good.n_reads, good.n_writes, good.tail_bytes)
    pack = lambda b: b.share_pack_device(d, out.ptr, out.cap)
    # a batch that holds something
    b = engine.ConflictBatch(cs)
    b.add_packed(good)
    assert status(engine, pack, b) == engine.FDBCS_E_STATE
    assert status(engine, b.share_pack_info) == engine.FDBCS_E_STATE
    b.close()
    # a device-added batch
    b = engine.ConflictBatch(cs)
    b.add_packed_device(d)
    assert status(engine, pack, b) == engine.FDBCS_E_STATE
    b.device_add_info()
    assert status(engine, pack, b) == engine.FDBCS_E_STATE
    b.close()
    assert out.untouched()
    # after a pack: no add but a routed one
    b = engine.ConflictBatch(cs)
    pack(b)
    assert status(engine, b.add_packed, good) == engine.FDBCS_E_STATE
    assert status(engine, b.add_transaction, good.to_transactions()[0]) == engine.FDBCS_E_STATE
    assert status(engine, b.add_packed_device, d) == engine.FDBCS_E_STATE
    assert b.share_pack_info() == header(engine.share_pack(good))
    assert status(engine, b.add_packed, good) == engine.FDBCS_E_STATE
    assert status(engine, b.add_packed_device, d) == engine.FDBCS_E_STATE
    pack(b)  # a further pack once _info has returned
    b.add_routed(out.ptr, out.cap, 1, good.n_txn, None, None, caps)  # waits for that pack itself
    assert b.share_pack_info() == header(engine.share_pack(good))
    assert status(engine, pack, b) == engine.FDBCS_E_STATE  # routed
    assert b.routed_info()[:3] == (good.n_txn, good.n_reads, good.n_writes)
    b.detect_async(1000, 0)
    v = b.wait()
    assert len(v) == good.n_txn
    assert status(engine, pack, b) == engine.FDBCS_E_STATE  # detected
    b.close()
    assert st.intact(torch_mod) and out.intact()
