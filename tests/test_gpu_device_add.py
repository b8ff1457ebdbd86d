"""Whole batches added from device memory (fdbcs_batch_add_packed_device): the raw arrays of a
packed batch, staged as torch device tensors, against the same batch added from the host
(add_packed) on a second set and against the semantic oracle."""
import numpy as np
import pytest

from foundationdb_amd.packing import CommitTransaction, DevicePackedBatch, KeyRange, PackedBatch
from tests import device_add_plan as P
from tests.device_add_helpers import Staged, Trio, keys_of, random_batch, repack
from tests.export_helpers import split_dump

pytestmark = pytest.mark.gpu

TILE = 256  # ingest.h kIngestTile: keys per workgroup of the add's scan (one per thread)


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch

    return torch


@pytest.fixture()
def trio(engine, oracle_built, torch_mod):
    t = Trio(engine, oracle_built, torch_mod)
    yield t
    t.close()


def rng_key(rng, n):
    return bytes(rng.integers(1, 250, size=n, dtype=np.uint8).tolist())


def tx(reads, writes, snap, report=False):
    return CommitTransaction([KeyRange(a, b) for a, b in reads], [KeyRange(a, b) for a, b in writes], snap, report)


# ---- 1. plan parity


def test_plan_parity(engine, oracle_built, torch_mod):
    t = Trio(engine, oracle_built, torch_mod, P.history())
    wants = [P.want_read_verdicts(), None, None]
    for i, (pb, now, oldest) in enumerate(P.sequence()):
        v = t.step(pb, now, oldest, what=i)
        if wants[i] is not None:
            np.testing.assert_array_equal(v, wants[i])
        t.check_state(i)
    # the dump holds the written keys' original bytes
    _, keys, vers = split_dump(t.d.dump_history())
    at = dict(zip(keys, vers))
    assert all(at.get(k) == P.NOW_WRITES for k in P.write_keys())
    t.close()


# ---- 2. alignment


def test_alignment_of_the_key_arena(engine, oracle_built, torch_mod):
    """The plan's read batch with key_bytes starting 0..7 bytes into its tensor, key_offsets[0]
    non-zero in half the runs, and the arena ending flush against the poison with a 16-byte and
    with a 17-byte key."""
    base = P.read_batch()
    k16, k17 = b"\x7e" * 15 + b"\x01", b"\x7e" * 15 + b"\x01\x02"
    seen = []
    for shift in range(8):
        last = k16 if shift % 2 else k17
        txns = base.to_transactions() + [tx([(b"\x7e", last)], [], P.NOW_READS, True)]
        pb = PackedBatch.from_transactions(txns)
        assert keys_of(pb)[2 * pb.n_reads - 1] == last and pb.n_writes == 0  # the arena's last key
        t = Trio(engine, oracle_built, torch_mod, P.history())
        v = t.step(pb, P.NOW_READS, P.OLDEST_AFTER_READS, what=shift, shift=shift, base=(5 if shift >= 4 else 0))
        np.testing.assert_array_equal(v[:-1], P.want_read_verdicts())
        seen.append(v.tolist())
        t.close()
    assert all(s == seen[0] for s in seen)


# ---- 3. shapes


def shape_batches():
    rng = np.random.default_rng(3)

    def rr():  # (keys of 1..29 bytes; the prefill's version is 10)
        a = rng_key(rng, int(rng.integers(1, 30)))
        return (a, a + b"\x01")

    def t(nr, nw, snap=None):
        return tx([rr() for _ in range(nr)], [rr() for _ in range(nw)], int(rng.choice([5, 15])) if snap is None else snap,
                  bool(rng.integers(0, 2)))

    out = {}
    out["T1"] = [t(1, 1)]
    out["empty_first_last_run70"] = [t(0, 0), t(1, 1)] + [t(0, 0) for _ in range(70)] + [t(2, 0), t(0, 1), t(0, 0)]
    out["read_only_write_only"] = [t(2, 0), t(0, 1), t(1, 0), t(0, 2)]
    out["R0"] = [t(0, 1) for _ in range(5)]
    out["W0"] = [t(1, 0) for _ in range(5)]
    out["big_txn"] = [t(1, 1) for _ in range(3)] + [t(3000, 300, 15)] + [t(1, 1) for _ in range(3)]
    return out


SHAPES = shape_batches()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(trio, name):
    pb = PackedBatch.from_transactions(SHAPES[name])
    trio.step(PackedBatch.from_transactions([tx([], [(b"\x01", b"\xf0")], 0)]), 10, 0, what="prefill")
    trio.step(pb, 20, 0, what=name)
    trio.check_state(name)


@pytest.mark.parametrize("n_ranges", [127, 128, 129, 511, 512, 513])
def test_key_counts_around_the_scan_tile(trio, n_ranges):
    """2 (R + W) = 254, 256, 258, 1022, 1024, 1026 keys and, with one transaction more than keys in
    the odd cases, scans of 255, 257, 1023 and 1025 elements (offset entries past the keys)."""
    rng = np.random.default_rng(n_ranges)
    rs = [(lambda a: (a, a + b"\x00"))(rng_key(rng, 20)) for _ in range(n_ranges)]
    txns = [tx([rs[0]], [], 5, True)] + [tx([], [r], 5) for r in rs[1:]]
    for pad in (0, 2 * n_ranges - len(txns)):  # T + 1 = 2 (R + W) + 1: the scan's last element is an offset entry
        pb = PackedBatch.from_transactions(txns + [tx([], [], 5)] * pad)
        assert pad == 0 or pb.n_txn + 1 == 2 * n_ranges + 1
        trio.step(pb, 20 + pad, 0, what=(n_ranges, pad))
    trio.check_state(n_ranges)


@pytest.mark.parametrize("width", [16, 40])
def test_c2_shape(trio, width):
    """5000 x (5R + 2W): 70,000 keys, more than 64 scan tiles; with 40-byte keys every tail offset
    comes out of the look-back."""
    rng = np.random.default_rng(width)
    trio.step(random_batch(rng, 400, 2, 2, width, 10, alphabet=200), 10, 0, what="prefill")
    pb = random_batch(rng, 5000, 5, 2, width, 20, alphabet=200, stale=15)
    assert len(pb.key_offsets) - 1 == 70000 > 64 * TILE
    v = trio.step(pb, 20, 0, what=width)
    assert {0, 2} <= set(v.tolist())
    trio.check_state(width)


# ---- 4. TooOld


def test_too_old_straddles_the_oldest_version(trio):
    trio.step(PackedBatch.from_transactions([tx([], [(b"a", b"z")], 0)]), 100, 50)
    txns = [tx([(b"b", b"c")], [(b"q", b"r")], s, True) for s in (48, 49, 50, 51)] + \
           [tx([], [(b"s", b"t")], s) for s in (48, 49, 50)]
    v = trio.step(PackedBatch.from_transactions(txns), 110, 50)
    assert v.tolist() == [1, 1, 0, 0, 2, 2, 2]
    trio.check_state()


def test_too_old_is_judged_at_detect_in_the_resolvers_order(engine, oracle_built, torch_mod):
    """A batch added before the previous batch's detect raised the oldest version gets the verdicts
    of the Resolver's order (add after that detect), not those of an add-time test."""
    cs, o = engine.ConflictSet(0), oracle_built.OracleConflictSet()
    first = PackedBatch.from_transactions([tx([], [(b"a", b"b")], 0)])
    second = PackedBatch.from_transactions([tx([(b"m", b"n")], [(bytes([s]), bytes([s + 1]))], s, True)
                                            for s in (10, 39, 40, 41)])
    st1, st2 = Staged(torch_mod, first), Staged(torch_mod, second)
    b1, b2 = engine.ConflictBatch(cs), engine.ConflictBatch(cs, {})
    b1.add_packed_device(st1.dpb)
    b2.add_packed_device(st2.dpb)  # oldest is still 0 here: an add-time test would admit all four
    assert b2.device_add_info() == (4, 4, 4, 0)
    with pytest.raises(engine.FdbcsError) as e:
        b2.get_too_old_transactions([])
    assert e.value.status == engine.FDBCS_E_STATE
    b1.detect_conflicts(100, 40)
    v = b2.detect_conflicts(110, 40)
    o.detect(first, 100, 40)
    want, _ = o.detect(second, 110, 40)
    assert v.tolist() == want.tolist() and want.tolist()[:2] == [1, 1] and 2 in want
    early, _ = oracle_built.OracleConflictSet().detect(second, 110, 40, add_oldest=0)
    assert early.tolist() != want.tolist()
    for b in (b1, b2):
        b.close()
    cs.close()


# ---- 5. reports


def test_report_flags_with_and_without_report_keys(trio):
    rng = np.random.default_rng(5)
    trio.step(random_batch(rng, 300, 1, 2, 18, 10), 10, 0, what="prefill")
    pb = random_batch(rng, 300, 3, 1, 18, 20, stale=15, report_frac=0.6)
    (hv, hr, he), _ = trio.host(pb, 20, 0, report=True)
    (dv, dr, de), dm = trio.device(pb, 20, 0, report=True)
    assert (dv, dr, de) == (hv, hr, he) and any(dr) and any(de)
    assert dm == trio.o.detect(pb, 20, 0)[1]
    pb2 = random_batch(rng, 300, 3, 1, 18, 30, stale=15, report_frac=0.6)
    (hv, hr, he), _ = trio.host(pb2, 30, 0, report=False)
    (dv, dr, de), _ = trio.device(pb2, 30, 0, report=False)
    assert 0 in dv and (dv, dr, de) == (hv, hr, he) and not any(dr) and not any(de)
    (dv, dr, de), _ = trio.device(random_batch(rng, 50, 3, 1, 18, 40, stale=25, report_frac=1.0), 40, 0, report=True,
                                  with_report=False)  # a NULL report array: all false
    assert 0 in dv and not any(dr) and not any(de)


# ---- 6. pipeline and mixing


def test_four_in_flight_and_mixed_with_host_adds(engine, oracle_built, torch_mod):
    rng = np.random.default_rng(6)
    seq = [(random_batch(rng, 200, 2, 2, 24, 10 + 5 * i, stale=16), 10 + 5 * i, 4 + 5 * i) for i in range(8)]
    ref = engine.ConflictSet(0)
    want = []
    for pb, now, oldest in seq:
        b = engine.ConflictBatch(ref)
        b.add_packed(pb)
        want.append(b.detect_conflicts(now, oldest).tolist())
        b.close()
    assert any(1 in w for w in want) and any(0 in w for w in want)
    # four device-added batches in flight, twice; the first group behind a ready flag a torch
    # stream op sets after the copies, with no synchronize before the call
    cs = engine.ConflictSet(0)
    got = []
    for g in range(2):
        flag = torch_mod.zeros(2, dtype=torch_mod.int32, device="cuda")
        stg = [Staged(torch_mod, pb, shift=i, sync=(g == 1)) for i, (pb, _, _) in enumerate(seq[4 * g: 4 * g + 4])]
        flag.fill_(7 + g)
        bs = []
        for st, (pb, now, oldest) in zip(stg, seq[4 * g: 4 * g + 4]):
            b = engine.ConflictBatch(cs)
            b.add_packed_device(st.dpb, flag.data_ptr() if g == 0 else 0, 7 + g)
            bs.append(b)
        for b, (pb, now, oldest) in zip(bs, seq[4 * g: 4 * g + 4]):
            b.detect_async(now, oldest)
        for b in bs:
            got.append(b.wait().tolist())
            b.close()
    assert got == want
    # host-added and device-added batches alternating on one set
    mix = engine.ConflictSet(0)
    got = []
    for i, (pb, now, oldest) in enumerate(seq):
        b = engine.ConflictBatch(mix)
        st = None
        if i % 2:
            st = Staged(torch_mod, pb)
            b.add_packed_device(st.dpb)
        else:
            b.add_packed(pb)
        got.append(b.detect_conflicts(now, oldest).tolist())
        b.close()
    assert got == want
    dumps = [s.dump_history() for s in (ref, cs, mix)]
    for d in dumps[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d[:3], dumps[0][:3])) and d[3] == dumps[0][3]
    for s in (ref, cs, mix):
        s.close()


# ---- 7. set_conflict_output


def test_conflict_output_equals_the_host_added_twin(trio, torch_mod):
    rng = np.random.default_rng(7)
    trio.step(random_batch(rng, 200, 1, 2, 16, 10), 10, 0)
    pb = random_batch(rng, 300, 2, 1, 16, 20, stale=15)
    ids = rng.permutation(500)[: pb.n_txn].astype(np.int32)
    outs = []
    for cs, dev in ((trio.h, False), (trio.d, True)):
        out = torch_mod.full((500,), 9, dtype=torch_mod.uint8, device="cuda")
        torch_mod.cuda.synchronize()
        b = trio.E.ConflictBatch(cs)
        st = Staged(torch_mod, pb) if dev else None
        b.add_packed_device(st.dpb) if dev else b.add_packed(pb)
        b.set_conflict_output(ids, 500, out.data_ptr())
        v = b.detect_conflicts(20, 0)
        cs.sync()
        outs.append((out.cpu().numpy().copy(), v))
        b.close()
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    want = np.zeros(500, np.uint8)
    want[ids] = 2 - outs[0][1]
    np.testing.assert_array_equal(outs[1][0], want)
    assert 2 in want


# ---- 8. rejections


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
    """Range r (reads first, then writes) with its two keys exchanged."""
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
    k = keys_of(pb)
    tie = list(k)
    assert len(tie[2]) == 16 and tie[3] == tie[2] + b"\x00"
    tie[2], tie[3] = tie[3], tie[2]  # [k\0, k): equal prefixes, the length decides
    return {
        "read_offset_decreases": off(pb, "read_offsets", 2, 0),
        "last_read_offset_is_not_n_reads": (off(pb, "read_offsets", 4, 5), (4, 5)),
        "write_offsets_start_at_1": off(pb, "write_offsets", 0, 1),
        "key_offset_decreases": off(pb, "key_offsets", 5, int(ko[4]) - 1),
        "last_key_offset_8_past_the_bytes": off(pb, "key_offsets", len(ko) - 1, int(ko[-1]) + 8),
        "first_key_offset_minus_8": off(pb, "key_offsets", 0, -8),
        "inverted_in_the_prefix": swapped(pb, 0),
        "inverted_by_length_on_tied_prefixes": repack(pb, keys=tie),
        "inverted_in_the_last_byte_of_40": swapped(pb, 4 + 1),
        "inverted_inside_a_too_old_transaction": swapped(pb, 3),
    }


REJECT = rejections()


@pytest.mark.parametrize("name", list(REJECT))
def test_rejections(engine, oracle_built, torch_mod, name):
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
    st = Staged(torch_mod, bad, sizes=sizes)
    m = {}
    b = engine.ConflictBatch(cs, m)
    b.add_packed_device(st.dpb)
    with pytest.raises(engine.FdbcsError) as e:
        if name == "inverted_inside_a_too_old_transaction":
            b.detect_conflicts(120, 50)
        else:
            b.device_add_info()
    assert e.value.status == engine.FDBCS_E_INVALID
    assert st.intact(torch_mod)
    after = cs.dump_history()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[:3], after[:3])) and before[3] == after[3]
    # the same batch object takes a valid device add and resolves correctly
    st2 = Staged(torch_mod, good)
    b.add_packed_device(st2.dpb)
    assert b.device_add_info() == (good.n_txn, good.n_reads, good.n_writes, 8 + 24 + 24)
    v = b.detect_conflicts(120, 50)
    want, conf = o.detect(good, 120, 50)
    assert v.tolist() == want.tolist() == [0, 2, 1, 2] and m == conf == {0: [0]}
    kern, host = b.device_add_timing()
    assert kern > 0 and host > 0
    b.close()
    cs.close()


def test_host_side_refusals(engine, torch_mod):
    cs = engine.ConflictSet(0)
    good = valid_batch()
    st = Staged(torch_mod, good)

    def status(f, *a):
        with pytest.raises(engine.FdbcsError) as e:
            f(*a)
        return e.value.status

    b = engine.ConflictBatch(cs, {})
    b.add_packed(good)
    assert status(b.add_packed_device, st.dpb) == engine.FDBCS_E_STATE  # the batch holds something
    assert status(b.device_add_info) == engine.FDBCS_E_STATE
    b.close()
    b = engine.ConflictBatch(cs, {})
    d = st.dpb
    bad = lambda **kw: DevicePackedBatch(**{**d.__dict__, **kw})
    for kw in ({"n_txn": -1}, {"n_reads": -1}, {"n_writes": -1}, {"key_bytes_len": -1}, {"read_offsets": 0},
               {"write_offsets": 0}, {"read_snapshot": 0}, {"key_offsets": 0}, {"key_bytes": 0}, {"n_txn": 49153}):
        assert status(b.add_packed_device, bad(**kw)) == engine.FDBCS_E_INVALID, kw
    assert status(b.add_packed_device, bad(key_bytes_len=1 << 32)) == engine.FDBCS_E_NOMEM
    b.add_packed_device(bad(n_txn=0))  # nothing added: the batch stays empty
    assert status(b.device_add_info) == engine.FDBCS_E_STATE
    b.add_packed_device(d)
    assert status(b.add_packed_device, d) == engine.FDBCS_E_STATE
    assert status(b.add_packed, good) == engine.FDBCS_E_STATE
    assert status(b.add_transaction, good.to_transactions()[0]) == engine.FDBCS_E_STATE
    out = torch_mod.zeros(64, dtype=torch_mod.uint8, device="cuda")
    assert status(b.set_report_output, out.data_ptr(), 5) == engine.FDBCS_E_STATE
    assert status(b.set_iops_sample) == engine.FDBCS_E_STATE
    assert status(b.routed_info) == engine.FDBCS_E_STATE
    assert status(b.get_too_old_transactions, []) == engine.FDBCS_E_STATE
    b.upload()  # a no-op
    assert b.device_add_info() == (4, 4, 5, 56)
    v = b.detect_conflicts(10, 0)
    assert len(v) == 4 and status(b.add_packed_device, d) == engine.FDBCS_E_STATE  # detected
    assert b.device_verdicts_ptr() != 0
    b.close()
    cs.close()
