"""Ownership of the engine's device buffers, pinned buffers, events and streams: whatever a set and
its batches allocate is back with the runtime once they are closed, in either order, and the slot
pool still pools.  Counted by fdbcs_debug_live_resources; each test starts from the counts it finds
(sets and batches other tests left to the garbage collector are collected first)."""
import gc

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.sharding import KeyResolvers
from tests.device_add_helpers import Staged
from tests.import_helpers import pack
from tests.route_map_helpers import gather

pytestmark = pytest.mark.gpu

LONG = 40  # bytes of the routed batch's bounds: past the 16 a key prefix holds, so their tails are uploaded


def baseline(engine):
    gc.collect()
    return engine.live_resources()


def small_batch(rng, now, report_frac=0.5):
    return W.random_small_batch(rng, 16, alphabet=4, max_len=6, now=now, staleness=10, report_frac=report_frac)


def detect_host(engine, cs, pb, now, reports=False):
    b = engine.ConflictBatch(cs, {} if reports else None)
    b.add_packed(pb)
    v = b.detect_conflicts(now, now - 10)
    b.close()
    return v


def history(n, version):
    """n boundaries, every third key longer than 16 bytes; adjacent versions differ."""
    ks = [b"k%04d" % i + (b"-long-key-tail-bytes" if i % 3 == 0 else b"") for i in range(n)]
    return 0, ks, [version + i % 5 for i in range(n)]


def routed(engine, torch, cs, pb, keep, lo=None, hi=None, kr=None, reports=False, sample=False):
    """A batch of `cs` routed from the one share of pb, under [lo, hi) or as resolver 0 of kr."""
    dev, stride = gather(engine, torch, pb, 1, pb.n_txn)
    out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
    rep = torch.full((max(pb.n_reads, 1),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    keep += [dev, out, rep]
    caps = (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
    b = engine.ConflictBatch(cs, {} if reports else None)
    if kr is None:
        b.add_routed(dev.data_ptr(), stride, 1, pb.n_txn, lo, hi, caps, out.data_ptr(), pb.n_txn)
    else:
        b.add_routed_map(dev.data_ptr(), stride, 1, pb.n_txn, kr, 0, caps, out.data_ptr(), pb.n_txn)
    if sample:
        b.set_iops_sample(1, 5)
    if reports:
        b.set_report_output(rep.data_ptr(), pb.n_reads)
    return b


def test_everything_a_set_and_its_batches_allocate_comes_back(engine):
    import torch

    base = baseline(engine)
    rng = np.random.default_rng(7)
    keep = []  # torch memory the engine reads or writes
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(1)
    cs.load_history(*pack(history(300, 10)))
    # past 65536 base boundaries, 16384 delta boundaries and 64 KiB of tails
    cs.reserve(400000, 300000, 64, 256, 20000)
    now = 100
    cs.set_timing(3)
    for _ in range(2):
        detect_host(engine, cs, small_batch(rng, now, 1.0), now, reports=True)
        now += 5
    cs.set_timing(0)
    assert all(x > y for x, y in zip(engine.live_resources(), base)), (engine.live_resources(), base)

    pb = small_batch(rng, now)
    out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = engine.ConflictBatch(cs)
    b.add_packed(pb)
    b.set_conflict_output(np.arange(pb.n_txn, dtype=np.int32), pb.n_txn, out.data_ptr())
    b.detect_conflicts(now, now - 10)
    b.close()
    now += 5

    pb = small_batch(rng, now, 1.0)
    b = routed(engine, torch, cs, pb, keep, lo=b"\x01" * LONG, hi=b"\x03" * LONG, reports=True, sample=True)
    b.detect_async(now, now - 10)
    b.wait()
    b.iops_sample_raw()
    b.close()
    now += 5

    pb = small_batch(rng, now)
    b = routed(engine, torch, cs, pb, keep, kr=KeyResolvers(2, [b"\x02"]))
    b.detect_async(now, now - 10)
    b.wait()
    b.close()
    now += 5

    pb = small_batch(rng, now)
    st = Staged(torch, pb)
    b = engine.ConflictBatch(cs)
    b.add_packed_device(st.dpb)
    b.detect_conflicts(now, now - 10)
    b.close()
    now += 5

    pb = small_batch(rng, now)
    st = Staged(torch, pb)
    cap = engine.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, st.dpb.key_bytes_len)
    share = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert share.data_ptr() % 64 == 0
    b = engine.ConflictBatch(cs)
    b.share_pack_device(st.dpb, share.data_ptr(), cap)
    assert b.share_pack_info()[1] == pb.n_txn
    b.close()

    n, nbytes, _ = cs.export_history()
    assert n > 0
    cs.read_export(n, nbytes)
    cs.digest()
    b = engine.ConflictBatch(cs)
    b.add_packed(small_batch(rng, now))
    b.upload()
    b.read_versions()
    b.close()

    src = engine.ConflictSet(0)
    src.load_history(*pack(history(40, now)))
    cs.merge_history(*src.dump_history(), into="base")
    cs.merge_history(*pack(history(40, now + 10)), into="delta")
    assert cs.import_info()["path"] == 1
    src.export_history()
    cs.merge_pending_export(src)
    src.close()

    cs.close()
    assert engine.live_resources() == base


def test_a_batch_that_outlives_its_set(engine):
    import torch

    base = baseline(engine)
    rng = np.random.default_rng(8)
    keep = []
    cs = engine.ConflictSet(0)
    b = routed(engine, torch, cs, small_batch(rng, 100), keep, sample=True)
    cs.close()
    for call in (lambda: b.iops_sample_raw(), lambda: b.detect_async(100, 90), lambda: b.upload()):
        with pytest.raises(engine.FdbcsError) as e:
            call()
        assert e.value.status == engine.FDBCS_E_STATE
    held = engine.live_resources()
    assert held[0] > base[0] and held[1] > base[1] and held[2] > base[2], (held, base)
    assert held[3] == base[3]
    b.close()
    assert engine.live_resources() == base


def test_the_slot_pool_still_pools(engine):
    base = baseline(engine)
    rng = np.random.default_rng(9)
    cs = engine.ConflictSet(0)
    now, seen = 100, []
    for _ in range(20):
        detect_host(engine, cs, small_batch(rng, now), now)
        seen.append(engine.live_resources())
        now += 5
    assert seen[2] == seen[19], seen
    cs.close()
    assert engine.live_resources() == base


def test_ten_sets_in_a_row(engine):
    base = baseline(engine)
    rng = np.random.default_rng(10)
    for i in range(10):
        cs = engine.ConflictSet(0)
        detect_host(engine, cs, small_batch(rng, 100), 100)
        cs.close()
        assert engine.live_resources() == base, i
