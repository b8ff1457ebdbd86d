"""Conflicting-key reports of device-routed batches (fdbcs_batch_add_routed on a batch created with
report_keys): the routed sub-transactions carry the shares' report flags, the host reads each
resolver's conflictingKeyRangeMap, and fdbcs_batch_set_report_output leaves the reports as device
bytes whose element-wise max over the resolvers is the set of the proxy's conflictingKRIndices
(CommitProxyServer.actor.cpp:1243-1261).  G resolvers on one GPU, each routing the same gathered
shares, against an oracle per resolver fed the host routing."""
import collections

import numpy as np
import pytest

from tests.routed_report_helpers import (KNOWN_SPLITS, KNOWN_TSHARE, RANDOM_CASES, Floors, bytes_as_sets,
                                         known_answer, make_splits, proxy_sets, sorted_map)

pytestmark = pytest.mark.gpu


def _gather(engine, torch, pb, G, Tshare):
    shares = [engine.share_pack(pb.slice_txns(g * Tshare, (g + 1) * Tshare)) for g in range(G)]
    stride = (max(len(x) for x in shares) + 255) // 256 * 256
    host = np.zeros(G * stride, np.uint8)
    for g, x in enumerate(shares):
        host[g * stride: g * stride + len(x)] = x
    return torch.from_numpy(host).cuda(), stride


class Routed:
    """One global batch routed on G resolvers: per resolver the batch object, its map, the device
    conflict bytes and report bytes (prefilled with 7, so an unwritten byte shows)."""

    def __init__(self, engine, torch, sets, splits, pb, Tshare, with_map=True, report_out=True, n_reads=None):
        G = len(sets)
        self.pb = pb
        self.dev, stride = _gather(engine, torch, pb, G, Tshare)
        torch.cuda.synchronize()
        tail = int(np.maximum(np.diff(pb.key_offsets) - 16, 0).sum())
        self.caps = (pb.n_txn, pb.n_reads, pb.n_writes, tail)
        self.objs, self.maps, self.outs, self.reps = [], [], [], []
        for g in range(G):
            lo = splits[g - 1] if g > 0 else None
            hi = splits[g] if g < G - 1 else None
            m = {} if with_map else None
            out = torch.full((pb.n_txn,), 7, dtype=torch.uint8, device="cuda")
            rep = torch.full((max(pb.n_reads, 1),), 7, dtype=torch.uint8, device="cuda")
            b = engine.ConflictBatch(sets[g], m)
            self.args = (self.dev.data_ptr(), stride, G, Tshare)
            b.add_routed(*self.args, lo, hi, self.caps, out.data_ptr(), pb.n_txn)
            if report_out:
                b.set_report_output(rep.data_ptr(), pb.n_reads if n_reads is None else n_reads)
            self.objs.append(b)
            self.maps.append(m)
            self.outs.append(out)
            self.reps.append(rep)

    def detect(self, now, oldest):
        for b in self.objs:
            b.detect_async(now, oldest)

    def wait(self):
        got = [b.wait() for b in self.objs]
        for b in self.objs:
            b.close()
        return got


def _check_against_oracle(sh, oras, rt, got, now, oldest, floors=None):
    """Every equality of the issue for one global batch: per resolver the verdicts, the filled map
    and the device bytes; over the resolvers the max of the bytes against the proxy's lists."""
    from foundationdb_amd import sharding

    pb = rt.pb
    routes = sh.route(pb)
    vs, ms = [], []
    mx = np.zeros(pb.n_reads, np.uint8)
    for g in range(sh.G):
        want_v, want_m = oras[g].detect(routes[g].batch, now, oldest)
        np.testing.assert_array_equal(got[g], want_v, err_msg=f"resolver {g}")
        assert sorted_map(rt.maps[g]) == sorted_map(want_m), f"resolver {g}"
        dev = rt.reps[g].cpu().numpy()[: pb.n_reads]
        np.testing.assert_array_equal(dev, sharding.report_bytes(pb, routes[g], want_m), err_msg=f"resolver {g}")
        mx = np.maximum(mx, dev)
        vs.append(want_v)
        ms.append(want_m)
    lists, sets_ = proxy_sets(pb, routes, ms, sharding.combine(pb.n_txn, routes, vs))
    assert bytes_as_sets(pb, mx) == sets_
    if floors is not None:
        floors.add(lists)
    return lists


def test_known_answer(engine, oracle_built):
    """The issue's two batches on two resolvers split at b"m": the per-resolver "first" of an
    intra-batch conflict (batch 1), a read reported by both owners and a reporting TooOld
    transaction that gets neither an entry nor a byte (batch 2)."""
    import torch

    from foundationdb_amd import sharding
    from foundationdb_amd.sharding import KeyRangeSharding

    sh = KeyRangeSharding(KNOWN_SPLITS)
    sets = [engine.ConflictSet(0) for _ in range(2)]
    oras = [oracle_built.OracleConflictSet() for _ in range(2)]
    for pb, now, oldest, verdicts, maps, byts, proxy in known_answer():
        rt = Routed(engine, torch, sets, KNOWN_SPLITS, pb, KNOWN_TSHARE)
        rt.detect(now, oldest)
        got = rt.wait()
        routes = sh.route(pb)
        comb = np.zeros(pb.n_txn, np.uint8)
        for g in range(2):
            assert sorted_map(rt.maps[g]) == maps[g], (g, rt.maps[g])
            assert rt.reps[g].cpu().numpy().tolist() == byts[g], g
            comb = np.maximum(comb, rt.outs[g].cpu().numpy())
        assert (2 - comb).tolist() == verdicts
        mx = np.maximum(rt.reps[0].cpu().numpy(), rt.reps[1].cpu().numpy())
        assert mx.tolist() == np.maximum(np.array(byts[0]), np.array(byts[1])).tolist()
        # the proxy's list from the maps the engine filled, remapped with the host routing's read ids
        assert sharding.combine_conflicting_keys(pb, routes, rt.maps, 2 - comb) == proxy
        _check_against_oracle(sh, oras, rt, got, now, oldest)
    for cs in sets:
        cs.close()


@pytest.mark.parametrize("case,submit_thread", [(c, None) for c in RANDOM_CASES] + [(RANDOM_CASES[0], "1"),
                                                                                   (RANDOM_CASES[0], "0")],
                         ids=lambda x: x if isinstance(x, str) else ("G%d-a%d-l%d" % x[0][:3] if x else "default"))
def test_random_against_host_routing(engine, oracle_built, monkeypatch, case, submit_thread):
    """The parameter sets, seeds, splits and batches of test_device_routing_matches_host_routing,
    every batch created with a map.  One set also with the helper submitting thread forced on and
    off (FDBCS_SUBMIT_THREAD), the two submission paths the report launch goes through."""
    import torch

    from foundationdb_amd import workloads as W
    from foundationdb_amd.sharding import KeyRangeSharding

    if submit_thread is not None:
        monkeypatch.setenv("FDBCS_SUBMIT_THREAD", submit_thread)
    (G, alphabet, max_len, long_split), want = case
    rng = np.random.default_rng(100 + G + alphabet)
    Tshare = 120
    splits = make_splits(rng, G, alphabet, long_split)
    sh = KeyRangeSharding(splits)
    sets = [engine.ConflictSet(0) for _ in range(G)]
    oras = [oracle_built.OracleConflictSet() for _ in range(G)]
    fl = Floors()
    now = 10
    for _ in range(10):
        pb = W.random_small_batch(rng, G * Tshare, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
        rt = Routed(engine, torch, sets, splits, pb, Tshare)
        got = []
        for g in range(G):  # one resolver after another, as the test this one mirrors
            rt.objs[g].detect_async(now, now - 9)
            got.append(rt.objs[g].wait())
            rt.objs[g].close()
        _check_against_oracle(sh, oras, rt, got, now, now - 9, fl)
        now += 4
    fl.check(G, want)
    for cs in sets:
        cs.close()


def test_pipelined(engine, oracle_built):
    """Two resolvers, 6 batches, up to 3 in flight: batch i+1 is routed before batch i's detect,
    every detect is asynchronous and the waits come in order.  The rotating workspaces must not
    leak one batch's rconf into the next batch's bytes."""
    import torch

    from foundationdb_amd import workloads as W
    from foundationdb_amd.sharding import KeyRangeSharding

    (G, alphabet, max_len, long_split), _ = RANDOM_CASES[0]
    rng = np.random.default_rng(4242)
    Tshare = 120
    splits = make_splits(rng, G, alphabet, long_split)
    sh = KeyRangeSharding(splits)
    sets = [engine.ConflictSet(0) for _ in range(G)]
    oras = [oracle_built.OracleConflictSet() for _ in range(G)]
    fl = Floors()
    inflight = collections.deque()
    routed = None

    def retire():
        rt, now_, old_ = inflight.popleft()
        _check_against_oracle(sh, oras, rt, rt.wait(), now_, old_, fl)

    now = 10
    for _ in range(6):
        pb = W.random_small_batch(rng, G * Tshare, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
        nxt = (Routed(engine, torch, sets, splits, pb, Tshare), now, now - 9)
        if routed is not None:  # the previous batch's detect after this batch's routing
            if len(inflight) == 3:
                retire()
            routed[0].detect(routed[1], routed[2])
            inflight.append(routed)
        routed = nxt
        now += 4
    if len(inflight) == 3:
        retire()
    routed[0].detect(routed[1], routed[2])
    inflight.append(routed)
    while inflight:
        retire()
    assert fl.reported > 0 and fl.multi > 0 and fl.dup > 0
    for cs in sets:
        cs.close()


def test_launch_accounting(engine):
    """Per-kernel profile (timing level 3): a routed batch created without a map launches neither
    the report kernel nor its zero fill; one created with a map and a report output launches each
    exactly once per batch."""
    import torch

    from foundationdb_amd import workloads as W

    rng = np.random.default_rng(5)
    cs = engine.ConflictSet(0)
    cs.set_timing(3)
    now = 10
    for k, with_map in enumerate([False, False, True, True, True]):
        pb = W.random_small_batch(rng, 120, alphabet=6, max_len=3, now=now, staleness=12)
        assert pb.n_reads > 0
        rt = Routed(engine, torch, [cs], [], pb, 120, with_map=with_map, report_out=with_map)
        rt.detect(now, now - 9)
        rt.wait()
        prof = cs.kernel_profile()
        assert "k_resolve_pre" in prof  # the profile is live
        n = max(0, k - 1)
        for name in ("k_report_bytes", "k_zero_bytes"):
            assert prof.get(name, {"launches": 0})["launches"] == n, (k, name, prof.get(name))
        now += 4
    cs.close()


def test_errors(engine, oracle_built):
    import torch

    from foundationdb_amd import workloads as W
    from foundationdb_amd.sharding import KeyRangeSharding

    rng = np.random.default_rng(77)
    pb = W.random_small_batch(rng, 100, alphabet=6, max_len=3, now=10, staleness=12)
    cs = engine.ConflictSet(0)
    buf = torch.full((pb.n_reads,), 7, dtype=torch.uint8, device="cuda")
    # an unrouted batch, with or without a map
    b = engine.ConflictBatch(cs, {})
    with pytest.raises(engine.FdbcsError) as e:
        b.set_report_output(buf.data_ptr(), pb.n_reads)
    assert e.value.status == engine.FDBCS_E_STATE
    b.close()
    # a routed batch created without a map
    rt = Routed(engine, torch, [cs], [], pb, 100, with_map=False, report_out=False)
    with pytest.raises(engine.FdbcsError) as e:
        rt.objs[0].set_report_output(buf.data_ptr(), pb.n_reads)
    assert e.value.status == engine.FDBCS_E_STATE
    # GetTooOldTransactions on a routed batch stays FDBCS_E_STATE
    with pytest.raises(engine.FdbcsError) as e:
        rt.objs[0].get_too_old_transactions([])
    assert e.value.status == engine.FDBCS_E_STATE
    rt.objs[0].close()
    # a wrong n_global_reads is found at detect; the batch is empty and can be routed again
    rt = Routed(engine, torch, [cs], [], pb, 100, n_reads=pb.n_reads - 1)
    b = rt.objs[0]
    with pytest.raises(engine.FdbcsError) as e:
        b.detect_async(10, 1)
    assert e.value.status == engine.FDBCS_E_INVALID
    assert rt.reps[0].cpu().numpy().tolist() == [7] * pb.n_reads  # nothing was written
    b.add_routed(*rt.args, None, None, rt.caps, rt.outs[0].data_ptr(), pb.n_txn)
    b.set_report_output(rt.reps[0].data_ptr(), pb.n_reads)
    with pytest.raises(engine.FdbcsError) as e:  # a null output
        b.set_report_output(0, pb.n_reads)
    assert e.value.status == engine.FDBCS_E_INVALID
    b.detect_async(10, 1)
    with pytest.raises(engine.FdbcsError) as e:  # already detected
        b.set_report_output(rt.reps[0].data_ptr(), pb.n_reads)
    assert e.value.status == engine.FDBCS_E_STATE
    got = [b.wait()]
    b.close()
    _check_against_oracle(KeyRangeSharding([]), [oracle_built.OracleConflictSet()], rt, got, 10, 1)
    cs.close()
