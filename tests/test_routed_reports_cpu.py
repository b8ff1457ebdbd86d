"""Conflicting-key reports of device-routed batches, the parts that need no GPU: the host
restatement of the device report bytes (sharding.report_bytes / combine_report_bytes) against the
proxy's conflictingKRIndices (sharding.combine_conflicting_keys, CommitProxyServer.actor.cpp:
1243-1261) with an oracle per resolver, and the new C-ABI entry points."""
import ctypes

import numpy as np
import pytest

from foundationdb_amd import sharding
from foundationdb_amd import workloads as W
from foundationdb_amd.sharding import KeyRangeSharding

from tests.routed_report_helpers import (KNOWN_SPLITS, RANDOM_CASES, Floors, bytes_as_sets, known_answer,
                                         make_splits, proxy_sets, sorted_map)


def test_known_answer_against_oracle(oracle_built):
    """The issue's two batches: local maps per resolver, bytes per resolver, their max and the
    proxy's list, all from the oracle fed the host routing."""
    O = oracle_built
    sh = KeyRangeSharding(KNOWN_SPLITS)
    oras = [O.OracleConflictSet() for _ in range(2)]
    for pb, now, oldest, verdicts, maps, byts, proxy in known_answer():
        assert pb.n_reads == 5
        routes = sh.route(pb)
        got_v, got_m = [], []
        for g in range(2):
            v, m = oras[g].detect(routes[g].batch, now, oldest)
            got_v.append(v)
            got_m.append(m)
            assert sorted_map(m) == maps[g], (g, m)
            np.testing.assert_array_equal(sharding.report_bytes(pb, routes[g], m), byts[g])
        combined = sharding.combine(pb.n_txn, routes, got_v)
        assert combined.tolist() == verdicts
        want_max = np.maximum(np.array(byts[0], np.uint8), np.array(byts[1], np.uint8))
        c = sharding.combine_report_bytes(pb, routes, got_m)
        np.testing.assert_array_equal(c, want_max)
        lists, sets = proxy_sets(pb, routes, got_m, combined)
        assert lists == proxy
        assert bytes_as_sets(pb, c) == sets


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "G%d-a%d-l%d" % c[0][:3])
def test_report_bytes_are_the_sorted_set_of_the_proxy_list(oracle_built, case):
    """Random batches over 1-4 resolvers (the parameter sets, seeds and batches of
    test_device_routing_matches_host_routing): the max of the resolvers' report bytes is, per
    transaction, the sorted set of the proxy's list; a transaction the proxy does not report has
    no ones."""
    O = oracle_built
    (G, alphabet, max_len, long_split), floors = case
    rng = np.random.default_rng(100 + G + alphabet)
    sh = KeyRangeSharding(make_splits(rng, G, alphabet, long_split))
    oras = [O.OracleConflictSet() for _ in range(G)]
    fl = Floors()
    now = 10
    for _ in range(10):
        pb = W.random_small_batch(rng, G * 120, alphabet=alphabet, max_len=max_len, now=now, staleness=12)
        routes = sh.route(pb)
        vs, ms = [], []
        for g in range(G):
            v, m = oras[g].detect(routes[g].batch, now, now - 9)
            vs.append(v)
            ms.append(m)
            b = sharding.report_bytes(pb, routes[g], m)
            assert b.dtype == np.uint8 and b.shape == (pb.n_reads,) and set(np.unique(b)) <= {0, 1}
        c = sharding.combine_report_bytes(pb, routes, ms)
        lists, sets = proxy_sets(pb, routes, ms, sharding.combine(pb.n_txn, routes, vs))
        assert bytes_as_sets(pb, c) == sets
        fl.add(lists)
        now += 4
    # the floors' table is the oracle's count on these inputs: here it must be met exactly
    assert (fl.reported, fl.multi, fl.dup) == floors
    fl.check(G, floors)


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_new_symbols_exist(lib):
    from foundationdb_amd import conflict_set as C

    for name in ("fdbcs_batch_set_report_output", "fdbcs_batch_report_entries"):
        assert name in C.SIGNATURES and getattr(lib, name)
    assert callable(C.ConflictBatch.set_report_output) and callable(C.ConflictBatch.report_entries)
    assert callable(sharding.report_bytes) and callable(sharding.combine_report_bytes)


def test_null_handle_is_invalid(lib):
    from foundationdb_amd import conflict_set as C

    buf = (ctypes.c_uint8 * 8)()
    assert lib.fdbcs_batch_set_report_output(None, ctypes.cast(buf, ctypes.c_void_p), 8) == C.FDBCS_E_INVALID
    assert lib.fdbcs_batch_report_entries(None, ctypes.cast(buf, ctypes.c_void_p), 8) == C.FDBCS_E_INVALID
