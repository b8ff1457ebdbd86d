"""The intra-batch half of detectConflicts against the batch-order model (tests/keyspace_model.py:
resolve, a dirty map over a key universe walked in batch order, independent of both oracle
restatements) on the directed batches of tests/resolution_plan.py.  No oracle library is consulted.

What the other GPU tests leave open: the constants EdgePairScan, k_edge_fill, k_resolve_pre,
k_resolve<5|8> and k_combine branch on.  The plan aims a batch at every one of them and proves on the
CPU, from the model's facts alone, that the batch reaches it: walks past exactly 0..9 writers aborted
in the rounds (every hand-over from the four writers held in registers to the packed list), write
groups of 1, 2, 12, 13 and 3000 members of every kind with the least committed member just before,
at and just after a reader, W = 1024 / 1025 / 12288 / 12289, transactions of 63 .. 129 reads with
255 .. 513 candidate edges in one 64-read chunk and live writers at flattened positions 63 | 64 and
255 | 256, reads over 1023 .. 4100 write-begins, P = k * 1024 - 1 .. + 1 pairs, a second trip of the
fill loop, and T / U on either side of 5120, 8192 and 16384.

Per batch: verdicts and conflicting-read maps exactly the model's, the exported state exactly the
model's run-length encoding (CoverScan / SegNumScan on both combine paths), and the three counters:
no fallback, rounds > 0 exactly when the model has an undecided transaction, and intra_edges equal to
the slot count derived from EdgePairScan::counts (K.batch_facts)."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests import resolution_plan as RP
from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu

KNOBS = [{"FDBCS_RESOLVE_PREPASS": "0"}, {"FDBCS_WRITE_GROUPS": "0"}, {"FDBCS_SKIP_EDGES": "0"}, {"FDBCS_SERIAL": "1"},
         {"FDBCS_SUBMIT_THREAD": "0"}]
EDGE_CAP = 1000  # below the slot count of every core batch with candidate edges


@pytest.fixture(scope="module")
def plans():
    """plan(kind, shape): the CPU-built plan, built once and shared, unchanged, by the tests that run
    it (building it asserts its coverage; a failure there is this fixture's, not a test's)."""
    built = {}

    def plan(kind, shape):
        if (kind, shape) not in built:
            built[kind, shape] = RP.build(kind, 1, shape)
        return built[kind, shape]

    return plan


def check_batch(got, m, s):
    want = s.want
    assert len(got) == len(want) == s.T  # none dropped from the comparison
    # a degenerate batch cannot pass: the shares the plan was built to (tests/resolution_plan.py)
    assert (got == K.COMMITTED).mean() >= s.shares[0] and (got == K.CONFLICT).mean() >= s.shares[1], s.name
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (s.name, bad.size, "of", len(want), bad[:10], got[bad[:10]], want[bad[:10]])
    assert {t: sorted(x) for t, x in m.items()} == s.reports, s.name


def run_plan(engine, plan, inflight=1, edge_cap=None):
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(1 << 22)
    cs.load_history(*plan.loaded)
    cs.set_oldest_version(RP.OLDEST)
    pending = []
    seen = {"intra_edges": 0, "intra_rounds": 0, "intra_fallbacks": 0}

    def drain(keep):
        while len(pending) > keep:
            b, m, s = pending.pop(0)
            check_batch(b.wait(), m, s)
            b.close()
            st = cs.stats()
            d = {k: st[k] - seen[k] for k in seen}
            seen.update({k: st[k] for k in seen})
            fallback = edge_cap is not None and s.slots > edge_cap
            assert d["intra_fallbacks"] == int(fallback), (s.name, d)
            if not fallback:
                assert d["intra_edges"] == s.slots, (s.name, d, s.slots)
                assert (d["intra_rounds"] > 0) == (s.U > 0), (s.name, d, s.U)

    for s in plan.steps:
        m = {}
        b = engine.ConflictBatch(cs, m)
        b.add_packed(s.pb)
        b.detect_async(s.now, s.oldest)
        pending.append((b, m, s))
        drain(inflight - 1)
        if inflight == 1:
            for f in (None, NO_FLOOR):
                K.assert_dump_equals(cs.dump_history(floor=f), s.state, (s.name, f))
    drain(0)
    K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), plan.steps[-1].state, "end")
    if edge_cap is not None:
        assert seen["intra_fallbacks"] == sum(s.slots > edge_cap for s in plan.steps) > 0
    cs.close()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_ladders_groups_prepass(engine, plans, shape):
    """The walk ladders (j = 0 .. 9 aborted writers before none / a writer committed in the rounds /
    one committed by the pre-pass; with dead writers between; with the writers in groups; T below
    and above 5120), the hot keys (groups of 1 .. 3000 members of all four kinds, W = 1024, 1025,
    12288 and, groups off, 12289) and the pre-pass transactions (63 .. 129 reads, 255 .. 513 edges
    in a chunk, 0 .. 6 live writers at the step edges), state and counters after every batch."""
    run_plan(engine, plans("core", shape))


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_ladders_groups_prepass_knobs(engine, plans, monkeypatch, knobs):
    """The same batches without the pre-pass (the rounds walk eoff / ecur themselves), without write
    groups (one edge per pair), with the no-edge launches always issued, and on the serial and
    caller-thread submission paths (knobs are read when the set is created)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    run_plan(engine, plans("core", "random16"))


def test_ladders_groups_prepass_edge_overflow(engine, plans, monkeypatch):
    """FDBCS_EDGE_CAP below the slot count: every batch with more candidate slots falls back to the
    sequential MiniConflictSet replay (intra_fallbacks counts them), the others resolve in rounds."""
    monkeypatch.setenv("FDBCS_EDGE_CAP", str(EDGE_CAP))
    plan = plans("core", "random16")
    assert all(s.slots == 0 or s.slots > EDGE_CAP for s in plan.steps)
    run_plan(engine, plan, edge_cap=EDGE_CAP)


def test_ladders_groups_prepass_four_in_flight(engine, plans):
    """Four batches in flight (detect_async / wait), the model walked in submission order."""
    run_plan(engine, plans("core", "prefix20"), inflight=4)


def test_edge_fill(engine, plans):
    """k_edge_fill's steps: reads over 1023 / 1024 / 1025 / 2049 / 4100 write-begins with later
    writers, the reader's own write and empty writes breaking the runs at lane 0, lane 63 and
    mid-wave; a step of 1024 one-pair ranges; P = 2047 .. 2049 and 4094 .. 4098; 72900 pairs from 540
    ranges (a second trip of the grid-stride loop)."""
    run_plan(engine, plans("fill", "prefix20"))


def test_sizes(engine, plans):
    """One read and one write per transaction: T = 5120 (U = 5000) and 5121 (k_resolve<5> | <8>),
    T = 8400 with U = 8192 and 8401 with U = 8193 (registers | global memory), T = 16384 and 16385
    (the status words' tail loop), T = 16600 (more than 128 scan tiles of ranges and of write
    endpoints) with U = 8100, with U = 16000 and without any candidate edge (the pre-pass's combine)."""
    run_plan(engine, plans("sizes", "random16"))
