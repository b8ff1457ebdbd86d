"""The read check against the dense key-space model (tests/keyspace_model.py): a numpy array over a
key universe, independent of both oracle restatements.  No oracle library is consulted here.

What the other GPU tests leave open: range_max's upper levels.  Level 2 is read only by a read over
more than 128*64 boundaries of one tier, level 3 (the replicas k_epilogue builds by atomicMax) only
past 128*4096 = 524288, and a wide read that meets a version above its snapshot in its first entries
returns before either matters.  Here every read is sent twice, with its span's true maximum as
snapshot (must commit: a stale-high level entry, `>=` for `>` or one entry read too many conflicts)
and with one less (must conflict: a stale-low entry or one entry read too few commits), over spans
that start and end around every block edge of every level, around isolated high versions
("spikes", their heights not monotone in position) at those edges, and around the highest versions
of all, which stand deep inside upper-level blocks.  Every version is offset by D, so the same runs also carry versions far
past 32 bits through the level build and the check.  The stored state is compared with the model's
run-length encoding after the batches."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu

OFFSETS = [0, 10 ** 14 + 7]
# small: a universe of about 40k keys (gaps of 1 to 3 after each of 20k boundaries); 2000 narrow writes
# per write batch, since with fewer the three batches leave under 8192 delta entries on so small a
# history (tests/test_keyspace_model.py counts them), and one wide write, since two would leave too
# little of it.  big: about 1.2M keys (gaps of 1 to 2), 1500 writes per write batch.
SMALL = dict(H=20_000, n_spikes=200, n_random=1500, n_writes=2000, n_wide=1, max_gap=3)
BIG = dict(H=800_000, n_spikes=200, n_random=3000, n_writes=1500, n_wide=4, checks=(0, 5, 6))


@pytest.fixture(scope="module")
def plans():
    """plan(shape, D, size): the CPU-built sequence, built once and shared, unchanged, by the tests
    that run it (a failure while building one is this fixture's, not a test's)."""
    built = {}

    def plan(shape, D, size):
        key = (shape, D, size)
        if key not in built:
            for k in [k for k in built if k[2] == "big"]:
                del built[k]  # a big plan holds hundreds of MB of batches and expected state: one at a time
            built[key] = K.build_plan(1, shape, D, **(BIG if size == "big" else SMALL))
        return built[key]

    return plan


def new_set(engine, loaded, D, H):
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(1 << 22)  # reads see base + delta + the previous batch's segments
    cs.load_history(*loaded)
    cs.set_oldest_version(D + 500)
    assert cs.history_size() == H
    return cs


def check_verdicts(got, want, what):
    assert len(got) == len(want)  # none dropped from the comparison
    assert not (got == K.TOO_OLD).any(), what
    assert (got == K.CONFLICT).mean() >= 0.3 and (got == K.COMMITTED).mean() >= 0.3, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, "of", len(want), bad[:10], got[bad[:10]], want[bad[:10]])


def check_state(cs, state, what):
    want, as_stored = state
    # once the oldest version has moved, what is stored below the floor depends on when the engine
    # collected garbage: from then on the plan compares at the default floor only
    for f in (None, NO_FLOOR) if as_stored else (None,):
        K.assert_dump_equals(cs.dump_history(floor=f), want, (what, f))


def run_plan(engine, plans, shape, D, size, inflight=1):
    loaded, steps = plans(shape, D, size)
    cs = new_set(engine, loaded, D, len(loaded[2]))
    pending = []

    def drain(keep):
        while len(pending) > keep:
            b, want, what = pending.pop(0)
            check_verdicts(b.wait(), want, what)
            b.close()

    for i, st in enumerate(steps):
        if st["gc_interval"] is not None:
            cs.set_gc_interval(st["gc_interval"])
        for j, (pb, now, new_oldest, want) in enumerate(st["batches"]):
            b = engine.ConflictBatch(cs)
            b.add_packed(pb)
            b.detect_async(now, new_oldest)
            pending.append((b, want, (shape, i, j)))
            drain(inflight - 1)
        if st["state"] is not None and (inflight == 1 or i == len(steps) - 1):
            drain(0)
            check_state(cs, st["state"], (shape, i))
            if st["gc_interval"] == 1:
                # the next step's reads were laid out by the model's ranks, the deep versions 2048 ranks
                # from their block's edges: the compacted base may hold a few boundaries more (between
                # adjacent writes of one batch), far fewer than that margin
                assert 0 <= cs.history_size() - st["boundaries"] <= 1024
    drain(0)
    cs.close()


@pytest.mark.parametrize("D", OFFSETS)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_big_history_reaches_level_3(engine, plans, shape, D):
    """800k loaded boundaries (more than 2*64*4096): reads over more than 524288 of them read
    level 3 and its replicas, after the load, over base + delta, and after the compaction that moves
    every position.  After the load and after the compaction the highest versions stand deep inside
    the second level-3 block and in the middle of level-2 blocks, and hundreds of reads around them
    have their maximum in level-3 (level-2) entries alone (the plan counts them by replaying
    range_max's climb), so an entry left stale-low commits a read that must conflict.  State
    compared after the load, the compaction and the GC."""
    run_plan(engine, plans, shape, D, "big")


@pytest.mark.parametrize("D", OFFSETS)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_small_history_every_batch(engine, plans, shape, D):
    """20k boundaries: levels 1 and 2 of base and delta (after the load and after the compaction
    the highest version stands in the middle of a level-2 block, and dozens of reads find it in a
    level-2 entry alone), state compared after every batch."""
    run_plan(engine, plans, shape, D, "small")


@pytest.mark.parametrize("D", OFFSETS)
@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("knobs", [{"FDBCS_SPLIT_CHECK": "0"}, {"FDBCS_SPLIT_CHECK": "1"}, {"FDBCS_SPLIT_CHECK": "2"},
                                   {"FDBCS_DIRECTORY": "0"}, {"FDBCS_SERIAL": "1"}, {"FDBCS_SUBMIT_THREAD": "0"}],
                         ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_small_history_knobs(engine, plans, monkeypatch, knobs, shape, D):
    """The same sequence on every read-check and submission path (knobs are read when the set is
    created)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    run_plan(engine, plans, shape, D, "small")


@pytest.mark.parametrize("D", OFFSETS)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_small_history_four_in_flight(engine, plans, shape, D):
    """Four batches in flight (detect_async / wait), the model walked in submission order: the
    levels are rebuilt per batch into alternating delta buffers while later checks are queued."""
    run_plan(engine, plans, shape, D, "small", inflight=4)


@pytest.mark.parametrize("D", OFFSETS)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_interleaved_reads_and_writes(engine, shape, D):
    """Reads and writes in one batch in random order (at most 300 transactions), the model walked
    in batch order; three batches, so later ones read the earlier ones' delta."""
    rng = np.random.default_rng(17)
    U, H = 40_000, 20_000
    model = K.KeyspaceModel(K.make_universe(rng, U, shape), D + 1234)
    hist = np.sort(rng.choice(np.arange(K.FIRST_BOUNDARY, U), size=H, replace=False))
    vers = D + 1000 + np.cumsum(rng.integers(1, 1000, size=H)) % 1000
    model.load(hist, vers)
    cs = new_set(engine, (*model.pack_keys(hist), vers, model.header), D, H)
    for i in range(3):
        now = D + 5000 + i
        pb, want = K.interleaved_step(170 + i, model, now, D + 500)
        assert pb.n_txn <= 300
        b = engine.ConflictBatch(cs)
        b.add_packed(pb)
        got = b.detect_conflicts(now, D + 500)
        b.close()
        check_verdicts(got, want, (shape, i))
        K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), model.rle(), (shape, i))
    cs.close()
