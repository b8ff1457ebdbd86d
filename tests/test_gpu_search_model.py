"""The endpoint search against the key-space model on keys of different lengths: the directed plan of
tests/search_plan.py (built and proved on the CPU from the model alone; no oracle library is consulted).

What the other GPU tests leave open: a read over thousands of boundaries conflicts whether
lower_bound is right or off by a hundred, and the model plans of the range-max levels and of the
batch order send keys of one length, 16 or 20 bytes, so lane_lower_bound_long, lane_prefix_run,
probe_cmp_long, load_qtail, k_seg_prep<true, true>, k_compact_search<2> and every comparison decided by
a key's length never ran under a model.  Here every read spans one to three segments whose
neighbours carry other versions, and goes out at its span's maximum (commits) and one below
(conflicts); over the plan's two polarities every directed key has a read that flips a verdict
under each of the four one-segment errors of its begin's or end's position
(tests/test_keyspace_model.py asserts it).

Which structure a check reads (engine.cpp, plan_layout / decide_y): unless the set runs serially, a
batch's check reads the delta as it stood before the previous batch's merge plus that batch's union
segments (PrevSegs, prev_seg_hit_quad).  So of the two identical read batches after a write batch the
first finds the new versions in the segments alone and the second in the delta alone; after the forced
compaction (gc_interval 1, decided in decide_y for the batch that follows) they stand in the base.
Anything that synchronizes the set (a dump, a workspace or tail buffer that grows) clears prev_segs, and
the next check reads the merged delta instead: run_plan sizes everything first and compares the state
after read batches only.

Counts of the core plan (polarity 0; polarity 1 differs in the last column's split only): 536 directed
keys, 41420 loaded boundaries, 535 narrow writes over four batches leaving 640 delta boundaries,
about 27000 reads per read batch and 354000 over the plan's 13 read batches; per family (reads
accounted / decided by the base / the delta / the previous batch alone): ladders 11361 / 7459 / 3072 /
830, tail edges 13125 / 7947 / 4080 / 1098, runs 15795 / 11225 / 3562 / 1008, run interiors 26725 /
16629 / 8132 / 1964, tier edges 998 / 656 / 281 / 61.  On an MI355X: the core plan 1.9 s per polarity,
the riders 0.4, 0.4 and under 1.5 s, the previous-batch segments 2.7 s, each knob and four in flight
1.0 s."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests import search_plan as SP
from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu

KNOBS = [{"FDBCS_DIRECTORY": "0"}, {"FDBCS_DIR_BITS": "4"}, {"FDBCS_SPLIT_CHECK": "0"}, {"FDBCS_SPLIT_CHECK": "1"},
         {"FDBCS_SPLIT_CHECK": "2"}, {"FDBCS_SERIAL": "1"}]


@pytest.fixture(scope="module")
def plans():
    """plan(kind, polarity): the CPU-built plan, built once and shared, unchanged, by the tests that
    run it (building it asserts its coverage; a failure there is this fixture's, not a test's)."""
    built = {}

    def plan(kind, polarity):
        if (kind, polarity) not in built:
            built[kind, polarity] = SP.build_path_d(polarity) if kind == "path-d" else SP.build(polarity, kind)
        return built[kind, polarity]

    return plan


def check_verdicts(got, want, what):
    assert len(got) == len(want)  # none dropped from the comparison
    assert not (got == K.TOO_OLD).any(), what
    assert (got == K.CONFLICT).mean() >= 0.3 and (got == K.COMMITTED).mean() >= 0.3, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, "of", len(want), bad[:10], got[bad[:10]], want[bad[:10]])


def run_plan(engine, plan, inflight=1, wide=False):
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(0)
    if wide:
        cs.set_delta_limit(1 << 22)
    cs.load_history(*plan.loaded)
    cs.set_oldest_version(SP.OLDEST)
    assert cs.history_size() == plan.H
    # A workspace or a batch-tail buffer that has to grow synchronizes the set, and so does a dump: the
    # next check then reads the merged delta, not the previous batch's segments.  So everything is
    # sized before the first batch (the plan's batch with the most tail bytes goes first, as reads
    # that change nothing, its verdicts not looked at), and the state is compared after read batches
    # only, never between a write batch and the read batch its segments are to decide.
    batches = [pb for s in plan.steps for pb, _, _, _ in s.batches]
    cs.reserve(2 * plan.H, 0, 49152, 49152, 49152)
    warm = max((pb for pb in batches if pb.n_writes == 0), key=lambda pb: pb.tail_bytes)
    assert warm.tail_bytes >= max(pb.tail_bytes for pb in batches)
    b = engine.ConflictBatch(cs)
    b.add_packed(warm)
    b.detect_conflicts(SP.FIRST_NOW, SP.OLDEST)
    b.close()
    pending = []

    def drain(keep):
        while len(pending) > keep:
            b, want, what = pending.pop(0)
            got = b.wait()
            b.close()
            if what[1] == "read":
                check_verdicts(got, want, what)
            else:
                assert (got == want).all(), what

    for s in plan.steps:
        if s.gc_interval is not None:
            drain(0)
            cs.set_gc_interval(s.gc_interval)
        if s.delta_before is not None and inflight == 1 and not wide:
            cs.reset_stats()
        for j, (pb, now, new_oldest, want) in enumerate(s.batches):
            b = engine.ConflictBatch(cs)
            b.add_packed(pb)
            b.detect_async(now, new_oldest)
            pending.append((b, want, (s.name, s.kind, j)))
            drain(inflight - 1)
        if inflight == 1:
            if s.delta_before is not None and not wide:
                # delta_sum adds each batch's delta size at the start of its merge (account_stats):
                # the plan's predicted delta before this write batch, and nothing compacted it
                st = cs.stats()
                assert st["compactions"] == 0 and st["delta_sum"] == s.delta_before, (s.name, st["delta_sum"], s.delta_before)
            if s.state is not None and s.kind == "read":
                for f in (None, NO_FLOOR) if s.as_stored else (None,):
                    K.assert_dump_equals(cs.dump_history(floor=f), s.state, (s.name, f))
    drain(0)
    last = [s for s in plan.steps if s.state is not None][-1]
    K.assert_dump_equals(cs.dump_history(floor=None), last.state, "end")
    cs.close()


@pytest.mark.parametrize("polarity", [0, 1])
def test_search_plan(engine, plans, polarity):
    """The core plan: the loaded base alone, four batches of narrow writes with the same read batch
    twice after each (decided by the previous batch's segments, then by the delta), a forced
    compaction, a GC that moves every rank; every batch has a key over 24 bytes, so everything goes by
    lane_lower_bound_long.  State after every write batch, the compaction and the GC, and the delta's
    predicted size before every write batch against stats()["delta_sum"]."""
    run_plan(engine, plans(None, polarity))


@pytest.mark.parametrize("rider", ["short", "long", "wide"])
def test_search_riders(engine, plans, monkeypatch, rider):
    """The queries and writes of at most 24 bytes alone: as they are (check by lane_lower_bound, merge
    by group_lower_bound), with one far read-only transaction on a 40-byte key in every batch
    (everything by lane_lower_bound_long) and with 24576 far one-key writes in every write batch (merge
    by lane_lower_bound: k_seg_prep<false, true>)."""
    if rider == "wide":
        # The far writes' 49152 endpoints fall between two of the splitters the read batch before them
        # left (D.Sort takes the previous batch's quantiles), so one workgroup would sort them all:
        # seconds per write batch.  Every batch ranks its own samples instead (the cold-start path).
        monkeypatch.setenv("FDBCS_SORT_COLD", "1")
    plan = plans(rider, 1 if rider == "long" else 0)
    longest = max(int(np.diff(pb.key_offsets).max()) for s in plan.steps for pb, _, _, _ in s.batches)
    assert (longest > 24) == (rider == "long")
    assert all((pb.n_writes >= 24576) == (rider == "wide") for s in plan.steps if s.kind == "write" for pb, _, _, _ in s.batches)
    run_plan(engine, plan, wide=rider == "wide")


@pytest.mark.parametrize("polarity", [0, 1])
def test_previous_batch_segments(engine, plans, polarity):
    """prev_seg_hit_quad: write batches of 1, 2, 16, 17, 18, 288, 289, 290 and over 4000 union segments,
    each followed by reads that end at a segment's begin, begin at its end or are degenerate at
    either, snapshots between the older history and the batch's version."""
    run_plan(engine, plans("path-d", polarity))


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_search_plan_knobs(engine, plans, monkeypatch, knobs):
    """The core plan without the directory, with a 16-slot directory (every slot wide), on every
    read-check split and serially (knobs are read when the set is created)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    run_plan(engine, plans(None, int(knobs.get("FDBCS_SPLIT_CHECK", "0")) % 2))


def test_search_plan_four_in_flight(engine, plans):
    """Four batches in flight (detect_async / wait), the model walked in submission order."""
    run_plan(engine, plans(None, 1), inflight=4)
