"""The Y half of a batch against the two models: the directed plans of tests/merge_plan.py (built and
proved on the CPU; tests/test_tier_model_cpu.py) run on the engine.

After every batch: verdicts exact, none dropped from the comparison, and history_size(),
stats()["compactions"], gc_runs, delta_sum, base_sum and segments_sum equal to tests/tier_model.TierSim's.
The sizes are what shows a superfluous or a missing end boundary: the canonical dump merges it away.
After every second read batch, every compaction and every GC: the dump at the oldest-version floor and
at NO_FLOOR (what is stored below the floor is TierSim's too: its GC runs when decide_y's does).

Between a write batch and the first read batch after it nothing synchronizes the set: no dump and no
history_size() (both end in sync_all, which clears prev_segs, and the next check would read the merged
delta instead of the previous batch's segments), and every buffer is sized before the first batch for
the same reason.  After a write batch the counters alone are compared (stats() reads host state); the
size is compared after every read batch, the one that follows a write batch included, which changes
nothing unless it compacts itself."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests import merge_plan as MP
from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu

CASES = [(f, lay) for f in MP.ALL_FAMILIES + ("import",) for lay in MP.LAYOUTS] + [
    ("tails", "long"), ("clear-reuse", "narrow"), ("clear-reuse", "long")]
MAIN = [("segment-tiles", "narrow"), ("glue-exact", "long"), ("delta-tiles", "narrow"), ("gc", "long")]
KNOBS = [{"FDBCS_SERIAL": "1"}, {"FDBCS_SUBMIT_THREAD": "0"}, {"FDBCS_SPLIT_CHECK": "0"}, {"FDBCS_SPLIT_CHECK": "2"},
         {"FDBCS_DIRECTORY": "0"}]


def check_verdicts(got, st, what):
    assert len(got) == len(st.want)  # none dropped from the comparison
    if st.kind == "read":
        assert not (got == K.TOO_OLD).any(), what
        assert (got == K.CONFLICT).mean() >= 0.3 and (got == K.COMMITTED).mean() >= 0.3, what
    bad = np.flatnonzero(got != st.want)
    assert bad.size == 0, (what, bad.size, "of", len(got), bad[:10], got[bad[:10]], st.want[bad[:10]])


def run_plan(engine, plan, inflight=1):
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(0)
    if plan.delta_limit:
        cs.set_delta_limit(plan.delta_limit)
    if plan.loaded is not None:
        cs.load_history(*plan.loaded)
    else:
        cs.clear(plan.header0)
    cs.set_oldest_version(plan.first_oldest)
    cs.reserve(20000, 1 << 20, 49152, 49152, 49152)
    # the read batch with the most tail bytes goes first, as reads that change nothing (their verdicts
    # are not looked at): no batch buffer grows later
    warm = max((s.pb for s in plan.steps if s.kind == "read"), key=lambda pb: pb.tail_bytes)
    b = engine.ConflictBatch(cs)
    b.add_packed(warm)
    b.detect_conflicts(plan.steps[0].now - 1, plan.first_oldest)
    b.close()
    cs.reset_stats()
    cleared = dict(plan.cleared)
    pending = []
    serial = inflight == 1

    def drain(keep):
        while len(pending) > keep:
            b, st = pending.pop(0)
            got = b.wait()
            b.close()
            what = (plan.name, plan.layout, st.name)
            check_verdicts(got, st, what)
            if not serial:
                continue
            if plan.sizes:
                stats = cs.stats()
                got_sizes = {k: stats[k] for k in MP.STAT_KEYS}
                if st.kind == "read":  # (never between a write batch and the read batch its segments decide)
                    got_sizes["history_size"] = cs.history_size()
                assert got_sizes == {k: st.expect[k] for k in got_sizes}, (what, got_sizes, st.expect)
            if st.dump is not None:
                K.assert_dump_equals(cs.dump_history(floor=None), st.dump[0], (what, "floor"))
                if plan.sizes:
                    K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), st.dump[1], (what, "no floor"))

    for i, st in enumerate(plan.steps):
        if st.gc_interval is not None or i in cleared or st.kind == "import":
            drain(0)
        if i in cleared:
            cs.clear(cleared[i])
        if st.gc_interval is not None:
            cs.set_gc_interval(st.gc_interval)
        if st.kind == "import":  # (no batch: the counters stay; the size and the delta's are the model's)
            n = cs.merge_history(*st.arrays, into="delta")
            info = cs.import_info()
            assert info["path"] == 1 and info["delta_before"] == 0, (plan.name, st.name, info)
            assert n == st.expect["history_size"] == info["base_boundaries"] + info["delta_after"], (st.name, n, info)
            continue
        b = engine.ConflictBatch(cs)
        b.add_packed(st.pb)
        b.detect_async(st.now, st.new_oldest)
        pending.append((b, st))
        drain(inflight - 1)
    drain(0)
    stats = cs.stats()
    last = plan.steps[-1]
    if last.dump is not None:  # the state after the last wait (every plan ends after a forced compaction)
        K.assert_dump_equals(cs.dump_history(floor=None), last.dump[0], (plan.name, "end"))
        if plan.sizes:
            K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), last.dump[1], (plan.name, "end, no floor"))
            assert cs.history_size() == last.expect["history_size"], (plan.name, "end")
    cs.close()
    return stats, last.expect


def run_case(engine, monkeypatch, family, layout, inflight=1):
    if layout == "wide":
        # the rider's 49152 endpoints fall above the last splitter the read batch before them left, so one
        # workgroup would rank them all: every batch ranks its own samples instead (the cold-start path)
        monkeypatch.setenv("FDBCS_SORT_COLD", "1")
    out = []
    for plan in MP.build(family, layout):
        for k, v in plan.env.items():
            monkeypatch.setenv(k, v)
        out.append(run_plan(engine, plan, inflight))
    return out


@pytest.mark.parametrize("family,layout", CASES, ids=lambda x: x)
def test_merge_plan(engine, monkeypatch, family, layout):
    """One family of the directed plan under one layout of k_seg_prep, serially: verdicts, sizes and
    counters after every batch, the dumps at both floors."""
    run_case(engine, monkeypatch, family, layout)


def test_single_far_range_rider(engine, monkeypatch):
    """The wide layout's rider as one far range sent 24576 times (49152 tied endpoints)."""
    run_case(engine, monkeypatch, "single-rider", "wide")


def test_gc_under_tail_reclaim(engine, monkeypatch):
    """The GC family on long keys under FDBCS_TAIL_RECLAIM=4096: the tail-triggered GC and the arena flip
    run on a small history.  The trigger is not TierSim's, so verdicts and the dumps at the floor alone."""
    (stats, model), = run_case(engine, monkeypatch, "gc-tail-reclaim", "long")
    # the knob is in force: more compactions and GC runs than decide_y's other triggers give the model
    assert stats["compactions"] > model["compactions"] and stats["gc_runs"] > model["gc_runs"], (stats, model)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_merge_plan_knobs(engine, monkeypatch, knobs):
    """The main plans serially on one stream, without the submit thread, on both other splits of the read
    check and without the directory (knobs are read when the set is created)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for family, layout in MAIN:
        run_case(engine, monkeypatch, family, layout)


def test_merge_plan_four_in_flight(engine, monkeypatch):
    """Four batches in flight (detect_async / wait): verdicts and, after the last wait, the dumps at both
    floors and history_size() (every main plan ends after a forced compaction, which folds whatever an
    in-flight upper bound of the delta's size may have shifted)."""
    for family, layout in MAIN:
        run_case(engine, monkeypatch, family, layout, inflight=4)
