"""D.Sort against the key-space model: the directed plans of tests/sort_plan.py (built and proved on the
CPU from the model alone; no oracle library is consulted).

What the other GPU tests leave open: FDBCS_VALIDATE=1 holds the device order to item_less_total, the
sort's own comparison, and looks at erec[p].x alone; the random batches of sort_bucket_batches() give no
run of tied keys an exact length or position and no bucket an exact size; the other model plans send
keys of 16 or 20 bytes.  So the register widths S = 1 | 2 | 4, the common-prefix strip through every
branch of key_word, the pair shortcut, the in-slot and the slow tie ranking, their fall-back past 112
bytes, the range-end flag, the workgroup path with its overflow gather and tiles, split_cmp_rest's
window ties, the cold sampling's exact ranks and put_quantiles below kQuant endpoints never decided a
verdict a model predicted.  Here every batch is a chain of readers and writers over sorted keys in
which an endpoint one place off changes a verdict, a report or the state
(tests/test_keyspace_model.py asserts it, move by move).

Per batch: verdicts and conflicting-read maps exactly the model's, the exported state exactly the
model's run-length encoding (both floors) when one batch is in flight, intra_edges equal to the model's
slot count with no fallback (the only sight of erec's class counts and of wbrange / rbrange), and the
sort_big_buckets delta equal to the plan's count of buckets past 256 endpoints (the plan's restated
partition against the device).

On an MI355X (the plan's CPU build included): the one-bucket plan 0.8 s with keys past 19 bytes and 0.4 s
without, the cold plans 1.1 s (64 a bucket) and 0.1 s (8), the warm splitters 0.5 s, each knob and four
in flight under 0.1 s, the two-bucket plans none among the suite's thirty slowest tests (1.5 s and up).
Six one-line wrong variants of the sort each fail at the first step that reaches them."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests import sort_plan as SP
from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu

KINDS = ["single-long", "single-short", "cold-64", "cold-8"]
KNOBS = [{"FDBCS_SERIAL": "1"}, {"FDBCS_WRITE_GROUPS": "0"}]


@pytest.fixture(scope="module")
def plans():
    """plan(kind): the CPU-built plan, built once and shared, unchanged, by the tests that run it
    (building it asserts its coverage; a failure there is this fixture's, not a test's)."""
    built = {}

    def plan(kind):
        if kind not in built:
            built[kind] = SP.build(kind)
        return built[kind]

    return plan


def check_batch(got, m, s):
    assert len(got) == len(s.want) == s.T  # none dropped from the comparison
    bad = np.flatnonzero(got != s.want)
    assert bad.size == 0, (s.name, bad.size, "of", s.T, bad[:10], got[bad[:10]], s.want[bad[:10]])
    assert {t: sorted(x) for t, x in m.items()} == s.reports, s.name


def run_plan(engine, plan, monkeypatch, knobs=None, inflight=1):
    for k, v in {**plan.env, **(knobs or {})}.items():  # read when the set is created
        monkeypatch.setenv(k, v)
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(1 << 22)
    cs.load_history(*plan.loaded)
    cs.set_oldest_version(SP.OLDEST)
    cs.reserve(1 << 16, 1 << 20, 8192, 8192, 8192)  # no workspace grows mid-plan; the slab holds 257 buckets
    pending, shares = [], {}
    seen = {"intra_edges": 0, "intra_fallbacks": 0, "sort_big_buckets": 0}

    def drain(keep):
        while len(pending) > keep:
            b, m, s = pending.pop(0)
            got = b.wait()
            check_batch(got, m, s)
            b.close()
            shares.setdefault(s.step, []).append(got)
            st = cs.stats()
            d = {k: st[k] - seen[k] for k in seen}
            seen.update({k: st[k] for k in seen})
            assert d == {"intra_edges": s.slots, "intra_fallbacks": 0, "sort_big_buckets": s.big}, (s.name, d, s.slots, s.big)

    for s in plan.batches:
        m = {}
        b = engine.ConflictBatch(cs, m)
        b.add_packed(s.pb)
        b.detect_async(s.now, SP.OLDEST)
        pending.append((b, m, s))
        drain(inflight - 1)
        if inflight == 1:
            for f in (None, NO_FLOOR):
                K.assert_dump_equals(cs.dump_history(floor=f), s.state, (s.name, f))
    drain(0)
    K.assert_dump_equals(cs.dump_history(floor=NO_FLOOR), plan.batches[-1].state, "end")
    cs.close()
    for step, got in shares.items():  # a degenerate step cannot pass: over its two parities
        got = np.concatenate(got)
        assert (got == K.CONFLICT).mean() >= 0.3 and (got == K.COMMITTED).mean() >= 0.3, step


@pytest.mark.parametrize("kind", KINDS)
def test_sort_plan(engine, plans, monkeypatch, kind):
    """One bucket (positions are the model's total order) with keys past 19 bytes and without, and
    several buckets of 64 and of 8 endpoints from the batch's own samples: sizes 2 .. 1026, runs of
    2 .. 40 tied keys at every placement, the pair shortcut, keys past 112 bytes, c = 1 .. 64."""
    run_plan(engine, plans(kind), monkeypatch)


@pytest.mark.parametrize("target", sorted(SP.HALVES))
def test_sort_plan_two_buckets(engine, plans, monkeypatch, target):
    """A batch has an even number of endpoints, so the odd sizes stand in two buckets of E / 2 (cold,
    nb = 2, both end buckets): 1, 63 | 65, 127 | 129, 255 | 257, 511 | 513 and about 1025 endpoints."""
    run_plan(engine, plans(f"halves-{target}"), monkeypatch)


def test_sort_plan_warm_splitters(engine, plans, monkeypatch):
    """The quantile table across batches: a cold batch of 9000 endpoints from 1024 samples, a directed
    batch under the table it left, a batch of under 4096 endpoints (several entries per position) and
    one that lands between two of its quantiles, a batch under 2048 endpoints that must leave the table
    alone, and populations wholly below the first and above the last splitter (one bucket of 3000)."""
    run_plan(engine, plans("warm"), monkeypatch)


@pytest.mark.parametrize("kind", ["single-long", "cold-8"])
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a[6:]}={b}" for a, b in k.items()))
def test_sort_plan_knobs(engine, plans, monkeypatch, kind, knobs):
    """The one-bucket and the several-bucket plan serially and without write groups."""
    run_plan(engine, plans(kind), monkeypatch, knobs)


@pytest.mark.parametrize("kind", ["single-long", "cold-64"])
def test_sort_plan_four_in_flight(engine, plans, monkeypatch, kind):
    """Four batches in flight (detect_async / wait), the model walked in submission order."""
    run_plan(engine, plans(kind), monkeypatch, inflight=4)
