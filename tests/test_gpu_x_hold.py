"""The held X half, the edge word and the workspace ring.

A batch's X half (read check, pre-pass, rounds, D.Combine) is recorded at its detect call and issued
at a later one: at the next call if the host has by then seen the batch's edge word (the count of
candidate intra-batch edges its stage A found, tagged with the batch's sequence number), at the call
after that whatever the word says, and earlier whenever somebody waits for the batch or a later one.
An X half issued knowing that the batch has no candidate edge goes out without `k_resolve` and
`k_combine` (and `k_intra_report` when the batch reports conflicting keys): 2 or 3 launches counted in
`x_launches_skipped`.  An edge-free batch issued before its word arrived goes out whole and is
counted in `x_edge_free_unskipped`.  Which of the two happens to a batch depends on timing; what
must hold whatever the timing:

* every verdict equals the CPU restatement's, batch by batch;
* `x_launches_skipped` = (2 or 3) x (edge-free batches - `x_edge_free_unskipped`): an X half with
  candidate edges that went out short would break it from above (and its verdicts), a stale word of
  the workspace's previous user likewise;
* the too-early counter moves by 0 or 1 per batch, and never for a batch with edges.

Shapes: 64-256 transactions over a history of 4000 boundaries; the cases differ in how many batches
are in flight (each window takes another route through the issue order: window 1 issues at the
wait, window 2 holds one batch, window 3 and up hold up to two), in the order of the waits, and in
what is still held when a batch or the set is closed.  Where a case is about a state of the hold, it
makes the state: with every stream stalled behind the engine's hold kernel (Run.stalled) no edge word
can arrive, so two batches are held after the second detect call, and the counters `x_held` (a
gauge), `x_forced` and `x_flushed` show which route each batch then took.
"""
from contextlib import contextmanager

import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import PackedBatch

pytestmark = pytest.mark.gpu

START = 10_000  # the prefilled history's versions lie below it
STEP = 10


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle

    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def history():
    return W.c2_history(W.C2Params(history=4000, window=5000), seed=5, start_version=START)


def make_batch(rng, T, now, hot, known, report):
    """T transactions of 3 reads and 2 single-key writes.  hot None: random 16-byte keys (no read of
    the batch meets a write of the batch: no candidate edge), a sixth of the reads on `known` keys
    (the history's and earlier batches': history conflicts).  hot: every key from that small set, so
    reads meet earlier transactions' writes (candidate edges, batch-order resolution)."""
    nr, nw = 3, 2
    R, Wn = T * nr, T * nw
    if hot is None:
        rb = rng.integers(0, 256, size=(R, 16), dtype=np.uint8)
        wb = rng.integers(0, 256, size=(Wn, 16), dtype=np.uint8)
        again = rng.random(R) < 1 / 6
        rb[again] = known[rng.integers(0, len(known), size=int(again.sum()))]
    else:
        rb = hot[rng.integers(0, len(hot), size=R)]
        wb = hot[rng.integers(0, len(hot), size=Wn)]
    re = W._add_be128(rb, rng.integers(1, 17, size=R))
    mat = np.zeros((2 * (R + Wn), 17), np.uint8)
    mat[0:2 * R:2, :16] = rb
    mat[1:2 * R:2, :16] = re
    mat[2 * R::2, :16] = wb
    mat[2 * R + 1::2, :16] = wb  # [k, k\0)
    lens = np.full(2 * (R + Wn), 16, np.int64)
    lens[2 * R + 1::2] = 17
    snap = now - rng.integers(1, 4 * STEP, size=T)
    rep = np.full(T, 1 if report else 0, np.uint8)
    pb = PackedBatch.from_key_matrix(snap, np.arange(T + 1, dtype=np.int32) * nr,
                                     np.arange(T + 1, dtype=np.int32) * nw, mat, lens, rep)
    return pb, wb


def make_sequence(history, kinds, sizes, report, seed):
    """[(batch, now, oldest, has_edges)]: kinds[i] True = a batch with candidate edges."""
    rng = np.random.default_rng(seed)
    kb, _, _ = history
    known = kb.reshape(-1, 16)
    hot = np.unique(rng.integers(0, 256, size=(24, 16), dtype=np.uint8), axis=0)
    seq, now = [], START + 100
    for i, edges in enumerate(kinds):
        pb, wb = make_batch(rng, sizes[i % len(sizes)], now, hot if edges else None, known, report)
        known = np.concatenate([known, wb])
        seq.append((pb, now, now - 4000, bool(edges)))
        now += STEP
    return seq


def reference(oracle_mod, history, seq):
    sl = oracle_mod.SkipListBaseline()
    sl.load_history(*history)
    return [sl.detect(pb, now, oldest)[0] for pb, now, oldest, _ in seq]


class Run:
    """One conflict set fed `seq`; every wait checks the batch against the reference and takes the
    counters' moves."""

    def __init__(self, engine, history, seq, want, report, gc_interval=0):
        self.engine, self.seq, self.want, self.report = engine, seq, want, report
        self.cs = engine.ConflictSet(0)
        self.cs.set_gc_interval(gc_interval)
        self.cs.load_history(*history)
        # every buffer at its final size: nothing grows (and drains the streams) while they are stalled
        self.cs.reserve(200_000, 1 << 16, 1024, 4096, 4096)
        self.waited = []       # batch indices, in wait order
        self.edge_free = 0     # edge-free batches waited for
        self.too_early = 0
        self.batches = {}

    def prepare(self, *idx):
        """Batches added and uploaded, not yet detected."""
        for i in idx:
            b = self.engine.ConflictBatch(self.cs, {} if self.report else None)
            b.add_packed(self.seq[i][0])
            b.upload()
            self.batches[i] = b
        self.cs.sync()

    def detect(self, i):
        _, now, oldest, _ = self.seq[i]
        self.batches[i].detect_async(now, oldest)
        return self.cs.stats()

    def submit(self, i):
        pb, now, oldest, _ = self.seq[i]
        b = self.engine.ConflictBatch(self.cs, {} if self.report else None)
        b.add_packed(pb)
        b.detect_async(now, oldest)
        self.batches[i] = b

    @contextmanager
    def stalled(self):
        """Every stream of the set behind a hold kernel (the set is drained first): no stage A
        runs, so no edge word arrives, and whatever is detected meanwhile is held as long as the
        rules allow.  Released on the way out, whatever happened inside."""
        self.cs.debug_hold(True)
        try:
            yield
        finally:
            self.cs.debug_hold(False)

    def wait(self, i):
        b = self.batches.pop(i)
        before = self.cs.stats()
        v = b.wait()
        after = self.cs.stats()
        b.close()
        bad = np.nonzero(v != self.want[i])[0]
        assert len(bad) == 0, (i, bad[:10], v[bad[:10]], self.want[i][bad[:10]])
        d_edges = after["intra_edges"] - before["intra_edges"]
        d_early = after["x_edge_free_unskipped"] - before["x_edge_free_unskipped"]
        assert after["intra_fallbacks"] == 0
        has_edges = self.seq[i][3]
        assert (d_edges > 0) == has_edges, (i, d_edges, has_edges)
        assert d_early in (0, 1) and not (has_edges and d_early), (i, d_early, has_edges)
        self.edge_free += not has_edges
        self.too_early += d_early
        self.waited.append(i)

    def pipelined(self, window):
        inflight = []
        for i in range(len(self.seq)):
            self.submit(i)
            inflight.append(i)
            if len(inflight) >= window:
                self.wait(inflight.pop(0))
        for i in inflight:
            self.wait(i)

    def finish(self):
        """The counters' identity over everything waited for; the stats."""
        st = self.cs.stats()
        per_batch = 3 if self.report else 2
        assert st["x_edge_free_unskipped"] == self.too_early
        assert st["x_launches_skipped"] == per_batch * (self.edge_free - self.too_early), (
            st["x_launches_skipped"], per_batch, self.edge_free, self.too_early)
        self.cs.close()
        return st


@pytest.mark.parametrize("report", [False, True])
def test_skip_count_alternating(engine, oracle_mod, history, report):
    """Window 8, 20 batches, edge-free and with edges in turn (odd sizes, one below a wave)."""
    kinds = [i % 2 == 1 for i in range(20)]
    seq = make_sequence(history, kinds, [200, 64, 129, 256, 61], report, seed=11 + report)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), report)
    run.pipelined(8)
    assert run.edge_free == 10
    st = run.finish()
    assert st["batches"] == 20


def test_ring_reuse_both_ways(engine, oracle_mod, history):
    """27 batches (more than twice any ring depth up to 13) in the pattern free, free, edges: a
    workspace's users i and i + depth differ in kind both ways for every depth that is no multiple
    of 3, so a batch with edges finds the word an edge-free batch left and the other way round."""
    kinds = [i % 3 == 2 for i in range(27)]
    for depth in (4, 5, 7, 8, 10, 11, 13):
        pairs = {(kinds[i], kinds[i + depth]) for i in range(27 - depth)}
        assert (False, True) in pairs and (True, False) in pairs
    seq = make_sequence(history, kinds, [128, 96, 255], True, seed=21)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), True)
    run.pipelined(8)
    assert run.edge_free == 18
    run.finish()


@pytest.mark.parametrize("window", [1, 2, 3])
def test_issue_order_by_window(engine, oracle_mod, history, window):
    """Window 1: every X half goes out at its batch's wait.  Window 2: one batch held at each call,
    issued by the next call or by its wait.  Window 3: up to two held (how many depends on when the
    words arrive; test_two_held_forced pins that route)."""
    kinds = [i % 2 == 0 for i in range(12)]
    seq = make_sequence(history, kinds, [100, 64, 131], False, seed=30 + window)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), False)
    run.pipelined(window)
    assert run.waited == list(range(12))
    run.finish()


@pytest.mark.parametrize("window", [3, 4, 8])
def test_compaction_every_batch(engine, oracle_mod, history, window):
    """Every batch compacts, so every check reads the tiers its predecessor's Y leaves and waits for
    that Y's event: an X half issued before the Y half of the batch before it would wait on the
    event's earlier record and miss that batch's writes.  Every second batch reads the previous
    one's keys a sixth of the time (make_batch), so such a miss shows in the verdicts."""
    kinds = [i % 4 == 3 for i in range(16)]
    seq = make_sequence(history, kinds, [64, 150], False, seed=60 + window)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), False, gc_interval=1)
    run.pipelined(window)
    st = run.finish()
    assert st["compactions"] == 16




def test_two_held_forced(engine, oracle_mod, history):
    """The route of a window of three and more while no word arrives: two batches held after the
    second call, and from the third call on the older one issued because it was held two calls."""
    seq = make_sequence(history, [False, True, False, False], [96, 64], False, seed=35)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), False)
    run.prepare(0, 1, 2, 3)
    with run.stalled():
        assert run.detect(0)["x_held"] == 1
        st = run.detect(1)
        assert (st["x_held"], st["x_forced"], st["x_flushed"]) == (2, 0, 0)
        st = run.detect(2)
        assert (st["x_held"], st["x_forced"], st["x_flushed"]) == (2, 1, 0)
        st = run.detect(3)
        assert (st["x_held"], st["x_forced"], st["x_flushed"]) == (2, 2, 0)
    for i in range(4):
        run.wait(i)  # 0 and 1 are out; 2 and 3 each go out at their own wait
    st = run.finish()
    assert (st["x_forced"], st["x_flushed"]) == (2, 2)
    assert st["x_launches_skipped"] <= 2 * 2  # 0 went out under the stall, whole; 1 has edges


def test_wait_newest_first(engine, oracle_mod, history):
    """Groups of three detected under the stall, then waited for newest first: the first wait finds
    two batches held and issues both, in order; the other waits find theirs issued."""
    kinds = [i % 2 == 1 for i in range(9)]
    seq = make_sequence(history, kinds, [90, 128], True, seed=41)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), True)
    for g in range(0, 9, 3):
        run.prepare(g, g + 1, g + 2)
        with run.stalled():
            for i in range(g, g + 3):
                st = run.detect(i)
        assert st["x_held"] == 2
        flushed = st["x_flushed"]
        run.wait(g + 2)
        st = run.cs.stats()
        assert (st["x_held"], st["x_flushed"]) == (0, flushed + 2)
        run.wait(g + 1)
        run.wait(g)
        assert run.cs.stats()["x_flushed"] == flushed + 2
    run.finish()


def test_close_with_two_held(engine, oracle_mod, history):
    """Two batches held and closed unwaited, the newer first (its close issues both, in order), then
    batches that read what those wrote; at the end the set itself is closed with two batches held,
    and a new set still works."""
    kinds = [False, True, False, False, True, False, False, True]
    seq = make_sequence(history, kinds, [120, 64], False, seed=51)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), False)
    run.prepare(0, 1)
    with run.stalled():
        run.detect(0)
        assert run.detect(1)["x_held"] == 2
    run.batches.pop(1).close()
    st = run.cs.stats()
    assert (st["x_held"], st["x_flushed"]) == (0, 2)
    run.batches.pop(0).close()
    for i in (2, 3, 4, 5):
        run.submit(i)
    for i in (2, 3, 4, 5):
        run.wait(i)
    run.prepare(6, 7)
    with run.stalled():
        run.detect(6)
        assert run.detect(7)["x_held"] == 2
    run.cs.close()  # issues and drains both
    for b in run.batches.values():
        b.close()
    seq2 = make_sequence(history, [False, True], [64], False, seed=52)
    run2 = Run(engine, history, seq2, reference(oracle_mod, history, seq2), False)
    run2.pipelined(2)
    run2.finish()


@pytest.mark.parametrize("report", [False, True])
def test_skip_when_the_word_has_arrived(engine, oracle_mod, history, report):
    """An edge-free batch b detected behind a larger batch a, then a waited for: b stays held, and
    its stage A (issued before a's X half, a fraction of a's chain of stage A, X and Y long, and
    followed by this test's own work on the host) is over when the next detect call comes.  That call
    issues b without the launches only candidate edges need, and b is never counted as too early."""
    seq = make_sequence(history, [True, False, False], [256, 64, 64], report, seed=71 + report)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), report)
    run.prepare(0, 1, 2)
    run.detect(0)
    run.detect(1)
    run.wait(0)
    st0 = run.cs.stats()
    assert st0["x_held"] == 1
    st1 = run.detect(2)
    assert st1["x_launches_skipped"] - st0["x_launches_skipped"] == (3 if report else 2)
    assert (st1["x_held"], st1["x_flushed"] - st0["x_flushed"]) == (1, 0)
    early = run.too_early
    run.wait(1)
    assert run.too_early == early
    run.wait(2)
    run.finish()


def test_two_at_one_call(engine, oracle_mod, history):
    """Batches 1 and 2 held while batch 0 (larger, issued first) runs to its end; by the next call
    both words have arrived, so both go out at that call: 1 because it was held two calls, 2 because
    its word is there.  The older one's X and Y are then issued from the calling thread before the
    newer one's X (which may wait on that Y's event), and both skip."""
    seq = make_sequence(history, [True, False, False, False], [256, 64, 64, 64], False, seed=81)
    run = Run(engine, history, seq, reference(oracle_mod, history, seq), False)
    run.prepare(0, 1, 2, 3)
    with run.stalled():
        run.detect(0)
        run.detect(1)
        st = run.detect(2)
    assert (st["x_held"], st["x_forced"]) == (2, 1)
    run.wait(0)
    st0 = run.cs.stats()
    assert st0["x_held"] == 2
    st1 = run.detect(3)
    assert (st1["x_held"], st1["x_forced"] - st0["x_forced"], st1["x_flushed"] - st0["x_flushed"]) == (1, 1, 1)
    assert st1["x_launches_skipped"] - st0["x_launches_skipped"] == 4
    for i in (1, 2, 3):
        run.wait(i)
    run.finish()
