"""The look-back windows and the record layouts behind the edge scan and the segment preparation.

A three-component look-back probes 64 predecessor tiles at a time (scan.h, tile_lookback); the
edge scan reads one 16-byte record per endpoint that the bucket sort wrote (SortOut::erec) and
the segment preparation and the batch's inserts take their keys from D.Combine's segk.  The shapes
here are the smallest at which that can go wrong, not the workload's: tile counts around the
multiples of the 64-tile probe and of four of them (a tile at index 64, 65, 128, 129, 256, 257
looks back over exactly one probe, one more, ..., four, one more), with keys that leave the batch
without a candidate edge (the pre-pass combine path) and with a hot key set (edges, write groups,
k_edge_fill), empty ranges included: an empty range's end sorts before its begin, so by position
it looks inverted, and its emptiness is read from the records.

Everything is exact against the CPU restatement of the reference: verdicts, conflicting-key lists,
and, for the segment cases, the stored history (boundary count and every boundary, through the
canonical export).  conftest.py runs the engine under FDBCS_VALIDATE=1, which re-checks the
device sort order and so the records' positions.
"""
import numpy as np
import pytest

from foundationdb_amd import workloads as W
from foundationdb_amd.packing import PackedBatch
from tests.export_helpers import canon, split_dump
from tests.helpers import prefixed

pytestmark = pytest.mark.gpu

EDGE_TILE = 256  # ranges per tile of the edge scan (one per thread)


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle

    oracle.build()
    return oracle


def be_add(keys, lo, hi, rng):
    return W._add_be128(keys, rng.integers(lo, hi, size=len(keys)))


def pack(rb, re, rlen, wb, we, wlen, roff, woff, snap, report):
    """PackedBatch of 16-byte begins and 16/17-byte ends (a 17th byte is \\0)."""
    R, Wn = len(rb), len(wb)
    mat = np.zeros((2 * (R + Wn), 17), np.uint8)
    mat[0:2 * R:2, :16] = rb
    mat[1:2 * R:2, :16] = re
    mat[2 * R::2, :16] = wb
    mat[2 * R + 1::2, :16] = we
    lens = np.full(2 * (R + Wn), 16, np.int64)
    lens[1:2 * R:2] = rlen
    lens[2 * R + 1::2] = wlen
    return PackedBatch.from_key_matrix(snap, roff, woff, mat, lens, report)


def shape(G):
    """Range offsets of a batch with exactly G ranges: 5R+2W transactions, then one with the rest."""
    full, rem = divmod(G, 7)
    nr = [5] * full + ([min(rem, 5)] if rem else [])
    nw = [2] * full + ([max(rem - 5, 0)] if rem else [])
    roff = np.concatenate([[0], np.cumsum(nr)]).astype(np.int32)
    woff = np.concatenate([[0], np.cumsum(nw)]).astype(np.int32)
    return roff, woff


def edge_batch(rng, G, now, hot, prev_writes):
    """G ranges.  hot = None: random 16-byte keys, short ranges and single keys, a tenth of the
    reads on keys the previous batch wrote (history conflicts, no candidate edge).  hot = a sorted
    array of keys: every endpoint from it, single keys and spans of up to three neighbours, so reads
    and earlier writes of the batch meet.  2 % of the reads and of the writes are empty."""
    roff, woff = shape(G)
    R, Wn, T = int(roff[-1]), int(woff[-1]), len(roff) - 1
    if hot is None:
        rb = rng.integers(0, 256, size=(R, 16), dtype=np.uint8)
        wb = rng.integers(0, 256, size=(Wn, 16), dtype=np.uint8)
        if prev_writes is not None and len(prev_writes):
            again = rng.random(R) < 0.1
            rb[again] = prev_writes[rng.integers(0, len(prev_writes), size=int(again.sum()))]
        re, we = be_add(rb, 1, 17, rng), be_add(wb, 1, 17, rng)
        r_single, w_single = rng.random(R) < 0.5, rng.random(Wn) < 0.5
    else:
        H = len(hot)
        ri, wi = rng.integers(0, H - 3, size=R), rng.integers(0, H - 3, size=Wn)
        rs, ws = rng.integers(1, 4, size=R), rng.integers(1, 4, size=Wn)
        rb, wb, re, we = hot[ri], hot[wi], hot[ri + rs], hot[wi + ws]
        r_single, w_single = rng.random(R) < 0.8, rng.random(Wn) < 0.8
    re[r_single], we[w_single] = rb[r_single], wb[w_single]  # [k, k\0)
    rlen, wlen = np.where(r_single, 17, 16), np.where(w_single, 17, 16)
    r_empty, w_empty = rng.random(R) < 0.02, rng.random(Wn) < 0.02
    re[r_empty], we[w_empty] = rb[r_empty], wb[w_empty]  # [k, k)
    rlen[r_empty], wlen[w_empty] = 16, 16
    snap = now - rng.integers(0, 20, size=T)
    report = (rng.random(T) < 0.5).astype(np.uint8)
    return pack(rb, re, rlen, wb, we, wlen, roff, woff, snap, report), wb


def detect(engine, cs, pb, now, oldest):
    m = {}
    b = engine.ConflictBatch(cs, m)
    b.add_packed(pb)
    v = b.detect_conflicts(now, oldest)
    b.close()
    return v, {t: sorted(x) for t, x in m.items()}


# tiles: 1, 2, 64, 65, 66, 128, 129, 256, 257, 258, 513 (a full last tile, or one range in it)
EDGE_G = [255, 257, 64 * EDGE_TILE, 64 * EDGE_TILE + 1, 65 * EDGE_TILE + 1, 128 * EDGE_TILE, 128 * EDGE_TILE + 1,
          256 * EDGE_TILE, 256 * EDGE_TILE + 1, 257 * EDGE_TILE + 1, 512 * EDGE_TILE + 1]


def test_edge_tile_counts():
    assert [-(-g // EDGE_TILE) for g in EDGE_G] == [1, 2, 64, 65, 66, 128, 129, 256, 257, 258, 513]
    for g in EDGE_G:
        roff, woff = shape(g)
        assert int(roff[-1]) + int(woff[-1]) == g


@pytest.mark.parametrize("keys", ["random", "hot"])
@pytest.mark.parametrize("G", EDGE_G)
def test_edge_scan_tile_counts(engine, oracle_mod, G, keys):
    """Two batches of exactly G ranges; the second reads what the first wrote.  hot: about 3 G
    candidate edges, well inside the edge capacity (no sequential fallback)."""
    rng = np.random.default_rng(G * 2 + (keys == "hot"))
    hot = None
    if keys == "hot":
        hot = np.unique(rng.integers(0, 256, size=(max(32, G // 16), 16), dtype=np.uint8), axis=0)
    cs = engine.ConflictSet(0)
    sl = oracle_mod.SkipListBaseline()
    now, prev = 100, None
    for i in range(2):
        pb, prev = edge_batch(rng, G, now, hot, prev)
        assert pb.n_reads + pb.n_writes == G
        v, conf = detect(engine, cs, pb, now, now - 50)
        want, wconf = sl.detect(pb, now, now - 50)
        bad = np.nonzero(v != want)[0]
        assert len(bad) == 0, (i, bad[:10], v[bad[:10]], want[bad[:10]])
        assert {t: x for t, x in conf.items() if x} == {t: sorted(x) for t, x in wconf.items() if x}, i
        now += 10
    st = cs.stats()
    assert st["intra_fallbacks"] == 0
    if keys == "hot":
        assert st["intra_edges"] > 0
    else:
        assert st["intra_edges"] == 0
    cs.close()


# ---------------------------------------------------------------- segment preparation


def seg_batch(rng, Wn, now, prev_writes, extra_reads=200):
    """Wn writing transactions (one single-key write of a fresh random key and one read of another
    each: all commit, so the batch has exactly Wn disjoint union segments), then read-only
    transactions on keys the previous batches wrote, with snapshots on both sides of them."""
    wb = rng.integers(0, 256, size=(Wn, 16), dtype=np.uint8)
    span = rng.random(Wn) < 0.5
    we = wb.copy()
    we[span] = be_add(wb[span], 1, 17, rng)
    wlen = np.where(span, 16, 17)
    n_old = extra_reads if prev_writes is not None else 0
    rb = rng.integers(0, 256, size=(Wn + n_old, 16), dtype=np.uint8)
    if n_old:
        rb[Wn:] = prev_writes[rng.integers(0, len(prev_writes), size=n_old)]
    re = rb.copy()
    rlen = np.full(Wn + n_old, 17)
    T = Wn + n_old
    roff = np.arange(T + 1, dtype=np.int32)
    woff = np.minimum(np.arange(T + 1), Wn).astype(np.int32)
    snap = np.full(T, now - 1, np.int64)
    snap[Wn:] = now - rng.integers(1, 30, size=n_old)  # batches are 10 versions apart
    report = np.ones(T, np.uint8)
    return pack(rb, re, rlen, wb, we, wlen, roff, woff, snap, report), wb


def run_segments(engine, oracle_mod, sizes, seed, prefix=None, gc_interval=0, delta_limit=0):
    """Batches of the given write counts with 4 in flight against the semantic oracle; then the
    stored history, exact."""
    rng = np.random.default_rng(seed)
    cs = engine.ConflictSet(0)
    cs.set_gc_interval(gc_interval)
    cs.set_delta_limit(delta_limit)
    ref = oracle_mod.OracleConflictSet()
    seq, now, prev = [], 100, None
    for Wn in sizes:
        pb, wb = seg_batch(rng, Wn, now, prev)
        prev = wb if prev is None else np.concatenate([prev, wb])
        seq.append((prefixed(pb, prefix) if prefix else pb, now, 0))
        now += 10
    inflight, got = [], {}

    def done(j, bj):
        got[j] = (bj.wait(), {t: sorted(x) for t, x in bj.conflicting_key_range_map.items() if x})
        bj.close()

    for i, (pb, now_i, no) in enumerate(seq):
        b = engine.ConflictBatch(cs, {})
        b.add_packed(pb)
        b.detect_async(now_i, no)
        inflight.append((i, b))
        if len(inflight) > 4:
            done(*inflight.pop(0))
    for j, bj in inflight:
        done(j, bj)
    conflicts = 0
    for i, (pb, now_i, no) in enumerate(seq):
        want, wconf = ref.detect(pb, now_i, no)
        v, conf = got[i]
        bad = np.nonzero(v != want)[0]
        assert len(bad) == 0, (i, bad[:10], v[bad[:10]], want[bad[:10]])
        assert conf == {t: sorted(x) for t, x in wconf.items() if x}, i
        assert (want[:sizes[i]] == 2).all()  # every writer commits: the batch has sizes[i] segments
        conflicts += int((want == 0).sum())
    assert conflicts > 0  # later batches did read the earlier segments
    st = cs.stats()
    assert st["segments_sum"] == sum(sizes), (st["segments_sum"], sum(sizes))
    keys, vers = ref.dump_history()
    want = canon(keys, vers, 0, ref.oldest_version)
    have = split_dump(cs.dump_history())
    assert len(have[1]) == len(want[1]), (len(have[1]), len(want[1]))  # the history's size
    assert have == want
    cs.close()
    return st


@pytest.mark.parametrize("k", [1, 2, 64, 65, 129, 257])
def test_seg_prep_tile_counts_narrow(engine, oracle_mod, k):
    """63 segments per tile (short keys, W < 24576): 63 k segments are k tiles, one more segment is
    one more tile, one fewer leaves the last tile a segment short.  Four consecutive batches, each
    merging into the delta the ones before left."""
    run_segments(engine, oracle_mod, [63 * k, 63 * k + 1, 63 * k - 1, 63 * k + 1], seed=k)


def test_seg_prep_wide_layout(engine, oracle_mod):
    """W >= 24576: 127 segments per tile, 258 tiles and 257."""
    run_segments(engine, oracle_mod, [127 * 257 + 1, 127 * 257, 24576], seed=7)


def test_seg_prep_long_keys(engine, oracle_mod):
    """Keys of 36 and 37 bytes behind a shared 20-byte prefix: the long-key layout, every key's tail
    reached through segk's offsets; 65 tiles, 66 and 2."""
    run_segments(engine, oracle_mod, [63 * 65, 63 * 65 + 1, 64], seed=8, prefix=b"\x02tenant\x00ledger\x00\x15\x01\x15\x02\x00")


def test_seg_prep_across_compactions(engine, oracle_mod):
    """A compaction and removeBefore every second batch between the merges."""
    st = run_segments(engine, oracle_mod, [63 * 65 + 1, 63 * 64, 63 * 65, 63 * 2 + 1, 63 * 129 + 1, 63], seed=9,
                      gc_interval=2)
    assert st["compactions"] >= 2, st["compactions"]
