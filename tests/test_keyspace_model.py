"""The dense key-space model (tests/keyspace_model.py) on the CPU: the batch sequence the GPU tests
send satisfies its own conditions from the model alone, and the model agrees with the semantic
oracle on a reduced sequence, verdicts and canonical state -- the one place the two meet, so that a
mistake in the model shows up here and not as a puzzling GPU failure."""
import numpy as np
import pytest

from tests import keyspace_model as K
from tests.export_helpers import NO_FLOOR, canon


def _rle_lists(state, klen):
    hdr, kb, ko, vv = state
    raw = kb.tobytes()
    return hdr, [raw[i * klen:(i + 1) * klen] for i in range(len(vv))], vv.tolist()


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("D", [0, 10 ** 14 + 7])
def test_model_matches_semantic_oracle(oracle_built, shape, D):
    loaded, steps = K.build_plan(5, shape, D, 5000, 30, 300, 400, 2, wide_min=200, max_gap=3)
    o = oracle_built.OracleConflictSet()
    o.load_history(*loaded)
    o.set_oldest_version(D + 500)
    header = loaded[3]
    klen = 16 if shape == "random16" else 20
    for i, st in enumerate(steps):
        for pb, now, new_oldest, want in st["batches"]:
            got, _ = o.detect(pb, now, new_oldest)
            assert len(got) == pb.n_txn and not (got == K.TOO_OLD).any()
            assert (got == want).all(), (i, np.flatnonzero(got != want)[:10])
            assert (want == K.CONFLICT).mean() >= 0.3 and (want == K.COMMITTED).mean() >= 0.3
        state, as_stored = st["state"]
        keys, vers = o.dump_history()
        # (adjacent writes of one batch keep the boundary between them: a few more than the model's)
        assert 0 <= o.history_size() - st["boundaries"] <= 64 or not as_stored
        assert _rle_lists(state, klen) == canon(keys, vers, header, o.oldest_version), i
        if as_stored:  # nothing is below the floor yet: the stored form itself
            assert _rle_lists(state, klen) == canon(keys, vers, header, NO_FLOOR), i


def test_interleaved_batch_matches_semantic_oracle(oracle_built):
    rng = np.random.default_rng(6)
    model = K.KeyspaceModel(K.make_universe(rng, 6000, "prefix20"), 1234)
    hist = np.sort(rng.choice(6000, size=3000, replace=False))
    vers = 1000 + np.cumsum(rng.integers(1, 1000, size=3000)) % 1000
    model.load(hist, vers)
    o = oracle_built.OracleConflictSet()
    o.load_history(*model.pack_keys(hist), vers, 1234)
    o.set_oldest_version(500)
    for i in range(3):
        pb, want = K.interleaved_step(60 + i, model, 5000 + i, 500)
        assert pb.n_txn <= 300
        got, _ = o.detect(pb, 5000 + i, 500)
        assert (got == want).all(), (i, np.flatnonzero(got != want)[:10])
        keys, v = o.dump_history()
        assert _rle_lists(model.rle(), 20) == canon(keys, v, 1234, NO_FLOOR)


def test_climb_level_replays_range_max():
    """climb_level against a brute-force walk of the 64-ary hierarchy."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(200, 600_000))
        lo = int(rng.integers(0, n - 130))
        hi = int(rng.integers(lo + 1, n))
        p = int(rng.integers(lo, hi))
        a, b, q, want = lo, hi, p, None
        for L in range(4):
            if b - a <= 128 or L == 3:
                want = L
                break
            a2, b2 = -(-a // 64), b // 64
            if q in range(a, a2 * 64) or q in range(b2 * 64, b):
                want = L
                break
            a, b, q = a2, b2, q // 64
        assert K.climb_level(lo, hi, [p]) == want
        assert K.climb_level(lo, hi, [lo - 1, hi]) is None


def test_plan_sizes_reach_the_upper_levels():
    """The sequences the GPU tests run, checked without a GPU.  Small: by the end of its three write
    steps more than 8192 boundaries begin or end a written run (the delta tier's entries: a wide
    read there uses the delta's level 2), and no batch exceeds the engine's transaction bound.
    Both: after the load and after the compaction at least 20 reads (each sent at its maximum and
    one below) are decided by level-2 entries alone, and on the big history by level-3 entries."""
    from tests.test_gpu_rangemax_model import BIG, SMALL

    loaded, steps = K.build_plan(1, "random16", 0, **SMALL)
    assert len(steps) == 9 and all(s["state"] is not None for s in steps)
    hdr, _, _, vv = steps[3]["state"][0][:4]
    first_now = steps[1]["batches"][0][1]
    prev = np.concatenate([[hdr], vv[:-1]])
    assert int(((vv >= first_now) | (prev >= first_now)).sum()) > 8192
    assert all(pb.n_txn <= 49152 for s in steps for pb, _, _, _ in s["batches"])
    assert all(steps[i]["reached"][2] >= 20 for i in (0, 6))
    _, steps = K.build_plan(1, "prefix20", 10 ** 14 + 7, **BIG)
    assert all(steps[i]["reached"][2] >= 20 and steps[i]["reached"][3] >= 20 for i in (0, 6))
    assert all(pb.n_txn <= 49152 for s in steps for pb, _, _, _ in s["batches"])


# ---- the batch-order model (K.resolve) against the semantic oracle


def random_txn_batch(rng, U, n, now, oldest, old_snap):
    """Multi-range transactions over a universe of U keys: touching and nested ranges abound on so
    few keys; empty ranges, transactions that read their own write, snapshots below `oldest`
    (TooOld) and at `old_snap` (below an earlier batch's writes: history conflicts)."""
    tb = K.TxnBatch()

    def rng_range():
        a = int(rng.integers(0, U))
        if rng.random() < 0.15:
            return a, a
        return a, min(U - 1, a + int(rng.integers(1, 4))) if a < U - 1 else a

    for _ in range(n):
        reads = [rng_range() for _ in range(int(rng.integers(0, 4)))]
        writes = [rng_range() for _ in range(int(rng.integers(0, 3)))]
        if reads and rng.random() < 0.2:
            writes.append(reads[0])  # reads its own write
        x = rng.random()
        snap = oldest - 1 - int(rng.integers(0, 3)) if x < 0.07 else (old_snap if x < 0.3 else now - 1)
        tb.add(reads, writes, snap, rng.random() < 0.6)
    return tb


def check_against_oracle(o, model, tb, now, oldest, header, what):
    pb = tb.pack(model)
    res = K.resolve(model, tb, now, oldest)
    got, conf = o.detect(pb, now, oldest)
    assert (got == res.verdicts).all(), (what, np.flatnonzero(got != res.verdicts)[:10])
    assert {t: sorted(x) for t, x in conf.items()} == res.reports, what
    keys, vers = o.dump_history()
    assert _rle_lists(model.rle(), model.klen) == canon(keys, vers, header, NO_FLOOR), what
    return res


@pytest.mark.parametrize("shape", K.SHAPES)
def test_resolve_matches_semantic_oracle_on_random_batches(oracle_built, shape):
    """A few hundred random multi-range batches over small universes: verdicts, reports (an entry for
    every reporting admitted transaction with reads) and the state after each batch."""
    rng = np.random.default_rng(11)
    seen = {K.CONFLICT: 0, K.TOO_OLD: 0, K.COMMITTED: 0}
    hist_conflicts = intra = own = 0
    for trial in range(60):
        U = int(rng.integers(6, 40))
        model = K.KeyspaceModel(K.make_universe(rng, U, shape), 600)
        hist = np.array([1, U // 2])
        model.load(hist, [700, 800])
        o = oracle_built.OracleConflictSet()
        o.load_history(*model.pack_keys(hist), np.array([700, 800]), 600)
        o.set_oldest_version(1000)
        now = 2000
        for i in range(5):
            tb = random_txn_batch(rng, U, int(rng.integers(3, 60)), now, 1000, 1500)
            res = check_against_oracle(o, model, tb, now, 1000, 600, (shape, trial, i))
            for v in seen:
                seen[v] += int((res.verdicts == v).sum())
            f = res.facts
            hist_conflicts += int((f.dead & (res.verdicts == K.CONFLICT)).sum())
            intra += len(res.first_intra)
            own += sum(1 for t in range(len(tb)) if res.verdicts[t] == K.COMMITTED
                       and any(a < b and (a, b) in tb.writes[t] for a, b in tb.reads[t]))
            now += 10
    assert min(seen.values()) > 300 and min(hist_conflicts, intra) > 300 and own > 50, (seen, hist_conflicts, intra, own)


@pytest.mark.parametrize("kind,shape", [("core", "random16"), ("fill", "prefix20"), ("sizes", "random16")])
def test_directed_resolution_plan_matches_semantic_oracle(oracle_built, kind, shape):
    """Every directed batch of tests/resolution_plan.py, at full size (the oracle takes them in
    milliseconds): building the plan asserts its coverage from the model's facts; then verdicts,
    reports and the state after every batch against the semantic oracle."""
    from tests import resolution_plan as RP

    p = RP.build(kind, 1, shape)
    assert set(p.coverage) == {"core": {"ladders", "groups", "prepass"}, "fill": {"fill"}, "sizes": {"sizes"}}[kind]
    o = oracle_built.OracleConflictSet()
    o.load_history(*p.loaded)
    o.set_oldest_version(RP.OLDEST)
    for s in p.steps:
        got, conf = o.detect(s.pb, s.now, s.oldest)
        assert s.pb.n_txn == s.T <= 49152
        assert (got == s.want).all(), (s.name, np.flatnonzero(got != s.want)[:10])
        assert {t: sorted(x) for t, x in conf.items()} == s.reports, s.name
        keys, vers = o.dump_history()
        assert _rle_lists(s.state, p.model.klen) == canon(keys, vers, RP.HEADER, NO_FLOOR), s.name
