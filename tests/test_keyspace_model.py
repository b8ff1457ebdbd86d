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
