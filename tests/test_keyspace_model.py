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
    if klen is None:  # keys of different lengths: by the offsets
        return hdr, K.split_keys(kb, ko), vv.tolist()
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


# ---- keys of different lengths, and the search plan (tests/search_plan.py)


def random_var_universe(rng, U):
    """U keys over two byte values, 0 to 40 bytes long: proper prefixes, \\0 extensions and keys that
    differ only past 16 and past 24 bytes abound."""
    keys = {b""}
    stems = [bytes(rng.integers(0, 2, size=int(n)).astype(np.uint8) * 255) for n in (15, 16, 23, 24, 31)]
    while len(keys) < U:
        s = stems[int(rng.integers(0, len(stems)))] if rng.random() < 0.7 else b""
        keys.add(s + bytes(rng.integers(0, 2, size=int(rng.integers(0, 9))).astype(np.uint8) * 255))
    return K.var_universe(keys)


def test_variable_length_resolve_matches_semantic_oracle(oracle_built):
    """A few hundred random multi-range batches over small universes of keys of different lengths:
    verdicts, reports and the state after each batch (pack_keys, rle, TxnBatch.pack on offsets)."""
    rng = np.random.default_rng(12)
    seen = {K.CONFLICT: 0, K.TOO_OLD: 0, K.COMMITTED: 0}
    for trial in range(60):
        U = int(rng.integers(6, 40))
        model = K.KeyspaceModel(random_var_universe(rng, U), 600)
        assert model.klen is None and model.U == U
        hist = np.array([1, U // 2])
        model.load(hist, [700, 800])
        o = oracle_built.OracleConflictSet()
        o.load_history(*model.pack_keys(hist), np.array([700, 800]), 600)
        o.set_oldest_version(1000)
        now = 2000
        for i in range(5):
            tb = random_txn_batch(rng, U, int(rng.integers(3, 60)), now, 1000, 1500)
            res = check_against_oracle(o, model, tb, now, 1000, 600, ("var", trial, i))
            for v in seen:
                seen[v] += int((res.verdicts == v).sum())
            now += 10
    assert min(seen.values()) > 300, seen


def test_variable_length_dump_comparison():
    """assert_dump_equals on keys of different lengths: equal states pass; a wrong version, a wrong
    byte and a wrong length are each found at their boundary."""
    model = K.KeyspaceModel(K.var_universe([b"", b"a", b"a\0", b"ab" * 20, b"b"]), 5)
    model.load(np.array([0, 2, 3]), [7, 8, 9])
    hdr, kb, ko, vv = model.rle()
    assert K.split_keys(kb, ko) == [b"", b"a\0", b"ab" * 20]
    K.assert_dump_equals((kb, ko, vv, hdr), model.rle())
    for at, dump in ((1, (kb, ko, np.array([7, 6, 9]), hdr)),
                     (2, (np.concatenate([kb[:-1], [0]]).astype(np.uint8), ko, vv, hdr)),
                     (1, (kb, ko + np.array([0, 0, 1, 1]), vv, hdr))):
        with pytest.raises(AssertionError) as e:
            K.assert_dump_equals(dump, model.rle())
        assert e.value.args[0][2] == at, e.value.args


@pytest.fixture(scope="module")
def search_plans():
    from tests import search_plan as SP

    return [SP.build(0), SP.build(1)]


def run_on_oracle(oracle_built, p):
    from tests import search_plan as SP

    o = oracle_built.OracleConflictSet()
    o.load_history(*p.loaded)
    o.set_oldest_version(SP.OLDEST)
    for s in p.steps:
        for pb, now, new_oldest, want in s.batches:
            got, _ = o.detect(pb, now, new_oldest)
            assert pb.n_txn <= 49152 and not (want == K.TOO_OLD).any()
            assert (got == want).all(), (s.name, np.flatnonzero(got != want)[:10])
        if s.state is not None:
            keys, vers = o.dump_history()
            assert _rle_lists(s.state, None) == canon(keys, vers, p.header, o.oldest_version), s.name
            if s.as_stored:
                assert _rle_lists(s.state, None) == canon(keys, vers, p.header, NO_FLOOR), s.name


@pytest.mark.parametrize("polarity", [0, 1])
def test_search_plan_matches_semantic_oracle(oracle_built, search_plans, polarity):
    """Every batch of the core search plan against the semantic oracle: verdicts, and the state after
    every write batch, the compaction and the GC."""
    run_on_oracle(oracle_built, search_plans[polarity])


@pytest.mark.parametrize("kind", ["short", "long", "wide", "path-d"])
def test_search_riders_match_semantic_oracle(oracle_built, search_plans, kind):
    """The riders and the previous-batch-segment batches against the semantic oracle; the riders'
    common reads have the core plan's verdicts (their keys and versions are the same)."""
    from tests import search_plan as SP

    p = SP.build_path_d(0) if kind == "path-d" else SP.build(0, kind)
    run_on_oracle(oracle_built, p)
    if kind == "path-d":
        assert sorted(p.coverage["path_d"]) == sorted(set(SP.PATH_D_SIZES[:-1]) | {max(p.coverage["path_d"])})
        assert max(p.coverage["path_d"]) > 4000
    else:
        core = search_plans[0]
        assert [s.name for s in p.steps] == [s.name for s in core.steps]
        longest = max(int(np.diff(pb.key_offsets).max()) for s in p.steps for pb, _, _, _ in s.batches)
        assert (longest > 24) == (kind == "long")


def test_search_plan_conditions(search_plans):
    """The plan's own conditions, from the model alone: no read is sent once (K.twice's single share is
    asserted 0 as each batch is built); over both polarities every directed key has a read that flips
    one of its two verdicts under each of the four one-segment errors, in the loaded base alone and
    over the written history; every tail-edge class over 16 bytes is queried at all eight tail
    residues in every read batch; the run starts stand at ranks 0, 1, 7 mod 8 and 0, 1, 63 mod 64 in
    the base and, by the predicted delta, in the delta; the crowded directory family and the sparse
    one; per-family counts of reads decided by one structure alone."""
    from tests import search_plan as SP

    counts = SP.check_sensitivity(search_plans)
    assert counts["base"] >= 400 and counts["delta"] == len(search_plans[0].directed) >= 500
    for p in search_plans:
        assert p.H > 32768 and all(v >= SP.OLDEST + 1 for v in (p.loaded[2].min(), p.header))
        assert all(p.align[L] == set(range(8)) for L in SP.TAIL_LENGTHS if L > 16)
        assert p.coverage["run_starts_base"] == [(0, 0), (1, 1), (7, 63)]
        d = p.coverage["run_starts_delta"]
        assert {0, 1, 7} <= {a for a, _ in d} and {0, 1, 63} <= {b for _, b in d}
        assert p.coverage["directory"]["crowded"] > 4096 and p.coverage["directory"]["sparse"] <= 8
        for fam, (n, base, delta, prev) in p.coverage["decided"].items():
            assert n >= 500 and min(base, delta, prev) >= 40, (fam, n, base, delta, prev)
        lens = {len(k) for k in p.directed}
        assert {0, 15, 16, 17, 23, 24, 25, 30, 63, 64, 65, 111, 112, 113, 120, 121, 122, 200, 201} <= lens
        writes = [s for s in p.steps if s.kind == "write"]
        assert [s.delta_before for s in writes][0] == 0 and writes[-1].delta_before < p.coverage["delta_size"]


def test_search_universe_is_sorted_in_the_reference_order(oracle_built, search_plans):
    """Python's order of bytes is the reference's order of keys (memcmp, then length): every
    neighbouring pair of the plan's universe through the oracle's point comparison."""
    u = search_plans[0].ukeys
    assert u[0] == b"" and len(set(u)) == len(u)
    for a, b in zip(u, u[1:]):
        assert oracle_built.point_compare(a, True, False, b, True, False) < 0, (a, b)


# ---- the batch sort's plan (tests/sort_plan.py)

SORT_KINDS = ["single-long", "single-short", "cold-64", "cold-8", "warm"] + [f"halves-{t}" for t in (1, 100, 200, 400, 800, 1600)]


@pytest.fixture(scope="module")
def sort_plans():
    """Every plan of tests/sort_plan.py, built once (building asserts the coverage of each: positions
    reached, run lengths, c values, bucket sizes)."""
    from tests import sort_plan as SP

    return {kind: SP.build(kind) for kind in SORT_KINDS}


def test_resolve_moved_moves_one_endpoint():
    """K.resolve_moved: one endpoint index of one range moves by one, an inverted range counts as empty,
    a move out of the universe is None, and the caller's model stays as it was."""
    model = K.KeyspaceModel(K.var_universe([b"a", b"b", b"c", b"d"]), 5)
    tb = K.TxnBatch()
    tb.add(writes=[(1, 2)], snap=9)
    tb.add(reads=[(0, 1)], snap=9, report=True)
    base = K.resolve(model, tb, 10, 1, facts=False)
    assert base.verdicts.tolist() == [K.COMMITTED, K.COMMITTED] and model.ver.tolist() == [5, 10, 5, 5]
    fresh = K.KeyspaceModel(K.var_universe([b"a", b"b", b"c", b"d"]), 5)
    m, res = K.resolve_moved(fresh, tb, 10, 1, "re", 0, 1)  # the read now holds the written key
    assert res.verdicts.tolist() == [K.COMMITTED, K.CONFLICT] and res.reports == {1: [0]}
    m, res = K.resolve_moved(fresh, tb, 10, 1, "wa", 0, -1)  # the write begins one key earlier
    assert res.verdicts.tolist() == [K.COMMITTED, K.CONFLICT] and m.ver.tolist() == [10, 10, 5, 5]
    m, res = K.resolve_moved(fresh, tb, 10, 1, "wa", 0, 1)  # the write becomes empty
    assert m.ver.tolist() == [5, 5, 5, 5] and K.outcome(m, res) != K.outcome(model, base)
    m, res = K.resolve_moved(fresh, tb, 10, 1, "we", 0, -1)
    assert m.ver.tolist() == [5, 5, 5, 5]
    assert K.resolve_moved(fresh, tb, 10, 1, "ra", 0, -1) is None and fresh.ver.tolist() == [5, 5, 5, 5]


def test_sort_plan_wrong_order_cannot_pass(sort_plans):
    """Every step of every plan re-resolved with one endpoint index moved by one (what an endpoint
    sorted one key off, or a class-order error at an equal key, comes to): each of the two moves of
    every endpoint at a directed key changes a verdict, a report or the state in at least one parity.
    The exempt moves are counted by reason: the extras, empty ranges, the pair families' outward moves
    and the endpoints whose neighbour in the direction of the move is no chain key."""
    proved = {}
    for kind, p in sort_plans.items():
        p.prove()
        proved[kind] = sum(p.proved.values())
        for name, ex in p.exempt.items():
            # nothing but the ends of the chain (of the pair families) is exempt for its place in the universe
            assert ex["edge"] <= 7, (kind, name, ex)
            assert ex["outward"] == 0 and ex["empty"] == 0 or name == "pairs", (kind, name, ex)
    assert proved["single-long"] >= 2000 and proved["cold-64"] >= 2000 and proved["cold-8"] >= 4000, proved
    assert min(proved.values()) >= 4, proved
    assert sort_plans["single-long"].proved["pairs"] == 8  # begin + 1 and end - 1 of the two pairs and the two triples


def test_sort_plan_conditions(sort_plans):
    """The plans' own conditions, from the model alone: conflicts and commits are each at least 0.3 of
    every step; the one-bucket plans reach every batch size, register width, tile count, run length and
    placement; the cold plans every c, the clamp under each, len - c = 18 | 19 | 20 and one bucket past
    256 from keys tied on the whole window; the two-bucket plans every odd size; the warm plan its
    table hand-overs.  (Each builder asserts the details; here what the GPU test relies on.)"""
    from tests import sort_plan as SP

    for kind, p in sort_plans.items():
        assert all(min(s.shares) >= 0.3 for s in p.steps), kind
        assert all(b.T == b.pb.n_txn == len(b.want) <= 8192 for b in p.batches), kind
        assert max(b.facts.nb for b in p.batches) <= 257 and max(b.facts.E for b in p.batches) <= 4 * 8192
    t = sort_plans["single-long"].tokens
    assert {("E", n) for n in SP.SIZES} <= t and SP.PLACEMENTS <= t
    assert {("run-keys", d) for d in SP.RUN_KEYS} <= t and {("run-endpoints", n) for n in SP.RUN_ENDPOINTS} <= t
    assert {("path", x) for x in ("pair", "simple", "pfall", "slow", "mlong")} <= t
    assert not any(x[0] == "path" for x in sort_plans["single-short"].tokens)
    for kind in ("cold-64", "cold-8"):
        t = sort_plans[kind].tokens
        assert {("c", c) for c in SP.COLD_C + (64,)} <= t and {("clamp", c) for c in SP.COLD_C} <= t
        assert {("len-c", n) for n in (0, 18, 19, 20)} <= t
        assert sum(b.big for b in sort_plans[kind].batches) == 2
    sizes = set().union(*(sort_plans[f"halves-{x}"].tokens for x in SP.HALVES))
    assert {("bucket", n) for n in SP.HALF_SIZES + (1025,)} <= sizes
    assert [b.big for b in sort_plans["warm"].batches] == [0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 1, 0]


@pytest.mark.parametrize("kind", SORT_KINDS)
def test_sort_plan_matches_semantic_oracle(oracle_built, sort_plans, kind):
    """Every batch of the sort's plans against the semantic oracle: verdicts, reports and the state."""
    from tests import sort_plan as SP

    p = sort_plans[kind]
    o = oracle_built.OracleConflictSet()
    o.load_history(*p.loaded)
    o.set_oldest_version(SP.OLDEST)
    for b in p.batches:
        got, conf = o.detect(b.pb, b.now, SP.OLDEST)
        assert (got == b.want).all(), (b.name, np.flatnonzero(got != b.want)[:10])
        assert {t: sorted(x) for t, x in conf.items()} == b.reports, b.name
        keys, vers = o.dump_history()
        assert _rle_lists(b.state, None) == canon(keys, vers, SP.HEADER, NO_FLOOR), b.name


def test_sort_plan_orders_like_the_reference(oracle_built, sort_plans):
    """The plan's total order (key, class, endpoint id, Python's order of bytes) through the oracle's
    point comparison, on the batches with the longest tie runs: neighbours in the order never compare
    the other way round."""
    from tests import sort_plan as SP

    cls_flags = {SP.RB: (True, False), SP.RE: (False, False), SP.WB: (True, True), SP.WE: (False, True)}
    p = sort_plans["single-long"]
    for b in p.batches:
        if b.step not in ("tails", "ladder", "long", "pairs", "cap19"):
            continue
        tb_keys, cls = SP.endpoint_table(b.arrays, p.ukeys)
        order = SP.total_order(tb_keys, cls)
        for x, y in zip(order, order[1:]):
            assert oracle_built.point_compare(tb_keys[x], *cls_flags[cls[x]], tb_keys[y], *cls_flags[cls[y]]) <= 0, (b.name, x, y)
