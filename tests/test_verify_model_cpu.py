"""CPU tests of tests/verify_model.py, the numpy restatement of fdbcs_history_verify the GPU tests
compare the device report with: tiers it builds itself are clean with the examined counts their
sizes imply, and every single-element mutation is flagged in the right class, at the right index,
with the exact count.  Short and long keys, X / X\\0 pairs, holes."""
import numpy as np
import pytest

from tests import verify_model as M

C = M.CLASSES.index
SIGN = 1 << 63


def state(seed=3, nb=5000, nd=700):
    rng = np.random.default_rng(seed)
    keys = M.make_keys(rng, nb + nd)
    pick = np.zeros(len(keys), bool)
    pick[rng.choice(len(keys), size=nd, replace=False)] = True
    pick[0] = False  # the empty key stays in the base
    bk = [k for k, p in zip(keys, pick) if not p]
    dk = [k for k, p in zip(keys, pick) if p]
    dk += [k for k in bk[::97]][:40]  # keys both tiers hold
    dk.sort()
    bv = rng.integers(100, 1000, size=len(bk))
    dv = rng.integers(2000, 3000, size=len(dk))
    dv[rng.random(len(dk)) < 0.4] = M.HOLE
    return M.build(bk, bv, dk, dv, header=50)


@pytest.fixture(scope="module")
def st():
    return state()


def only(rows, *flagged):
    """Exactly the (tier, class, violations, first) entries given are violations."""
    got = sorted((t, c, r[1], r[2]) for t in range(2) for c, r in enumerate(rows[t]) if r[1])
    assert got == sorted((t, C(c), v, f) for t, c, v, f in flagged), got


def test_built_tiers_are_clean_with_the_counts_their_sizes_imply(st):
    rows = M.verify(st)
    assert M.clean(rows)
    for tier, t in enumerate(st.tiers):
        want = M.expected_examined(t.n, int((t.ln > 16).sum()), tier)
        for name, ex in want.items():
            assert rows[tier][C(name)] == (ex, 0, -1), (tier, name)
    # every delta boundary with a version pairs with its base predecessor; inside pairs come on top
    versioned = int((st.tiers[1].ver != M.HOLE).sum())
    assert rows[1][C("dominance")][0] > versioned > 0
    assert rows[0][C("dir")] == rows[1][C("edir")] == (0, 0, -1)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097])
def test_sizes_around_every_block_edge(n):
    keys = M.make_keys(np.random.default_rng(n), n)
    s = M.build(keys, np.arange(n) % 17 + 1, header=0)
    rows = M.verify(s)
    assert M.clean(rows)
    want = M.expected_examined(n, int((s.tiers[0].ln > 16).sum()), 0)
    assert {k: rows[0][C(k)][0] for k in want} == (want if n else dict.fromkeys(want, 0))


def test_the_key_mix(st):
    base = st.tiers[0]
    lens = set(int(x) for x in base.ln)
    assert set(range(0, 17)) <= lens and {17, 24, 25, 40, 113} <= lens
    tie = (base.hi[:-1] == base.hi[1:]) & (base.lo[:-1] == base.lo[1:])
    both_long = (base.ln[:-1] > 16) & (base.ln[1:] > 16)
    assert (tie & both_long).sum() > 50  # order decided by tails
    assert (tie & ~both_long).sum() > 50  # X / X\0 and prefix pairs: order decided by length


def test_key_prefix_mutations(st):
    base = st.tiers[0]
    i = 1001  # not a group start, not a block start
    assert i % 8 and int(base.ln[i]) >= 4
    # a low prefix bit inside the key: order breaks against one neighbour, or not at all; never padding
    rows = M.verify(st, ("key", 0, i, 0, 1 << 62))
    assert rows[0][C("padding")][1] == 0 and rows[0][C("order")][1] == 1 and rows[0][C("order")][2] in (i - 1, i)
    # a bit past a short key's length: padding at i (and the key now sorts after its X\0 successor or not)
    j = next(k for k in range(8 * 100 + 1, base.n) if k % 8 and int(base.ln[k]) < 16)
    rows = M.verify(st, ("key", 0, j, 1, 0))
    assert rows[0][C("padding")] == (base.n, 1, j)
    # a group start that is also a block and sample start: skey8, every tree level that samples it
    rows = M.verify(st, ("key", 0, 512, 1 << 63, 0), checks=("skey8", "skey", "lvl1"))
    only(rows, (0, "skey8", 1, 64), (0, "skey", 2, 8))  # level 0 entry 8, level 1 entry 1 (1 << 48 | 1)
    rows = M.verify(st, ("key", 0, 0, 1, 0), checks=("skey",))
    assert rows[0][C("skey")][1:] == (M.IDX_LEVELS, 0)  # boundary 0 is entry 0 of every level


def test_len_tail_mutations(st):
    base = st.tiers[0]
    i = next(k for k in range(base.n) if int(base.ln[k]) == 40)
    far = (st.tail_used // 8) ^ int(base.tu[i])  # the unit becomes tail_used / 8: past the arena
    rows = M.verify(st, ("len_tail", 0, i, 0, far))
    assert rows[0][C("tails")][1:] == (1, i)
    # the order of a pair that needs that tail is not judged
    assert rows[0][C("order")][1] == 0
    # a long key's length cut to 16: the tail is no longer read, X\0-style length order may break
    rows = M.verify(st, ("len_tail", 0, i, 40 ^ 8, 0))
    assert rows[0][C("tails")][0] == int((base.ln > 16).sum()) - 1
    assert rows[0][C("padding")][1:] == (1, i)


def test_tail_word_mutation(st):
    base = st.tiers[0]
    tie = np.flatnonzero((base.hi[:-1] == base.hi[1:]) & (base.lo[:-1] == base.lo[1:]) & (base.ln[:-1] > 16)
                         & (base.ln[1:] > 16))
    i = int(tie[len(tie) // 2])
    # the first tail byte of key i + 1 (the lowest byte of its first arena word) falls below key i's
    w = int(base.tu[i + 1])
    first = int(st.arena[w]) & 0xFF
    rows = M.verify(st, ("tail_word", 0, w, first))  # byte -> 0
    assert rows[0][C("order")][1] >= 1 and rows[0][C("order")][2] in (i, i + 1)
    assert sum(r[1] for t in rows for c, r in enumerate(t) if c != C("order")) == 0


def test_version_mutations(st):
    base = st.tiers[0]
    b = 20
    blk = base.ver[64 * b:64 * b + 64]
    top = int(blk.argmax())
    assert (blk == blk[top]).sum() >= 1
    # a non-maximum lowered: nothing (the base has no delta boundary above it that it could now exceed)
    low = next(k for k in range(64) if blk[k] < blk[top] and int(blk[k]) & 1)
    assert M.clean(M.verify(st, ("version", 0, 64 * b + low, 1), checks=("lvl1", "lvl2", "lvl3", "versions")))
    # any element raised above everything: one entry of each level
    rows = M.verify(st, ("version", 0, 64 * b + low, 1 << 40), checks=("lvl1", "lvl2", "lvl3", "versions"))
    only(rows, (0, "lvl1", 1, b), (0, "lvl2", 1, 0), (0, "lvl3", 1, 0))
    # a base version that becomes a hole
    i = 64 * b + low
    rows = M.verify(st, ("version", 0, i, int(base.ver[i]) ^ SIGN), checks=("versions",))
    only(rows, (0, "versions", 1, i))


def test_level_and_sample_mutations(st):
    for tier in (0, 1):
        t = st.tiers[tier]
        for what, idx in (("lvl1", 0), ("lvl1", len(t.lvl1) - 1), ("lvl2", len(t.lvl2) - 1), ("skey8", len(t.skey8[0]) - 1)):
            only(M.verify(st, (what, tier, idx, 4, 0)), (tier, what, 1, idx))
        L = 1
        d = len(t.skey[L][0]) - 1
        only(M.verify(st, ("skey", tier, d, 0, 1, L)), (tier, "skey", 1, L << 48 | d))


def test_lvl3_replicas(st):
    base = st.tiers[0]
    holder = 0  # entry 0's maximum stands in replica 0
    top = int(base.lvl3[holder])
    assert top == int(base.ver.max())
    # a replica below the maximum, changed but still below: nothing
    assert M.clean(M.verify(st, ("lvl3", 0, 3, SIGN | 5)))  # HOLE -> 5
    # the only holder lowered: the entry
    only(M.verify(st, ("lvl3", 0, holder, 1 if top & 1 else top)), (0, "lvl3", 1, 0))
    # any replica raised above the maximum: the entry
    only(M.verify(st, ("lvl3", 0, 5, SIGN | (1 << 40))), (0, "lvl3", 1, 0))


def test_dominance(st):
    base, delta = st.tiers
    # a versioned delta boundary whose base predecessor is a real boundary
    j = next(k for k in range(10, delta.n) if int(delta.ver[k]) != M.HOLE)
    v = int(delta.ver[j])
    rows = M.verify(st, ("version", 1, j, v ^ 1), checks=("dominance",))  # 1 stands below every base version
    assert rows[1][C("dominance")][1] >= 1 and rows[1][C("dominance")][2] == j
    # a hole is never judged
    h = next(k for k in range(delta.n) if int(delta.ver[k]) == M.HOLE)
    assert M.clean(M.verify(st, ("version", 1, h, 0), checks=("dominance",)))  # (xor 0: as stored)
    # a base version above the delta boundary that covers it: reported at that delta boundary
    rows0 = M.verify(st, checks=("dominance",))
    ab = st.arena.tobytes()
    for i in (base.n // 2, base.n // 3, base.n - 1):
        rows = M.verify(st, ("version", 0, i, 1 << 50), checks=("dominance",))
        assert rows[1][C("dominance")][0] == rows0[1][C("dominance")][0]
        # the pairs that meet base boundary i: versioned delta boundaries whose base predecessor it is
        # (the first delta boundary at or after it up to the next base boundary), and the delta
        # boundary strictly below it when that one carries a version
        want = []
        for k in range(delta.n):
            c = M.stored_cmp(st, 1, k, 0, i, ab)
            nxt = M.stored_cmp(st, 1, k, 0, i + 1, ab) if i + 1 < base.n else -1
            if c >= 0 and nxt < 0 and int(delta.ver[k]) != M.HOLE:
                want.append(k)
        below = [k for k in range(delta.n) if M.stored_cmp(st, 1, k, 0, i, ab) <= 0]
        if below and M.stored_cmp(st, 1, below[-1], 0, i, ab) < 0 and int(delta.ver[below[-1]]) != M.HOLE:
            want.append(below[-1])
        assert rows[1][C("dominance")][1:] == ((len(want), min(want)) if want else (0, -1)), i


def test_empty_tiers():
    s = M.build([], [], [], [], header=9)
    rows = M.verify(s)
    assert all(r == (0, 0, -1) for t in rows for r in t)
