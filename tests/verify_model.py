"""numpy restatement of fdbcs_history_verify (include/fdb_conflict_set.h has the definition) over raw
tier arrays, for every check class but DIR and EDIR.

A tier is held the way the engine stores it: per boundary the zero-padded 16-byte prefix as two
big-endian words, the length, the 8-byte unit of a long key's tail in a shared arena, and the version
(HOLE in the delta); the derived arrays (range-max levels with level 3 as eight replica words, skey8,
the sample tree) are built here from the keys and versions, by numpy reductions and strides, never by
anything of the engine.  verify() then judges the stored form, so a single mutated element (the
`override`: the stored words XOR two masks, as the device's what-if) shows in exactly the classes
that read it.  The report has the device report's fields: rows[tier][class] = (examined, violations,
first)."""
import numpy as np

HOLE = -(1 << 63)
CLASSES = ("order", "padding", "tails", "versions", "dominance", "lvl1", "lvl2", "lvl3", "skey8", "skey", "dir", "edir")
MODELLED = tuple(c for c in CLASSES if c not in ("dir", "edir"))
FAN, ARITY, L3REP, IDX_LEVELS = 64, 8, 8, 12
U64 = (1 << 64) - 1


class Tier:
    """The stored arrays of one tier."""

    def __init__(self, keys, vers, arena):
        """keys: ascending bytes; vers: int64 (HOLE allowed); arena: the bytearray the tails are appended to
        (8-byte aligned, zero padded: fdbcs_load_history's layout)."""
        n = self.n = len(keys)
        pre = np.zeros((n, 16), np.uint8)
        self.ln = np.array([len(k) for k in keys], np.uint32)
        self.tu = np.zeros(n, np.uint32)
        for i, k in enumerate(keys):
            pre[i, :min(len(k), 16)] = np.frombuffer(k[:16], np.uint8)
            if len(k) > 16:
                self.tu[i] = len(arena) // 8
                arena += k[16:] + bytes(-(len(k) - 16) % 8)
        words = pre.reshape(-1).view(">u8").astype(np.uint64).reshape(n, 2) if n else np.zeros((0, 2), np.uint64)
        self.hi, self.lo = words[:, 0].copy(), words[:, 1].copy()
        self.ver = np.array(vers, np.int64).reshape(n)
        self.lvl1, self.lvl2 = span_max(self.ver, FAN), span_max(self.ver, FAN ** 2)
        top = span_max(self.ver, FAN ** 3)
        self.lvl3 = np.full(len(top) * L3REP, HOLE, np.int64)  # replica j % 8 holds entry j's maximum
        for j, v in enumerate(top):
            self.lvl3[j * L3REP + j % L3REP] = v
        self.skey8 = (self.hi[::8].copy(), self.lo[::8].copy())
        self.skey = [(self.hi[::s].copy(), self.lo[::s].copy()) for s in skey_strides()]

    def copy(self):
        c = object.__new__(Tier)
        c.__dict__.update(self.__dict__)
        c.skey = list(self.skey)
        return c


def skey_strides():
    return [FAN * ARITY ** L for L in range(IDX_LEVELS)]


def span_max(ver, span):
    """Maximum of every `span` versions, the last span clipped."""
    n = len(ver)
    m = -(-n // span)
    pad = np.full(m * span, HOLE, np.int64)
    pad[:n] = ver
    return pad.reshape(m, span).max(axis=1) if m else np.zeros(0, np.int64)


def build(base_keys, base_vers, delta_keys=(), delta_vers=(), header=0):
    """Both tiers over one arena: (base, delta, arena words, tail_used, header)."""
    arena = bytearray()
    base = Tier(list(base_keys), base_vers, arena)
    delta = Tier(list(delta_keys), delta_vers, arena)
    return State(base, delta, np.frombuffer(bytes(arena), "<u8").astype(np.uint64), len(arena), header)


class State:
    def __init__(self, base, delta, arena, tail_used, header):
        self.tiers, self.arena, self.tail_used, self.header = [base, delta], arena, tail_used, int(header)


def xor64(a, i, m):
    a = a.copy()
    a[i] = np.uint64((int(a[i]) ^ m) & U64)
    return a


def xor_i64(a, i, m):
    a = a.copy()
    a[i] = np.array([(int(a[i]) ^ m) & U64], np.uint64).view(np.int64)[0]
    return a


def overridden(st, ov):
    """The state as the verifier reads it under override (what, tier, index, xor_lo, xor_hi, level)."""
    if ov is None:
        return st
    what, tier, index, lo, hi = ov[0], ov[1], ov[2], ov[3] & U64, (ov[4] if len(ov) > 4 else 0) & U64
    level = ov[5] if len(ov) > 5 else 0
    out = State(st.tiers[0], st.tiers[1], st.arena, st.tail_used, st.header)
    if what == "tail_word":
        out.arena = xor64(st.arena, index, lo)
        return out
    t = st.tiers[tier].copy()
    out.tiers = list(st.tiers)
    out.tiers[tier] = t
    if what == "key":
        t.hi, t.lo = xor64(t.hi, index, hi), xor64(t.lo, index, lo)
    elif what == "len_tail":
        t.ln, t.tu = t.ln.copy(), t.tu.copy()
        t.ln[index] = (int(t.ln[index]) ^ lo) & 0xFFFFFFFF
        t.tu[index] = (int(t.tu[index]) ^ hi) & 0xFFFFFFFF
    elif what == "version":
        t.ver = xor_i64(t.ver, index, lo)
    elif what in ("lvl1", "lvl2", "lvl3"):
        setattr(t, what, xor_i64(getattr(t, what), index, lo))
    elif what == "skey8":
        t.skey8 = (xor64(t.skey8[0], index, hi), xor64(t.skey8[1], index, lo))
    elif what == "skey":
        h, l = t.skey[level]
        t.skey[level] = (xor64(h, index, hi), xor64(l, index, lo))
    else:
        raise ValueError(what)
    return out


def tail_ok(st, ln, tu):
    return 8 * int(tu) + 8 * (-(-(int(ln) - 16) // 8)) <= st.tail_used


def stored_cmp(st, ta, i, tb, j, abytes):
    """The full order over two stored keys; None when a tail it needs lies outside the arena."""
    a, b = st.tiers[ta], st.tiers[tb]
    ka, kb = (int(a.hi[i]), int(a.lo[i])), (int(b.hi[j]), int(b.lo[j]))
    if ka != kb:
        return -1 if ka < kb else 1
    la, lb = int(a.ln[i]), int(b.ln[j])
    if la > 16 and lb > 16:
        if not tail_ok(st, la, a.tu[i]) or not tail_ok(st, lb, b.tu[j]):
            return None
        m = min(la, lb) - 16
        oa, ob = 8 * int(a.tu[i]), 8 * int(b.tu[j])
        x, y = abytes[oa:oa + m], abytes[ob:ob + m]
        if x != y:
            return -1 if x < y else 1
    return (la > lb) - (la < lb)


class Rows:
    def __init__(self):
        self.rows = [[[0, 0, -1] for _ in CLASSES] for _ in range(2)]

    def note(self, tier, cls, examined, bad_idx):
        """examined elements of class cls; bad_idx: the violating indices (one entry per violation)."""
        r = self.rows[tier][CLASSES.index(cls)]
        bad_idx = np.asarray(bad_idx, np.int64)
        r[0] += int(examined)
        r[1] += len(bad_idx)
        if len(bad_idx):
            r[2] = int(bad_idx.min()) if r[2] < 0 else min(r[2], int(bad_idx.min()))


def verify(st, override=None, checks=None, order_clean=False):
    """rows[tier][class] = (examined, violations, first) of the state under `override`.
    order_clean: the caller has seen verify(st) report ORDER clean, so of the pairs whose 16-byte
    prefixes tie (judged one by one) only those the override can change are judged again: the two
    around an overridden key or (len, tail), none for a version or a derived array, all for a tail word."""
    touched = None
    if order_clean and override is not None and override[0] != "tail_word":
        touched = (override[1], {override[2] - 1, override[2]} if override[0] in ("key", "len_tail") else set())
    st = overridden(st, override)
    abytes = st.arena.astype("<u8").tobytes()
    want = set(MODELLED if checks is None else checks)
    out = Rows()
    for tier, t in enumerate(st.tiers):
        n = t.n
        if n == 0:
            continue
        idx = np.arange(n, dtype=np.int64)
        ln = t.ln.astype(np.int64)
        if "padding" in want:
            ones = np.uint64(U64)
            sh = lambda k: np.right_shift(ones, (8 * np.clip(k, 0, 7)).astype(np.uint64))
            mh = np.where(ln >= 8, np.uint64(0), sh(ln))
            ml = np.where(ln >= 16, np.uint64(0), np.where(ln <= 8, ones, sh(ln - 8)))
            out.note(tier, "padding", n, idx[((t.hi & mh) != 0) | ((t.lo & ml) != 0)])
        long_ = ln > 16
        if "tails" in want:
            ok = 8 * t.tu.astype(np.int64) + 8 * (-(-(ln - 16) // 8)) <= st.tail_used
            out.note(tier, "tails", int(long_.sum()), idx[long_ & ~ok])
        if "versions" in want and tier == 0:
            out.note(tier, "versions", n, idx[t.ver == HOLE])
        if "order" in want and n > 1:
            gt = (t.hi[:-1] > t.hi[1:]) | ((t.hi[:-1] == t.hi[1:]) & (t.lo[:-1] > t.lo[1:]))
            tie = (t.hi[:-1] == t.hi[1:]) & (t.lo[:-1] == t.lo[1:])
            bad = list(np.flatnonzero(gt))
            ties = np.flatnonzero(tie)
            if touched is not None:
                ties = [i for i in sorted(touched[1]) if tier == touched[0] and 0 <= i < n - 1 and tie[i]]
            for i in ties:
                c = stored_cmp(st, tier, int(i), tier, int(i) + 1, abytes)
                if c is not None and c >= 0:
                    bad.append(int(i))
            out.note(tier, "order", n - 1, bad)
        for name, span in (("lvl1", FAN), ("lvl2", FAN ** 2)):
            if name in want:
                true = span_max(t.ver, span)
                out.note(tier, name, len(true), np.flatnonzero(getattr(t, name)[:len(true)] != true))
        if "lvl3" in want:
            true = span_max(t.ver, FAN ** 3)
            top = t.lvl3[:len(true) * L3REP].reshape(len(true), L3REP).max(axis=1)
            out.note(tier, "lvl3", len(true), np.flatnonzero(top != true))
        if "skey8" in want:
            h, l = t.skey8
            out.note(tier, "skey8", len(h), np.flatnonzero((h != t.hi[::8]) | (l != t.lo[::8])))
        if "skey" in want:
            for L, s in enumerate(skey_strides()):
                h, l = t.skey[L]
                out.note(tier, "skey", len(h), (L << 48) | np.flatnonzero((h != t.hi[::s]) | (l != t.lo[::s])))
    if "dominance" in want and st.tiers[1].n:
        base, delta = st.tiers
        ex, bad = 0, []

        def count_le(ts, tq, q):
            """Boundaries of tier ts at or below boundary q of tier tq, as the device's binary search walks."""
            lo, hi, eq = 0, st.tiers[ts].n, False
            while lo < hi:
                mid = (lo + hi) >> 1
                c = stored_cmp(st, ts, mid, tq, q, abytes)
                if c is None:
                    return None, False
                if c <= 0:
                    lo, eq = mid + 1, eq or c == 0
                else:
                    hi = mid
            return lo, eq

        for j in range(delta.n):
            v = int(delta.ver[j])
            if v == HOLE:
                continue
            p, _ = count_le(0, 1, j)
            if p is None:
                continue
            ex += 1
            if (int(base.ver[p - 1]) if p > 0 else st.header) > v:
                bad.append(j)
        for i in range(base.n):
            q, eq = count_le(1, 0, i)
            if q is None or q == 0 or eq:
                continue
            v = int(delta.ver[q - 1])
            if v == HOLE:
                continue
            ex += 1
            if int(base.ver[i]) > v:
                bad.append(q - 1)
        out.note(1, "dominance", ex, bad)
    return [[tuple(r) for r in t] for t in out.rows]


FAMILY = b"family/9_"  # the shared 9-byte prefix


def make_keys(rng, n):
    """n distinct ascending keys: the empty key, short keys of 1 to 16 bytes outside and inside a
    family behind a shared 9-byte prefix, long keys of 17, 24, 25, 40 and 113 bytes (many behind equal
    16-byte prefixes, so their order is decided by tails), and X / X\\0 pairs at both sides of 16."""
    keys = {b""} if n else set()
    long_lens = (17, 24, 25, 40, 113)
    while len(keys) < n:
        m = max(64, (n - len(keys)) * 5 // 4)  # one round of draws, sliced below
        kind, ln, dl = rng.integers(0, 100, m), rng.integers(1, 17, m), rng.integers(1, 8, m)
        ll = rng.integers(0, len(long_lens), m)
        rand = rng.integers(0, 256, (m, 16), dtype=np.uint8).tobytes()
        digits = rng.integers(48, 58, (m, 7), dtype=np.uint8).tobytes()
        few = rng.integers(48, 52, (m, 7), dtype=np.uint8).tobytes()
        tails = rng.integers(97, 100, (m, 97), dtype=np.uint8).tobytes()
        for i in range(m):
            r = int(kind[i])
            if r < 10:
                k = rand[16 * i:16 * i + int(ln[i])]
            elif r < 75:
                k = FAMILY + digits[7 * i:7 * i + int(dl[i])]
            else:
                k = FAMILY + few[7 * i:7 * i + 7] + tails[97 * i:97 * i + long_lens[int(ll[i])] - 16]
            keys.add(k)
            if r % 5 == 0:
                keys.add(k + b"\0")
    return sorted(keys)[:n]


def clean(rows):
    return not any(r[1] for t in rows for r in t)


def expected_examined(n, n_long, tier):
    """What a clean tier of n boundaries (n_long of them over 16 bytes) examines, per modelled class
    but dominance."""
    per = lambda s: -(-n // s)
    return {"order": max(n - 1, 0), "padding": n, "tails": n_long, "versions": n if tier == 0 else 0, "lvl1": per(FAN),
            "lvl2": per(FAN ** 2), "lvl3": per(FAN ** 3), "skey8": per(8),
            "skey": sum(per(s) for s in skey_strides())}
