"""A dense key-space model of the conflict set, independent of both oracle restatements.

A sorted universe of U distinct keys and an int64 array `ver[U]`: entry i is the version a point read
of universe key i sees.  Every endpoint a test sends is a universe key, so the model is exact:

    read  [key_a, key_b), snapshot s   conflicts iff ver[a:b].max() > s
    write [key_a, key_b) at `now`      ver[a:b] = now
    below the first boundary           ver holds the header version
    degenerate read [key_a, key_a)     looks at the segment just below key_a (the reference's fingers
                                       never diverge, SkipList.cpp:650-666): ver[a-1], the header at 0

The stored state is the run-length encoding of `ver` (clamped at the floor, as
tests/export_helpers.canon describes the canonical form).  Range maxima come from a sparse table so
that reads over a million entries stay cheap; `check_table` compares it with plain slices.

The universe is a uint8[U, klen] matrix of keys of one length or, for keys of different lengths, a
(key_bytes, key_offsets) pair sorted by memcmp and then by length (var_universe; Python's order of
bytes); everything below works on universe indices and packs keys through pack_keys in either form.

The batch-order half (TxnBatch, resolve, batch_facts, below): multi-range transactions walked in
batch order over a bool array `dirty[U]` marked by the writes of the transactions that committed
earlier in the batch, and the facts about the batch's candidate edges that key geometry alone gives.
resolve_moved re-resolves a batch with one endpoint index moved by one: what an endpoint sorted one
place off comes to (tests/sort_plan.py proves with it that a wrong endpoint order cannot pass).
"""
import copy
from types import SimpleNamespace

import numpy as np

from foundationdb_amd.packing import PackedBatch

CONFLICT, TOO_OLD, COMMITTED = 0, 1, 2
SHAPES = ("random16", "prefix20")


def make_universe(rng, n, shape):
    """uint8[n, klen]: n distinct keys in ascending order.  "random16": 16 random bytes (comparisons
    stay in the prefix words); "prefix20": a 12-byte shared prefix and an 8-byte big-endian index
    (every comparison is decided in the tail)."""
    if shape == "random16":
        raw = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
        w = raw.view(">u8")
        keys = raw[np.lexsort((w[:, 1], w[:, 0]))]
    else:
        idx = np.cumsum(rng.integers(1, 1 << 24, size=n, dtype=np.int64))
        keys = np.empty((n, 20), np.uint8)
        keys[:, :12] = np.frombuffer(b"\x15\x2asubspace\x00\x02", np.uint8)
        keys[:, 12:] = idx.astype(">u8").view(np.uint8).reshape(n, 8)
    assert (keys[1:] != keys[:-1]).any(axis=1).all()
    return np.ascontiguousarray(keys)


def var_universe(keys):
    """(key_bytes, key_offsets) of distinct keys of any lengths, sorted by memcmp and then by length
    (the reference's order of byte strings, which is Python's order of bytes): the variable-length form
    of a universe, which KeyspaceModel takes in place of a uint8[U, klen] matrix."""
    keys = sorted(set(keys))
    ko = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=ko[1:])
    return np.frombuffer(b"".join(keys), np.uint8).copy(), ko


def split_keys(kb, ko):
    """The keys of a (key_bytes, key_offsets) pair as a list of bytes."""
    raw, ko = np.asarray(kb, np.uint8).tobytes(), np.asarray(ko).tolist()
    return [raw[a:b] for a, b in zip(ko, ko[1:])]


class KeyspaceModel:
    def __init__(self, keys, header):
        """keys: uint8[U, klen], or (key_bytes, key_offsets) for keys of different lengths (klen is
        None then).  Sorted and distinct either way."""
        if isinstance(keys, tuple):
            self.kb, self.ko = np.asarray(keys[0], np.uint8), np.asarray(keys[1], np.int64)
            self.keys, self.U, self.klen = None, len(self.ko) - 1, None
            ks = split_keys(self.kb, self.ko)
            assert all(x < y for x, y in zip(ks, ks[1:]))
        else:
            self.keys = keys
            self.U, self.klen = keys.shape
        self.header = int(header)
        self.ver = np.full(self.U, header, np.int64)
        self._tab = None

    def load(self, hist_idx, vers):
        """The state after load_history of boundaries keys[hist_idx] with `vers`."""
        seg = np.searchsorted(hist_idx, np.arange(self.U), "right") - 1
        self.ver = np.where(seg >= 0, np.asarray(vers, np.int64)[np.maximum(seg, 0)], self.header)
        self._tab = None

    def write(self, a, b, now):
        for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
            self.ver[x:y] = now
        self._tab = None

    def clamp(self, floor):
        """Versions below the oldest version read as floor - 1 (nothing admitted can tell them apart)."""
        self.ver = np.where(self.ver >= floor, self.ver, floor - 1)
        self.header = self.header if self.header >= floor else floor - 1
        self._tab = None

    def _table(self):
        if self._tab is None:
            tab, w = [self.ver], 1
            while 2 * w <= self.U:
                p = tab[-1]
                tab.append(np.maximum(p[:-w], p[w:]))
                w *= 2
            self._tab = tab
        return self._tab

    def read_max(self, a, b):
        """What each read [a, b) (universe indices, a <= b) compares its snapshot with."""
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        assert (a <= b).all() and (a >= 0).all() and (b <= self.U).all()
        tab = self._table()
        out = np.empty(len(a), np.int64)
        deg = a == b
        out[deg] = np.where(a[deg] > 0, self.ver[np.maximum(a[deg] - 1, 0)], self.header)
        n = np.maximum(b - a, 1)
        lvl = np.floor(np.log2(n)).astype(np.int64)
        lvl -= (1 << lvl) > n  # guard the float log at powers of two
        for k in np.unique(lvl[~deg]).tolist():
            s = ~deg & (lvl == k)
            out[s] = np.maximum(tab[k][a[s]], tab[k][b[s] - (1 << k)])
        return out

    def check_table(self, a, b, rng, n=48):
        """The sparse table against plain slices on a sample of non-degenerate reads."""
        got = self.read_max(a, b)
        for i in rng.choice(len(a), size=min(n, len(a)), replace=False).tolist():
            if a[i] < b[i]:
                assert got[i] == self.ver[a[i]:b[i]].max()

    def boundaries(self):
        """Universe indices where the version changes (the header stands before index 0)."""
        return np.flatnonzero(self.ver != np.concatenate([[self.header], self.ver[:-1]]))

    def rle(self):
        """(header, key_bytes, key_offsets, versions): the canonical stored state."""
        s = self.boundaries()
        return (self.header, *self.pack_keys(s), self.ver[s])

    def pack_keys(self, idx):
        idx = np.asarray(idx, np.int64)
        if self.klen is None:
            ln = self.ko[idx + 1] - self.ko[idx]
            off = np.zeros(len(idx) + 1, np.int64)
            np.cumsum(ln, out=off[1:])
            return self.kb[np.repeat(self.ko[idx] - off[:-1], ln) + np.arange(off[-1])], off
        return self.keys[idx].ravel(), np.arange(len(idx) + 1, dtype=np.int64) * self.klen

    def batch(self, is_write, a, b, snap):
        """PackedBatch of one-range transactions: transaction t reads or writes [keys[a], keys[b])."""
        is_write = np.asarray(is_write, bool)
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        T = len(a)
        roff = np.zeros(T + 1, np.int32)
        woff = np.zeros(T + 1, np.int32)
        np.cumsum(~is_write, out=roff[1:])
        np.cumsum(is_write, out=woff[1:])
        ends = np.concatenate([np.stack([a[~is_write], b[~is_write]], 1).ravel(),
                               np.stack([a[is_write], b[is_write]], 1).ravel()])
        kb, ko = self.pack_keys(ends)
        return PackedBatch(np.asarray(snap, np.int64), np.zeros(T, np.uint8), roff, woff, kb, ko)


def assert_dump_equals(dump, want, what=None):
    """ConflictSet.dump_history()'s tuple against a model's rle(), exactly."""
    kb, ko, vv, hdr = dump
    whdr, wkb, wko, wvv = want
    assert hdr == whdr, (what, "header", hdr, whdr)
    if np.array_equal(vv, wvv) and np.array_equal(ko, wko) and np.array_equal(kb, wkb):
        return
    n = min(len(vv), len(wvv))
    bad = vv[:n] != wvv[:n]
    if n:  # keys of either form: a boundary is wrong if its length is, or a byte of it
        ko, wko = np.asarray(ko, np.int64), np.asarray(wko, np.int64)
        bad |= np.diff(ko[: n + 1]) != np.diff(wko[: n + 1])
        same = np.array_equal(ko[: n + 1], wko[: n + 1])
        m = int(wko[n]) if same else 0  # (after a wrong length the bytes no longer line up)
        if m:
            bad |= np.add.reduceat((kb[:m] != wkb[:m]).astype(np.int64), wko[:n].clip(max=m - 1)) * (np.diff(wko[: n + 1]) > 0) > 0
    d = int(np.argmax(bad)) if bad.any() else n
    raise AssertionError((what, "first difference at boundary", d, "of", len(vv), len(wvv),
                          vv[d:d + 3].tolist(), wvv[d:d + 3].tolist()))


def twice(model, a, b, oldest):
    """Every read sent twice: with its span's maximum m as snapshot (must commit) and with m - 1
    (must conflict).  A read whose m - 1 would be TooOld goes once, with max(m, oldest).
    Returns (a, b, snapshot, expected verdict, the share of reads sent once)."""
    m = model.read_max(a, b)
    two = m - 1 >= oldest
    aa = np.concatenate([a, a[two]])
    bb = np.concatenate([b, b[two]])
    snap = np.concatenate([np.maximum(m, oldest), m[two] - 1])
    want = np.concatenate([np.full(len(a), COMMITTED, np.uint8), np.full(int(two.sum()), CONFLICT, np.uint8)])
    return aa, bb, snap, want, 1.0 - two.mean()


# ---- the batch sequence of tests/test_gpu_rangemax_model.py, built on the CPU from the model alone

STARTS = (0, 1, 63, 64, 65, 127, 128, 4095, 4096, 4097, 262143, 262144, 262145)
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 4095, 4096, 4097, 8191, 8192, 8193, 8320,
           262143, 262144, 262145, 524289)
FIRST_BOUNDARY = 5  # universe keys below the first loaded boundary: the header's segment


def spike_positions(rng, H, n_random):
    """Ranks in the loaded history whose version stands far above its neighbours': the last and first
    entries of level-1 blocks (64k - 1, 64k), of level-2 blocks (4096k - 1, 4096k) and of the first
    level-3 block (262143, 262144), and random ranks."""
    pos = []
    for unit in (64, 4096):
        ks = np.unique(np.concatenate([[1, 2], rng.integers(1, max(2, H // unit), size=4)]))
        pos += [unit * k - 1 for k in ks.tolist()] + [unit * k for k in ks.tolist()]
    pos += [262143, 262144] + rng.integers(0, H, size=n_random).tolist()
    return np.unique([p for p in pos if 0 <= p < H])


def deep_positions(H):
    """Ranks deep inside upper-level blocks, where the single highest versions stand: the first deep
    inside the second level-3 block (a history past 150 * 4096 boundaries, so that reads over more than
    128 level-2 entries hold that block whole), the others in the middle
    of level-2 blocks (4096 boundaries), on a big history inside that level-3 block too, so that a
    read over it finds them all in level-3 entries."""
    if H > 150 * 4096:
        return np.array([262144 + 100000] + [262144 + 4096 * k + 2048 for k in (5, 40, 55)], np.int64)
    return np.array([4096 * k + 2048 for k in (2, 1, 3) if 4096 * (k + 1) < H], np.int64)


def climb_level(lo, hi, ps):
    """range_max's climb over ranks [lo, hi) replayed: the level at which it first reads an entry
    that holds one of the ranks `ps` (None: none of them lies in the span)."""
    ps = np.asarray(ps, np.int64)
    ps = ps[(ps >= lo) & (ps < hi)]
    if not len(ps):
        return None
    for L in range(4):
        if hi - lo <= 128 or L == 3:
            return L
        lo2, hi2 = (lo + 63) // 64, hi // 64
        if ((ps < lo2 * 64) | (ps >= hi2 * 64)).any():
            return L
        lo, hi, ps = lo2, hi2, ps // 64


def deep_spans(model, bnd, deep_u):
    """Reads around the deep ranks whose span reaches the block's upper-level entry, with starts and
    ends at and around block edges.  Returns the spans (universe indices) and {2: n, 3: n}: how many
    of them have every holder of their maximum inside level-2 (level-3) entries, by climb_level."""
    nb = len(bnd)
    edge = (-1, 0, 1, 63, 64, 65, 1000)
    cand = set()
    for p in np.searchsorted(bnd, deep_u).tolist():
        b2 = p // 4096
        for lo in [4096 * (b2 - k) + e for k in (1, 2) for e in edge] + [0, 1]:
            for hi in [4096 * (b2 + k) + e for k in (1, 2, 3) for e in edge]:
                cand.add((lo, hi))
        b3 = p // 262144
        for lo in [262144 * b3 - 4096 * k + e for k in (0, 1, 30, 63) for e in edge] + [0, 1, 64, 4097]:
            for hi in [262144 * (b3 + 1) + 4096 * k + e for k in (0, 1, 30, 40, 50, 64, 65) for e in edge] + [nb - 1]:
                cand.add((lo, hi))
    cand = np.array(sorted((lo, hi) for lo, hi in cand if 0 <= lo and hi <= nb - 1 and hi - lo > 8192), np.int64)
    reached = {2: 0, 3: 0}
    if not len(cand):
        return np.zeros((0, 2), np.int64), reached
    a, b = bnd[cand[:, 0]], bnd[cand[:, 1]]
    m = model.read_max(a, b)
    where = {}  # version -> the ranks that hold it
    for (lo, hi), top in zip(cand.tolist(), m.tolist()):
        if top not in where:
            where[top] = np.unique(np.searchsorted(bnd, np.flatnonzero(model.ver == top), "right") - 1)
        level = climb_level(lo, hi, where[top])
        if level in reached:
            reached[level] += 1
    return np.stack([a, b], 1), reached


def directed_spans(bnd):
    """Reads over ranks [lo, lo + len) of the boundaries `bnd` (universe indices), each beginning at
    the boundary key and once more at a non-boundary key inside the preceding segment."""
    nb, out = len(bnd), []
    for lo in STARTS:
        if lo >= nb - 1:
            continue
        for ln in LENGTHS + (nb - 1 - lo,):
            a, b = int(bnd[lo]), int(bnd[min(lo + ln, nb - 1)])
            out.append((a, b))
            if a - 1 > (int(bnd[lo - 1]) if lo else -1):
                out.append((a - 1, b))
    return np.array(out, np.int64).reshape(-1, 2)


def spike_spans(bnd, spike_u):
    """Around every spike (rank p among `bnd`), for every length: [p+1, p+1+len) and [p-len, p) leave
    the spike just outside; [p, p+len) and [p-len+1, p+1) hold it as first or last element."""
    nb = len(bnd)
    p = np.searchsorted(bnd, spike_u)[:, None]
    ln = np.array(LENGTHS, np.int64)[None, :]
    lo = np.stack([p + 1 + 0 * ln, p - ln, p + 0 * ln, p - ln + 1]).ravel()
    hi = np.stack([p + 1 + ln, p + 0 * ln, p + ln, p + 1 + 0 * ln]).ravel()
    lo, hi = np.clip(lo, 0, nb - 1), np.clip(hi, 0, nb - 1)
    keep = lo < hi
    return np.stack([bnd[lo[keep]], bnd[hi[keep]]], 1)


def other_spans(rng, U, n_random, min_len):
    """Log-uniform random spans, degenerate [k, k) reads, reads beginning in the header's segment
    and one read of the whole key space, [first key, last key): every end is a universe key, so the
    last key itself (in the last boundary's segment, like the two before it) can only be an end."""
    a = rng.integers(0, U - 1 - min_len, size=n_random)
    ln = np.exp(rng.uniform(np.log(min_len), np.log(U), size=n_random)).astype(np.int64)
    rnd = np.stack([a, np.minimum(a + ln, U - 1)], 1)
    k = np.concatenate([[0, 1, U - 1], rng.integers(0, U, size=40)])
    hdr = np.stack([rng.integers(0, FIRST_BOUNDARY, size=20), rng.integers(FIRST_BOUNDARY, U - 1, size=20)], 1)
    return np.concatenate([rnd, np.stack([k, k], 1), hdr, [[0, U - 1]]])


def build_plan(seed, shape, D, H, n_spikes, n_random, n_writes, n_wide, wide_min=8193, chunk=40000, checks=None,
               max_gap=2):
    """The sequence: a list of steps {"gc_interval": value or None, "batches": [(PackedBatch, now,
    new_oldest, expected verdicts)], "boundaries": the model's boundary count after the step, "reached":
    the step's reads decided by level 2 / level 3 entries alone, "state": (model.rle(), as_stored) or
    None}, and the loaded history (key_bytes, key_offsets, versions, header).  checks: the steps whose
    end state is kept (None: all).  Universe keys follow the boundaries at gaps of 1 to max_gap."""
    rng = np.random.default_rng(seed)
    gap = rng.integers(1, max_gap + 1, size=H)
    gap[[s for s in STARTS if s < H]] = 2  # a non-boundary key before every directed start
    gap[0] = FIRST_BOUNDARY
    hist_idx = np.cumsum(gap)
    U = int(hist_idx[-1]) + 3
    model = KeyspaceModel(make_universe(rng, U, shape), D + 1234)
    vers = D + 1000 + np.cumsum(rng.integers(1, 1000, size=H)) % 1000  # neighbours always differ
    spikes = spike_positions(rng, H, n_spikes)
    vers[spikes] = D + 10 ** 6 + rng.permutation(len(spikes))  # not monotone in position
    deep = deep_positions(H)  # (unsorted: the first is the main one)
    vers[deep] = D + 1_500_000 + np.arange(len(deep))[::-1]  # above every spike; the first the highest
    model.load(hist_idx, vers)
    assert len(model.boundaries()) == H
    loaded = (*model.pack_keys(hist_idx), vers, model.header)
    spike_u = hist_idx[spikes]
    deep_u = hist_idx[deep]

    oldest, now = D + 500, D + 2_000_000
    steps = []

    def step(n_w=0, wide=0, gc_interval=None, new_oldest=None, min_len=1, probe=False, deep_writes=False):
        nonlocal oldest, now, deep_u
        bnd = model.boundaries() if steps else hist_idx
        dspans, reached = deep_spans(model, bnd, deep_u)
        if probe and H >= 4 * 4096:  # reads whose maximum only entries of level 2 (of level 3) hold: a stale-low
            assert reached[2] >= 20 and (reached[3] >= 20 or H <= 150 * 4096), reached  # entry commits them
        spans = np.unique(np.concatenate([directed_spans(bnd), spike_spans(bnd, spike_u), dspans,
                                          other_spans(rng, U, n_random, min_len)]), axis=0)
        spans = spans[rng.permutation(len(spans))]
        model.check_table(spans[:, 0], spans[:, 1], rng)
        a, b, snap, want, once = twice(model, spans[:, 0], spans[:, 1], oldest)
        assert once <= 0.2, once
        assert (want == CONFLICT).mean() >= 0.3 and (want == COMMITTED).mean() >= 0.3
        assert (snap >= oldest).all()
        order = rng.permutation(len(a))
        a, b, snap, want = a[order], b[order], snap[order], want[order]
        wa = rng.integers(0, U - 4, size=n_w)
        wb = wa + rng.integers(1, 4, size=n_w)
        if deep_writes:  # single keys at deep ranks, far enough apart that a read around one meets no other
            # in its lower-level tails (this batch's version stands nowhere else); deep by today's ranks
            du = bnd[deep_positions(len(bnd))]
            deep_u = du = du if len(bnd) > 150 * 4096 else du[:1]
            wa, wb = np.concatenate([wa, du]), np.concatenate([wb, du + 1])
        if wide:  # a few very wide writes, each over more than `wide_min` boundaries
            width = rng.integers(wide_min, max(wide_min + 2, min(len(bnd) // 6, 3 * wide_min)), size=wide)
            lo = np.array([rng.integers(0, len(bnd) - 1 - w) for w in width])
            wa, wb = np.concatenate([wa, bnd[lo]]), np.concatenate([wb, bnd[lo + width]])
        batches = []
        cuts = list(range(0, len(a), chunk)) or [0]
        for c in cuts:
            last = c == cuts[-1]
            now += 10
            n_r = min(chunk, len(a) - c)
            w = slice(0, len(wa) if last else 0)
            pb = model.batch(np.arange(n_r + len(wa[w])) >= n_r, np.concatenate([a[c:c + n_r], wa[w]]),
                             np.concatenate([b[c:c + n_r], wb[w]]),
                             np.concatenate([snap[c:c + n_r], np.full(len(wa[w]), oldest)]))
            batches.append((pb, now, new_oldest if last and new_oldest is not None else oldest,
                            np.concatenate([want[c:c + n_r], np.full(len(wa[w]), COMMITTED, np.uint8)])))
        model.write(wa, wb, now)
        floor = None
        if new_oldest is not None:
            oldest = floor = new_oldest
            model.clamp(oldest)
        keep = checks is None or len(steps) in checks
        # as_stored: the oldest version has not moved yet, so nothing is below the floor and the stored
        # form is the canonical one (afterwards what is stored below the floor depends on when the engine
        # collected garbage, and only the default floor compares)
        steps.append({"gc_interval": gc_interval, "batches": batches, "boundaries": len(model.boundaries()),
                      "reached": reached, "state": (model.rle(), oldest == D + 500) if keep else None})

    step(probe=True)  # 0: the loaded base alone
    for _ in range(3):  # 1-3: the delta grows past 8192 boundaries at keys that were no boundaries
        step(n_w=n_writes)
    step(wide=n_wide)  # 4: long runs become one segment each: holes over the base
    step(deep_writes=True, gc_interval=1)  # 5: compaction; every position moves, the top version deep in blocks
    step(n_w=n_writes // 4, new_oldest=D + 1500, probe=True)  # 6: reads the rebuilt levels; GC coalesces the clamped
    for i in range(2):  # 7-8: a delta again over the rebuilt base
        step(n_w=n_writes // 2, gc_interval=0 if i == 0 else None, min_len=4)
    return loaded, steps


def interleaved_step(seed, model, now, oldest, n=300):
    """One batch of reads and writes in random order (one range each), the model walked in batch
    order.  A read that meets an earlier write of its own batch conflicts whatever its snapshot
    (the intra-batch check compares no versions), so it is sent with both snapshots and conflicts
    twice.  Returns (PackedBatch, expected verdicts); the model holds the batch's writes."""
    rng = np.random.default_rng(seed)
    U = model.U
    is_write, aa, bb, snap, want = [], [], [], [], []
    dirty = np.zeros(U, bool)
    for _ in range(n // 3):
        a = int(rng.integers(0, U - 2))
        b = min(U - 1, a + int(np.exp(rng.uniform(0, np.log(U)))))
        if rng.random() < 0.4:
            w = min(b, a + int(rng.integers(1, 200)))
            model.ver[a:w] = now
            dirty[a:w] = True
            is_write.append(True); aa.append(a); bb.append(w); snap.append(oldest); want.append(COMMITTED)
            continue
        m = int(model.ver[a:b].max()) if not dirty[a:b].any() else None
        for s, v in ((0, COMMITTED), (1, CONFLICT)):
            sn = (now if m is None else m) - s
            if sn < oldest:
                continue
            is_write.append(False); aa.append(a); bb.append(b); snap.append(sn)
            want.append(CONFLICT if m is None else v)
    model._tab = None
    return model.batch(is_write, aa, bb, snap), np.array(want, np.uint8)


# ---- the batch-order model: multi-range transactions walked in batch order over a dirty map of the
# universe, and the facts about a batch that follow from key geometry alone


class TxnBatch:
    """Multi-range transactions over universe indices, in batch order: per transaction its reads and
    writes ((a, b) pairs, a <= b; a == b is an empty range), its snapshot and its report flag."""

    def __init__(self):
        self.reads, self.writes, self.snap, self.report, self.tag = [], [], [], [], []

    def __len__(self):
        return len(self.snap)

    def add(self, reads=(), writes=(), snap=0, report=False, tag=None):
        self.reads.append([(int(a), int(b)) for a, b in reads])
        self.writes.append([(int(a), int(b)) for a, b in writes])
        self.snap.append(int(snap))
        self.report.append(bool(report))
        self.tag.append(tag)
        return len(self.snap) - 1

    def arrays(self):
        T = len(self)
        roff, woff = np.zeros(T + 1, np.int32), np.zeros(T + 1, np.int32)
        np.cumsum([len(x) for x in self.reads], out=roff[1:])
        np.cumsum([len(x) for x in self.writes], out=woff[1:])
        r = np.array([x for tr in self.reads for x in tr], np.int64).reshape(-1, 2)
        w = np.array([x for tr in self.writes for x in tr], np.int64).reshape(-1, 2)
        assert (r[:, 0] <= r[:, 1]).all() and (w[:, 0] <= w[:, 1]).all()
        return SimpleNamespace(T=T, roff=roff, woff=woff, ra=r[:, 0], re=r[:, 1], wa=w[:, 0], we=w[:, 1],
                               rt=np.repeat(np.arange(T), np.diff(roff)), wt=np.repeat(np.arange(T), np.diff(woff)),
                               snap=np.array(self.snap, np.int64), report=np.array(self.report, bool))

    def pack(self, model):
        A = self.arrays()
        ends = np.concatenate([np.stack([A.ra, A.re], 1).ravel(), np.stack([A.wa, A.we], 1).ravel()])
        kb, ko = model.pack_keys(ends)
        return PackedBatch(A.snap, A.report.astype(np.uint8), A.roff, A.woff, kb, ko)


def admitted_arrays(A, too_old):
    """The batch without the ranges of its TooOld transactions, which are never registered (the
    reference skips them when the transaction is added): what the sorted endpoints, the candidate
    edges and the counts R and W are made of.  Transactions keep their numbers."""
    kr, kw = ~too_old[A.rt], ~too_old[A.wt]
    roff, woff = np.zeros(A.T + 1, np.int32), np.zeros(A.T + 1, np.int32)
    np.cumsum(np.where(too_old, 0, np.diff(A.roff)), out=roff[1:])
    np.cumsum(np.where(too_old, 0, np.diff(A.woff)), out=woff[1:])
    return SimpleNamespace(T=A.T, roff=roff, woff=woff, ra=A.ra[kr], re=A.re[kr], wa=A.wa[kw], we=A.we[kw],
                           rt=A.rt[kr], wt=A.wt[kw], snap=A.snap, report=A.report)


def batch_facts(A, verdicts, dead):
    """What key geometry alone says about a batch (A: admitted_arrays()), given the verdicts:

    slots[r]      of a non-empty read [ra, re): the writes, empty ones included, that begin strictly
                  inside it plus the non-empty writes that cover its begin (wa <= ra < we); 0 for an
                  empty read.  n_slots is their sum.
    P             the candidate pairs: over every read, the write-begins strictly inside it (non-empty
                  reads) plus the non-empty writes covering its begin (every read).  P_grouped counts
                  the covering side once per write group and read-begin instead.
    cand[r]       the candidate writers of read r, as transactions in write order (None: none): earlier
                  transactions' non-empty writes that overlap the non-empty read; direct[r] says which
                  of them begin strictly inside the read (the others cover its begin).
    dead          history conflict or TooOld: decided before the rounds (a TooOld transaction has no
                  ranges here, so only a history-conflicted one can be a dead candidate writer).
    n_live[t]     t's candidate writers that are not dead, over its reads in order; walked[t]: how many
                  of them abort before the first that commits (all of them if none does); exact[t]: no
                  read of t has more than one live candidate, so that order is the only one possible.
    U             transactions that are not dead and have a live candidate.
    groups        maximal runs of writes, in (begin key, write index) order, that are non-empty and
                  contain the same non-empty set of read-begins: gorder (the order), gstart[j] (the
                  position where position j's group starts, -1: in none), giv[j] (the interval of sorted
                  read-begins position j's write contains)."""
    T, R, W = A.T, len(A.ra), len(A.wa)
    ne_r, ne_w = A.ra < A.re, A.wa < A.we
    wa_s = np.sort(A.wa)
    inside = np.where(ne_r, np.searchsorted(wa_s, A.re, "left") - np.searchsorted(wa_s, A.ra, "right"), 0)
    cover = np.searchsorted(np.sort(A.wa[ne_w]), A.ra, "right") - np.searchsorted(np.sort(A.we[ne_w]), A.ra, "right")
    slots = np.where(ne_r, inside + cover, 0)
    cand, direct = [None] * R, [None] * R
    # the non-empty writes by begin key: an overlapping one begins in (ra - longest write, re)
    by_begin = np.flatnonzero(ne_w)[np.argsort(A.wa[ne_w], kind="stable")]
    wa_n = A.wa[by_begin]
    longest = int((A.we - A.wa).max()) if W else 0
    first = np.searchsorted(wa_n, A.ra - longest, "right")
    last = np.searchsorted(wa_n, A.re, "left")
    for r in np.flatnonzero(slots > 0).tolist():
        x = np.sort(by_begin[first[r]:last[r]])
        x = x[(A.wt[x] < A.rt[r]) & (A.ra[r] < A.we[x])]
        if len(x):
            cand[r], direct[r] = A.wt[x], A.wa[x] > A.ra[r]
    n_cand, n_live = np.zeros(T, np.int64), np.zeros(T, np.int64)
    walked, exact = np.zeros(T, np.int64), np.ones(T, bool)
    for t in np.unique(A.rt[slots > 0]).tolist():
        live = []
        for r in range(A.roff[t], A.roff[t + 1]):
            if cand[r] is None:
                continue
            n_cand[t] += len(cand[r])
            lv = cand[r][~dead[cand[r]]]
            exact[t] &= len(lv) <= 1
            live.extend(lv.tolist())
        n_live[t] = len(live)
        commits = np.flatnonzero(verdicts[live] == COMMITTED) if live else np.zeros(0, np.int64)
        walked[t] = commits[0] if len(commits) else len(live)
        if not dead[t]:  # the model against itself: the dirty map and the candidate writers agree
            assert (verdicts[t] == CONFLICT) == bool(len(commits)), t
    # write groups
    gorder = np.lexsort((np.arange(W), A.wa))
    rb_s = np.sort(A.ra)
    lo = np.searchsorted(rb_s, A.wa[gorder], "left")
    hi = np.where(ne_w[gorder], np.searchsorted(rb_s, A.we[gorder], "left"), lo)
    member = hi > lo
    same = np.zeros(W, bool)
    same[1:] = member[1:] & member[:-1] & (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])
    start = np.where(member & ~same, np.arange(W), -1)
    gstart = np.where(member, np.maximum.accumulate(start), -1)
    n_groups = int((member & ~same).sum())
    P = int(inside.sum() + cover.sum())
    P_grouped = int(inside.sum() + (hi - lo)[member & ~same].sum())
    return SimpleNamespace(slots=slots, n_slots=int(slots.sum()), P=P, P_grouped=P_grouped, cand=cand, direct=direct,
                           dead=dead, n_cand=n_cand, n_live=n_live, walked=walked, exact=exact,
                           U=int((~dead & (n_live > 0)).sum()), gorder=gorder, gstart=gstart,
                           giv=np.stack([lo, hi], 1), n_groups=n_groups, rb_sorted=rb_s)


def resolve(model, tb, now, oldest, facts=True):
    """One batch against the model, walked in batch order.  TooOld iff the transaction has reads and
    snapshot < oldest; a history conflict per read from read_max; an intra-batch conflict iff a
    non-empty read [a, b) meets dirty[a:b].any(), dirty marked by the non-empty writes of the
    transactions that committed earlier in the batch (an empty read never conflicts intra-batch, a
    history-conflicted transaction is not looked at); a committed transaction's writes then stand at
    `now` in the model.  Returns verdicts, reports (an entry for every reporting, admitted
    transaction with reads: every history-conflicting read, else the first intra-batch one, else
    nothing), the arrays, and admitted_arrays with their batch_facts."""
    A = tb.arrays() if isinstance(tb, TxnBatch) else tb
    T = A.T
    has_reads = np.diff(A.roff) > 0
    too_old = has_reads & (A.snap < oldest)
    hist_read = model.read_max(A.ra, A.re) > A.snap[A.rt] if len(A.ra) else np.zeros(0, bool)
    hist = np.zeros(T, bool)
    hist[A.rt[hist_read]] = True
    hist &= ~too_old
    dead = too_old | hist
    verdicts = np.full(T, COMMITTED, np.uint8)
    verdicts[too_old], verdicts[hist] = TOO_OLD, CONFLICT
    dirty = np.zeros(model.U, bool)
    first_intra = {}
    ra, re, wa, we, roff, woff = (x.tolist() for x in (A.ra, A.re, A.wa, A.we, A.roff, A.woff))
    for t in np.flatnonzero(~dead).tolist():
        for r in range(roff[t], roff[t + 1]):
            if ra[r] < re[r] and dirty[ra[r]:re[r]].any():
                verdicts[t], first_intra[t] = CONFLICT, r - roff[t]
                break
        else:
            for w in range(woff[t], woff[t + 1]):
                dirty[wa[w]:we[w]] = True
    cw = (verdicts[A.wt] == COMMITTED) & (A.wa < A.we)
    model.write(A.wa[cw], A.we[cw], now)
    reports = {}
    for t in np.flatnonzero(A.report & has_reads & ~too_old).tolist():
        if hist[t]:
            reports[t] = [r - roff[t] for r in range(roff[t], roff[t + 1]) if hist_read[r]]
        else:
            reports[t] = [first_intra[t]] if t in first_intra else []
    adm = admitted_arrays(A, too_old)
    return SimpleNamespace(verdicts=verdicts, reports=reports, arrays=A, admitted=adm, first_intra=first_intra,
                           facts=batch_facts(adm, verdicts, dead) if facts else None)


ENDS = ("ra", "re", "wa", "we")


def outcome(model, res):
    """What a batch leaves for anyone to see: verdicts, reports and the model's versions (their
    run-length encoding is the stored state), in a form that compares with ==."""
    return res.verdicts.tobytes(), tuple(sorted((t, tuple(x)) for t, x in res.reports.items())), model.ver.tobytes()


def resolve_moved(model, tb, now, oldest, which, r, d):
    """resolve() of the batch with one endpoint index moved by d = +-1: `which` of ENDS, range r of
    that kind.  In index space this is the endpoint sorted one distinct key too late or too early,
    and, between endpoints at one key, what a class-order error does (the class order ReadEnd <
    WriteEnd < WriteBegin < ReadBegin makes a range that ends at a key lie wholly before one that
    begins there).  A range that becomes inverted counts as empty.  The model is a copy: the caller's
    stays as it is.  Returns (the copy, its resolve()), or None when the index would leave the universe."""
    A = tb.arrays() if isinstance(tb, TxnBatch) else tb
    x = getattr(A, which).copy()
    x[r] += d
    if x[r] < 0 or x[r] >= model.U:
        return None
    other = getattr(A, {"ra": "re", "re": "ra", "wa": "we", "we": "wa"}[which])
    if (which[1] == "a" and x[r] > other[r]) or (which[1] == "e" and x[r] < other[r]):
        x[r] = other[r]
    B = SimpleNamespace(**vars(A))
    setattr(B, which, x)
    m = copy.copy(model)
    m.ver, m._tab = model.ver.copy(), None
    return m, resolve(m, B, now, oldest, facts=False)
