"""The directed batches of tests/test_gpu_merge_model.py: the Y half of a batch (k_seg_prep, k_merge_copy,
the compaction, the GC and the epilogue) held to the two models, tests/keyspace_model.py for what a read
sees and tests/tier_model.py for what is stored.  Built on the CPU from the models alone; every count a
family is meant to reach is asserted here, from TierSim's facts, while the plan is built.

Universe.  About 13000 keys: a short region under \\x40 (random keys of 2..24 bytes, with pairs X, X\\0),
a long region under \\x50 (groups behind shared 16-byte prefixes: the bare prefix, 17 bytes, two tails
that differ in their last byte only, X and X\\0, and a 60-byte key) and two far 39-byte keys.  The wide
layout adds a chain of far 5-byte keys.  The short region comes first, so its indices are the same in
every layout: a gap of GAP keys that no directed boundary uses (over a thousand narrow writes fit between
two adjacent delta boundaries there), then the directed keys D(j) at every second index, so that both
neighbours of a directed boundary are keys that are never boundaries.

Layouts of k_seg_prep.  "narrow": keys of at most 24 bytes and fewer than 24576 write ranges.  "wide": the
same with a rider of 24576 one-range writes [f_i, f_i+2) over the far chain, which overlap into one union
segment above every directed key (a single far range sent 24576 times would put 49152 tied endpoints into
one bucket of the batch sort, which one workgroup then ranks quadratically: right, and seconds per
batch; one step of the segment-tile family sends exactly that).  "long": one read-only transaction on a
39-byte key in every batch.

Probes.  Every directed boundary i gets the reads [i-1, i), [i, i+1) and the degenerate read at i, each
sent twice (K.twice: at the span's maximum it commits, one below it conflicts), plus wide reads between
random directed boundaries.  The same read batch goes out twice after each write batch: the first is
decided by the previous batch's segments, the second by the merged delta and the levels the epilogue
built.  Every read batch holds at least 0.3 commits and 0.3 conflicts (asserted)."""
import bisect
from types import SimpleNamespace

import numpy as np

from foundationdb_amd.packing import PackedBatch
from tests import keyspace_model as K
from tests import tier_model as TM

HEADER, OLDEST, FIRST_NOW = 900, 100, 5000
N_SHORT, GAP0, GAP, D0 = 10600, 20, 2100, 2140
N_RIDER = 24576  # kSegWideMinW
SEG_PER = {"narrow": 63, "wide": 127, "long": 63}  # seg_per(): segments per tile of k_seg_prep
# kScanTile = kScanThreads * kScanPer (scan.h): elements per tile of k_scan<GcScan> and k_scan<CompactSumScan>;
# tests/test_tier_model_cpu.py reads this and the other restated constants out of the sources
SCAN_TILE = 1024
LAYOUTS = ("narrow", "wide", "long")
PROBE_CAP = 2500
STAT_KEYS = ("compactions", "gc_runs", "delta_sum", "base_sum", "segments_sum")
_UNIVERSES = {}


def D(j):
    """The j-th directed key of the short region (both neighbours are never boundaries)."""
    assert 0 <= j and D0 + 2 * j < N_SHORT - 4
    return D0 + 2 * j


def universe(layout):
    if layout in _UNIVERSES:
        return _UNIVERSES[layout]
    rng = np.random.default_rng(20)
    short = set()
    while len(short) < N_SHORT - 60:
        n = int(rng.integers(1, 24))
        short.add(b"\x40" + bytes(rng.integers(0, 256, size=n).astype(np.uint8)))
    for k in sorted(short)[50::170]:
        if len(short) < N_SHORT and len(k) < 24:
            short.add(k + b"\0")
    while len(short) < N_SHORT:
        short.add(b"\x40" + bytes(rng.integers(0, 256, size=9).astype(np.uint8)))
    long_ = []
    for g in range(400):
        p16 = b"\x50" + g.to_bytes(2, "big") + bytes(rng.integers(0, 256, size=13).astype(np.uint8))
        t = bytes(rng.integers(0x20, 0x7f, size=12).astype(np.uint8))
        long_ += [p16, p16 + b"\x10", p16 + t, p16 + t + b"\0", p16 + t[:-1] + bytes([t[-1] + 1]),
                  p16 + b"\x90" + bytes(rng.integers(0, 256, size=43).astype(np.uint8))]
    far_long = [b"\x70" + b"\x66" * 38, b"\x70" + b"\x67" * 38]
    chain = [b"\x60" + i.to_bytes(4, "big") for i in range(N_RIDER + 2)] if layout == "wide" else []
    kb, ko = K.var_universe(set(short) | set(long_) | set(far_long) | set(chain))
    keys = K.split_keys(kb, ko)
    u = SimpleNamespace(kb=kb, ko=ko, keys=keys, U=len(keys), n_short=N_SHORT, long0=N_SHORT, n_long=len(long_),
                        chain0=N_SHORT + len(long_), far_long=len(keys) - 2, len=np.diff(ko))
    assert sorted(short) == keys[:N_SHORT] and (u.len[:N_SHORT] <= 24).all()
    assert keys[u.far_long] == far_long[0] and (not chain or keys[u.chain0] == chain[0])
    u.pairs = [i for i in range(D0, N_SHORT - 8) if keys[i + 1] == keys[i] + b"\0"]  # X at i, X\0 at i + 1
    shapes = (u.len[:N_SHORT] <= 16).sum(), (u.len[:N_SHORT] > 16).sum(), (u.len > 24).sum()
    assert min(shapes) > 800 and len(u.pairs) >= 20, (shapes, len(u.pairs))
    _UNIVERSES[layout] = u
    return u


class Plan:
    def __init__(self, name, layout, header=HEADER, delta_limit=0, offset=0, env=None, sizes=True):
        self.name, self.layout, self.offset, self.env, self.sizes = name, layout, offset, env or {}, sizes
        self.uni = u = universe(layout)
        self.rng = np.random.default_rng(len(name) + 7)
        self.model = K.KeyspaceModel((u.kb, u.ko), header + offset)
        self.sim = TM.TierSim(header + offset, delta_limit)
        self.delta_limit, self.header0 = delta_limit, header + offset
        self.now, self.oldest = FIRST_NOW + offset, OLDEST  # (the offset moves versions, not the floor)
        self.sim.oldest = self.first_oldest = self.oldest
        self.single_rider = False
        self.rider_b = 2 if layout == "wide" else 0  # the far chain's B and E stand in the delta too
        self.steps, self.facts, self.coverage, self.loaded = [], [], {}, None
        self.directed = np.zeros(0, np.int64)
        self.cleared = []  # (step index, version): clear() before that step
        self.loaded_idx = None
        self.empty_writes = []  # keys of empty writes inside written spans (the reference's sweep splits there)

    # ------------------------------------------------------------------ state

    def load(self, idx, vers):
        idx, vers = np.asarray(idx, np.int64), np.asarray(vers, np.int64) + self.offset
        assert (np.diff(idx) > 0).all() and (vers[1:] != vers[:-1]).all() and vers.min() > self.oldest
        self.model.load(idx, vers)
        self.sim.load(idx, vers, self.model.header)
        self.loaded = (*self.model.pack_keys(idx), vers, self.model.header)
        self.loaded_idx = idx
        self.direct(idx)

    def state(self, floor):
        hdr, s, v = self.sim.canonical(self.uni.U, floor)
        return (hdr, *self.model.pack_keys(s), v)

    def direct(self, keys, keep=False):
        """The boundaries the next read batches probe: `keys` and their neighbours in the delta."""
        u = self.uni
        ks = set(int(k) for k in keys)
        dk = self.sim.dk
        for k in list(ks):
            p = bisect.bisect_left(dk, k)
            ks.update(dk[max(p - 1, 0):p + 2])
        if keep:
            ks.update(self.directed.tolist())
        ok = lambda k: 0 < k < u.n_short - 1 or (self.layout == "long" and u.long0 < k < u.long0 + u.n_long - 1)
        ks = np.array(sorted(k for k in ks if ok(k)), np.int64)
        if len(ks) > PROBE_CAP:  # both ends whole, the middle thinned
            mid = ks[400:-400]
            ks = np.concatenate([ks[:400], mid[:: len(mid) // (PROBE_CAP - 800) + 1], ks[-400:]])
        self.directed = ks

    def expect(self, f):
        return dict(history_size=f.n_base + f.n_delta, **{k: f.stats[k] for k in STAT_KEYS})

    def step(self, name, kind, pb, want, f, new_oldest, gc_interval, dump, replay, reads=None):
        """replay: (write ranges, union segments): what TierSim.batch took; reads: (a, b, snapshot)."""
        bk, bv = self.sim.folded()
        st = SimpleNamespace(name=name, kind=kind, pb=pb, now=self.now, new_oldest=new_oldest, want=want,
                             gc_interval=gc_interval, expect=self.expect(f), dump=None, replay=replay, reads=reads,
                             compacted=f.compact is not None, gc_ran=f.gc is not None,
                             gc_dropped=len(f.gc.dropped) if f.gc is not None else 0,
                             raw=(np.array(bk, np.int64), np.array(bv, np.int64)))
        # after every batch: the canonical form of what is stored is the clamped step function's
        hdr, idx, vv = self.sim.canonical(self.uni.U, self.sim.oldest)
        ver = np.where(self.model.ver >= self.sim.oldest, self.model.ver, self.sim.oldest - 1)
        want_hdr = self.model.header if self.model.header >= self.sim.oldest else self.sim.oldest - 1
        want_idx = np.flatnonzero(ver != np.concatenate([[want_hdr], ver[:-1]]))
        assert hdr == want_hdr and np.array_equal(idx, want_idx) and np.array_equal(vv, ver[want_idx]), (self.name, name)
        if dump or st.compacted or st.gc_ran:
            st.dump = ((hdr, *self.model.pack_keys(idx), vv), self.state(None))
        self.steps.append(st)
        self.facts.append((name, f))
        return f

    # ------------------------------------------------------------------ batches

    def write(self, name, segs, aborted=(), too_old=(), multi=(), new_oldest=None, gc_interval=None, probe=None):
        """One write batch: `segs` one-range writers that commit, `multi` writers of several ranges
        that commit, `aborted` / `too_old`: (read key, [write ranges]) writers whose read conflicts with
        the history (snapshot one below what it sees) or is too old.  Their writes must leave no trace."""
        m, u = self.model, self.uni
        if gc_interval is not None:
            self.sim.gc_interval = gc_interval
        txns = [((), [s], self.now, K.COMMITTED) for s in segs] + [((), list(ws), self.now, K.COMMITTED) for ws in multi]
        for r, ws in aborted:
            top = int(m.read_max([r], [r + 1])[0])
            if top - 1 < self.oldest:  # (nothing to conflict with: one below would be too old)
                too_old = list(too_old) + [(r, ws)]
            else:
                txns.append(([(r, r + 1)], list(ws), top - 1, K.CONFLICT))
        for r, ws in too_old:
            txns.append(([(r, r + 1)], list(ws), self.oldest - 1, K.TOO_OLD))
        if self.layout == "long":
            f = u.far_long
            txns.append(([(f, f + 1)], [], max(int(m.read_max([f], [f + 1])[0]), self.oldest), K.COMMITTED))
        tb = K.TxnBatch()
        order = self.rng.permutation(len(txns)).tolist()
        for i in order:
            tb.add(reads=txns[i][0], writes=txns[i][1], snap=txns[i][2])
        want = np.array([txns[i][3] for i in order], np.uint8)  # by construction (the CPU test resolves them too)
        A, pb = tb.arrays(), tb.pack(m)
        n_ranges = len(A.wa)
        if self.layout == "wide":
            pb, want, n_ranges = self.add_rider(pb, want), np.append(want, np.full(N_RIDER, K.COMMITTED, np.uint8)), n_ranges + N_RIDER
        committed = [w for ws, v in zip(tb.writes, want.tolist()) if v == K.COMMITTED for w in ws] + self.far_seg
        usegs = TM.union_segments(committed)
        self.now += 10
        no = self.oldest if new_oldest is None else new_oldest
        assert (n_ranges >= N_RIDER) == (self.layout == "wide")
        f = self.sim.batch(n_ranges, usegs, self.now, no)
        ne = [(a, b) for a, b in committed if a < b]
        m.write([a for a, _ in ne], [b for _, b in ne], self.now)
        self.oldest = self.sim.oldest
        own = [s for s in f.merge.segs if s.E <= u.long0 + u.n_long]
        self.direct([x for s in (own if probe is None else []) for x in (s.B, s.E)] + list(probe or ()))
        return self.step(name, "write", pb, want, f, no, gc_interval, False, (n_ranges, usegs))

    def add_rider(self, pb, want):
        """The batch with the rider's 24576 one-range writers appended: [f_i, f_i+2) over the far chain (the
        sweep of union_segments makes one segment of them: far_seg), or one far range 24576 times."""
        u = self.uni
        i = np.zeros(N_RIDER, np.int64) if self.single_rider else np.arange(N_RIDER)
        kb, ko = self.model.pack_keys(np.stack([u.chain0 + i, u.chain0 + i + 2], 1).ravel())
        return PackedBatch(np.concatenate([pb.read_snapshot, np.full(N_RIDER, self.now, np.int64)]),
                           np.concatenate([pb.report, np.zeros(N_RIDER, np.uint8)]),
                           np.concatenate([pb.read_offsets, np.full(N_RIDER, pb.read_offsets[-1], np.int32)]),
                           np.concatenate([pb.write_offsets, pb.write_offsets[-1] + np.arange(1, N_RIDER + 1, dtype=np.int32)]),
                           np.concatenate([pb.key_bytes, kb]), np.concatenate([pb.key_offsets, pb.key_offsets[-1] + ko[1:]]))

    @property
    def far_seg(self):
        u = self.uni
        if self.layout != "wide":
            return []
        return [(u.chain0, u.chain0 + 2)] if self.single_rider else [(u.chain0, u.chain0 + N_RIDER + 1)]

    def spans(self):
        ks = self.directed
        assert len(ks) >= 2, self.name
        sp = np.concatenate([np.stack([ks - 1, ks], 1), np.stack([ks, ks + 1], 1), np.stack([ks, ks], 1)])
        i = np.sort(self.rng.integers(0, len(ks), size=(24, 2)), axis=1)
        wide = np.stack([ks[i[:, 0]], ks[i[:, 1]]], 1)
        return np.unique(np.concatenate([sp, wide, [[ks[0] - 1, ks[-1] + 1]]]), axis=0)

    def reads(self, name, new_oldest=None, gc_interval=None, dump=False):
        m, u = self.model, self.uni
        if gc_interval is not None:
            self.sim.gc_interval = gc_interval
        sp = self.spans()
        sp = sp[self.rng.permutation(len(sp))]
        a, b, snap, want, _ = K.twice(m, sp[:, 0], sp[:, 1], self.oldest)
        shares = (want == K.CONFLICT).mean(), (want == K.COMMITTED).mean()
        assert min(shares) >= 0.3, (self.name, name, shares)
        if self.layout == "long":
            f = u.far_long
            a, b = np.append(a, f), np.append(b, f + 1)
            snap = np.append(snap, max(int(m.read_max([f], [f + 1])[0]), self.oldest))
            want = np.append(want, K.COMMITTED).astype(np.uint8)
        assert len(a) <= 45000 and (snap >= self.oldest).all()
        self.now += 10
        no = self.oldest if new_oldest is None else new_oldest
        f = self.sim.batch(0, [], self.now, no)
        self.oldest = self.sim.oldest
        return self.step(name, "read", m.batch(np.zeros(len(a), bool), a, b, snap), want, f, no, gc_interval, dump,
                         (0, []), (a, b, snap))

    def read_twice(self, name):
        """The same probes twice: decided by the previous batch's segments, then by the merged delta."""
        self.reads(name + "-prev")
        return self.reads(name + "-delta", dump=True)

    def compact(self, name, new_oldest=None):
        """A forced compaction: a read batch under gc_interval 1, then the cadence off again and the same
        reads against the rebuilt base."""
        f = self.reads(name + "-compact", new_oldest=new_oldest, gc_interval=1)
        assert f.compact is not None
        self.sim.gc_interval = 0
        self.reads(name + "-compacted", gc_interval=0, dump=True)
        return f

    def imported(self, name, idx, vers):
        """merge_history(into="delta") of boundaries above every version the set holds, with the set's own
        header: the delta (empty before) then holds exactly these boundaries, each with its version, the
        last one too, which no batch can leave (the highest end always inherits a hole).  No batch:
        no counter moves."""
        idx, vers = [int(i) for i in idx], [int(v) + self.offset for v in vers]
        m, sim = self.model, self.sim
        assert not sim.dk and vers == sorted(vers) and len(set(vers)) == len(vers) and vers[0] > m.ver.max()
        assert not sim.bk or idx[0] < sim.bk[0]  # (below it nothing but the header, which the import repeats)
        for i, v in zip(idx, vers):
            m.ver[i:] = v
        m._tab = None
        sim.dk, sim.dv = list(idx), list(vers)
        f = SimpleNamespace(n_base=sim.n_base, n_delta=sim.n_delta, stats=dict(sim.stats), compact=None, gc=None,
                            merge=SimpleNamespace(U=0))
        self.direct(idx + sim.bk[:20] + sim.bk[-20:])
        self.step(name, "import", None, None, f, self.oldest, None, False, None)
        self.steps[-1].arrays = (*m.pack_keys(np.array(idx, np.int64)), np.array(vers, np.int64), m.header)

    def clear(self, version):
        self.cleared.append((len(self.steps), version))
        self.sim.clear(version)
        self.model.header = version
        self.model.ver[:] = version
        self.model._tab = None
        self.direct([D(1), D(2)])



def singles(j0, n):
    """n non-touching segments [D(j), D(j + 1)) from j0 on, two directed keys each."""
    return [(D(j0 + 2 * k), D(j0 + 2 * k + 1)) for k in range(n)]


def chain(j0, n):
    """n touching segments [D(j0), D(j0 + 1)) | [D(j0 + 1), D(j0 + 2)) | ..: they stay n segments."""
    return [(D(j0 + k), D(j0 + k + 1)) for k in range(n)]


def exactly(j0, n):
    """Segments from D(j0) on that leave exactly n new boundaries in a tier that has none there: singles
    (B and E: two each) and, for an odd n, one chain of two (three)."""
    assert n >= 2
    if n % 2 == 0:
        return singles(j0, n // 2)
    return chain(j0, 2) + singles(j0 + 4, (n - 3) // 2)


def gap_exactly(nd):
    """Narrow writes inside the gap, which no directed boundary lies in, that leave exactly nd delta
    boundaries there."""
    assert 2 <= nd and nd + 6 <= GAP
    if nd % 2 == 0:
        return [(GAP0 + 2 * i, GAP0 + 2 * i + 1) for i in range(nd // 2)]
    return [(GAP0, GAP0 + 1), (GAP0 + 1, GAP0 + 2)] + [(GAP0 + 4 + 2 * i, GAP0 + 5 + 2 * i) for i in range((nd - 3) // 2)]


def short_delta(p):
    """The delta's boundaries inside the short region (the wide layout's far chain stands above them)."""
    return [k for k in p.sim.dk if k < p.uni.n_short]


# ---------------------------------------------------------------------------------- families


def segment_tiles(layout, offset=0, p=None):
    """U = 0 (every writer aborts or is TooOld), 1, and around one, two and three tiles of k_seg_prep, on
    both tiers empty at first; each batch's segments begin one directed key after the last batch's, so
    every E after the first batch is an exact hit.  Ends with a compaction into the empty base."""
    p = p or Plan("segment-tiles", layout, offset=offset)
    sp, rider = SEG_PER[layout], 1 if layout == "wide" else 0
    sizes = (0, 1, sp - 1, sp, sp + 1, 2 * sp - 1, 2 * sp, 2 * sp + 1, 3 * sp)
    if layout == "wide":
        sizes = (sp - 1, sp, sp + 1, 2 * sp - 1, 2 * sp, 2 * sp + 1)
    if sizes[0] == 0 and p.model.header - 1 < p.oldest:  # (after clear(0) no read of an unwritten key can conflict)
        sizes = sizes[1:]
    first = len(p.facts)
    for i, U in enumerate(sizes):
        if U == 0:
            f = p.write("U=0", [], aborted=[(D(3), [(D(5), D(6))])], too_old=[(D(4), [(D(8), D(9)), (D(20), D(21))])],
                        probe=[D(3), D(5), D(8)])
            assert f.n_delta == 0
        else:
            f = p.write(f"U={U}", singles(10 + i, U - rider), aborted=[(D(1), [(D(2), D(700))])] if i % 2 else ())
        assert f.merge.U == U, (U, f.merge.U)
        if U == sizes[0] + (sizes[0] == 0) or (layout == "wide" and i == 0):  # both tiers empty: nothing to inherit
            assert all(s.hi == 0 and s.vend is TM.HOLE for s in f.merge.segs) and f.merge.n_before == 0 and p.sim.n_base == 0
        p.read_twice(f"U={U}")
    ms = [f.merge for _, f in p.facts[first:] if f.merge.U]
    us = [m.U for m in ms]
    assert set(sizes) - {0} <= set(us) and any(x % sp == 0 for x in us) and any(x % sp == 1 for x in us)
    f = p.compact("into-empty-base")
    assert f.compact.n_before == 0 and f.compact.nd > 0 and f.compact.last_is_hole
    p.coverage["segment-tiles"] = dict(U=sorted(set(us) | ({0} & set(sizes))), exact=sum(s.exact for m in ms for s in m.segs))
    assert p.coverage["segment-tiles"]["exact"] > sp
    return p


def single_rider():
    """The wide layout's rider as one far range sent 24576 times: 49152 tied endpoints in one batch."""
    p = Plan("single-rider", "wide")
    p.single_rider = True
    f = p.write("U=127", singles(10, 126))
    assert f.merge.U == 127 and f.n_delta == 2 * 126 + 2
    p.read_twice("U=127")
    return p


def glue_and_exact(layout, p=None):
    """Chains of 2, 3 and 64 touching segments (the long one across a segment-tile edge), near-glue by
    length alone, an empty write inside a written span, ends that hit a delta boundary, a base boundary
    the delta lacks, the inside of an older span, and nothing at all below the first boundary."""
    sp = SEG_PER[layout]
    if p is None:
        p = Plan("glue-exact", layout)
        p.load([D(j) for j in range(600, 700)], 1200 + (np.arange(100) * 37) % 500 + np.arange(100) % 2)
    else:  # on a set in use: the base boundaries D(600) .. D(699) by writes and a compaction
        p.write("seed-base", singles(600, 50))
        p.read_twice("seed-base")
        p.compact("seed-base")
        assert all(D(j) in p.sim.bk for j in range(600, 700))
    u = p.uni
    segs = singles(10, 3) + chain(20, 2) + chain(30, 3)
    segs += singles(40, sp - 40 - len(segs))  # the 64-chain's segments then number sp - 40 .. sp + 23
    first_chain = len(segs)
    segs += chain(300, 64)
    pairs = [x for x in u.pairs if D(400) < x < D(590)][:6]
    assert len(pairs) >= 3
    for x in pairs:  # [.., X) | [X\0, ..): one key apart, so E = X is stored
        segs += [(x - 2, x), (x + 1, x + 3)]
    segs += [(D(598), D(600)), (D(610) + 1, D(612))]  # E at a base boundary the delta lacks
    segs += [(D(800), D(840))]  # an older span for the next batch's ends to fall into
    f = p.write("chains", sorted(segs), multi=[[(D(900), D(910)), (D(905), D(905))]])  # the empty write splits nothing
    p.empty_writes.append(D(905))
    ms, chains_now = f.merge.segs, p.now
    runs, n = [], 0
    for s in ms:
        n += 1
        if not s.glue:
            runs.append(n)
            n = 0
    assert sorted(r for r in runs if r > 1) == [2, 3, 64], runs
    assert ms[sp - 1].glue and ms[sp - 2].glue and first_chain <= sp - 2 and not ms[first_chain - 1].glue
    near = [s for s, t in zip(ms, ms[1:]) if t.B == s.E + 1]
    assert len(near) >= 3 and all(s.endins for s in near)
    assert sum(1 for s in ms if s.B == D(900) and s.E == D(910)) == 1
    assert ms[0].hi == 0 and ms[0].vend is TM.HOLE
    p.read_twice("chains")
    d = p.sim.dk
    seg2 = [(D(2), D(4)),  # below the first delta boundary: hi == 0 in a delta that is not empty
            (D(9), D(10)),  # E = a B of the last batch
            (D(12), D(13)), (D(15) - 1, D(15)),  # E = a hole of the last batch
            (D(805), D(810)), (D(820), D(839)),  # inside the older span: E inherits its version
            (D(640) - 1, D(642))]  # over base boundaries, E at one of them
    f = p.write("ends", sorted(seg2))
    by = {(s.B, s.E): s for s in f.merge.segs}
    assert by[D(2), D(4)].hi == 0 and by[D(2), D(4)].endins and f.merge.n_before > 0
    assert by[D(9), D(10)].exact and by[D(15) - 1, D(15)].exact and by[D(12), D(13)].exact
    assert d[bisect.bisect_left(d, D(15))] == D(15) and by[D(15) - 1, D(15)].vend is not TM.HOLE
    assert by[D(805), D(810)].endins and by[D(805), D(810)].vend == chains_now == by[D(820), D(839)].vend
    p.read_twice("ends")
    f = p.compact("holes")
    holes_exact = sum(h.exact for h in f.compact.holes)
    assert holes_exact >= 3 and any(h.lo == 0 for h in f.compact.holes) and f.compact.last_is_hole
    p.coverage["glue-exact"] = dict(chains=[2, 3, 64], near_glue=len(near), exact=sum(s.exact for s in by.values()),
                                    holes_over_base=holes_exact, holes=len(f.compact.holes))
    return p


def tails(p=None):
    """Segments over the long region: B long with E short, B short with E long, both long, and E long
    but exact or glued (no tail consumed); kept and removed long boundaries.  The dumps prove the bytes."""
    p = p or Plan("tails", "long")
    u = p.uni
    ln = u.len
    g = lambda i, k: u.long0 + 6 * i + k  # group i: 16, 17, 28, 29 (X\0), 28 (last byte + 1), 60 bytes
    assert [int(ln[g(3, k)]) for k in range(6)] == [16, 17, 28, 29, 28, 60]
    assert u.keys[g(3, 3)] == u.keys[g(3, 2)] + b"\0" and u.keys[g(3, 4)][:-1] == u.keys[g(3, 2)][:-1]
    segs = []
    for i in range(10, 40, 3):
        segs += [(g(i, 2), g(i + 1, 0)),  # long B, short E
                 (g(i + 1, 1), g(i + 1, 5)),  # short B, long E (60 bytes)
                 (g(i + 2, 2), g(i + 2, 3)), (g(i + 2, 4), g(i + 2, 5))]  # [.., X\0) | [X', ..): both long, E stored
    segs += [(g(50, 2), g(50, 4)), (g(50, 4), g(51, 2)), (g(51, 2), g(51, 5))]  # long E glued twice
    f = p.write("tails", sorted(segs))
    ms = f.merge.segs
    kinds = {(int(ln[s.B]) > 24, int(ln[s.E]) > 24, s.endins) for s in ms if s.B >= u.long0}
    assert {(True, False, True), (False, True, True), (True, True, True), (True, True, False)} <= kinds
    assert any(t.B == s.E + 1 and s.endins for s, t in zip(ms, ms[1:]))  # ends one key before the next begin
    p.read_twice("tails")
    f = p.write("tails-exact", [(g(i, 1), g(i, 5)) for i in range(12, 40, 3)] + [(g(45, 3), g(50, 2))])
    assert sum(s.exact and ln[s.E] > 24 for s in f.merge.segs) >= 9
    p.read_twice("tails-exact")
    p.compact("tails")
    p.coverage["tails"] = dict(kinds=len(kinds))
    return p


def delta_tiles(layout, p=None):
    """The copy tiles of k_merge_copy<BatchIns, 256>: delta sizes 0, 255 .. 257 and 511 .. 513 before a
    merge, segments with lo at 255 | 256 | 257 and at n, a span over two whole tiles, five tiles that no
    segment begins in, and 1 .. 9 segments in one tile."""
    p = p or Plan("delta-tiles", layout)
    seen_n, seen_lo = set(), set()
    for n in (255, 256, 257, 511, 512, 513):
        f = p.write(f"fill-{n}", exactly(10, n - p.rider_b))
        assert f.merge.n_before == 0 and f.n_delta == n
        d = short_delta(p)
        segs = [(d[q] - 1, d[q]) for q in (255, 256, 257) if q < len(d)] + [(d[-1] + 3, d[-1] + 5)]
        f = p.write(f"probe-{n}", segs)
        seen_n.add(f.merge.n_before)
        seen_lo.update(s.lo for s in f.merge.segs)
        assert f.merge.n_before == n and any(s.lo == n - p.rider_b for s in f.merge.segs)  # past the short region's last
        p.read_twice(f"probe-{n}")
        p.compact(f"after-{n}")
    assert {255, 256, 257} <= seen_lo and seen_n == {255, 256, 257, 511, 512, 513}
    assert layout == "wide" or {511, 512, 513} <= seen_lo  # lo == n: the segment owns position n alone
    # ---- 3300 boundaries: a span over tiles 1 and 2, tiles 4 .. 8 without a segment, cnt = 1 .. 9
    p.write("fill-3300", exactly(10, 3300))
    d = short_delta(p)
    f = p.write("span", [(d[100], d[901]), (d[1000] - 1, d[1000]), (d[2350] - 1, d[2350])])
    cnt = f.merge.cnt.tolist()
    assert f.merge.segs[0].lo == 100 and f.merge.segs[0].hi == 901 and cnt[1] == cnt[2] == 0
    assert cnt[3] == 1 and cnt[9] >= 1 and not any(cnt[4:9])
    p.read_twice("span")
    d = short_delta(p)
    assert len(d) > 8 * 256
    want = (1, 2, 3, 4, 5, 7, 8, 9)
    f = p.write("counts", [(d[256 * t + 2 * i + 1] - 1, d[256 * t + 2 * i + 1]) for t, c in enumerate(want) for i in range(c)])
    assert tuple(f.merge.cnt[:8].tolist()) == want
    p.read_twice("counts")
    p.compact("end")
    p.coverage["delta-tiles"] = dict(sizes=sorted(seen_n), lo=sorted(seen_lo & {255, 256, 257}), cnt=list(want))
    return p


def big_counts(layout):
    """511 .. 513 and 1023 .. 1026 segments in one copy tile (kSegLds = 1024: the lifting's top step and
    the binary-search fallback), two ways: a batch right after a compaction (one tile owns every
    segment) and narrow writes between two adjacent boundaries of a delta of 302."""
    p = Plan("big-counts", layout)
    rider = 1 if layout == "wide" else 0
    counts = (511, 512, 513, 1023, 1024, 1025, 1026)
    reached = {0: [], 1: []}
    for way in (0, 1):
        for c in counts:
            if way:
                p.write(f"bracket-{c}", [(GAP0 - 10, GAP0 - 8)] + singles(10, 150))
            f = p.write(f"count-{c}-{way}", gap_exactly(2 * (c if way else c - rider)))
            assert f.merge.cnt[0] == c and (f.merge.n_before == 0) == (way == 0), (c, way, f.merge.cnt[:3])
            assert way == 0 or f.merge.segs[0].lo == f.merge.segs[c - 1].lo == 2
            reached[way].append(int(f.merge.cnt[0]))
            p.read_twice(f"count-{c}-{way}")
            p.compact(f"count-{c}-{way}")
    assert reached[0] == list(counts) and reached[1] == list(counts)
    p.coverage["big-counts"] = dict(cnt=reached)
    return p


def compaction(layout, header=HEADER):
    """k_compact_search, k_scan<CompactSumScan> and k_merge_copy<CompactIns, 1024>: bases of 1023 .. 1025 and
    2049 boundaries, delta boundaries at base positions 1023 | 1024 and n, 1023 .. 1025 delta boundaries
    with their lo in base tile 0 (1025: the fallback), a span over two whole base tiles, holes below the
    first base boundary (they take the header), holes over base boundaries, an empty delta."""
    plans = []
    for n in (1023, 1024, 1025, 2049):
        p = Plan(f"compaction-{n}", layout, header=header)
        p.load([D(j) for j in range(n)], 1500 + (np.arange(n) * 53) % 700 + np.arange(n) % 2)
        target = min(n, 1025)

        def segs_for(nd):
            segs = gap_exactly(nd) + [(D(n - 1) + 3, D(n - 1) + 5)]
            if n == 2049:
                return segs + [(D(0) - 1, D(2048))]  # takes base tiles 0 and 1 whole
            return segs + [(D(1023) - 1, D(1023))] * (n > 1023) + [(D(1024) - 1, D(1024))] * (n > 1024)

        t = p.sim.copy()  # what else has its lo in base tile 0: a dry run with ten boundaries in the gap
        t.merge(sorted(segs_for(10) + p.far_seg), 1)
        nd = target - (int(t.compact().cnt[0]) - 10)
        p.write("delta", sorted(segs_for(nd)))
        p.read_twice("delta")
        c = p.compact("fold").compact
        assert c.n_before == n and c.cnt[0] == target and max(c.lo) == n and c.last_is_hole
        assert c.most_between >= nd  # (over 1024 of them between two base boundaries)
        assert sum(h.lo == 0 and h.val == p.model.header for h in c.holes) >= nd // 2
        if 1023 < n < 2049:
            assert 1023 in c.lo and (n == 1024 or 1024 in c.lo) and sum(h.exact for h in c.holes) >= 1
        if n == 2049:
            assert c.n_after < 1200
        f = p.reads("empty-delta", gc_interval=1)  # a compaction of nothing
        assert f.compact is not None and f.compact.nd == 0
        p.sim.gc_interval = 0
        p.reads("after-empty", gc_interval=0, dump=True)
        p.coverage["compaction"] = dict(base=n, delta=c.nd, in_tile0=int(c.cnt[0]), holes=len(c.holes),
                                        header=p.model.header)
        plans.append(p)
    return plans


def gc_family(layout, env=None):
    """k_scan<GcScan> over a base of three scan tiles (SCAN_TILE = kScanTile): boundaries dropped and kept
    on both sides of 1023 | 1024 and 2047 | 2048, tile 2 dropped whole, the first boundary dropped (under
    a header below the floor) and the last; then everything dropped and a merge into the empty set.
    Layout "long": long boundaries, kept and dropped, above them, so that every kept tail moves."""
    p = Plan("gc", layout, env=env, sizes=not env)
    n, T = 3 * SCAN_TILE + 40, SCAN_TILE
    low = np.zeros(n, bool)
    low[[0, 1]] = True  # boundary 0 goes only because the header is below the floor too
    low[T - 4:T + 1] = True  # T - 3 .. T dropped, T + 1 kept
    low[2 * T - 2:3 * T] = True  # 2T - 1 dropped, tile 2 whole
    low[n - 2:] = True
    idx = [D(j) for j in range(n)]
    vers = np.where(low, 1000 + (np.arange(n) * 7) % 600 + np.arange(n) % 2, 2500 + (np.arange(n) * 11) % 400 + np.arange(n) % 2)
    if layout == "long":
        u = p.uni
        li = np.arange(u.long0 + 1, u.long0 + 1500, 2)
        j = np.arange(len(li))
        lv = np.where((j // 3) % 2 == 0, 1100 + j % 300, 2600 + j % 200)
        idx, vers, low = idx + li.tolist(), np.concatenate([vers, lv]), np.concatenate([low, lv < 2000])
        assert (u.len[li] > 24).sum() > 300
    p.load(idx, vers)
    p.reads("base")
    f = p.reads("gc", new_oldest=2000, gc_interval=1)
    p.sim.gc_interval = 0
    g = f.gc
    dropped = set(g.dropped)
    assert {0, 1, T - 1, T, 2 * T - 1, n - 1} <= dropped and not {T - 4, T + 1, 3 * T, 2 * T - 2} & dropped
    assert set(range(2 * T, 3 * T)) <= dropped
    assert g.n_after == len(idx) - len(dropped) and len(dropped) == int((low[1:] & low[:-1]).sum()) + 1
    p.reads("after-gc", gc_interval=0, dump=True)
    p.write("merge-after-gc", singles(5, 40) + [(D(3 * T - 30), D(3 * T + 5))])
    p.read_twice("merge-after-gc")
    # ---- everything dropped: a read-only batch moves the floor past every version, then a merge into
    # the empty set
    p.compact("fold")
    top = int(p.model.ver.max())
    f = p.reads("drop-all", new_oldest=top + 5, gc_interval=1)
    p.sim.gc_interval = 0
    assert f.gc is not None and f.gc.n_after == 0 and p.sim.history_size() == 0
    p.now = max(p.now, top + 100)
    f = p.write("into-nothing", singles(20, 300) + chain(1000, 5), gc_interval=0)
    assert f.merge.n_before == 0 and p.sim.n_base == 0
    p.read_twice("into-nothing")
    p.compact("end")
    p.coverage["gc"] = dict(base=len(idx), dropped=len(dropped))
    return p


EPI_SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
TOP = 4150  # the wide span of the epilogue family ends at D(TOP)


def epilogue(layout, tier, sizes=EPI_SIZES):
    """The changed tier's size after a batch around 64, 256, 1024 (kEpiSpan) and 4096 (one level-2 word):
    tier "delta" (k_epilogue<false>), "base" (after a compaction) or "gc" (after a compaction with a GC).
    An old write and a wide one cover everything, singles inside bring the tier to the size less two, and a
    last narrow write near the top carries the tier's highest version in its last, partial block."""
    p = Plan(f"epilogue-{tier}", layout)
    far = p.far_seg
    reached = []
    for n in sizes:
        for m in range(n, n - 9, -1):  # the fill that brings the tier to n: a dry run on a copy
            t = p.sim.copy()
            t.batch(1, [(D(0), D(10))] + far, p.now + 10, t.oldest)
            t.batch(1, [(D(10), D(TOP))] + far, p.now + 15, t.oldest)
            t.batch(1, exactly(12, m) + far, p.now + 20, t.oldest)
            t.batch(1, [(D(TOP - 20), D(TOP - 19))] + far, p.now + 30, t.oldest)
            if tier != "delta":
                t.gc_interval = 1
                t.batch(0, [], p.now + 70, p.now + 11 if tier == "gc" else t.oldest)
            if (t.n_delta if tier == "delta" else t.n_base) == n:
                break
        else:
            raise AssertionError(("no fill reaches", n))
        p.write(f"old-{n}", [(D(0), D(10))])  # the one version the GC's floor passes: boundary 0 goes
        w_now = p.now
        p.write(f"wide-{n}", [(D(10), D(TOP))])
        p.write(f"fill-{n}", exactly(12, m))
        f = p.write(f"top-{n}", [(D(TOP - 20), D(TOP - 19))])
        p.direct(short_delta(p))
        if tier == "delta":
            assert f.n_delta == n, (n, f.n_delta)
            p.read_twice(f"size-{n}")
        else:
            f = p.compact(f"size-{n}", new_oldest=w_now + 1 if tier == "gc" else None)
            assert f.n_base == n and (tier != "gc" or 0 in f.gc.dropped), (n, f.n_base)
        reached.append(n)
    if tier == "delta":  # one wide write shrinks the 4097-boundary delta, reads over what lay beyond it
        assert p.sim.n_delta == sizes[-1]
        f = p.write("shrink", [(D(30), D(TOP))], probe=[D(30), D(TOP), D(40), D(2000), D(TOP - 20), D(7), D(9)])
        assert f.n_delta < 70
        p.read_twice("shrink")
    f = p.reads("empty", gc_interval=1)  # size 0: the delta after a compaction
    p.sim.gc_interval = 0
    assert f.n_delta == 0
    p.reads("after", gc_interval=0, dump=True)
    p.coverage[f"epilogue-{tier}"] = dict(sizes=reached)
    return p


def clear_and_reuse(layout="narrow"):
    """The segment-tile family with every version offset by 10^14 + 7, then clear(0) and, at small
    versions, the segment-tile, glue-and-exact, (long layout) tail and copy-tile families again, the base
    boundaries of the second seeded by writes: what they leave must be a fresh set's
    (stale-high level entries, directory epochs).  The floor stays at OLDEST throughout."""
    p = segment_tiles(layout, offset=10 ** 14 + 7)
    p.name = "clear-reuse"
    p.clear(0)
    p.now = FIRST_NOW
    segment_tiles(layout, p=p)
    glue_and_exact(layout, p=p)
    if layout == "long":
        tails(p=p)
    delta_tiles(layout, p=p)
    return p


def import_family(layout):
    """What no batch leaves in the delta, through merge_history(into="delta"): a delta of one boundary before
    a merge, and a last delta boundary that carries a version at a compaction (CompactSumScan's hi_of
    takes the base's size there: every base boundary above it goes)."""
    p = Plan("import", layout)
    p.load([D(j) for j in range(60, 100)], 1000 + (np.arange(40) * 13) % 100 + np.arange(40) % 2)
    p.reads("base")
    p.imported("import-1", [D(50)], [1200])
    p.reads("imported")
    c = p.compact("fold").compact  # one delta boundary, with a version, below the whole base
    assert c.nd == 1 and not c.last_is_hole and c.n_before == 40 and c.n_after == 1 and c.lo == [0]
    p.imported("import-1b", [D(40)], [p.now + 1])
    p.now += 10
    f = p.write("below", [(D(20), D(21))])
    assert f.merge.n_before == 1 and f.merge.segs[0].lo == 0 and f.merge.segs[0].hi == 0
    p.read_twice("below")
    p.compact("fold-2")
    p.imported("import-3", [D(5), D(8), D(12)], [p.now + 1, p.now + 2, p.now + 3])
    p.now += 10
    f = p.write("past", [(D(13), D(14))])  # lo == 3, past the imported three: the end inherits the last one's version
    assert f.merge.n_before == 3 and f.merge.segs[0].lo == 3 and f.merge.segs[0].vend == p.sim.dv[2] != TM.HOLE
    p.read_twice("past")
    p.compact("end")
    p.coverage["import"] = dict(delta_before=[1, 3])
    return p


FAMILIES = {"segment-tiles": segment_tiles, "glue-exact": glue_and_exact, "delta-tiles": delta_tiles,
            "big-counts": big_counts, "gc": gc_family}
ALL_FAMILIES = ("segment-tiles", "glue-exact", "delta-tiles", "big-counts", "compaction", "gc", "epilogue-delta",
                "epilogue-base", "epilogue-gc")
_BUILT = {}


def build(family, layout):
    """The plans of one family under one layout, as a list (built once)."""
    if (family, layout) not in _BUILT:
        if family == "compaction":
            out = compaction(layout, header=HEADER if layout != "wide" else 2300)
        elif family.startswith("epilogue-"):
            out = [epilogue(layout, family[9:])]
        elif family == "tails":
            out = [tails()]
        elif family == "single-rider":
            out = [single_rider()]
        elif family == "import":
            out = [import_family(layout)]
        elif family == "clear-reuse":
            out = [clear_and_reuse(layout)]
        elif family == "gc-tail-reclaim":
            out = [gc_family(layout, env={"FDBCS_TAIL_RECLAIM": "4096"})]
        else:
            out = [FAMILIES[family](layout)]
        _BUILT[family, layout] = out
    return _BUILT[family, layout]
