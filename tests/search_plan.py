"""The directed batches of tests/test_gpu_search_model.py: the endpoint search (lower_bound of a read's
or a write's key over a tier's boundaries) held to the key-space model (tests/keyspace_model.py) on
keys of different lengths.  Built on the CPU from the model alone; every count a family is meant to
reach is asserted here while the plan is built, and the engine is never consulted for it.

The engine has four forms of the search (foundationdb_amd/csrc/search.h): lane_lower_bound (A),
lane_lower_bound_long with lane_sample_range / lane_prefix_run / load_qtail and the run search (B, a
batch with a key over 24 bytes), group_lower_bound (C, the merge of a short-key batch below
kSegWideMinW = 24576 writes) and prev_seg_hit_quad (D, the previous batch's union segments).  A read
whose span holds thousands of boundaries conflicts whether lower_bound is right or off by a hundred;
here every read spans one to three segments, adjacent segments carry different versions, and every
read goes out twice (K.twice): with its span's maximum as snapshot (commits) and with one less
(conflicts).

Layout.  Every loaded key begins with PFX (the directory's common prefix, dir_p = 1); the byte after it
orders the regions: ladders, tail edges, short prefix runs, the crowded runs, each preceded by random
16-byte filler keys whose number places the family at the chosen rank of the base tier (a key's rank
in the base is its index in the loaded array).  The empty-prefix ladder lies below PFX and the keys of
ABOVE above it: the base never holds them before the compaction (directory slot 0 and dir_top, the
header's segment and lb == n); the delta does, once the write batches have run.

Versions.  Loaded versions stand in [BASE_LO, BASE_HI), neighbours different; polarity 1 loads
BASE_LO + BASE_HI - 1 - v instead, a high header instead of a low one, and writes family segment i in
batch 3 - i % 4 instead of i % 4, so that over both polarities every segment is a local minimum once
and a local maximum once.  Nothing is ever at or below OLDEST, so no read is sent once."""
import bisect
from types import SimpleNamespace

import numpy as np

from tests import keyspace_model as K

PFX = b"\x40"
OLDEST, GC_OLDEST = 1000, 1050  # the GC's floor lies above the victims' versions only
VICTIM_LO = 1010  # versions of the filler boundaries the GC removes (no read meets them)
BASE_LO, BASE_HI = 1200, 2200
HEADERS = (1100, 2300)  # by polarity: below and above every loaded version
FIRST_NOW = 5000
H_TARGET = 40000  # > 32768: sz[0] > 512, so the sample tree has three levels above level 0 and
#                   lane_sample_range's wide-slot descent (for L = 1 .. top - 1) can start below the top
CHUNK = 40000  # transactions per batch (the engine's bound is kMaxTxnLds = 49152)

# tail edges: lengths around the 16-byte prefix, the 24-byte path switch (engine.cpp: p.long_keys =
# max_len > 24), whole tail words (16 + 8j), the first kHW = 6-word round (48 tail bytes: 64), kQW = 12
# words in registers (96 tail bytes: 112) and tail_cmp's fall-back from memory (past 112)
TAIL_LENGTHS = (15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 63, 64, 65, 111, 112, 113, 120, 121, 200)
RUN_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 1000, 5000)
RUN_STARTS = (0, 1, 63)  # mod 64, hence 0, 1, 7 mod 8 (skey8 group starts, level-0 samples)
SHARED = (0, 7, 8, 9, 47, 48, 49, 95, 96, 97, 120)  # tail bytes a run's interior members share
LADDER_STEMS = (b"", PFX, PFX + b"\x02\x77", PFX + b"\x04" + bytes(range(0x51, 0x5e)))  # 0, 1, 3, 15 bytes
LADDER_MAX = 30
ABOVE = (b"\x41", b"\x41\x00", b"\xff" * 3, b"\xff" * 17, b"\xff" * 30)
NARROW = 6  # a family segment is written if it holds at most this many loaded boundaries
ERRORS = ("begin takes one segment more", "begin loses its first segment", "end takes one segment more",
          "end loses its last segment")


def ladder(stem):
    return [stem + b"\0" * k for k in range(LADDER_MAX - len(stem) + 1)]


def tail_edge(rng, cls, L):
    """Five keys of one class: three of length L that first differ in their last byte, and the middle
    one extended by \\0 and by \\xff (the proper-prefix cases, length L + 1)."""
    stem = (PFX + b"\x06" + bytes([cls]) + bytes(rng.integers(1, 255, size=L).astype(np.uint8)))[:L - 1]
    mid = stem + b"\x11"
    return [stem + b"\x10", mid, mid + b"\0", mid + b"\xff", stem + b"\x12"]


def run_members(rng, p16, R, interior, tail_len=8):
    """R keys sharing the 16-byte prefix p16 (which ends in two zero bytes when `interior`).  Plain
    members: p16 + a big-endian counter.  interior: also the bare prefix and its two shorter forms
    (their zero-padded prefix words are the same, so they sit in the run, ordered by length alone) and,
    for every s in SHARED, three members that share s tail bytes with the deeper ones and then differ:
    tails A[:s] + (A[s] +- 1) + j, nested under one 130-byte string A, so that the two probes that
    bracket a query share different numbers of whole tail words with it."""
    out, directed = [], []
    if interior:
        assert p16.endswith(b"\0\0")
        out += [p16[:14], p16[:15], p16]
        A = bytes([0x90]) + bytes(rng.integers(1, 255, size=129).astype(np.uint8))
        for i, s in enumerate(SHARED):
            out += [p16 + A[:s] + bytes([A[s] + (1 if i % 2 else -1), j]) for j in (3, 4, 5)]
        directed += out
    n = R - len(out)
    assert n >= 0
    ctr = np.cumsum(rng.integers(1, 1 << 40, size=n, dtype=np.int64))  # first byte far below A[0]
    plain = [p16 + int(c).to_bytes(8, "big") + b"\x33" * (tail_len - 8) for c in ctr.tolist()]
    directed += plain[:2] + plain[-2:]
    return sorted(out + plain), directed


def filler(rng, lead, n):
    """n random keys of 16 bytes under the prefix `lead`."""
    raw = rng.integers(0, 256, size=(n, 16 - len(lead)), dtype=np.uint8)
    return [lead + r.tobytes() for r in raw]


def queries_of(k):
    """k itself, its greatest proper predecessor and least successor in byte order, and k with its
    last byte one lower and one higher."""
    q = [k, k + b"\0"]
    if k:
        q.append(k[:-1])
        if k[-1] > 0:
            q.append(k[:-1] + bytes([k[-1] - 1]))
        if k[-1] < 255:
            q.append(k[:-1] + bytes([k[-1] + 1]))
    return q


def restated_max(bk, bv, header, qa, qb, err=None):
    """tier_conflict's index rule restated over the sorted boundary list `bk` (bytes) with versions
    `bv`: what the read [qa, qb) compares its snapshot with (None: nothing).  err: one of the four
    one-segment errors of ERRORS (an index), applied to the begin's or the end's position."""
    lb = bisect.bisect_left(bk, qa)
    eq = lb < len(bk) and bk[lb] == qa
    if qa == qb:  # degenerate: the greatest boundary below qa
        lo = lb - 1 + (-1 if err == 0 else 1 if err == 1 else 0)
        hi = lo + 1
    else:
        lo = lb + (1 if eq else 0) - 1  # the segment that holds qa (-1: the header's)
        hi = bisect.bisect_left(bk, qb)  # segments [lo, hi)
        lo += -1 if err == 0 else 1 if err == 1 else 0
        hi += 1 if err == 2 else -1 if err == 3 else 0
    lo, hi = max(lo, -1), min(hi, len(bk))
    vals = [header if i < 0 else bv[i] for i in range(lo, hi)]
    return max(vals) if vals else None


class DeltaSim:
    """The delta tier's boundaries by the merge rule (SkipList.cpp:899-924 over a tier of holes): a
    write [a, b) at `now` removes the boundaries inside it, puts `a` at now and, where `b` is no
    boundary yet, `b` at what stood there (a hole where nothing was written).  Keys are universe
    indices.  Writes of one batch never touch here, so no boundary is shared or dropped."""
    HOLE = None

    def __init__(self):
        self.keys, self.val = [], {}

    def write(self, a, b, now):
        i, j = bisect.bisect_left(self.keys, a), bisect.bisect_left(self.keys, b)
        at_b = j < len(self.keys) and self.keys[j] == b
        end = self.val[b] if at_b else (self.val[self.keys[j - 1]] if j > 0 else self.HOLE)
        for k in self.keys[i:j]:
            del self.val[k]
        self.keys[i:j] = [a] if at_b else [a, b]
        self.val[a] = now
        if not at_b:
            self.val[b] = end

    def rank(self, k):
        i = bisect.bisect_left(self.keys, k)
        return i if i < len(self.keys) and self.keys[i] == k else None


class Plan:
    """polarity 0 | 1.  rider: None (the core plan: every directed key), or "short" / "long" / "wide":
    the queries and writes of at most 24 bytes alone, as they are (check by A, merge by C), with one
    far read-only transaction on a 40-byte key in every batch (everything by B), or with 24576 far
    one-key writes in every write batch (merge by A)."""

    def __init__(self, polarity, rider=None, seed=1):
        self.polarity, self.rider = polarity, rider
        self.pad_tails = not rider  # (the riders send no key of a tail-edge class over 24 bytes)
        self.rng = rng = np.random.default_rng(seed)
        self.header = HEADERS[polarity]
        self.steps, self.coverage = [], {}
        self.families = {}  # name -> directed keys
        self.run_starts = []  # (first key of the run, size)
        self.reservoir = []  # (first key of a run, its delta rank mod 64 to be, universe keys below it)
        loaded = []  # in ascending order, built region by region
        self.victims = []

        def place(fam, bulk_fill, at=None, pad_lead=None):
            """Appends bulk filler, then pad filler under `pad_lead` (which sorts between the two) until
            the next rank is `at` mod 64, then the family."""
            loaded.extend(sorted(bulk_fill))
            if at is not None:
                loaded.extend(sorted(filler(rng, pad_lead, (at - len(loaded)) % 64)))
                assert len(loaded) % 64 == at
            assert not loaded or loaded[-1] < fam[0]
            loaded.extend(fam)

        # ---- the ladders with a stem under PFX (the empty stem's keys lie below every loaded key)
        n_bulk = 6
        directed_total = 5 * len(TAIL_LENGTHS) + sum(RUN_SIZES[:11]) * len(RUN_STARTS) + 3 * 200 + 1000 + 5000 + 80
        bulk = (H_TARGET - directed_total) // n_bulk
        self.families["ladders"] = sum((ladder(s) for s in LADDER_STEMS), [])
        place(ladder(LADDER_STEMS[1]), [])
        assert loaded[0] == PFX  # the first boundary: every key below PFX lies in the header's segment
        fill1 = sorted(filler(rng, PFX + b"\x01", bulk))
        self.victims = fill1[16:-16]  # removed by the GC: far from every read
        place(ladder(LADDER_STEMS[2]), fill1)
        place(ladder(LADDER_STEMS[3]), filler(rng, PFX + b"\x03", bulk))
        # ---- tail edges: one class per length, each under a 2-byte prefix of its own (sparse slots)
        self.tail_class = {}
        fam = []
        for c, L in enumerate(TAIL_LENGTHS):
            ks = tail_edge(rng, 2 * c + 2, L)
            for k in ks:
                self.tail_class[k] = L
            fam += ks
        self.families["tail"] = fam
        place(fam, filler(rng, PFX + b"\x05", bulk))
        # ---- prefix runs: R boundaries sharing one 16-byte prefix, at ranks 0, 1, 63 mod 64
        runs, big = [], []
        first = True
        i = 0
        for R in RUN_SIZES[:11]:
            for at in RUN_STARTS:
                p16 = PFX + b"\x08" + bytes([2 * i + 2]) + bytes(rng.integers(0, 256, size=13).astype(np.uint8))
                mem, d = run_members(rng, p16, R, False, tail_len=8 if i % 2 == 0 else 11)
                place(mem, filler(rng, PFX + b"\x07", bulk) if first else [], at, p16[:2] + bytes([2 * i + 1]))
                self.run_starts.append((mem[0], R))
                runs += sorted(set(d))
                first, i = False, i + 1
        # ---- the crowded family: thousands of boundaries under one 5-byte prefix (one directory slot
        # whatever the slot budget: more than kLaneProbe = 16 skey8 entries and level-0 samples, so both
        # `<= kLaneProbe` tests fail and lane_sample_range's w0 / w1 descent runs), runs with interiors
        first = True
        for i, (R, at) in enumerate(((200, 0), (200, 1), (200, 63), (1000, 63), (5000, 1))):
            p16 = PFX + b"\x0a\x00\x00\x00" + bytes([2 * i + 2]) + bytes(rng.integers(0, 256, size=8).astype(np.uint8)) + b"\0\0"
            mem, d = run_members(rng, p16, R, True)
            place(mem, filler(rng, PFX + b"\x09", bulk) if first else [], at, p16[:5] + bytes([2 * i + 1]))
            self.run_starts.append((mem[0], R))
            big += sorted(set(d))
            if i < 3:  # universe keys just below the run, never loaded: the delta pads (delta_pads)
                self.reservoir.append((mem[0], (0, 1, 63)[i], [p16[:5] + bytes([2 * i + 1, 255]) + j.to_bytes(2, "big") for j in range(140)]))
            first = False
        self.families["runs"], self.families["interiors"] = runs, big
        # ---- the last loaded keys: a run of 77 from rank 63 (polarity 1: 55) mod 64 over the last two
        # level-0 samples to the end of the tier, which lies 12 (4) boundaries past the second, so that
        # lane_prefix_run's hi is n and its group starts number NG = 17 (16): kLaneProbe + 1 and
        # kLaneProbe (prefix_run_groups)
        p16 = PFX + b"\xfe" + bytes(rng.integers(0, 256, size=14).astype(np.uint8))  # (dir_p stays 1)
        top, d = run_members(rng, p16, 77, False, tail_len=9)
        place(top, filler(rng, PFX + b"\x0b", bulk), 55 if polarity else 63, PFX + b"\xfd")
        self.last_run = (top[0], len(top))
        self.families["edges"] = sorted(set(d)) + list(ABOVE)
        assert loaded == sorted(set(loaded)) and len(loaded) > 32768, len(loaded)
        self.loaded_keys = loaded
        self.H = len(loaded)
        crowded = sum(1 for k in loaded if k.startswith(PFX + b"\x0a\x00\x00\x00"))
        sparse = max(sum(1 for k in loaded if k.startswith(PFX + b"\x06" + bytes([2 * c + 2]))) for c in range(len(TAIL_LENGTHS)))
        assert crowded > 64 * 16 * 4 and sparse <= 8
        self.coverage["directory"] = dict(crowded=crowded, sparse=sparse)

        # ---- directed keys and the universe
        if rider:
            for f in self.families:
                self.families[f] = [k for k in self.families[f] if len(k) <= 24]
        self.directed = sorted(set(sum(self.families.values(), [])))
        self.family_of = {k: f for f, ks in self.families.items() for k in ks}
        qs = set()
        for k in self.directed:
            qs.update(q for q in queries_of(k) if not rider or len(q) <= 24)
        self.pads = [PFX + b"\x0c" + b"\x55" * (14 + t) for t in range(1, 8)]  # tails of 1 .. 7 bytes
        far = []
        if rider == "long":
            far = [PFX + b"\xf0" + b"\x66" * 38, PFX + b"\xf0" + b"\x67" * 38]
        if rider == "wide":
            far = sorted(filler(rng, PFX + b"\xf1", 2 * 24576))
        self.far = far
        self.pad_end = PFX + b"\x0d"
        uni = set(loaded) | qs | set(self.pads) | set(far) | {self.pad_end} | {k for _, _, ks in self.reservoir for k in ks}
        self.model = K.KeyspaceModel(K.var_universe(uni), self.header)
        self.ukeys = K.split_keys(self.model.kb, self.model.ko)
        self.index = {k: i for i, k in enumerate(self.ukeys)}
        hist_idx = np.array([self.index[k] for k in loaded], np.int64)
        # the two polarities' versions mirror each other key by key: one sequence, from which the
        # polarity with fewer pad keys before the last run leaves their versions out
        n_own = sum(1 for k in loaded[-77 - 64:] if k.startswith(PFX + b"\xfd"))
        cut = self.H - 77 - n_own
        n_pads = [(at - cut) % 64 for at in (63, 55)]
        assert n_pads[polarity] == n_own
        drop = max(n_pads) - n_own
        vers = BASE_LO + np.cumsum(np.random.default_rng(seed + 77).integers(1, BASE_HI - BASE_LO, size=self.H + drop)) % (BASE_HI - BASE_LO)
        vers = np.concatenate([vers[:cut], vers[cut + drop:]])
        if polarity:
            vers = BASE_LO + BASE_HI - 1 - vers
        vi = np.searchsorted(hist_idx, [self.index[k] for k in self.victims])
        vers[vi] = VICTIM_LO + (np.arange(len(vi)) % 2) * 7 + (np.arange(len(vi)) % 3)
        assert (vers[1:] != vers[:-1]).all() and vers.min() > OLDEST and self.header > OLDEST
        self.model.load(hist_idx, vers)
        assert len(self.model.boundaries()) == self.H
        self.loaded = (*self.model.pack_keys(hist_idx), vers, self.header)
        self.base_rank = {k: i for i, k in enumerate(loaded)}
        for k, R in self.run_starts:
            assert self.base_rank[k] % 64 in RUN_STARTS
        self.coverage["run_starts_base"] = sorted({(self.base_rank[k] % 8, self.base_rank[k] % 64) for k, _ in self.run_starts})
        shapes = {prefix_run_groups(self.base_rank[k], self.base_rank[k] + R, self.H) for k, R in self.run_starts + [self.last_run]}
        # runs with 0, 1, 2 and many level-0 samples; 7 and 15 group starts, kLaneProbe (+ 1) and more
        assert {0, 1, 2} <= {n for n, _ in shapes} and max(n for n, _ in shapes) > 16
        assert {7, 15, 17 - polarity} <= {g for _, g in shapes} and max(g for _, g in shapes) > 17
        self.coverage["run_shapes_base"] = sorted(shapes)
        self.now = FIRST_NOW
        self.oldest = OLDEST
        # where the version a universe key shows came from: 0 base, 1 delta, 2 the previous batch
        self.src = np.zeros(self.model.U, np.int8)
        self.delta = DeltaSim()
        self.flips = {}  # (phase, directed key) -> set of errors that flip a verdict of some read
        self.decided = {}  # family -> [reads, by the base, by the delta, by the previous batch]
        self.align = {}  # tail-edge class -> residues mod 8 its long queries' tails were sent at

    # ------------------------------------------------------------------ reads

    def read_spans(self):
        """One to three segments around every query of every directed key: the query as a read's begin
        (the read ends at the first, second or third boundary above it), as its end, and as the
        degenerate read [q, q).  Returns universe index pairs and, per read, the directed key that owns
        its begin and the one that owns its end (-1: none: the other end of a span is just a boundary)."""
        m = self.model
        bnd = m.boundaries().tolist()
        spans = []
        for d, k in enumerate(self.directed):
            for q in queries_of(k):
                if q not in self.index or (self.rider and len(q) > 24):
                    continue
                u = self.index[q]
                for n in ((1, 2, 3) if q == k else (1, 2 + d % 2)):
                    j = bisect.bisect_right(bnd, u) - 1 + n  # the n-th boundary above q
                    if j < len(bnd):
                        spans.append((u, bnd[j], d, -1))
                    i = bisect.bisect_left(bnd, u) - n  # the n-th boundary below q (-1: the first key of all)
                    a = bnd[i] if i >= 0 else (0 if i == -1 else None)
                    if a is not None and a < u:
                        spans.append((a, u, -1, d))
                spans.append((u, u, d, -1))
        sp = np.array(sorted(set(spans)), np.int64)
        if self.rider:  # the other end of a span is a boundary of any length: keep the short ones
            ln = np.diff(m.ko)
            sp = sp[(ln[sp[:, 0]] <= 24) & (ln[sp[:, 1]] <= 24)]
        return sp[self.rng.permutation(len(sp))]

    def account(self, sp, phase):
        """Sensitivity and per-family counts of one read batch, by the restated rule."""
        m = self.model
        bnd = m.boundaries()
        bk, bv = [self.ukeys[i] for i in bnd.tolist()], m.ver[bnd].tolist()
        top = m.read_max(sp[:, 0], sp[:, 1])
        for (a, b, db, de), mx in zip(sp.tolist(), top.tolist()):
            qa, qb = self.ukeys[a], self.ukeys[b]
            assert restated_max(bk, bv, m.header, qa, qb) == mx  # the restatement against the model
            for e in range(4):
                d = db if e < 2 else de
                if d >= 0 and restated_max(bk, bv, m.header, qa, qb, e) != mx and (a != b or e < 2):
                    self.flips.setdefault((phase, d), set()).add(e)
            d = db if db >= 0 else de
            lo, hi = (a - 1, a) if a == b else (a, b)
            holders = np.unique(self.src[lo:hi][m.ver[lo:hi] == mx]) if lo >= 0 else [0]
            c = self.decided.setdefault(self.family_of[self.directed[d]], [0, 0, 0, 0])
            c[0] += 1
            if len(holders) == 1:
                c[1 + int(holders[0])] += 1

    def alignment(self, a, b):
        """load_qtail shifts by the query tail's address mod 8; the batch's tails are packed unpadded in
        endpoint order (engine.cpp, fdbcs_batch_add_packed: out->tail = tb; tb += len - 16).  Returns
        each endpoint's tail offset mod 8 (reads only, one range per transaction: begin, end, ...)."""
        ln = np.diff(self.model.ko)
        ends = np.stack([a, b], 1).ravel()
        t = np.maximum(ln[ends] - 16, 0)
        off = np.concatenate([np.cumsum(t[c:c + 2 * CHUNK]) - t[c:c + 2 * CHUNK] for c in range(0, len(t), 2 * CHUNK)])
        return ends, off % 8, int((off[-1] + t[-1]) % 8)  # (every batch of CHUNK reads starts at 0)

    def read_batches(self, name, phase=None, record=True):
        """The read batches of the current state (K.twice: no read is sent once), with pad reads
        appended until every tail-edge class has had a long query at all eight tail residues."""
        m = self.model
        sp = self.read_spans()
        if record:
            self.account(sp, phase)
        a, b, snap, want, once = K.twice(m, sp[:, 0], sp[:, 1], self.oldest)
        assert once == 0.0, once
        if self.pad_tails:
            a, b, snap, want = self.pad_alignment(a, b, snap, want)
        assert (want == K.CONFLICT).mean() >= 0.3 and (want == K.COMMITTED).mean() >= 0.3
        out = []
        for c in range(0, len(a), CHUNK):
            s = slice(c, c + CHUNK)
            n = len(a[s])
            aa, bb, sn, wt = a[s], b[s], snap[s], want[s]
            if self.rider == "long":  # one far read-only transaction on a 40-byte key: long_keys
                f = self.index[self.far[0]]
                aa, bb = np.append(aa, f), np.append(bb, f + 1)
                sn, wt = np.append(sn, m.read_max([f], [f + 1])[0]), np.append(wt, K.COMMITTED).astype(np.uint8)
                n += 1
            self.now += 10
            out.append((m.batch(np.zeros(n, bool), aa, bb, sn), self.now, self.oldest, wt))
        return SimpleNamespace(name=name, kind="read", batches=out, state=None, gc_interval=None, as_stored=True,
                               delta_before=None)

    def pad_alignment(self, a, b, snap, want):
        """Appends, for every (tail-edge class, residue) the reads have not sent a long query at, a pad
        read [pad key with a tail of w bytes, a short key) and then the degenerate read of a key of the
        class, whose tail then starts at the residue."""
        m = self.model
        extra = []
        long_keys = {L: next(k for k, c in self.tail_class.items() if c == L and len(k) > 16) for L in TAIL_LENGTHS if L > 16}
        assert len(a) % CHUNK + 2 * 8 * len(long_keys) < CHUNK  # the appended reads stay in the last batch
        for _ in range(2):
            ends, res, cur = self.alignment(np.concatenate([a, [x[0] for x in extra]]).astype(np.int64),
                                            np.concatenate([b, [x[1] for x in extra]]).astype(np.int64))
            seen = {}
            for e, r in zip(ends.tolist(), res.tolist()):
                k = self.ukeys[e]
                if k in self.tail_class and len(k) > 16:
                    seen.setdefault(self.tail_class[k], set()).add(r)
            missing = [(L, r) for L in long_keys for r in range(8) if r not in seen.get(L, set())]
            if not missing:
                break
            for L, r in missing:
                w = (r - cur) % 8
                if w:
                    extra.append((self.index[self.pads[w - 1]], self.index[self.pad_end]))
                u = self.index[long_keys[L]]
                extra.append((u, u))
                cur = (cur + w + 2 * (len(long_keys[L]) - 16)) % 8
        else:
            raise AssertionError(("tail residues still missing", missing[:5]))
        for L in TAIL_LENGTHS:
            if L > 16:
                self.align.setdefault(L, set()).update(seen[L])
                assert seen[L] == set(range(8)), (L, seen[L])
        if extra:
            ea, eb = np.array(extra, np.int64).T
            mx = m.read_max(ea, eb)
            a, b = np.concatenate([a, ea]), np.concatenate([b, eb])
            snap, want = np.concatenate([snap, mx]), np.concatenate([want, np.full(len(ea), K.COMMITTED, np.uint8)])
        return a, b, snap, want

    # ------------------------------------------------------------------ writes

    def family_segments(self):
        """Segment i = [directed key i, directed key i + 1) where both lie in one family and the span
        holds at most NARROW loaded boundaries (a narrow write), with its write batch: i mod 4, or
        3 - i mod 4 in polarity 1."""
        segs = []
        ranks = np.searchsorted([self.index[k] for k in self.loaded_keys], [self.index[k] for k in self.directed])
        for i in range(len(self.directed) - 1):
            ka, kb = self.directed[i], self.directed[i + 1]
            if self.family_of[ka] == self.family_of[kb] and ranks[i + 1] - ranks[i] <= NARROW:
                segs.append((self.index[ka], self.index[kb], 3 - i % 4 if self.polarity else i % 4))
        return segs

    def delta_pads(self, segs):
        """Writes on the reservoir keys below three runs that bring the run starts' ranks in the delta,
        once the four write batches have run, to 0, 1 and 63 mod 64 (the delta then holds exactly the
        segments' endpoints: no two writes overlap).  A pair [r0, r1) adds two boundaries, a triple
        [r0, r1) | [r1, r2) in two batches three."""
        ends = sorted({x for a, b, _ in segs for x in (a, b)})
        out, shift = [], 0
        for start, target, keys in sorted(self.reservoir):
            if start not in self.index or self.rider:
                continue
            c = (target - bisect.bisect_left(ends, self.index[start]) - shift) % 64
            c += 64 if c == 1 else 0
            shift += c
            r = [self.index[k] for k in keys]
            if c % 2:
                out += [(r[0], r[1], 0), (r[1], r[2], 1)]
                r, c = r[3:], c - 3
            out += [(r[2 * j], r[2 * j + 1], 2 * (j % 2)) for j in range(c // 2)]
        return out

    def write_batch(self, name, segs, checks=False):
        """One batch of one-range write transactions [a, b) (universe indices); with rider "wide",
        24576 far one-key writes beside them."""
        m = self.model
        wa, wb = np.array([s[0] for s in segs], np.int64), np.array([s[1] for s in segs], np.int64)
        o = np.argsort(wa)
        assert (wb[o][:-1] < wa[o][1:]).all()  # no two writes of a batch touch
        if self.rider == "wide":
            f = np.array([self.index[k] for k in self.far], np.int64)
            wa, wb = np.concatenate([wa, f[0::2]]), np.concatenate([wb, f[1::2]])
            assert len(wa) >= 24576  # kSegWideMinW
        o = self.rng.permutation(len(wa))
        wa, wb = wa[o], wb[o]
        self.now += 10
        T = len(wa)
        aa, bb, isw, sn = wa, wb, np.ones(T, bool), np.full(T, self.now - 1)
        want = np.full(T, K.COMMITTED, np.uint8)
        if self.rider == "long":
            f = self.index[self.far[0]]
            aa, bb, isw = np.append(f, aa), np.append(f + 1, bb), np.append(False, isw)
            sn, want = np.append(m.read_max([f], [f + 1])[0], sn), np.append(K.COMMITTED, want).astype(np.uint8)
        pb = m.batch(isw, aa, bb, sn)
        before = len(self.delta.keys)
        self.src[self.src == 2] = 1
        for x, y in segs:  # (the riders' far writes are in no read's span and in no prediction)
            self.delta.write(int(x), int(y), self.now)
            self.src[x:y] = 2
        m.write(wa, wb, self.now)
        st = SimpleNamespace(name=name, kind="write", batches=[(pb, self.now, self.oldest, want)], state=m.rle(),
                             delta_before=before if checks else None, segments=len(segs), gc_interval=None,
                             as_stored=True)
        self.steps.append(st)
        return st


def prefix_run_groups(s, e, n):
    """lane_sample_range and lane_prefix_run replayed for a query whose 16-byte prefix the boundaries
    of ranks [s, e) share, in a tier of n boundaries: the level-0 samples (ranks 64 i) inside the run
    and the number NG of skey8 group starts the run is counted among (kLaneProbe = 16 at most are
    loaded at once; more take the branch that bisects on prefixes)."""
    c, b = -(-s // 64), -(-e // 64)  # samples below the run, samples below its end
    lo1, hi = (64 * (c - 1) + 1 if c else 0), min(n, 64 * b)
    g0 = (lo1 + 7) // 8
    return b - c, ((hi - 1) // 8 - g0 + 1 if hi > 8 * g0 else 0)


def run_ranks(p, tier_rank):
    return sorted({(r % 8, r % 64) for k, _ in p.run_starts for r in [tier_rank(k)] if r is not None})


def build(polarity, rider=None):
    """The core plan (rider None) or a rider: the base alone; four write batches, the same read batch
    twice after each (the first decided by the previous batch's segments where the batch wrote, the
    second by the delta); a forced compaction (gc_interval 1) and a read; a GC (the oldest version
    moves past the victims' versions) and a read."""
    p = Plan(polarity, rider)
    p.steps.append(p.read_batches("base", phase="base"))
    segs = p.family_segments()
    segs += p.delta_pads(segs)
    p.coverage["segments"] = len(segs)
    for w in range(4):
        st = p.write_batch(f"write-{w}", [(a, b) for a, b, k in segs if k == w], checks=True)
        p.steps.append(p.read_batches(f"read-{w}-prev", phase="prev" if w == 3 else None, record=w == 3))
        p.src[p.src == 2] = 1  # the next batch's check reads them in the delta
        rd = p.read_batches(f"read-{w}-delta", phase="delta" if w == 3 else None, record=w == 3)
        rd.state = st.state
        p.steps.append(rd)
    p.coverage["delta_size"] = len(p.delta.keys)
    p.coverage["run_starts_delta"] = got = run_ranks(p, lambda k: p.delta.rank(p.index[k]))
    if not rider:  # the delta ranks of the run starts, by the predicted delta: group starts and samples
        assert {0, 1, 7} <= {r8 for r8, _ in got} and {0, 1, 63} <= {r64 for _, r64 in got}, got
    # the compaction: a read batch under gc_interval 1 (its half Y compacts, by k_compact_search<2>
    # when the batch has a key over 24 bytes), then the same reads against the rebuilt base
    st = p.read_batches("compact", record=False)
    st.gc_interval, st.state = 1, p.model.rle()
    p.steps.append(st)
    p.src[:] = 0
    st = p.read_batches("read-compacted", phase="compacted")
    st.state = p.model.rle()
    p.steps.append(st)
    # the GC: every victim falls below the floor and coalesces, every rank above them moves
    st = p.read_batches("gc", record=False)
    st.batches = [(pb, now, GC_OLDEST, want) for pb, now, _, want in st.batches]
    p.oldest = GC_OLDEST
    before = len(p.model.boundaries())
    p.model.clamp(GC_OLDEST)
    # (what is stored below the floor depends on when the engine collected: the default floor compares)
    st.state, st.as_stored = p.model.rle(), False
    p.steps.append(st)
    assert len(p.model.boundaries()) == before - len(p.victims) + 1  # the victims coalesce into one
    st = p.read_batches("read-gc", phase="gc")
    st.state, st.as_stored = p.model.rle(), False
    p.steps.append(st)
    p.coverage["decided"] = {f: tuple(c) for f, c in p.decided.items()}
    p.coverage["reads"] = sum(pb.n_txn for s in p.steps if s.kind == "read" for pb, _, _, _ in s.batches)
    return p


def check_sensitivity(plans):
    """Over both polarities: for every directed key, some read flips one of its two verdicts under
    each of the four one-segment errors, in the base alone (loaded keys) and over the written history
    (every key).  The first boundary of all has nothing below it but the header, which no written
    version lies below: that one error is exempt there."""
    p0 = plans[0]
    assert plans[0].directed == plans[1].directed
    counts = {}
    for phase, keys in (("base", [d for d, k in enumerate(p0.directed) if k in p0.base_rank]),
                        ("delta", range(len(p0.directed)))):
        for d in keys:
            got = set().union(*(p.flips.get((phase, d), set()) for p in plans))
            need = {0, 1, 2, 3}
            if phase == "delta" and d == 0:
                need.discard(0)
            if phase == "delta" and d == len(p0.directed) - 1:
                need.discard(2)  # (and the last of all nothing above it but the loaded version it restores)
            assert need <= got, (phase, p0.directed[d], sorted(got))
        counts[phase] = len(list(keys))
    return counts


# ---------------------------------------------------------------------------------- path D


PATH_D_SIZES = (1, 2, 16, 17, 18, 288, 289, 290, 5000)  # union segments: 17-ary rounds of 16 probes


def build_path_d(polarity):
    """prev_seg_hit_quad: write batches of U = 1 .. 5000 union segments over consecutive members of the
    runs and the tail-edge classes, each followed by one read batch that the previous batch's segments
    decide: reads that end exactly at a segment's begin, begin exactly at its end, and the degenerate
    reads at both (of those only the degenerate read at the end meets the segment), one to three
    model segments long, snapshots at the span's maximum and one below."""
    p = Plan(polarity)
    p.pad_tails = False
    pool = [k for k in p.loaded_keys if k[:2] in (PFX + b"\x0a", PFX + b"\x08") and len(k) > 16] + p.families["tail"]
    idx = [p.index[k] for k in sorted(pool)]
    cov = {}
    assert len(idx) >= 2 * 4000 + 60
    for n, U in enumerate(PATH_D_SIZES):
        # segments [member 2j, member 2j + 1): the next segment begins one member on, so none touch
        first = (n * 131) % 50
        U = min(U, (len(idx) - 60) // 2)  # the last one: as many as the families hold (over 4000)
        pairs = [(idx[first + 2 * j], idx[first + 2 * j + 1]) for j in range(U)]
        p.write_batch(f"segments-{U}", pairs)
        keys = sorted({p.ukeys[x] for ab in (pairs if U <= 300 else pairs[::7] + pairs[:20] + pairs[-20:]) for x in ab})
        p.directed = keys
        p.family_of = {k: "path-d" for k in keys}
        sp_before = p.decided.get("path-d", [0, 0, 0, 0])[3]
        st = p.read_batches(f"reads-{U}", phase=("d", U))
        st.state = p.steps[-1].state
        p.steps.append(st)
        cov[U] = p.decided["path-d"][3] - sp_before
        assert cov[U] >= min(U, 100), cov  # reads the previous batch's segments alone decide
    p.coverage["path_d"] = cov
    return p
