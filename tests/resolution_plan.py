"""The directed batches of tests/test_gpu_resolution_model.py, built on the CPU from the batch-order
model alone (tests/keyspace_model.py: TxnBatch, resolve, batch_facts).  Each family aims at constants
the intra-batch kernels branch on, and every count a family is meant to reach is asserted here, from
the model's facts, while the plan is built: the engine is never consulted for it.

Two geometries decide the kind of a candidate edge, and every family with writers uses both:
    "inside"           write [k, k+1) under read [k-1, k+1): the write begins strictly inside the read,
                       a direct edge enumerated from the read;
    "same" / "below"   write [k, k+1) or [k-1, k+1) under read [k, k+1): the write covers the read's
                       begin, with write groups on a group edge enumerated from the write.

Versions: the loaded history stands between OLDEST and DEAD_SNAP (nothing is below the floor); the
first batch of every plan writes the poison keys at FIRST_NOW; a transaction is made dead before the
rounds by reading a poison key at DEAD_SNAP (history conflict) or anything at OLD_SNAP (TooOld);
every other snapshot is its batch's now - 1."""
from types import SimpleNamespace

import numpy as np

from tests import keyspace_model as K

HEADER, OLDEST, OLD_SNAP, DEAD_SNAP, FIRST_NOW = 1050, 1000, 900, 1500, 2000
GEOMS = ("inside", "same", "below")
FILL = 13000  # filler keys at either end of the universe (single-key writes no read meets)


def wr(geom, k):
    return (k - 1, k + 1) if geom == "below" else (k, k + 1)


def rd(geom, k):
    return (k - 1, k + 1) if geom == "inside" else (k, k + 1)


def txn(reads=(), writes=(), snap=None, report=False, tag=None):
    return dict(reads=list(reads), writes=list(writes), snap=snap, report=report, tag=tag)


class Plan:
    def __init__(self, seed, shape, universe=1 << 18):
        self.rng = np.random.default_rng(seed)
        self.model = K.KeyspaceModel(K.make_universe(self.rng, universe, shape), HEADER)
        hist = np.array([2, 5])
        self.model.load(hist, [1100, 1200])
        self.loaded = (*self.model.pack_keys(hist), np.array([1100, 1200], np.int64), HEADER)
        self.low, self.high = 8, universe - 2 - FILL
        self.next = self.low + FILL + 4
        self.now = FIRST_NOW
        self.steps, self.coverage = [], {}
        self.poison = [self.key() for _ in range(8)]
        self.emit("history", [txn(writes=[(k, k + 1)]) for k in self.poison], shares=(1.0, 0.0))

    def block(self, n):
        """n consecutive fresh universe indices; the index before and after them stays unused."""
        a = self.next
        self.next += n + 1
        assert self.next < self.high
        return a

    def key(self):
        """A fresh key k with k - 2, k - 1 and k + 1 its own."""
        return self.block(4) + 2

    def dead(self, i, writes, tag="dead"):
        """A writer decided before the rounds: a history conflict (even i) or TooOld (odd i; its ranges
        are never registered, so it is no candidate writer at all and its write is in no group)."""
        p = self.poison[i % len(self.poison)]
        return txn([(p, p + 1)], writes, DEAD_SNAP if i % 2 == 0 else OLD_SNAP, i % 3 == 0, tag)

    def merge(self, seqs):
        """Sequences of chunks (lists of transactions that stay adjacent) interleaved at random, each
        sequence keeping its own order."""
        order = self.rng.permutation(np.repeat(np.arange(len(seqs)), [len(s) for s in seqs]))
        at = [0] * len(seqs)
        out = []
        for s in order.tolist():
            out += seqs[s][at[s]]
            at[s] += 1
        return out

    def emit(self, name, txns, shares=(0.3, 0.3)):
        """Resolves the batch on the model and records the step: the packed batch, the expected
        verdicts, reports and state, and the sizes and counts the engine's counters are held to."""
        tb = K.TxnBatch()
        for x in txns:
            tb.add(x["reads"], x["writes"], self.now - 1 if x["snap"] is None else x["snap"], x["report"], x["tag"])
        res = K.resolve(self.model, tb, self.now, OLDEST)
        f, A, v = res.facts, res.admitted, res.verdicts
        got = ((v == K.COMMITTED).mean(), (v == K.CONFLICT).mean())
        assert got[0] >= shares[0] and got[1] >= shares[1], (name, got)
        assert (v == K.COMMITTED).any() and (shares[1] == 0 or (v == K.CONFLICT).any())
        self.steps.append(SimpleNamespace(
            name=name, pb=tb.pack(self.model), now=self.now, oldest=OLDEST, want=v, reports=res.reports,
            shares=shares, state=self.model.rle(), T=A.T, R=len(A.ra), W=len(A.wa), slots=f.n_slots, U=f.U, P=f.P,
            P_grouped=f.P_grouped, n_groups=f.n_groups))
        self.now += 10
        return tb, res


# ---------------------------------------------------------------------------------- walk ladders

LASTS = ("none", "rounds", "pre")


def ladder(p, j, last, geom, n_dead, grouped):
    """A reader X with one read per writer, in a fixed order: j writers that are live after the
    pre-pass and abort in the rounds (each reads a key written by an earlier transaction that commits
    with no candidate), then none (X commits), a writer that commits only in the rounds (it reads a key
    whose writer aborts in the rounds) or a writer the pre-pass commits (X aborts); n_dead dead writers'
    reads interleaved; grouped: every ladder writer shares its key with a dead writer, so that with the
    covering geometries it is one member of a group of two."""
    seq, reads = [], []
    n = 0

    def aborter(tag="A"):
        nonlocal n
        s, w = p.key(), p.key()
        seq.append([txn(writes=[wr(geom, s)], tag="S")])
        if grouped:
            seq.append([p.dead(2 * n, [wr(geom, w)])])
        seq.append([txn([rd(geom, s)], [wr(geom, w)], report=n % 2 == 0, tag=tag)])
        n += 1
        return w

    for _ in range(j):
        reads.append(rd(geom, aborter()))
    if last == "pre":
        w = p.key()
        seq.append([txn(writes=[wr(geom, w)], tag="D")])
        reads.append(rd(geom, w))
    elif last == "rounds":
        b, w = aborter("B"), p.key()
        seq.append([txn([rd(geom, b)], [wr(geom, w)], report=True, tag="C")])
        reads.append(rd(geom, w))
    for d in range(n_dead):
        w = p.key()
        seq.append([p.dead(j + d, [wr(geom, w)])])
        reads.insert(min(len(reads), (d * (len(reads) + 1)) // n_dead + d), rd(geom, w))
    seq.append([txn(reads, [wr(geom, p.key())], report=(j + n_dead) % 3 != 0, tag=("X", j, last))])
    return seq


def count_ladders(p, tb, res, into):
    """The ladder readers by the model's facts: walked[t] is the number of live writers that abort
    before the one that decides t, and the order of t's packed list is the only one possible."""
    f = res.facts
    for t, tag in enumerate(tb.tag):
        if isinstance(tag, tuple) and tag[0] == "X":
            _, j, last = tag
            assert f.exact[t] and not f.dead[t] and f.walked[t] == j, (t, tag, f.walked[t])
            assert f.n_live[t] == j + (last != "none")
            assert (res.verdicts[t] == K.COMMITTED) == (last == "none")
            c = into.setdefault(j, {"commit": 0, "abort": 0, "dead_between": 0})
            c["commit" if last == "none" else "abort"] += 1
            c["dead_between"] += int(f.n_cand[t] > f.n_live[t])
        elif tag == "A" or tag == "B":  # live after the pre-pass, aborted in the rounds
            assert not f.dead[t] and f.n_live[t] == 1 and res.verdicts[t] == K.CONFLICT
        elif tag == "C":  # committed in the rounds: its only live writer aborts there
            assert f.n_live[t] == 1 and f.walked[t] == 1 and res.verdicts[t] == K.COMMITTED
        elif tag == "D" or tag == "S":  # committed by the pre-pass: no candidate at all
            assert f.n_cand[t] == 0 and res.verdicts[t] == K.COMMITTED


def ladder_steps(p):
    counts = {}
    every = [(j, last, nd) for j in range(10) for last in LASTS for nd in range(4)]
    for geom in GEOMS:
        for grouped in (False, True):
            seqs = [ladder(p, j, last, geom, nd, grouped) for j, last, nd in every]
            tb, res = p.emit(f"ladders-{geom}-{'grouped' if grouped else 'single'}", p.merge(seqs))
            assert len(tb) <= 5120  # k_resolve<5>
            count_ladders(p, tb, res, counts)
    seqs = [ladder(p, j, last, geom, nd, grouped) for j, last, nd in every
            for geom in GEOMS for grouped in (False, True)]
    tb, res = p.emit("ladders-all", p.merge(seqs))
    assert len(tb) > 5120  # k_resolve<8>
    count_ladders(p, tb, res, counts)
    for j in range(10):
        c = counts[j]
        assert c["commit"] + c["abort"] >= 20 and min(c["commit"], c["abort"], c["dead_between"]) >= 5, (j, c)
    p.coverage["ladders"] = counts


# ---------------------------------------------------------------------------------- write groups


def hot_key(p, N, first, geom, s0, b0, sparse=False):
    """One hot key written by N transactions, readers interleaved in batch order.  The members before
    the first that commits are dead or abort in the rounds; that one (`first`) is committed by the
    pre-pass ("pre"), commits in the rounds ("rounds") or is a read-modify-write of the key ("rmw", its
    own write in the group its read meets); a reader stands just before it and just after it.  The
    members after it are of all kinds.  "below": the members begin at three different keys."""
    h = p.key()
    seq = []
    m = N // 2
    hw = lambda i: (h - i % 3, h + 1) if geom == "below" else (h, h + 1)
    hr = rd(geom, h)
    rs, rb = rd("same", s0), rd("same", b0)

    def member(i, kind):
        if kind == "dead":  # by a history conflict: a TooOld transaction's write is never registered
            return p.dead(2 * i, [hw(i)])
        reads = {"abort": [rs], "rmw_abort": [rs, hr], "rounds": [rb], "pre": [], "rmw": [hr]}[kind]
        return txn(reads, [hw(i)], report=i % 2 == 1, tag=("M", kind))

    reader = lambda i: txn([hr], report=i % 2 == 0, tag="R")
    before = ("dead", "abort", "dead", "abort", "rmw_abort")
    after = ("pre", "abort", "dead", "rounds") + (("rmw",) if not sparse else ())
    gap = max(1, N // 6)
    seq.append([reader(0)])
    for i in range(N):
        if i == m:
            seq.append([reader(i), member(i, first), reader(i + 1)])
            continue
        kind = before[i % len(before)] if i < m else after[i % len(after)]
        if sparse and i % 40 == 7:
            kind = "rmw_abort" if i < m else "rmw"
        seq.append([member(i, kind)])
        if i % gap == gap - 1:
            seq.append([reader(i)])
    return seq


def adjacent_groups(p, s0):
    """Two groups next to each other in write-begin order whose read-begin sets differ by one
    read-begin: writes [h, h+2) hold the read-begins at h and h+1, writes [h+1, h+2) only those at
    h+1; exactly one read begins at h.  No write over h commits, one over h+1 alone does: the read at
    h, last in the batch, commits unless the second group is taken for a part of the first."""
    h = p.block(5) + 1
    rs = rd("same", s0)
    seq = [[txn([(h + 1, h + 2)], tag="R")]]
    for i, (wide, narrow) in enumerate((("dead", "dead"), ("abort", "abort"), ("abort", "pre"))):
        for a, kind in ((h, wide), (h + 1, narrow)):
            seq.append([p.dead(2 * i, [(a, h + 2)]) if kind == "dead" else
                        txn([rs] if kind == "abort" else [], [(a, h + 2)], tag=("M", kind))])
        seq.append([txn([(h + 1, h + 2)], report=True, tag="R")])
    seq.append([txn([(h, h + 1)], report=True, tag=("R", "adjacent"))])
    return seq


def group_facts(tb, res):
    """Per reader of a covering geometry, from the model's groups: decided by group edges alone (it has
    candidates, none of them direct), the least committed member of the groups its reads meet, whether
    a write of its own is a member of one of them."""
    f, A = res.facts, res.admitted
    wt_sorted = A.wt[f.gorder]
    committed = res.verdicts[wt_sorted] == K.COMMITTED
    out = {}
    for t, tag in enumerate(tb.tag):
        if f.dead[t] or f.n_cand[t] == 0 or not (tag == "R" or (isinstance(tag, tuple) and tag[1].startswith("rmw"))):
            continue
        rs = [r for r in range(A.roff[t], A.roff[t + 1]) if f.cand[r] is not None]
        if any(f.direct[r].any() for r in rs):
            continue
        least, own = None, False
        for r in rs:
            rank = np.searchsorted(f.rb_sorted, A.ra[r], "left")
            inn = (f.gstart >= 0) & (f.giv[:, 0] <= rank) & (rank < f.giv[:, 1])
            own |= bool((wt_sorted[inn] == t).any())
            c = wt_sorted[inn & committed & (wt_sorted < t)]
            if len(c):
                least = int(c.min()) if least is None else min(least, int(c.min()))
        assert (res.verdicts[t] == K.CONFLICT) == (least is not None)
        out[t] = (least, own)
    return out


def group_steps(p):
    """Four batches with W exactly 1024, 1025 (k_resolve holds per = ceil(W / 1024) members per thread:
    1 | 2), 12288 (groups on, per = 12) and 12289 (groups off): hot keys of 1, 2, 12 and 13 writers with
    each kind of first committed member, in all three geometries, one or two big ones, the adjacent
    groups, and single-key filler writes no read meets that bring W to the number."""
    cov = {"group_only": 0, "least_at_t-1": 0, "own_write_commits": 0, "W": {}}
    big = {1024: [(300, "same"), (300, "inside")], 1025: [(300, "below")],
           12288: [(3000, "below"), (300, "inside")], 12289: [(3000, "same")]}
    for Wtot in (1024, 1025, 12288, 12289):
        s0, b0 = p.key(), p.key()
        head = [txn(writes=[wr("same", s0)], tag="S"), txn([rd("same", s0)], [wr("same", b0)], tag="B")]
        seqs, target, i = [adjacent_groups(p, s0)], None, 0
        for N in (1, 2, 12, 13):
            for first in ("pre", "rounds", "rmw"):
                seqs.append(hot_key(p, N, first, GEOMS[1 + i % 2] if i % 4 else "inside", s0, b0))
                i += 1
                if N == 13 and first == "rmw":  # (a covering one, "below": its least begin key)
                    target = min(x["writes"][0][0] for c in seqs[-1] for x in c if x["writes"])
        for N, geom in big[Wtot]:
            first = ("pre", "rounds", "rmw")[N % 3 if N < 1000 else 2]
            seqs.append(hot_key(p, N, first, geom, s0, b0, sparse=N > 1000))
        n_writes = len(head) + sum(len(x["writes"]) for q in seqs for c in q for x in c)
        # fillers bring W to Wtot exactly; those below the hot keys place the 13-member group across
        # a wave boundary of k_resolve's member runs (64 threads of `per` write-begin indices each)
        per = -(-Wtot // 1024)
        n_fill = Wtot - n_writes
        below = sum(1 for q in seqs for c in q for x in c for a, _ in x["writes"] if a < target)
        n_low = (-6 - below) % (64 * per)
        assert 0 <= n_low <= n_fill <= FILL
        fill = [txn(writes=[(p.low + k, p.low + k + 1)]) for k in range(n_low)]
        fill += [txn(writes=[(p.high + k, p.high + k + 1)]) for k in range(n_fill - n_low)]
        body = head + p.merge(seqs + [[[x] for x in fill[i::8]] for i in range(8)])
        tb, res = p.emit(f"groups-W{Wtot}", body, shares=(0.3, 0.05))
        f, A = res.facts, res.admitted
        assert len(A.wa) == Wtot and len(tb) <= 49152
        # the groups the family is about, by the model's facts
        size = np.bincount(f.gstart[f.gstart >= 0], minlength=Wtot)
        starts = np.flatnonzero(size > 0)
        cross = lambda unit: any(s // unit != (s + size[s] - 1) // unit for s in starts.tolist() if 12 <= size[s] <= 13)
        assert cross(64 * per) and cross(per) and size.max() >= max(N for N, _ in big[Wtot])
        assert {1, 2, 12, 13} <= set(size[starts].tolist())
        begins = A.wa[f.gorder]
        # one group whose members begin at three different keys
        assert any(len(set(begins[s:s + size[s]].tolist())) == 3 for s in starts.tolist())
        nxt = starts[:-1] + size[starts[:-1]]
        adj = (nxt == starts[1:]) & (f.giv[starts[:-1], 1] == f.giv[starts[1:], 1]) & \
              (f.giv[starts[:-1], 0] + 1 == f.giv[starts[1:], 0])
        assert adj.any()  # adjacent groups that differ by one read-begin
        last = [t for t, tag in enumerate(tb.tag) if tag == ("R", "adjacent")]
        assert len(last) == 1 and res.verdicts[last[0]] == K.COMMITTED and f.n_cand[last[0]] == 3
        kinds = {}
        for t, tag in enumerate(tb.tag):
            if isinstance(tag, tuple) and tag[0] == "M":
                k = ("dead" if f.dead[t] else "abort" if res.verdicts[t] == K.CONFLICT else
                     "pre" if f.n_live[t] == 0 else "rounds")
                kinds[k] = kinds.get(k, 0) + 1
            elif tag == "dead":
                kinds["dead"] = kinds.get("dead", 0) + 1
        assert min(kinds.get(k, 0) for k in ("dead", "abort", "pre", "rounds")) >= 5, kinds
        for t, (least, own) in group_facts(tb, res).items():
            cov["group_only"] += 1
            cov["least_at_t-1"] += int(least == t - 1)
            cov["own_write_commits"] += int(own and res.verdicts[t] == K.COMMITTED)
        cov["W"][Wtot] = dict(T=len(tb), groups=f.n_groups, largest=int(size.max()), per=per, slots=f.n_slots)
    assert cov["group_only"] >= 20 and cov["least_at_t-1"] >= 5 and cov["own_write_commits"] >= 5, cov
    p.coverage["groups"] = cov


# ---------------------------------------------------------------------------------- pre-pass

PRE_EDGES = (255, 256, 257, 513)
PRE_LIVE = ((), (63,), (63, 64), (255, 256), (0, 64), (62, 63, 64, 65, 255, 256), (60, 61, 62, 63),
            (61, 62, 63, 64, 65), (254, 255), (256,), (511, 512))  # flattened positions of the live writers
PRE_READS = (63, 64, 65, 129)


def prepass_steps(p):
    """k_resolve_pre walks a transaction's reads 64 at a time and their flattened edges 256 (4 x 64
    lanes) at a time.  The dead pool: 520 single-key writers, two keys apart, decided before the rounds
    by a history conflict (a TooOld transaction's ranges are never registered), so that a read over n
    of them holds exactly n write-begins (direct edges whatever the group setting) and the flattened
    position of every later read's edge is known."""
    n_pool = 520
    dbase = p.block(2 * n_pool + 2)
    s0 = p.key()
    live_keys = [p.key() for _ in range(6)]
    dkey = p.key()
    body = [txn(writes=[wr("same", s0)], tag="S")]
    body += [p.dead(2 * i, [(dbase + 2 * i + 1, dbase + 2 * i + 2)]) for i in range(n_pool)]
    body += [txn([rd("same", s0)], [wr(GEOMS[i % 3], k)], report=True, tag="A") for i, k in enumerate(live_keys)]
    body.append(txn(writes=[wr("inside", dkey)], tag="D"))
    want = {}

    def reader(blocks, n_reads, commit_last, tail):
        """blocks: ("dead", n) or ("live",) in flattened order; padded with reads nothing meets up to
        n_reads; tail: one more live edge as the transaction's last read."""
        reads, cur, li = [], 0, 0
        n_live = sum(1 for b in blocks if b[0] == "live") + (1 if tail else 0)

        def live_read():
            nonlocal li
            li += 1
            if li == n_live and commit_last:
                return rd("inside", dkey)
            return rd(GEOMS[(li - 1) % 3], live_keys[li - 1])

        for b in blocks:
            if b[0] == "dead":
                reads.append((dbase + 2 * cur, dbase + 2 * (cur + b[1])))
                cur += b[1]
            else:
                reads.append(live_read())
        while len(reads) < n_reads - (1 if tail else 0):
            k = p.block(2)
            reads.append((k, k + 1))
        if tail:
            reads.append(live_read())
        assert len(reads) == n_reads and cur <= n_pool
        return txn(reads, report=True, tag="X")

    k = 0
    for E in PRE_EDGES:
        for live in PRE_LIVE:
            if live and live[-1] >= E:
                continue
            blocks, pos = [], 0
            for lp in live:
                if lp > pos:
                    blocks.append(("dead", lp - pos))
                blocks.append(("live",))
                pos = lp + 1
            if E > pos:
                blocks.append(("dead", E - pos))
            n_reads = PRE_READS[k % 4]
            tail = n_reads > 64 and len(live) < 6 and k % 2 == 0
            want[len(body)] = (n_reads, E, live, len(live) + tail)
            body.append(reader(blocks, n_reads, k % 3 == 0, tail))
            k += 1
    for n_reads in PRE_READS:  # one edge per read: the flattened position is the read's index in its chunk
        for live in ((), (62,), (63,), (62, 63, 64), (0, 63, 64, 65, 127, 128)):
            live = tuple(x for x in live if x < n_reads)
            blocks = [("live",) if i in live else ("dead", 1) for i in range(n_reads)]
            want[len(body)] = (n_reads, min(64, n_reads), tuple(x for x in live if x < 64), len(live))
            body.append(reader(blocks, n_reads, k % 3 == 0, False))
            k += 1
    tb, res = p.emit("prepass", body, shares=(0.02, 0.3))
    f, A = res.facts, res.admitted
    cov = {"reads": set(), "chunk_edges": set(), "live": set(), "live_positions": set()}
    for t, (n_reads, E, live, n_live) in want.items():
        r0 = A.roff[t]
        assert A.roff[t + 1] - r0 == n_reads and f.exact[t] and f.n_live[t] == n_live
        sl = f.slots[r0:r0 + min(64, n_reads)]
        assert sl.sum() == E, (t, sl.sum(), E)  # candidate edges inside the first 64-read chunk
        start = np.cumsum(sl) - sl
        got = tuple(int(start[i]) for i in range(len(sl)) if f.cand[r0 + i] is not None and
                    (~f.dead[f.cand[r0 + i]]).any())
        assert got == live, (t, got, live)  # the flattened positions of the live writers
        cov["reads"].add(n_reads)
        cov["chunk_edges"].add(E)
        cov["live"].add(n_live)
        cov["live_positions"] |= set(live)
    assert cov["reads"] == set(PRE_READS) and set(PRE_EDGES) <= cov["chunk_edges"]
    assert set(range(7)) <= cov["live"] and {63, 64, 255, 256} <= cov["live_positions"]
    p.coverage["prepass"] = {k: sorted(v) for k, v in cov.items()}


# ---------------------------------------------------------------------------------- edge fill


def fill_steps(p):
    """k_edge_fill: kFillPairs = 1024 pairs per workgroup step, four pairs per thread (pair q of a step
    is lane (q / 4) % 64 of its wave), one slot atomic per run of lanes filing under the same read, runs
    broken by filtered pairs.  Every pair here is a write-begin strictly inside a read, so P is the
    same with write groups on and off."""
    cov = {}
    # a read over 1023 .. 4100 write-begins; among them later writers, the reader's own write and
    # empty writes at lane 0, lane 63 and mid-wave of the first reader's pairs (which start at pair 0)
    sizes = (1023, 1024, 1025, 2049, 4100)
    base = p.block(2 * 4100 + 2)
    key = lambda i: base + 2 * i + 1
    special = {0: "late", 122: "own", 253: "empty", 256: "late", 511: "empty", 1022: "late", 1024: "empty", 2048: "own"}
    owner = {122: 1023, 2048: 2049}  # the reader that writes the slot
    early = [txn(writes=[(key(i), key(i) + (0 if special.get(i) == "empty" else 1))])
             for i in range(4100) if special.get(i) in (None, "empty")]
    readers = [txn([(base, base + 2 * n)], [(key(q), key(q) + 1) for q in owner if owner[q] == n], report=True, tag="X")
               for n in sizes]
    late = [txn(writes=[(key(q), key(q) + 1)]) for q, s in special.items() if s == "late"]
    tb, res = p.emit("fill-wide", early + readers + late, shares=(0.9, 1e-4))
    f, A = res.facts, res.admitted
    assert f.P == f.P_grouped == sum(sizes) and f.slots.tolist() == list(sizes)
    r = 0  # the first read: its k-th pair is the k-th write-begin inside it, in key order
    assert A.rt[r] == len(early)
    inside = np.sort(A.wa[(A.wa > A.ra[r]) & (A.wa < A.re[r])])
    assert len(inside) == 1023
    by_key = {int(a): (int(b) > int(a), int(t)) for a, b, t in zip(A.wa, A.we, A.wt)}
    ok = np.array([by_key[int(a)][0] and by_key[int(a)][1] < A.rt[r] for a in inside])
    lanes = {(q // 4) % 64 for q in np.flatnonzero(~ok).tolist()}
    assert {0, 63} <= lanes and any(0 < x < 63 for x in lanes) and len(f.cand[r]) == ok.sum()
    assert (res.verdicts[[len(early) + i for i in range(len(sizes))]] == K.CONFLICT).all()
    cov["wide"] = dict(reads=list(sizes), P=f.P, filtered_lanes=sorted(lanes))
    # a workgroup step made of 1024 ranges with one pair each (1100 reads over one write-begin each)
    keys = [p.key() for _ in range(1100)]
    body = [txn(writes=[wr("inside", k)]) for k in keys[::2]]
    body += [txn([rd("inside", k) for k in keys[100 * i:100 * (i + 1)]], report=True) for i in range(11)]
    body += [txn(writes=[wr("inside", k)]) for k in keys[1::2]]  # later writers: filtered pairs
    tb, res = p.emit("fill-one-pair-each", body, shares=(0.9, 1e-4))
    assert res.facts.P == res.facts.P_grouped == 1100 and (res.facts.slots == 1).all()
    cov["one_pair_each"] = dict(ranges=1100, P=res.facts.P)
    # P = 2 * 1024 - 1, 2 * 1024 and 2 * 1024 + 1: the last step holds 1023, 1024 pairs, or one
    for n in (2047, 2048, 2049):
        b2 = p.block(2 * n + 2)
        body = [txn(writes=[(b2 + 2 * i + 1, b2 + 2 * i + 2)]) for i in range(n)]
        body.insert(n // 2, txn([(b2, b2 + 2 * n)], report=True))  # half of the writers come later
        body.append(txn([(b2, b2 + 2 * n)], report=True))
        tb, res = p.emit(f"fill-P{2 * n}", body, shares=(0.9, 1e-4))
        assert res.facts.P == res.facts.P_grouped == 2 * n
    for n, extra in ((2047, 0), (2048, 0), (2048, 1)):
        b2 = p.block(2 * 2049 + 2)
        body = [txn(writes=[(b2 + 2 * i + 1, b2 + 2 * i + 2)]) for i in range(n + extra)]
        body.append(txn([(b2, b2 + 2 * n)] + ([(b2 + 2 * n, b2 + 2 * n + 2)] if extra else []), report=True))
        tb, res = p.emit(f"fill-P{n + extra}", body, shares=(0.9, 1e-4))
        assert res.facts.P == res.facts.P_grouped == n + extra
    cov["P"] = [2047, 2048, 2049, 4094, 4096, 4098]
    # 270 reads over 270 write-begins each: P = 72900 > 64 workgroups x 1024 pairs from G = 540 < 1024
    # ranges, so k_edge_fill's grid-stride loop takes a second trip
    b2 = p.block(2 * 270 + 2)
    body = [txn(writes=[(b2 + 2 * i + 1, b2 + 2 * i + 2)]) for i in range(270)]
    body.append(txn([(b2, b2 + 2 * 270)] * 270, report=True))
    tb, res = p.emit("fill-second-trip", body, shares=(0.9, 1e-4))
    f = res.facts
    assert f.P == f.P_grouped == 72900 > 65536 and len(res.admitted.ra) + len(res.admitted.wa) == 540
    cov["second_trip"] = dict(P=f.P, G=540)
    p.coverage["fill"] = cov


# ---------------------------------------------------------------------------------- sizes


def fan(p, slots, S, n1, n2, poisoned=0):
    """One read and one write per transaction, so G = 2T ranges and 2T write endpoints.  S sources
    (each reads a key nobody writes), n1 transactions that read a source's key (live candidate: they
    abort in the rounds), n2 that read one of those transactions' keys (they commit in the rounds):
    U = n1 + n2 exactly.  poisoned: that many of the sources read a poison key at DEAD_SNAP instead."""
    T = S + n1 + n2
    assert n2 <= n1 and T <= len(slots) and (n1 == 0 or S > 0)
    body, src, free = [], [], iter(slots)

    def sources(upto):
        while len(src) < upto:
            k = next(free)
            if len(src) < poisoned:
                body.append(p.dead(2 * len(src), [wr(GEOMS[len(src) % 3], k)], tag="P"))
            else:
                body.append(txn([(k + 1, k + 2)], [wr(GEOMS[len(src) % 3], k)], report=len(body) % 16 == 0, tag="S"))
            src.append(k)

    for i in range(n1):
        s = i * S // n1
        sources(s + 1)
        k1 = next(free)
        body.append(txn([rd(GEOMS[s % 3], src[s])], [wr(GEOMS[i % 3], k1)], report=len(body) % 16 == 0, tag="L1"))
        if i < n2:
            body.append(txn([rd(GEOMS[i % 3], k1)], [wr("same", next(free))], report=len(body) % 16 == 0, tag="L2"))
    sources(S)
    assert len(body) == T
    return body


SIZES = (  # name, S, n1, n2, poisoned: T = S + n1 + n2, U = n1 + n2
    ("T5120", 120, 2500, 2500, 0), ("T5121", 121, 2500, 2500, 0),
    ("T8400-U8192", 208, 4096, 4096, 0), ("T8401-U8193", 208, 4097, 4096, 0),
    ("T16384", 8384, 5000, 3000, 0), ("T16385", 8385, 5000, 3000, 0),
    ("T16600-U8100", 8500, 5100, 3000, 0), ("T16600-U16000", 600, 8000, 8000, 0),
    ("T16600-no-edges", 16600, 0, 0, 5600),
)


def size_steps(p):
    slots = [p.key() for _ in range(16600)]
    cov = {}
    for name, S, n1, n2, poisoned in SIZES:
        tb, res = p.emit("size-" + name, fan(p, slots, S, n1, n2, poisoned))
        f, A = res.facts, res.admitted
        T = S + n1 + n2
        assert A.T == T and len(A.ra) == T and len(A.wa) == T and f.U == n1 + n2
        assert (f.n_slots > 0) == (n1 > 0)
        cov[name] = dict(T=T, U=f.U, G=2 * T, write_endpoints=2 * T, slots=f.n_slots, groups_on=T <= 12288)
    assert cov["T5120"]["U"] >= 5000 and cov["T8400-U8192"]["U"] == 8192 and cov["T8401-U8193"]["U"] == 8193
    assert cov["T16600-U8100"]["U"] <= 8192 < cov["T16600-U16000"]["U"] and cov["T16600-U8100"]["G"] > 32768
    assert cov["T16600-no-edges"]["slots"] == 0
    p.coverage["sizes"] = cov


FAMILIES = {"core": (ladder_steps, group_steps, prepass_steps), "fill": (fill_steps,), "sizes": (size_steps,)}


def build(kind, seed=1, shape="random16"):
    """The plan of one kind: "core" (ladders, groups, pre-pass: the families run again under every
    knob), "fill" (edge fill) or "sizes".  Every batch of a plan with candidate slots has an undecided
    transaction and the other way round, so the engine's round counter, which counts the round that
    finds nothing left to decide, is > 0 exactly when the model's U is."""
    p = Plan(seed, shape)
    for fam in FAMILIES[kind]:
        fam(p)
    for s in p.steps:
        assert (s.U > 0) == (s.slots > 0), s.name
    return p
