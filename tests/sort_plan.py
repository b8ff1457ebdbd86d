"""The directed batches of tests/test_gpu_sort_model.py: D.Sort (k_sample, k_quant_cold,
k_sort_partition, k_sort_bucket<LONG> in foundationdb_amd/csrc/kernels.hip) held to the key-space model
(tests/keyspace_model.py).  Built on the CPU from the model alone; every position, run length, bucket
size and common-prefix length a family is meant to reach is asserted here while the plan is built, and
the engine is never consulted for it.

The probe.  A step has a chain of sorted distinct keys k0 < k1 < ... < kn.  Its batch holds one reader
transaction per gap [k_i, k_i+1) and, earlier in the batch, one writer transaction (one write, no
reads) per gap of one parity; the step is built in both parities.  Readers of written gaps conflict,
the others commit, writers commit: 1/3 and 2/3 of the batch.  The history is loaded below every
snapshot, so nothing conflicts with it and every verdict is the intra-batch check's, which reads
nothing but the order D.Sort gave the batch's endpoints (erec: the position and the class counts
before it; wbrange / rbrange).  Extras beside the chain: second readers of a gap, empty reads and
writes [k, k), reads over two or three gaps, transactions of several reads (report entries), and the
"raw" ranges of the pair families, whose keys are no chain keys.

Why a wrong order cannot pass.  prove() re-resolves every step, in its own universe
(K.var_universe of the step's keys), with one endpoint index of one range moved by one
(K.resolve_moved), and asserts that each of the two moves of every endpoint at a directed key changes
a verdict, a report or the run-length state in at least one parity.  Exempt, and listed per step: the
extras, the endpoints whose neighbour key in the direction of the move is no chain key (the pair
families' outward moves, the ends of the chain) and empty ranges, which no move changes.

Where an endpoint stands.  With FDBCS_SORT_BUCKET at or above E there is one bucket, no splitter and
c = 0: a position in the wave, or in the workgroup path, is the position in the model's total order
(key, class, endpoint id), computed here.  For several buckets only integer arithmetic is restated:
sample rank -> quantile (q + 1) S / (kQuant + 1), quantile -> splitter (split_index), sorted position
-> quantile (quant_pos, put_quantiles), and the projection order (the 64-byte zero-padded window,
min(len, 65), class and id when both keys fit the window); from them the buckets, their sizes, the
bytes c their bounding splitters share and the runs of keys tied on the 19 bytes after c.  The one
counter the device has for it, stats()["sort_big_buckets"], is held to the plan's count of buckets
over 256 endpoints, batch by batch."""
import bisect
from types import SimpleNamespace

import numpy as np

from tests import keyspace_model as K

HEADER, OLDEST, FIRST_NOW = 1050, 1000, 2000
HIST = ((b"\xff\xff\xfd", 1100), (b"\xff\xff\xfe", 1200))  # in no batch; below every snapshot
RE, WE, WB, RB = 0, 1, 2, 3  # the class order at one key: ReadEnd < WriteEnd < WriteBegin < ReadBegin
NX = 19  # kSortNxLen: the bytes the sort words hold
SLAB = 256  # kSlab: endpoints one wave sorts
QW_BYTES = 112  # 16 + 8 kQW: the longest key whose tail words the tie rankings hold
QUANT, QUANT_MIN_E, MAX_SAMPLE, WINDOW, TARGET = 4096, 2048, 8192, 64, 64
ONE_BUCKET = 1 << 20
# key bytes after the 19 the sort words hold: the last one decides; from byte 16 these are tails of
# 4, 7 .. 12 and 95 .. 100 bytes (whole tail words at 8 and 96, kQW = 12 words)
XLENS = (1, 4, 5, 6, 7, 8, 9, 92, 93, 94, 95, 96, 97)
RUN_KEYS = (2, 3, 15, 16, 17, 18, 40)  # distinct keys of a run
RUN_ENDPOINTS = (2, 3, 15, 16, 17, 18)  # endpoints of a run (the simple ranking takes up to 16)
SIZES = (2, 62, 64, 126, 128, 254, 256, 258, 260, 512, 514, 1026)  # endpoints of a batch: always even
COLD_C = (1, 7, 8, 9, 15, 16, 17, 24, 45)


def txn(reads=(), writes=(), report=False, extra=False):
    return SimpleNamespace(reads=list(reads), writes=list(writes), report=report, extra=extra)


class Step:
    """A chain and its extras.  dups: gaps with a second reader; empty_r / empty_w: chain keys with an
    empty read / write; wide: (gap, span) reads over `span` gaps; multi: lists of gaps read by one
    transaction; raw(parity) -> (transactions before the readers, after them) on keys of their own;
    directed: the keys whose endpoints prove() moves (None: every chain key but the first and last)."""

    def __init__(self, name, chain, directed=None, dups=(), empty_r=(), empty_w=(), wide=(), multi=(), raw=None,
                 raw_keys=(), seed=0):
        assert list(chain) == sorted(set(chain)), name
        self.name, self.chain = name, list(chain)
        self.directed = set(self.chain[1:-1] if directed is None else directed)
        self.dups, self.empty_r, self.empty_w, self.wide, self.multi = dups, empty_r, empty_w, wide, multi
        self.raw, self.raw_keys, self.seed = raw, list(raw_keys), seed

    def keys(self):
        return set(self.chain) | set(self.raw_keys)

    def txns(self, parity):
        ks, G = self.chain, len(self.chain) - 1
        rng = np.random.default_rng(1000 + self.seed + parity)
        pre = [txn(writes=[(ks[i], ks[i + 1])]) for i in range(G) if i % 2 == parity]
        pre += [txn(writes=[(ks[i], ks[i])], extra=True) for i in self.empty_w]
        post = [txn([(ks[i], ks[i + 1])], report=i % 3 == 0) for i in range(G)]
        post += [txn([(ks[i], ks[i + 1])], report=True, extra=True) for i in self.dups]
        post += [txn([(ks[i], ks[i + n])], report=True, extra=True) for i, n in self.wide]
        post += [txn([(ks[i], ks[i + 1]) for i in gaps], report=True, extra=True) for gaps in self.multi]
        post += [txn([(ks[i], ks[i])], report=True, extra=True) for i in self.empty_r]
        rpre, rpost = self.raw(parity) if self.raw else ([], [])
        pre, post = pre + rpre, post + rpost
        # endpoint ids in no key order: equal (key, class) ties are decided by the id
        return [pre[i] for i in rng.permutation(len(pre))] + [post[i] for i in rng.permutation(len(post))]


def to_batch(txns, index, snap):
    tb = K.TxnBatch()
    for x in txns:
        tb.add([(index[a], index[b]) for a, b in x.reads], [(index[a], index[b]) for a, b in x.writes], snap,
               x.report, x)
    return tb


# ---------------------------------------------------------------------------------- the order and the buckets


def endpoint_table(A, ukeys):
    """Key and class of every endpoint id p = 2 range + is_end (reads first, as the engine numbers them)."""
    R, W = len(A.ra), len(A.wa)
    idx = np.concatenate([np.stack([A.ra, A.re], 1).ravel(), np.stack([A.wa, A.we], 1).ravel()]).tolist()
    return [ukeys[i] for i in idx], [RB, RE] * R + [WB, WE] * W


def total_order(key, cls):
    return sorted(range(len(key)), key=lambda p: (key[p], cls[p], p))


def projection(k, c, p):
    """The splitter an endpoint projects to, as a tuple that compares as split_cmp_rest does."""
    fits = len(k) <= WINDOW
    return (k[:WINDOW].ljust(WINDOW, b"\0"), min(len(k), WINDOW + 1), c if fits else -1, p if fits else -1)


def split_index(k, nb):
    return ((k + 1) * QUANT) // nb


def cold_table(key, cls, nb):
    """k_sample / k_quant_cold: the quantile table from the batch's own samples, ranked among themselves."""
    E = len(key)
    S = min(E, min(MAX_SAMPLE, max(1024, 4 * nb)))
    ids = [(i * E) // S for i in range(S)]
    assert len(set(ids)) == S
    ranked = sorted(ids, key=lambda p: (key[p], cls[p], p))
    tied = sum(1 for a, b in zip(ranked, ranked[1:]) if min(len(key[a]), len(key[b])) > NX and key[a][:NX] == key[b][:NX])
    return [ranked[((q + 1) * S) // (QUANT + 1)] for q in range(QUANT)], S, tied


def warm_table(order):
    """put_quantiles: entry q is the endpoint at sorted position (q + 1) E / (kQuant + 1); every entry is
    written whatever E is, several per position when E < kQuant."""
    E = len(order)
    return [order[((q + 1) * E) // (QUANT + 1)] for q in range(QUANT)]


def layout(key, cls, order, splitters, long_keys):
    """Buckets of the sorted endpoints between the splitters ((key, class, id) triples) and each
    interior bucket's c (split_lcp: the bytes the zero-padded windows of its bounding splitters share,
    at most either's length; 0 for the end buckets and for batches of keys up to 19 bytes)."""
    sp = [projection(*s) for s in splitters]
    assert sp == sorted(sp)
    nb = len(sp) + 1
    buckets = [[] for _ in range(nb)]
    for p in order:
        buckets[bisect.bisect_right(sp, projection(key[p], cls[p], p))].append(p)
    cs, clamped = [0] * nb, [False] * nb
    for bk in range(1, nb - 1):
        if long_keys:
            (a, la), (b, lb) = ((sp[i][0], len(splitters[i][0])) for i in (bk - 1, bk))
            c = next((i for i in range(WINDOW) if a[i] != b[i]), WINDOW)
            cs[bk], clamped[bk] = min(c, la, lb), c > min(la, lb)
    return buckets, cs, clamped


def bucket_runs(eps, c, key):
    """Maximal runs of positions of one sorted bucket whose keys are longer than c + 19 bytes and equal
    on bytes [c, c + 19): what the wave's tie ranking orders by the tails.  (start, end) inclusive."""
    tk = [key[p][c:c + NX] if len(key[p]) - c > NX else None for p in eps]
    runs, st = [], None
    for i in range(len(eps)):
        tied = i + 1 < len(eps) and tk[i] is not None and tk[i] == tk[i + 1]
        if tied and st is None:
            st = i
        if not tied and st is not None:
            runs.append((st, i))
            st = None
    return runs


def run_path(eps, st, en, key):
    """Which ranking k_sort_bucket gives the run: "pair" (the two ends of one range, left as the
    range-end flag sorted them), "simple" (inside one 64-position slot, at most 16 long, every key's
    tail words held: in-slot shuffles), "pfall" (such a run with a key past 112 bytes: the slow path
    after all), "slow" (crossing a slot or longer than 16), "mlong" (slow, with a key past 112 bytes)."""
    long_member = any(len(key[p]) > QW_BYTES for p in eps[st:en + 1])
    if en == st + 1 and eps[st] >> 1 == eps[en] >> 1:
        return "pair"
    if st // 64 == en // 64 and en - st < 16:
        return "pfall" if long_member else "simple"
    return "mlong" if long_member else "slow"


def sort_facts(A, ukeys, target, table, cold):
    """Everything the plan asserts about where a batch's endpoints stand.  table: the quantile table the
    batch finds (None: none yet); cold: FDBCS_SORT_COLD.  Returns the facts and the table it leaves."""
    key, cls = endpoint_table(A, ukeys)
    E = len(key)
    order = total_order(key, cls)
    long_keys = max(len(k) for k in key) > NX
    nb = max(1, -(-E // target))
    assert nb <= 257  # the slab of the smallest workspace holds as many buckets
    f = SimpleNamespace(E=E, nb=nb, long_keys=long_keys, samples=0, sample_ties=0, tokens=set())
    table_in = table
    if nb > 1 and (cold or table is None):
        ids, f.samples, f.sample_ties = cold_table(key, cls, nb)
        table = [(key[p], cls[p], p) for p in ids]
    splitters = [table[split_index(k, nb)] for k in range(nb - 1)]
    buckets, cs, clamped = layout(key, cls, order, splitters, long_keys)
    f.sizes = [len(b) for b in buckets]
    f.big = sum(n > SLAB for n in f.sizes)
    f.cs = sorted({c for b, c in zip(buckets, cs) if 0 < len(b) <= SLAB})
    f.clamped = sorted({c for b, c, x in zip(buckets, cs, clamped) if x and 0 < len(b) <= SLAB})
    f.runs = []  # (bucket, c, start, end, path, distinct keys)
    split16 = {s[0][:16].ljust(16, b"\0") for s in splitters}
    f.tie16 = {cls[p] for p in order if key[p][:16].ljust(16, b"\0") in split16}
    for bk, (eps, c) in enumerate(zip(buckets, cs)):
        assert all(key[p][:c] == key[eps[0]][:c] for p in eps)  # every key of a bucket shares its c bytes
        f.tokens |= {("len-c", len(key[p]) - c) for p in eps if c and 0 <= len(key[p]) - c <= NX + 1}
        if len(eps) > SLAB or not long_keys:
            continue
        for st, en in bucket_runs(eps, c, key):
            f.runs.append((bk, c, st, en, run_path(eps, st, en, key), len({key[p] for p in eps[st:en + 1]})))
    # a batch of at least kQuantMinE endpoints leaves its quantiles; any other leaves the table alone
    return f, ([(key[p], cls[p], p) for p in warm_table(order)] if E >= QUANT_MIN_E else table_in)


# ---------------------------------------------------------------------------------- the move-by-one proof


def prove(step):
    """Each of the two moves of every endpoint at a directed key changes a verdict, a report or the
    state in at least one parity.  An endpoint moves over the chain's keys and the directed ones; of
    the raw families (the pairs) only the inward moves are held, begin + 1 and end - 1: what the two
    ends of a range come to when their order is wrong.  Returns (endpoints proved, the exempt moves by
    reason, the verdicts of the two parities in the step's own universe)."""
    ukeys = sorted(step.keys())
    uni = K.var_universe(ukeys)
    index = {k: i for i, k in enumerate(ukeys)}
    chain = set(step.chain)
    movable = chain | step.directed
    flips, exempt, verdicts = {}, {"extra": 0, "edge": 0, "empty": 0, "outward": 0}, []
    for parity in (0, 1):
        pristine, model = K.KeyspaceModel(uni, HEADER), K.KeyspaceModel(uni, HEADER)
        tb = to_batch(step.txns(parity), index, FIRST_NOW - 1)
        A = tb.arrays()
        res = K.resolve(model, A, FIRST_NOW, OLDEST, facts=False)
        base = K.outcome(model, res)
        verdicts.append(res.verdicts)
        seen = {}
        for which in K.ENDS:
            idx, owner = getattr(A, which), (A.rt if which[0] == "r" else A.wt)
            other = getattr(A, {"ra": "re", "re": "ra", "wa": "we", "we": "wa"}[which])
            for r in range(len(idx)):
                k = ukeys[idx[r]]
                if k not in step.directed:
                    continue
                if tb.tag[owner[r]].extra or idx[r] == other[r]:
                    exempt["extra" if tb.tag[owner[r]].extra else "empty"] += 1
                    continue
                ident = (which, k, ukeys[other[r]])
                n = seen[ident] = seen.get(ident, -1) + 1
                for d in (-1, 1):
                    j = idx[r] + d
                    if k not in chain and d != (1 if which[1] == "a" else -1):
                        exempt["outward"] += 1
                    elif not 0 <= j < len(ukeys) or ukeys[j] not in movable:
                        exempt["edge"] += 1
                    else:
                        m, moved = K.resolve_moved(pristine, A, FIRST_NOW, OLDEST, which, r, d)
                        flips.setdefault((ident, n, d), False)
                        flips[ident, n, d] |= K.outcome(m, moved) != base
    missing = [x for x, hit in flips.items() if not hit]
    assert not missing, (step.name, len(missing), missing[:5])
    return len(flips), exempt, verdicts


# ---------------------------------------------------------------------------------- the plan


class Plan:
    """The steps of one engine configuration, resolved in order on one model over every step's keys."""

    def __init__(self, name, steps, target=ONE_BUCKET, cold=False):
        self.name, self.target, self.cold, self.steps = name, target, cold, steps
        self.env = {"FDBCS_SORT_BUCKET": str(target)}
        if cold:
            self.env["FDBCS_SORT_COLD"] = "1"
        keys = set().union(*(s.keys() for s in steps)) | {k for k, _ in HIST}
        self.model = K.KeyspaceModel(K.var_universe(keys), HEADER)
        self.ukeys = K.split_keys(self.model.kb, self.model.ko)
        self.index = {k: i for i, k in enumerate(self.ukeys)}
        hist = np.array([self.index[k] for k, _ in HIST])
        self.model.load(hist, [v for _, v in HIST])
        self.loaded = (*self.model.pack_keys(hist), np.array([v for _, v in HIST], np.int64), HEADER)
        self.batches, self.tokens, self.proved, self.exempt = [], set(), {}, {}
        now, table = FIRST_NOW, None
        for s in steps:
            verdicts = []
            for parity in (0, 1):
                txns = s.txns(parity)
                tb = to_batch(txns, self.index, now - 1)
                res = K.resolve(self.model, tb, now, OLDEST)
                v = res.verdicts
                # readers of written gaps conflict, the others commit, writers commit
                gap = {(a, b): i for i, (a, b) in enumerate(zip(s.chain, s.chain[1:]))}
                for t, x in enumerate(txns):
                    if len(x.reads) == 1 and not x.writes and x.reads[0] in gap:
                        assert (v[t] == K.CONFLICT) == (gap[x.reads[0]] % 2 == parity), (s.name, parity, t)
                    if x.writes and not x.reads:
                        assert v[t] == K.COMMITTED
                f, table = sort_facts(res.admitted, self.ukeys, target, table, cold)
                self.batches.append(SimpleNamespace(
                    name=f"{s.name}/{parity}", step=s.name, pb=tb.pack(self.model), now=now, want=v,
                    reports=res.reports, state=self.model.rle(), T=len(tb), slots=res.facts.n_slots, facts=f,
                    big=f.big, arrays=res.admitted))
                verdicts.append(v)
                now += 10
            v = np.concatenate(verdicts)  # a degenerate step cannot pass
            s.shares = ((v == K.CONFLICT).mean(), (v == K.COMMITTED).mean())
            assert min(s.shares) >= 0.3, (s.name, s.shares)

    def prove(self):
        """prove() of every step with directed keys; the step's verdicts in its own universe are those
        of the plan's (one model over every step's keys, the earlier steps' writes below every snapshot)."""
        for s in self.steps:
            if s.directed:
                self.proved[s.name], self.exempt[s.name], verdicts = prove(s)
                want = [b.want for b in self.batches if b.step == s.name]
                assert all((x == y).all() for x, y in zip(verdicts, want)), s.name
        return self.proved


# ---------------------------------------------------------------------------------- keys


def filler(rng, lead, n, lens):
    """n random keys under `lead` whose first 19 bytes differ, of the lengths `lens` in turn."""
    out, heads = [], set()
    while len(out) < n:
        ln = lens[len(out) % len(lens)]
        k = lead + bytes(rng.integers(1, 255, size=max(ln, NX) - len(lead)).astype(np.uint8))
        k = k[:ln] if ln >= len(lead) + 4 else k
        if not any(k[:i] in heads for i in range(len(lead) + 4, NX + 1)) and k[:NX] not in heads:
            heads |= {k[:i] for i in range(len(lead) + 4, NX + 1)}
            out.append(k)
    return sorted(out)


LONG_LENS = (16, 17, 19, 20, 24, 33, 70)
SHORT_LENS = (5, 8, 12, 15, 16, 17, 18, 19)


def stem(i, j=0):
    """19 bytes: what the members of a run share."""
    return b"\x80" + bytes([i, j]) + b"0123456789abcdef"


def by_last(st, xl, d):
    """d keys: `st`, xl - 1 common bytes and a last byte that differs."""
    body = bytes((7 * t + 3) % 251 + 1 for t in range(xl - 1))
    return [st + body + bytes([16 + j]) for j in range(d)]


def fit(rng, fam, E, lens, lead=(b"\x20", b"\xc0"), low=None, ranges=0):
    """A chain around the family `fam` with an even number of gaps and `extra` second readers, so that
    the batch has exactly E endpoints in both parities: 3 per gap, 2 per second reader and 2 for each
    of the `ranges` other extras the step adds."""
    G = ((E - 2 * ranges) // 3) & ~1
    extra = (E - 2 * ranges - 3 * G) // 2
    n_fill = G + 1 - len(fam)
    assert n_fill >= 2 and extra <= 2, (E, len(fam))
    n_low = n_fill // 2 if low is None else low
    chain = filler(rng, lead[0], n_low, lens) + fam + filler(rng, lead[1], n_fill - n_low, lens)
    return chain, list(range(extra))


# ---------------------------------------------------------------------------------- one bucket


def pair_raw(parity):
    """The pair shortcut's placements on keys of their own, each family under one 19-byte stem between a
    short key p below it and q above it.  read pair: reader [a, b) alone in its run, under a writer
    [p, q) in parity 0; write pair: writer [a, b) in parity 0 under a reader [p, q); empty pair: the
    empty read and the empty write [k, k).  With a third tied endpoint beside it (a reader or writer
    that begins at c, in the same run) the run is no pair any more."""
    pre, post = [], []
    for n, (kind, third) in enumerate((k, t) for k in ("read", "write", "empty-r", "empty-w") for t in (False, True)):
        st = stem(200 + n)
        p, q = st[:10], st[:10] + b"\xff"
        a, b, c = st + b"\x31tail", st + b"\x32tail", st + b"\x33"
        if kind == "read":
            pre += [txn(writes=[(p, q)])] if parity == 0 else []
            post += [txn([(a, b)], report=True)] + ([txn([(c, q)], report=True)] if third else [])
        elif kind == "write":
            pre += [txn(writes=[(a, b)])] if parity == 0 else []
            pre += [txn(writes=[(c, q)])] if third and parity == 0 else []
            post += [txn([(p, q)], report=True)]
        else:
            e = txn([(a, a)], report=True) if kind == "empty-r" else txn(writes=[(a, a)])
            (post if kind == "empty-r" else pre).append(e)
            pre += [txn(writes=[(p, q)])]
            post += [txn([(c, q) if third else (p, q)], report=True)]
    return pre, post


def pair_keys():
    out = []
    for n in range(8):
        st = stem(200 + n)
        out += [st[:10], st[:10] + b"\xff", st + b"\x31tail", st + b"\x32tail"] + ([st + b"\x33"] if n % 2 else [])
    return out


def single_steps(long_keys):
    """The steps of the one-bucket plans.  long_keys False: the same shapes with every key at most 19
    bytes (k_sort_bucket<false>: no strip, no tie ranking)."""
    rng = np.random.default_rng(5 if long_keys else 6)
    lens = LONG_LENS if long_keys else SHORT_LENS
    steps = []
    if long_keys:
        fam = []
        for n, xl in enumerate(XLENS):
            fam += by_last(stem(1 + n), xl, 2)
        x = stem(40) + b"\x07"
        fam += [x, x + b"\0", x + b"\0\0"]  # length alone
        x = stem(41) + b"\x07\x08"
        fam += [x, x + b"\xff", stem(42) + b"\x55" * 30]  # a \xff extension; a key alone in its run
        fam += [stem(1), stem(40)]  # the 19 bytes themselves: before their run, by length alone
        fam.sort()
        chain = filler(rng, b"\x20", 3, lens) + fam + filler(rng, b"\xc0", 3, lens)
        steps.append(Step("tails", chain, fam, dups=[4, 5, 9, 10], empty_r=[6], empty_w=[7]))
        # runs of 1 .. 40 distinct keys; empty reads bring runs of 4 and 5 keys to 16 and 17 endpoints
        for name, spec in (("runs-a", ((1, 0), (2, 0), (3, 0), (5, 0), (4, 2), (5, 1), (6, 0))),
                           ("runs-b", ((15, 0), (16, 0), (17, 0))), ("runs-c", ((18, 0), (40, 0)))):
            fam, empties = [], []
            for n, (d, e) in enumerate(spec):
                mem = by_last(stem(50 + n, d), 3 + n, d)
                empties += mem[1:1 + e]
                fam += mem
            fam.sort()
            chain = filler(rng, b"\x20", 2, lens) + fam + filler(rng, b"\xc0", 2, lens)
            steps.append(Step(name, chain, fam, empty_r=[chain.index(k) for k in empties]))
        # a zero-padding ladder of 8 keys: 24 endpoints, past what the simple ranking takes, ordered by
        # length alone
        fam = [stem(43) + b"\x07" + b"\0" * k for k in range(8)]
        steps.append(Step("ladder", filler(rng, b"\x20", 2, lens) + fam + filler(rng, b"\xc0", 2, lens), fam))
        # two runs adjacent, differing in byte 18
        a, b = stem(60), stem(60)[:18] + b"g"
        fam = sorted(by_last(a, 5, 3) + by_last(b, 5, 3))
        steps.append(Step("adjacent", filler(rng, b"\x20", 2, lens) + fam + filler(rng, b"\xc0", 2, lens), fam))
        # keys of 112 | 113 and 200 bytes among shorter ones, in runs the simple ranking takes (up to 16
        # endpoints in one slot) and in longer ones
        def sized(st, sizes):
            return sorted(st + bytes([0x40 + n]) * (ln - NX) for n, ln in enumerate(sizes))
        fam = sized(stem(70), (40, 111, 112)) + sized(stem(71), (40, 112, 113, 200)) + \
            sized(stem(72), (21, 30, 64, 65, 100, 112, 110, 111)) + sized(stem(73), (20, 22, 113, 114, 200, 201, 300, 28))
        fam.sort()
        steps.append(Step("long", filler(rng, b"\x20", 1, lens) + fam + filler(rng, b"\xc0", 2, lens), fam))
        steps.append(Step("pairs", filler(rng, b"\x20", 9, lens), raw=pair_raw, raw_keys=pair_keys(),
                          directed=[k for k in pair_keys() if len(k) > NX]))
    else:
        S = b"\x50\x51\x52"
        fam = sorted({b"", b"\x01", b"\x60" * 15, b"\x60" * 16, b"\x60" * 17, b"\x60" * 18, b"\x60" * 19} |
                     {S + b"\0" * k for k in range(17)} | {b"\x70" * 16 + b"\0" * k for k in range(4)})
        ff = [b"\xff" * n for n in (16, 17, 18, 19)]
        steps.append(Step("lengths", fam + filler(rng, b"\xc0", 2, lens) + ff, fam[1:] + ff[:-1], dups=[0, 1, 20, 21]))
    # a run (long keys) or a zero-padding ladder (short ones) at every placement: filler below it from
    # none to 70 keys, with and without filler above it, with and without an empty read shifting it
    def placed(n_low, n_high, shift):
        if long_keys:
            fam = by_last(stem(80, n_low), 6, 3)
        else:
            fam = [b"\x80" + bytes([n_low]) + b"\0" * k for k in range(3)]
        chain = filler(rng, b"\x20", n_low, lens) + fam + filler(rng, b"\xc0", n_high, lens)
        return Step(f"place-{n_low}-{n_high}-{shift}", chain, fam, empty_r=[n_low + 1] if shift else [])
    steps += [placed(n_low, n_high, shift) for n_low in range(0, 66) for n_high in (0, 2) for shift in (0, 1)]
    if long_keys:
        # a key of exactly 19 bytes and one longer key that begins with it, in the workgroup path, where
        # item_aux's capped length alone (19 | 20) puts the shorter first
        fam = [stem(95), stem(95) + b"tail"]
        chain, dups = fit(rng, fam, 300, lens)
        steps.append(Step("cap19", chain, fam, dups=dups))
    # sizes: the register widths S = 1 | 2 | 4 with and without padding lanes, and the workgroup path
    # with 2, 4, .. overflow items and one, two, three and five tiles
    for E in SIZES:
        if E == 2:
            fam = by_last(stem(90), 4, 2) if long_keys else [b"\xff" * 18, b"\xff" * 19]
            steps.append(Step("size-2", fam, fam))
            continue
        if long_keys:
            fam = sorted(by_last(stem(91, E % 251), 9, 3) + by_last(stem(92, E % 251), 97, 40 if E > 200 else 2))
            chain, dups = fit(rng, fam, E, lens, ranges=7 if E > 100 else 0)
        else:  # keys of sixteen to nineteen \xff bytes at the bucket's end, beside the padding lanes
            fam = [b"\xff" * n for n in (16, 17, 18, 19)]
            x = 7 if E > 100 else 0
            chain, dups = fit(rng, fam, E, lens, low=(((E - 2 * x) // 3) & ~1) + 1 - len(fam), ranges=x)
        steps.append(Step(f"size-{E}", chain, fam[:8], dups=dups, wide=[(1, 2), (4, 3)] if E > 100 else (),
                          multi=[[0, 3, 6], [2, 5]] if E > 100 else ()))
    return steps


def run_tokens(p, step=None):
    """Coverage of a plan, from its batches' facts: ("E", n), ("S", width), ("run-keys", d),
    ("run-endpoints", n), ("path", name), ("start", pos), ("end", pos), ("cross", pos), "ends-bucket",
    "adjacent", ("c", value), ("bucket", size), ("clamp", c)."""
    t = set()
    for b in p.batches:
        if step is not None and b.step != step:
            continue
        f = b.facts
        t |= f.tokens
        t.add(("E", f.E))
        t |= {("bucket", n) for n in f.sizes} | {("c", c) for c in f.cs} | {("clamp", c) for c in f.clamped}
        t |= {("S", 1 if n <= 64 else 2 if n <= 128 else 4) for n in f.sizes if 0 < n <= SLAB}
        t |= {("tiles", -(-n // 256)) for n in f.sizes if n > SLAB} | {("overflow", n - SLAB) for n in f.sizes if n > SLAB}
        for i, (bk, c, st, en, path, d) in enumerate(f.runs):
            t |= {("run-keys", d), ("run-endpoints", en - st + 1), ("path", path), ("start", st), ("end", en),
                  ("run-c", c, d)}
            t |= {("cross", x) for x in (63, 127, 191) if st <= x < en}
            if en == f.sizes[bk] - 1:
                t.add("ends-bucket")
            if i and f.runs[i - 1][0] == bk and f.runs[i - 1][3] + 1 == st:
                t.add("adjacent")
            if bk == 0 and f.nb > 1:
                t.add("run-in-first-bucket")
            if bk == f.nb - 1 and f.nb > 1:
                t.add("run-in-last-bucket")
    return t


def prune(steps, wanted, target=ONE_BUCKET, cold=False):
    """The placement candidates that add coverage, greedily (every other step stays): a candidate's
    tokens are its own two batches', whatever stands before it (one bucket, or cold splitters)."""
    kept, have = [], set()
    for s in steps:
        if s.name.startswith("place-"):
            if len(s.chain) < 7 * len(s.empty_r):  # (too few conflicts beside the empty read)
                continue
            new = (run_tokens(Plan("candidate", [s], target, cold)) & wanted) - have
            if not new:
                continue
            have |= new
        kept.append(s)
    return kept


PLACEMENTS = {("start", 0), ("start", 1), ("end", 62), ("end", 63), ("cross", 63), ("cross", 127), ("cross", 191),
              "ends-bucket"}


def build_single(long_keys=True):
    """One bucket, c = 0 (FDBCS_SORT_BUCKET at or above E): positions are the model's total order."""
    wanted = PLACEMENTS if long_keys else set()
    steps = prune(single_steps(long_keys), wanted)
    p = Plan("single-long" if long_keys else "single-short", steps)
    t = p.tokens = run_tokens(p)
    assert all(b.facts.nb == 1 and b.facts.long_keys == long_keys for b in p.batches)
    assert {("E", n) for n in SIZES} <= t and {("S", 1), ("S", 2), ("S", 4)} <= t
    assert {("tiles", n) for n in (2, 3, 5)} <= t and {("overflow", n) for n in (2, 4, 256, 258)} <= t
    assert sum(b.big for b in p.batches) == sum(b.facts.E > SLAB for b in p.batches) >= 8
    lens = {len(k) for s in steps for k in s.keys()}
    if long_keys:
        assert wanted <= t, wanted - t
        assert {("run-keys", d) for d in RUN_KEYS} <= t and {("run-endpoints", n) for n in RUN_ENDPOINTS} <= t
        assert {("path", x) for x in ("pair", "simple", "pfall", "slow", "mlong")} <= t and "adjacent" in t
        assert {NX + x for x in XLENS} | {112, 113, 200} <= lens
    else:
        assert not any(b.facts.runs for b in p.batches) and max(lens) == NX and {0, 1, 15, 16, 17, 18, 19} <= lens
    return p


# ---------------------------------------------------------------------------------- several buckets


def cold_steps(target):
    """Families whose members all differ at byte L behind a shared L-byte prefix, several buckets large:
    every interior bucket between two members has c = L whichever members became splitters.  Under each
    c: keys with len - c = 18 | 19 | 20, runs of 3 and 17 keys tied on the 19 bytes after c, the key
    exactly c long, and second readers at keys a splitter equals on 16 bytes."""
    rng = np.random.default_rng(target)
    steps = []
    n_mem = 120 if target == TARGET else 40
    def family(L, j17):
        P = (b"\x90" + bytes([L]) + b"PREFIXprefixPREFIXprefixPREFIXprefixPREFIXprefix")[:L]
        # the key exactly L long, and after it one that goes on with zero bytes: with more than `target`
        # endpoints at each, splitters fall on both, their zero-padded windows share more than L bytes,
        # and split_lcp's clamp to the shorter length gives the L
        special = [P, P + b"\0\0\0" + b"z" * 20]
        fam = list(special)
        rng = np.random.default_rng(100 * target + L)
        for j in range(1, n_mem + 1):
            head = P + bytes([j])
            rest = bytes(rng.integers(1, 255, size=40).astype(np.uint8))
            if j == j17:
                fam += by_last((head + rest)[:L + NX], 5, 17)
            elif j % 10 == 3:
                fam += by_last((head + rest)[:L + NX], 2 + j % 7, 3)  # a run of 3 under c = L
            else:
                fam.append((head + rest)[:L + (18, 19, 20, 1, 30)[j % 5]])
        fam = sorted(set(fam))
        chain = filler(rng, b"\x20", 2, LONG_LENS) + fam + filler(rng, b"\xc0", 2, LONG_LENS)
        assert chain[2:4] == special
        directed = fam if target != TARGET else [k for k in fam if len(k) > L + NX + 1][:24] + fam[:8]
        st = Step(f"c{L}", chain, directed, dups=[2] * target + list(range(5, len(chain) - 2, 9)), seed=L)
        assert 3 * len(chain) + 2 * len(st.dups) <= 1024
        return st

    for L in COLD_C:
        # at 64 endpoints a bucket the run of 17 keys (51 endpoints) is placed where no splitter falls
        # inside it in either parity: the first such place, by the restated ranks
        for j17 in range(17, 60):
            st = family(L, j17)
            if target != TARGET or all(("run-c", L, 17) in run_tokens(SimpleNamespace(batches=[b]))
                                       for b in Plan("candidate", [st], target, True).batches):
                break
        steps.append(st)
    # c = 64: keys equal on the whole window, of 65, 83 | 84 and 130 bytes; their projections tie, so
    # they fill one bucket, past 256 endpoints; the window itself (64 bytes) stands before them
    W = b"\xa0" + b"window-of-sixty-four-bytes/" * 3
    W = W[:WINDOW]
    fam = [W] + [W + bytes([1 + j]) + b"t" * ((65, 83, 84, 130)[j % 4] - WINDOW - 1) for j in range(92)]
    fam = sorted(set(fam))
    assert {len(k) for k in fam} == {64, 65, 83, 84, 130}
    chain = filler(rng, b"\x20", 6, LONG_LENS) + fam + filler(rng, b"\xc0", 6, LONG_LENS)
    # more than `target` endpoints at the window itself: a splitter falls among them, the next one is a
    # member's, and the bucket between them, the rest of the window's endpoints, has c = 64 = its key's length
    steps.append(Step("c64", chain, fam[:12] + fam[-4:], dups=[6] * (target + 2) + [5], seed=64))
    # a batch whose first and last buckets hold a run each
    a, b = by_last(stem(1), 8, 4), by_last(b"\xf0" + stem(2)[1:], 8, 4)
    chain = a + filler(rng, b"\x90", 60 if target == TARGET else 12, LONG_LENS) + b
    steps.append(Step("end-runs", chain, a[1:] + b[:-1], seed=7))
    return steps


def build_cold(target):
    """Several buckets from the batch's own samples (FDBCS_SORT_COLD=1, E <= 1024: every endpoint is a
    sample), target 64 or 8 endpoints a bucket."""
    p = Plan(f"cold-{target}", cold_steps(target), target, cold=True)
    t = p.tokens = run_tokens(p)
    for b in p.batches:
        assert b.facts.samples == b.facts.E <= 1024 and b.facts.nb == -(-b.facts.E // target) > 1, b.name
    want_c = set(COLD_C) | {WINDOW}
    assert {("clamp", c) for c in COLD_C} <= t, sorted(x for x in t if x[0] == "clamp")
    assert {("c", c) for c in want_c} <= t, sorted(x for x in t if x[0] == "c")
    assert {("len-c", n) for n in (0, 18, 19, 20)} <= t
    for c in COLD_C:
        # at 64 endpoints a bucket the runs of 3 and of 17 keys stand whole in a bucket with c = L; at 8
        # splitters fall inside them, and their parts are sorted with the strip reaching into the tails
        ts = run_tokens(p, f"c{c}")
        if target == TARGET:
            assert ("run-c", c, 3) in ts and ("run-c", c, 17) in ts, c
        else:
            assert any(x[0] == "run-c" and x[1] == c for x in ts) and ("path", "simple") in ts, c
            assert c > 40 or any(x[0] == "c" and x[1] > c + NX for x in ts), c
    assert sum(b.big for b in p.batches if b.step == "c64") == 2 and "run-in-first-bucket" in t and "run-in-last-bucket" in t
    assert set().union(*(b.facts.tie16 for b in p.batches)) == {RE, WE, WB, RB}
    assert {("path", x) for x in ("simple", "slow")} <= t
    return p


# E is even, so one bucket never holds an odd number of endpoints.  Two buckets do: with nb = 2 the
# one splitter is the sample of rank 2049 S / 4097 = S / 2, both buckets are end buckets (c = 0), and a
# position in either is the model's position less the first bucket's size.  target -> batch sizes.
HALVES = {1: (2,), 100: (126, 130), 200: (254, 258), 400: (510, 514), 800: (1022, 1026), 1600: (2050,)}
HALF_SIZES = (1, 63, 65, 127, 129, 255, 257, 511, 513)


def build_halves(target):
    """Batches of E endpoints in two buckets of E / 2: 1, 63 | 65, 127 | 129, 255 | 257, 511 | 513
    endpoints (a wave with one lane, padding lanes or none; one overflow item), and 2050 endpoints from
    1024 samples, two buckets of about 1025."""
    rng = np.random.default_rng(target)
    steps = []
    for E in HALVES[target]:
        if E == 2:
            fam = by_last(stem(90), 4, 2)
            steps.append(Step("half-2", fam, fam))
            continue
        # (keys within the 64-byte window: no two endpoints share a projection, so the halves are exact)
        fam = sorted(by_last(stem(91, E % 251), 9, 3) + by_last(stem(92, E % 251), 30, 40 if E > 200 else 2))
        chain, dups = fit(rng, fam, E, LONG_LENS)
        steps.append(Step(f"half-{E}", chain, fam[:8], dups=dups))
    p = Plan(f"halves-{target}", steps, target, cold=True)
    for b in p.batches:
        f = b.facts
        assert f.nb == 2 or (target == 1 and f.sizes == [1] * f.E), b.name
        if f.samples == f.E:
            assert f.sizes == [f.E // 2] * f.nb or target == 1, (b.name, f.sizes)
        else:
            assert f.samples == 1024 < f.E and min(f.sizes) > 0.45 * f.E, (b.name, f.sizes)
    p.tokens = run_tokens(p)
    assert {("bucket", E // 2) for E in HALVES[target] if E <= 1024} <= p.tokens
    return p


# ---------------------------------------------------------------------------------- warm splitters


def spread(rng, lead, n):
    return filler(rng, lead, n, LONG_LENS)


def build_warm():
    """The quantile table across batches (default target, splitters from the last batch of at least
    kQuantMinE = 2048 endpoints).  0: a cold batch of 9000 endpoints (1024 samples, tied long keys among
    them) that leaves a table; 1: a directed batch under it; 2: a batch of 2048 <= E < 4096 (several
    table entries per position; its first parity stands between two quantiles of batch 0's: one bucket
    of about 2700); 3: a batch that lands between two of its quantiles (one bucket past
    256); 4: a batch under 2048 endpoints, which must leave the table alone: its keys lie among those of
    5: a population wholly below the table's first splitter (one bucket of about 3000, the overflow path
    at size; it leaves a table of its own), and 6: one wholly above that table's last splitter."""
    rng = np.random.default_rng(11)
    run = by_last(stem(3), 9, 60)  # 180 endpoints tied on 19 bytes: about 20 of them are samples
    big0 = sorted(spread(rng, b"\x81", 1400) + spread(rng, b"\x85", 1536) + run)
    s0 = Step("cold-9000", big0, [], seed=1)
    d1 = sorted(by_last(b"\x81" + stem(4)[1:], 6, 5) + by_last(b"\x85" + stem(5)[1:], 97, 20) + spread(rng, b"\x83", 40))
    s1 = Step("under-9000", spread(rng, b"\x80\x10", 30) + d1 + spread(rng, b"\x86", 30), d1, seed=2)
    mid = sorted(spread(rng, b"\x82", 400) + spread(rng, b"\x84", 500))
    s2 = Step("warm-2700", mid, [], seed=3)
    # between two neighbouring keys of s2: every key shares their first bytes
    lo, hi = mid[449], mid[450]
    inner = sorted({lo + bytes([1 + j // 200, 1 + j % 200]) + b"x" * (j % 9) for j in range(130)})
    assert lo < inner[0] and inner[-1] < hi
    s3 = Step("between-quantiles", inner, inner[1:-1], seed=4)
    s4 = Step("small-among", spread(rng, b"\x30", 200), [], seed=5)
    low = sorted(spread(rng, b"\x30", 960) + by_last(b"\x30" + stem(6)[1:], 8, 40))
    s5 = Step("below-first", low, [], seed=6)
    high = sorted(spread(rng, b"\x98", 960) + by_last(b"\x98" + stem(7)[1:], 8, 40))
    s6 = Step("above-last", high, [], seed=7)
    p = Plan("warm", [s0, s1, s2, s3, s4, s5, s6], TARGET, cold=False)
    by = {}
    for b in p.batches:
        by.setdefault(b.step, []).append(b.facts)
    f = by["cold-9000"][0]
    assert f.E >= 8900 and f.samples == 1024 < f.E and f.sample_ties >= 5 and by["cold-9000"][1].samples == 0
    assert all(x.nb > 1 and x.big == 0 for x in by["under-9000"]) and {("path", "slow"), ("path", "simple")} <= run_tokens(p)
    assert all(QUANT_MIN_E <= x.E < QUANT for x in by["warm-2700"])
    assert all(x.big == 1 and max(x.sizes) == x.E > SLAB for x in by["between-quantiles"])
    assert all(x.E < QUANT_MIN_E and x.big == 1 and max(x.sizes) == x.E for x in by["small-among"])
    # (the second parity of a batch that leaves a table finds the first one's: spread over many buckets)
    assert all(x[0].big == 1 and max(x[0].sizes) == x[0].E > 2900 for x in (by["below-first"], by["above-last"]))
    assert all(x[1].big == 0 and x[1].nb > 40 for x in (by["below-first"], by["above-last"]))
    p.tokens = run_tokens(p)
    return p


BUILDERS = {"single-long": lambda: build_single(True), "single-short": lambda: build_single(False),
            "cold-64": lambda: build_cold(64), "cold-8": lambda: build_cold(8), "warm": build_warm}


def build(kind):
    return build_halves(int(kind[7:])) if kind.startswith("halves-") else BUILDERS[kind]()
