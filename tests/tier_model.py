"""The two tiers of the stored history as they are stored: plain Python over universe indices (the keys
of a tests/keyspace_model.KeyspaceModel universe).

KeyspaceModel keeps the step function a read sees; its run-length form is the *canonical* history.
What the engine stores is larger: an end boundary E that repeats the version before it, a hole, a
boundary below the floor that the GC has not met yet.  None of that shows in a verdict or a canonical
dump; it shows in history_size() and in the delta_sum / base_sum / segments_sum counters, and a
superfluous or a missing E is exactly what a wrong merge leaves.  TierSim restates four rules of
DESIGN.md (sections 4 and 5) and of the kernels' comments, and nothing else of the kernels:

  merge      for each union segment [B, E) of a batch's committed writes: delta boundaries in [B, E) go,
             B is stored at `now`, E is stored at the value that stood before it (HOLE if none) unless
             E is a delta boundary already or the next segment begins at E.
  compact    a versioned delta boundary j overwrites the base over [d_j, d_j+1) (to the end for the
             last one); a hole becomes a base boundary that carries the base's version there (the
             header below the first boundary) unless the base has that key.
  gc         a base boundary goes when it and its *source* predecessor (the header for the first) are
             both below the oldest version.
  policy     (engine.cpp, decide_y) a batch of W write ranges compacts when nd + 2 W exceeds the delta
             limit, or on the gc_interval cadence; the GC runs with every cadence compaction and with
             every GC_EVERY-th size-triggered one, and only if the oldest version moved past the last
             GC's.  (The tail-reclaim trigger is not modelled: plans that rely on sizes stay below it.)

Every merge and compaction also returns the facts a directed plan asserts its coverage on: per segment
lo, hi, exact, glue, endins and the inherited value; per copy tile the number of segments (delta
boundaries) whose lo falls in it.

`mutant` switches one rule off (MUTANTS): tests/test_tier_model_cpu.py proves with them that a merge,
a compaction or a GC that is wrong in one of these ways changes something the GPU test asserts."""
import bisect
from types import SimpleNamespace

import numpy as np

HOLE = None
DELTA_TILE = 256  # kDeltaTile: the copy tile of k_merge_copy<BatchIns>
BASE_TILE = 1024  # the compaction's copy tile below 16M base boundaries
SEG_LDS = 1024  # kSegLds: segments a copy tile stages; more take the binary-search fallback
GC_EVERY = 4  # kGcEveryCompactions
DEFAULT_DELTA_LIMIT = 1 << 16  # delta_limit_for() of a base below a million boundaries

MUTANTS = {
    1: "E omitted where it is needed",
    2: "E inserted where it is exact",
    3: "E inserted where it is glued",
    4: "E inherits the value at hi instead of before it",
    "5a": "removal one short at the begin",
    "5b": "removal one long at the begin",
    "5c": "removal one short at the end",
    "5d": "removal one long at the end",
    6: "B stored at the old value",
    7: "compaction: a hole filled from the delta's predecessor",
    8: "compaction: a hole inserted over an exact base boundary",
    "9a": "compaction: a span's removal ends one boundary early",
    "9b": "compaction: a span's removal ends one boundary late",
    10: "GC uses the kept predecessor",
    11: "GC looks at the boundary's own version alone",
}
SIZE_ONLY = (2, 3, 8)  # mutants that no verdict and no canonical dump can show


def union_segments(writes, empty_splits=False):
    """combineWriteConflictRanges over universe indices: the union segments of the committed,
    non-empty writes [(a, b)].  An end sorts before a begin at the same key, so [a, b) and [b, c)
    stay two segments.  empty_splits: the reference's sweep (SkipList.cpp:926-939) counts empty writes
    too; the end of an empty write [k, k) sorts before its begin, so inside a written span it closes
    the segment at k and opens the next one there: one more boundary at the same version, which no
    read can tell.  The engine's D.Combine leaves empty writes out (False)."""
    ev = sorted([(b, 0) for a, b in writes if a < b or empty_splits] +
                [(a, 1) for a, b in writes if a < b or empty_splits])
    out, active = [], 0
    for k, begin in ev:
        if begin:
            active += 1
            if active == 1:
                out.append([k, None])
        else:
            active -= 1
            if active == 0:
                out[-1][1] = k
    return [(a, b) for a, b in out]


class TierSim:
    def __init__(self, header=0, delta_limit=0, gc_interval=0, mutant=None):
        self.header = int(header)
        self.bk, self.bv = [], []  # the base: sorted universe indices, versions
        self.dk, self.dv = [], []  # the delta: versions or HOLE (the base shows through)
        self.delta_limit, self.gc_interval, self.mutant = delta_limit, gc_interval, mutant
        self.oldest = self.gc_applied = 0
        self.since_compact = self.since_gc = 0
        self.reached = 0  # how often the mutant's rule applied
        self.stats = dict(delta_sum=0, base_sum=0, segments_sum=0, compactions=0, gc_runs=0, batches=0)

    # ------------------------------------------------------------------ state

    def load(self, keys, vers, header):
        self.bk, self.bv, self.header = [int(k) for k in keys], [int(v) for v in vers], int(header)
        self.dk, self.dv = [], []

    def clear(self, version):
        self.bk, self.bv, self.dk, self.dv, self.header = [], [], [], [], int(version)

    @property
    def n_base(self):
        return len(self.bk)

    @property
    def n_delta(self):
        return len(self.dk)

    def history_size(self):
        return len(self.bk) + len(self.dk)

    def limit(self):
        return self.delta_limit if self.delta_limit > 0 else DEFAULT_DELTA_LIMIT

    def copy(self, mutant=None):
        c = TierSim(self.header, self.delta_limit, self.gc_interval, mutant)
        c.bk, c.bv, c.dk, c.dv = list(self.bk), list(self.bv), list(self.dk), list(self.dv)
        c.oldest, c.gc_applied = self.oldest, self.gc_applied
        c.since_compact, c.since_gc, c.stats = self.since_compact, self.since_gc, dict(self.stats)
        return c

    def folded(self):
        """The raw boundary set both tiers stand for: compact() applied to a copy."""
        c = self.copy(self.mutant)
        c.compact()
        return c.bk, c.bv

    def versions(self, U):
        """The step function over a universe of U keys: what a point read of each key sees."""
        bk, bv = self.folded()
        seg = np.searchsorted(np.array(bk, np.int64), np.arange(U), "right") - 1
        return np.array(bv + [self.header], np.int64)[seg]  # (seg -1: below the first boundary)

    def canonical(self, U, floor=None):
        """(header, boundary indices, versions): run-length encoded, clamped at `floor`."""
        ver, hdr = self.versions(U), self.header
        if floor is not None:
            ver = np.where(ver >= floor, ver, floor - 1)
            hdr = hdr if hdr >= floor else floor - 1
        s = np.flatnonzero(ver != np.concatenate([[hdr], ver[:-1]]))
        return hdr, s, ver[s]

    # ------------------------------------------------------------------ merge

    def merge(self, segments, now):
        """segments: sorted, disjoint [B, E) (they may touch).  Returns the facts of the merge."""
        dk, dv, n, mu = self.dk, self.dv, len(self.dk), self.mutant
        segs, spans, inserts = [], [], []
        for s, (B, E) in enumerate(segments):
            assert B < E and (s == 0 or segments[s - 1][1] <= B)
            lo, hi = bisect.bisect_left(dk, B), bisect.bisect_left(dk, E)
            exact = hi < n and dk[hi] == E
            glue = s + 1 < len(segments) and segments[s + 1][0] == E
            endins = not exact and not glue
            vend = dv[hi - 1] if hi > 0 else HOLE
            segs.append(SimpleNamespace(B=B, E=E, lo=lo, hi=hi, exact=exact, glue=glue, endins=endins, vend=vend))
            # ---- the mutants change what is stored, never the facts above
            r_lo, r_hi, ins_e, v_b = lo, hi, endins, now
            if mu == 1 and endins:
                ins_e = False
            if mu == 2 and exact:
                ins_e = True
            if mu == 3 and glue and not exact:
                ins_e = True
            if mu == 4 and endins and hi < n:
                vend = dv[hi]
            if mu == "5a" and hi - lo >= 1:
                r_lo = lo + 1
            if mu == "5b" and lo > 0 and (not spans or spans[-1][1] < lo):
                r_lo = lo - 1
            if mu == "5c" and hi - lo >= 1:
                r_hi = hi - 1
            if mu == "5d" and hi < n and not exact:
                r_hi = hi + 1
            if mu == 6:
                v_b = dv[lo - 1] if lo > 0 else HOLE
            self.reached += (r_lo, r_hi, ins_e, v_b, vend) != (lo, hi, endins, now, segs[-1].vend)
            spans.append((r_lo, r_hi))
            inserts.append((B, v_b))
            if ins_e:
                inserts.append((E, vend))
        removed = np.zeros(n + 1, bool)
        for a, b in spans:
            removed[a:b] = True
        kept = [(k, 1, v) for i, (k, v) in enumerate(zip(dk, dv)) if not removed[i]]
        # (a mutant may leave two entries at one key: the insert stands before the old boundary, as the
        # copy places it, and both count in the sizes)
        out = sorted(kept + [(k, 0, v) for k, v in inserts], key=lambda x: x[:2])
        self.dk, self.dv = [k for k, _, _ in out], [v for _, _, v in out]
        cnt = np.bincount([s.lo // DELTA_TILE for s in segs], minlength=n // DELTA_TILE + 1) if segs else \
            np.zeros(n // DELTA_TILE + 1, np.int64)
        return SimpleNamespace(n_before=n, n_after=len(self.dk), segs=segs, cnt=cnt, U=len(segs))

    # ------------------------------------------------------------------ compaction

    def compact(self):
        bk, bv, dk, dv, nb, nd, mu = self.bk, self.bv, self.dk, self.dv, len(self.bk), len(self.dk), self.mutant
        lo = [bisect.bisect_left(bk, k) for k in dk]
        exact = [p < nb and bk[p] == k for p, k in zip(lo, dk)]
        removed, true = np.zeros(nb + 2, bool), np.zeros(nb + 2, bool)
        inserts, holes = [], []
        for j in range(nd):
            if dv[j] is not HOLE:
                hi = lo[j + 1] if j + 1 < nd else nb
                true[lo[j]:hi] = True
                if mu == "9a" and hi > lo[j]:
                    hi -= 1
                if mu == "9b" and hi < nb and not (j + 1 < nd and exact[j + 1]):
                    hi += 1
                removed[lo[j]:hi] = True
                inserts.append((dk[j], dv[j]))
            else:
                val = bv[lo[j] - 1] if lo[j] > 0 else self.header
                if mu == 7:
                    true_val, val = val, next((dv[i] for i in range(j - 1, -1, -1) if dv[i] is not HOLE), self.header)
                    self.reached += val != true_val
                self.reached += mu == 8 and exact[j]
                holes.append(SimpleNamespace(j=j, lo=lo[j], exact=exact[j], val=val, last=j == nd - 1))
                if not exact[j] or mu == 8:  # (mutant 8: a second entry at the key, before the base's own)
                    inserts.append((dk[j], val))
        self.reached += int((removed != true).sum())
        out = sorted([(k, 1, v) for i, (k, v) in enumerate(zip(bk, bv)) if not removed[i]] +
                     [(k, 0, v) for k, v in inserts], key=lambda x: x[:2])
        self.bk, self.bv = [k for k, _, _ in out], [v for _, _, v in out]
        self.dk, self.dv = [], []
        cnt = np.bincount([p // BASE_TILE for p in lo], minlength=nb // BASE_TILE + 1) if lo else \
            np.zeros(nb // BASE_TILE + 1, np.int64)
        between = np.bincount(lo, minlength=nb + 1) if lo else np.zeros(nb + 1, np.int64)
        return SimpleNamespace(n_before=nb, nd=nd, n_after=len(self.bk), lo=lo, exact=exact, holes=holes, cnt=cnt,
                               most_between=int(between.max()) if lo else 0,
                               last_is_hole=bool(nd) and dv[-1] is HOLE)

    # ------------------------------------------------------------------ GC

    def gc(self, oldest):
        bv, mu = self.bv, self.mutant
        keep, kept_prev = [], self.header
        for i, v in enumerate(bv):
            pv = (bv[i - 1] if i else self.header) if mu != 10 else kept_prev
            k = v >= oldest or (pv >= oldest and mu != 11)
            self.reached += k != (v >= oldest or (bv[i - 1] if i else self.header) >= oldest)
            keep.append(k)
            if k:
                kept_prev = v
        dropped = [i for i, k in enumerate(keep) if not k]
        self.bk = [k for k, f in zip(self.bk, keep) if f]
        self.bv = [v for v, f in zip(self.bv, keep) if f]
        return SimpleNamespace(n_before=len(keep), n_after=len(self.bk), dropped=dropped, keep=keep)

    # ------------------------------------------------------------------ one batch under the policy

    def batch(self, n_write_ranges, segments, now, new_oldest):
        """One batch as half Y runs it: the merge, then what decide_y decides.  n_write_ranges: every
        write range the batch carries (aborted and TooOld writers' too: the bound is taken before any
        verdict is known).  Returns the batch's facts and the sizes after it."""
        nd_after_ub = len(self.dk) + 2 * n_write_ranges
        self.oldest = max(self.oldest, new_oldest)
        compact = nd_after_ub > self.limit()
        if self.gc_interval > 0:
            self.since_compact += 1
            if self.since_compact >= self.gc_interval:
                compact = True
        gc = False
        if compact:
            self.since_compact = 0
            turn = self.gc_interval > 0
            if not turn:
                self.since_gc += 1
                turn = self.since_gc >= GC_EVERY
            gc = self.oldest > self.gc_applied and turn
            if gc:
                self.since_gc = 0
        st = self.stats
        st["batches"] += 1
        st["delta_sum"] += len(self.dk)
        st["segments_sum"] += len(segments)
        out = SimpleNamespace(merge=self.merge(segments, now), compact=None, gc=None)
        if compact:
            out.compact = self.compact()
            st["compactions"] += 1
        if gc:
            out.gc = self.gc(max(self.oldest, self.gc_applied))
            self.gc_applied = self.oldest
            st["gc_runs"] += 1
        st["base_sum"] += len(self.bk)
        out.n_base, out.n_delta, out.stats = len(self.bk), len(self.dk), dict(st)
        return out


def run_batch(model, sim, tb, now, new_oldest, empty_splits=False):
    """One batch of multi-range transactions (keyspace_model.TxnBatch or its arrays) through both
    models: KeyspaceModel.resolve gives the verdicts and the step function, the committed non-empty
    writes give the union segments, TierSim.batch stores them under the policy.  Returns (resolve's
    result, TierSim.batch's facts)."""
    from tests import keyspace_model as K

    res = K.resolve(model, tb, now, sim.oldest, facts=False)
    A = res.arrays
    cw = res.verdicts[A.wt] == K.COMMITTED
    segs = union_segments(list(zip(A.wa[cw].tolist(), A.we[cw].tolist())), empty_splits)
    return res, sim.batch(len(A.wa), segs, now, new_oldest)
