"""Randomized parity stress of the HIP engine against the skip-list restatement (run on the GPU box).

Each round draws a key alphabet (arbitrary bytes, decimal digits, a sparse byte set, a tiny
alphabet), a shared prefix, key lengths around 16 and 24 bytes, a loaded history, engine knobs
read at set creation (directory slot budget, split check, stream layout, submitting threads),
compaction and GC cadence, and a sequence of batches whose snapshots straddle the oldest version; verdicts and
conflicting-read reports must match oracle/skiplist_baseline.cpp batch by batch.

    python3 scripts/stress_parity.py [seconds] [first_seed] [--state-every K] [--digest-every K]
                                     [--import-every K] [--import-into delta] [--read-versions-every K]
                                     [--verify-every K]

--state-every K (default off) also feeds the semantic oracle and compares the engine's exported
history (ConflictSet.dump_history at floor = oldest version) with the canonical form of the oracle's
step function every K batches: a wrong version or a lost boundary shows in the batch that made it,
not when a later read happens to meet it.

--digest-every K (default off) also feeds the semantic oracle and compares, every K batches, the
engine's digest of its state (ConflictSet.digest at floor = oldest version: no export, no copy) with
digest_arrays of the canonical form of the oracle's step function.  When they differ, the first
diverging key range (locate_divergence: digest_ranges against digest_arrays_ranges) is printed too.

--import-every K (default off; implies --state-every 1 unless given) merges, every K batches, a
random key range of a second set's history into the engine (ConflictSet.merge_history, every other
time merge_pending_export), compares the exported state with merge_max over the canonical forms
(tests/import_helpers.py) and reloads both oracles with it, so the batches that follow check the
verdicts the merged history gives.

--import-into delta sends those merges through into="delta" (fdbcs_history_import_delta, which falls
back to the fold when the delta could pass its bound); the final line counts the merges that took
the delta path.

--read-versions-every K (default off) also feeds the semantic oracle and compares, every K batches,
ConflictSet.read_versions over a few hundred random ranges (ends drawn from the batch's own keys and
the oracle's boundaries, by a generator of its own: the other options' streams are unchanged; every
tenth range empty) with the plain-Python model (tests/read_versions_model.py) on the oracle's dump,
at floor = oldest version.

--verify-every K (default off) runs ConflictSet.verify every K batches (and after a merge of
--import-every): the stored tiers, the range-max levels, the samples and both directories are
recomputed where they lie, so a wrong index shows in the batch that built it whether or not a later
read goes through it.  On a violation the report is printed and the round fails.

Exit status 1 and the failing seed on the first mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from foundationdb_amd import conflict_set as C  # noqa: E402
from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.export_helpers import canon, split_dump  # noqa: E402
from tests.helpers import EngineDriver  # noqa: E402
from tests.import_helpers import merge_max_fast, pack  # noqa: E402
from tests import read_versions_model  # noqa: E402

DIGESTS = [0]  # digests compared (--digest-every)
QUERIES = [0]  # ranges compared (--read-versions-every)
VERIFIES = [0]  # clean verify reports (--verify-every)

KNOBS = {
    "FDBCS_DIR_BITS": ["0", "0", "16", "18"],
    "FDBCS_SPLIT_CHECK": ["2", "1"],
    "FDBCS_SERIAL": ["0", "0", "0", "1"],
    "FDBCS_SKIP_EDGES": ["1", "0"],
    "FDBCS_SUBMIT_THREAD": ["1", "1", "0"],
}


PATHS = [0, 0]  # merges that folded into a new base / went into the delta (import_info)


def merge_round(rng, e, o, so, key, hdr, now, pending, into="base"):
    """Merge a random range of a second set's random history (versions up to `now`) into the engine
    and reload the oracles with merge_max; returns (error, the first set's header afterwards)."""
    ks = sorted({key(True) for _ in range(int(rng.integers(0, 3000)))})
    e2 = C.ConflictSet(0)
    e2.load_history(*pack((int(rng.integers(0, now + 1)), ks, rng.integers(0, now + 1, size=len(ks)))))
    lo = key() if rng.random() < 0.7 else None
    hi = key() if rng.random() < 0.7 else None
    if lo is not None and hi is not None and lo > hi:
        lo, hi = hi, lo
    dump = e2.dump_history(lo, hi, C.NO_FLOOR)
    oldest = so.oldest_version
    own = canon(*so.dump_history(), hdr, oldest)
    merged = merge_max_fast(own, split_dump(dump), lo, hi)
    want = canon(merged[1], merged[2], merged[0], oldest)
    if pending:
        e2.export_history(lo, hi, C.NO_FLOOR)
        e.cs.merge_pending_export(e2, lo, hi, into=into)
    else:
        e.cs.merge_history(*dump, lo=lo, hi=hi, into=into)
    PATHS[e.cs.import_info()["path"]] += 1
    e2.close()
    got = split_dump(e.cs.dump_history())
    if got != want:
        return f"merged state [{lo!r}, {hi!r}) pending={pending} into={into}: {len(got[1])} boundaries, merge_max {len(want[1])}", hdr
    kb, ko, vv, h = pack(want)
    for x in (o, so):
        if len(vv):
            x.load_history(kb, ko, vv, h)
        else:
            x.clear(h)
        x.set_oldest_version(oldest)
    return None, h


def verify_state(e, what):
    """None if ConflictSet.verify reports the stored state clean, else the error (the report is printed)."""
    rep = e.cs.verify()
    VERIFIES[0] += 1
    if rep.ok:
        return None
    print(rep.as_dict(), flush=True)
    return f"verify {what}: {rep!r}"


def one(seed, state_every=0, import_every=0, import_into="base", digest_every=0, read_versions_every=0,
        verify_every=0):
    rng = np.random.default_rng(seed)
    qrng = np.random.default_rng([seed, 15])
    for k, vals in KNOBS.items():
        os.environ[k] = vals[int(rng.integers(0, len(vals)))]
    kind = ["bytes", "digits", "sparse", "tiny"][int(rng.integers(0, 4))]
    prefix = bytes(rng.integers(0, 256, size=int(rng.integers(0, 20))).astype(np.uint8))
    top = int(rng.choice([8, 16, 30]))

    def suffix(n, hist):
        if kind == "bytes":
            return bytes(rng.integers(0, 256, size=n).astype(np.uint8))
        if kind == "digits":
            return bytes(rng.integers(0x30, 0x3a, size=n).astype(np.uint8))
        if kind == "tiny":
            return bytes(rng.integers(0, 3, size=n).astype(np.uint8))
        if hist:  # sparse: even values in the history, any value in the batches
            return bytes((2 * rng.integers(0x10, 0x40, size=n)).astype(np.uint8))
        return bytes(rng.integers(0x10, 0x91, size=n).astype(np.uint8))

    def key(hist=False):
        k = prefix + suffix(int(rng.integers(0, top)), hist)
        if rng.random() < 0.05:  # outside the shared prefix
            k = bytes(rng.integers(0, 256, size=int(rng.integers(0, 6))).astype(np.uint8))
        return k

    n_hist = int(rng.integers(0, 40000))
    hist = sorted({key(True) for _ in range(n_hist)})
    kb = np.frombuffer(b"".join(hist), np.uint8) if hist else np.zeros(0, np.uint8)
    ko = np.zeros(len(hist) + 1, np.int64)
    if hist:
        np.cumsum([len(k) for k in hist], out=ko[1:])
    vers = rng.integers(0, 1000, size=len(hist)).astype(np.int64)
    e = EngineDriver(C, gc_interval=int(rng.integers(0, 4)), delta_limit=int(rng.choice([0, 2000, 20000])))
    o = oracle.SkipListBaseline()
    e.load_history(kb, ko, vers)
    o.load_history(kb, ko, vers)
    so = None
    if state_every or digest_every or read_versions_every:  # the skip-list restatement has no dump: the semantic oracle holds the state
        so = oracle.OracleConflictSet()
        so.load_history(kb, ko, vers)
    now, oldest, hdr, merges = 1000, 0, 0, 0
    for i in range(int(rng.integers(3, 10))):
        now += int(rng.integers(1, 200))
        txns = []
        for _ in range(int(rng.integers(1, 1500))):
            def rr():
                a, b = key(), key()
                return KeyRange(min(a, b), max(a, b))

            txns.append(CommitTransaction([rr() for _ in range(int(rng.integers(0, 4)))],
                                          [rr() for _ in range(int(rng.integers(0, 3)))],
                                          now - int(rng.integers(0, 700)), bool(rng.random() < 0.3)))
        pb = PackedBatch.from_transactions(txns)
        if rng.random() < 0.5:
            oldest = max(oldest, now - int(rng.integers(100, 600)))
        ve, ce = e.detect(pb, now, oldest)
        vo, co = o.detect(pb, now, oldest)
        if not (ve == vo).all():
            return f"verdicts batch {i}: {int((ve != vo).sum())} differ, first {np.nonzero(ve != vo)[0][:5].tolist()}"
        ce = {t: v for t, v in ce.items() if v}
        co = {t: sorted(v) for t, v in co.items() if v}
        if ce != co:
            return f"conflicting reads batch {i}"
        if verify_every and (i + 1) % verify_every == 0:
            err = verify_state(e, f"batch {i}")
            if err:
                return err
        if so is not None:
            so.detect(pb, now, oldest)
            if digest_every and (i + 1) % digest_every == 0:
                keys, hv = so.dump_history()
                want = C.digest_arrays(*pack(canon(keys, hv, hdr, so.oldest_version)))
                got = e.cs.digest()
                DIGESTS[0] += 1
                if got != want:
                    # where: bisect the engine's state against the oracle's canonical arrays
                    arr = pack(canon(keys, hv, hdr, so.oldest_version))
                    where = C.locate_divergence(lambda b, ol, oh: e.cs.digest_ranges(b, None, ol, oh),
                                                lambda b, ol, oh: C.digest_arrays_ranges(*arr, b, ol, oh),
                                                e.cs.split_keys, leaf=4)
                    return f"digest batch {i}: {got}, oracle {want}; first diverging range {where[0] if where else None}"
            if read_versions_every and (i + 1) % read_versions_every == 0:
                keys, hv = so.dump_history()
                pool = sorted(set(keys) | {pb.key(k) for k in range(len(pb.key_offsets) - 1)} | {b""})
                ranges = []
                for _ in range(300):
                    a, b = sorted(qrng.integers(0, len(pool), size=2).tolist())
                    ranges.append((pool[a], pool[a] if qrng.random() < 0.1 else pool[b]))
                want = read_versions_model.read_versions(keys, hv.tolist(), hdr, ranges, so.oldest_version)
                got = e.cs.read_versions(ranges).tolist()
                QUERIES[0] += len(ranges)
                if got != want:
                    d = next(j for j in range(len(want)) if j >= len(got) or got[j] != want[j])
                    return f"read versions batch {i}: range {ranges[d]!r}: {got[d:d + 1]}, model {want[d]}"
            if state_every and (i + 1) % state_every == 0:
                keys, hv = so.dump_history()
                want = canon(keys, hv, hdr, so.oldest_version)
                got = split_dump(e.cs.dump_history())
                if got != want:
                    return f"exported state batch {i}: {len(got[1])} boundaries, oracle {len(want[1])}"
            if import_every and (i + 1) % import_every == 0:
                err, hdr = merge_round(rng, e, o, so, key, hdr, now, merges & 1, import_into)
                merges += 1
                if err:
                    return f"batch {i}: {err}"
                if verify_every:
                    err = verify_state(e, f"after the merge behind batch {i}")
                    if err:
                        return err
    e.cs.close()
    return None


def main():
    args = sys.argv[1:]
    state_every = 0
    if "--state-every" in args:
        k = args.index("--state-every")
        state_every = int(args[k + 1])
        del args[k:k + 2]
    digest_every = 0
    if "--digest-every" in args:
        k = args.index("--digest-every")
        digest_every = int(args[k + 1])
        del args[k:k + 2]
    import_every = 0
    if "--import-every" in args:
        k = args.index("--import-every")
        import_every = int(args[k + 1])
        del args[k:k + 2]
        state_every = state_every or 1
    import_into = "base"
    if "--import-into" in args:
        k = args.index("--import-into")
        import_into = args[k + 1]
        del args[k:k + 2]
    read_versions_every = 0
    if "--read-versions-every" in args:
        k = args.index("--read-versions-every")
        read_versions_every = int(args[k + 1])
        del args[k:k + 2]
    verify_every = 0
    if "--verify-every" in args:
        k = args.index("--verify-every")
        verify_every = int(args[k + 1])
        del args[k:k + 2]
    budget = float(args[0]) if len(args) > 0 else 120.0
    seed = int(args[1]) if len(args) > 1 else 1
    oracle.build()
    t0 = time.time()
    n = 0
    while time.time() - t0 < budget:
        err = one(seed, state_every, import_every, import_into, digest_every, read_versions_every, verify_every)
        knobs = {k: os.environ[k] for k in KNOBS}
        if err:
            print(f"MISMATCH seed {seed} knobs {knobs}: {err}", flush=True)
            sys.exit(1)
        n += 1
        if n % 10 == 0:
            print(f"{n} rounds ok ({time.time() - t0:.0f} s), last seed {seed}", flush=True)
        seed += 1
    print(f"stress: {n} random rounds, every batch exact ({time.time() - t0:.0f} s)")
    if digest_every:
        print(f"stress: {DIGESTS[0]} digests equal to the oracle's")
    if read_versions_every:
        print(f"stress: {QUERIES[0]} read versions equal to the model's")
    if verify_every:
        print(f"stress: {VERIFIES[0]} verify reports clean")
    if import_every:
        print(f"stress: {PATHS[1]} merges into the delta, {PATHS[0]} folded into a new base")


if __name__ == "__main__":
    main()
