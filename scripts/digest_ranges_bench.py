"""Device and wall time of the partitioned history digest (fdbcs_history_digest_ranges) against the
single digest's, on the set of digest_bench.py's first state: a C2 history under the delta that
`--batches` C2 batches leave (no compaction in between).

Per round, in one process: one whole-range digest (the yardstick: code the partitioned digest leaves
alone), then digest_ranges over the same span with K in {1, 16, 256, 4096} ranges whose bounds are
K - 1 split keys of the set, then for K in {16, 256} the same K ranges as K sequential digest calls,
then split_keys for 256 keys.  2 warm-up rounds, `--reps` timed ones; kernel time is what
digest_timing / split_keys_timing report (events around the launches), wall time is around the call.

    python3 scripts/digest_ranges_bench.py [--history N] [--batches B] [--reps R] [--out FILE]

Every round checks that the ranges' n and key bytes plus those of the bounds that are canonical
boundaries (counted once, against one export) add up to the whole-range digest's, and the sequential
calls that each equals its entry of digest_ranges; exit status 1 on a difference.
Prints one JSON line (and appends it to FILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

torch.cuda.is_available()
from foundationdb_amd import conflict_set as C  # noqa: E402
from foundationdb_amd import workloads as W  # noqa: E402

KS = (1, 16, 256, 4096)
SEQUENTIAL = (16, 256)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def canonical_hits(dump, bounds):
    """(count, key bytes) of the bounds that are boundaries of the exported canonical history."""
    kb, ko, vv, _ = dump
    raw = kb.tobytes()
    n, hits, nbytes = len(vv), 0, 0
    for b in bounds:
        lo, hi = 0, n
        while lo < hi:
            mid = (lo + hi) // 2
            if raw[ko[mid]:ko[mid + 1]] < b:
                lo = mid + 1
            else:
                hi = mid
        if lo < n and raw[ko[lo]:ko[lo + 1]] == b:
            hits += 1
            nbytes += len(b)
    return hits, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=5_000_000)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = W.C2Params(history=a.history)
    start = 10_000_000
    kb, ko, vers = W.c2_history(p, seed=1, start_version=start)
    cs = C.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(8 * (a.batches + 2) * p.txns * p.writes)  # the delta keeps every batch: no compaction
    cs.load_history(kb, ko, vers, 0)
    rng = np.random.default_rng(7)
    now = start
    for _ in range(a.batches):
        now += p.version_step
        b = C.ConflictBatch(cs, None)
        b.add_packed(W.c2_batch(p, rng, now))
        b.detect_conflicts(now, now - p.window)
        b.close()
    total = cs.history_size()
    bounds = {K: cs.split_keys(None, None, K - 1) for K in KS}
    assert all(len(bounds[K]) == K - 1 for K in KS)
    dump = cs.dump_history()
    hits = {K: canonical_hits(dump, bounds[K]) for K in KS}
    del dump
    t = {"digest": ([], []), "split_keys_256": ([], [])}
    t.update({f"ranges_{K}": ([], []) for K in KS})
    t.update({f"sequential_{K}": ([], []) for K in SEQUENTIAL})
    ok = True

    def note(name, r, kernels_ms, t0):
        if r >= a.warmup:
            t[name][0].append(kernels_ms * 1e3)
            t[name][1].append((time.perf_counter() - t0) * 1e6)

    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        whole = cs.digest()
        note("digest", r, cs.digest_timing()[0], t0)
        got = {}
        for K in KS:
            t0 = time.perf_counter()
            got[K] = cs.digest_ranges(bounds[K], None, True, True)
            note(f"ranges_{K}", r, cs.digest_timing()[0], t0)
            ok &= len(got[K]) == K
            ok &= sum(d.n for d in got[K]) + hits[K][0] == whole.n
            ok &= sum(d.key_bytes for d in got[K]) + hits[K][1] == whole.key_bytes
        ok &= got[1] == [whole]
        for K in SEQUENTIAL:
            edges = [None] + bounds[K] + [None]
            kernels, seq = 0.0, []
            t0 = time.perf_counter()
            for lo, hi in zip(edges, edges[1:]):
                seq.append(cs.digest(lo, hi))
                kernels += cs.digest_timing()[0]
            note(f"sequential_{K}", r, kernels, t0)
            ok &= seq == got[K]
        t0 = time.perf_counter()
        keys = cs.split_keys(None, None, 256)
        note("split_keys_256", r, cs.split_keys_timing()[0], t0)
        ok &= len(keys) == 256 and all(x < y for x, y in zip(keys, keys[1:]))
    cs.close()
    out = {"bench": "digest_ranges", "history": int(len(vers)), "batches": a.batches, "reps": a.reps,
           "boundaries_in": int(total), "boundaries_out": int(whole.n), "equal": bool(ok),
           "bounds_that_are_canonical_boundaries": {str(K): hits[K][0] for K in KS}}
    for name, (kernels, wall) in t.items():
        out[name] = {"kernels_us": summary(kernels), "wall_us": summary(wall)}
    dk = out["digest"]["kernels_us"]
    out["ranges_1_kernels_inside_digest_spread_plus_10pct"] = bool(
        dk["min"] * 0.9 <= out["ranges_1"]["kernels_us"]["median"] <= dk["max"] * 1.1)
    for K in SEQUENTIAL:
        out[f"sequential_over_ranges_wall_{K}"] = (out[f"sequential_{K}"]["wall_us"]["median"]
                                                   / out[f"ranges_{K}"]["wall_us"]["median"])
    out["ranges_4096_over_digest_kernels"] = out["ranges_4096"]["kernels_us"]["median"] / dk["median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
