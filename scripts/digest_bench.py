"""Device time of the history digest (fdbcs_history_digest) against the export's on a C2 history.

Two states of one set: the loaded base under the delta that `--batches` C2 batches leave (no
compaction in between), and the same set right after a compaction.  Per state, in one process and
alternating (digest, export + read, digest, ...): 2 warm-up rounds, then `--reps` timed ones; per
round the device time of the digest's kernels and of the export's kernels (events around them),
the wall time of the digest call, and the wall time of the export end to end (export_history +
read_export).  The yardstick is the export's own kernel time: the digest runs the export's first
three launches and a fourth with the same loads and no key stores.  The device bytes a first digest
and a first export of the state allocate are restated from the sizes the two entry points ask for
(transfer.cpp; before the allocator's rounding).

    python3 scripts/digest_bench.py [--history N] [--batches B] [--reps R] [--out FILE]

Every round also checks digest == digest_arrays(export); exit status 1 on a difference.
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


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def measure(cs, warmup, reps):
    dk, dw, xk, xw = [], [], [], []
    ok = True
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        d = cs.digest()
        t1 = time.perf_counter()
        n, nbytes, hdr = cs.export_history()
        kb, ko, vv = cs.read_export(n, nbytes)
        t2 = time.perf_counter()
        ok &= d == C.digest_arrays(kb, ko, vv, hdr)
        if r >= warmup:
            dk.append(cs.digest_timing()[0] * 1e3)
            dw.append((t1 - t0) * 1e6)
            xk.append(cs.export_timing()[0] * 1e3)
            xw.append((t2 - t1) * 1e6)
    out = {"boundaries_in": int(cs.history_size()), "boundaries_out": int(n), "key_bytes": int(nbytes),
           "tail_bytes": int(np.maximum(np.diff(ko) - 16, 0).sum()),
           "digest_kernels_us": summary(dk), "export_kernels_us": summary(xk),
           "export_end_to_end_us": summary(xw), "digest_wall_us": summary(dw), "equal": bool(ok)}
    out["digest_over_export_kernels"] = out["digest_kernels_us"]["median"] / out["export_kernels_us"]["median"]
    return out


def first_call_bytes(total, nd, tail_used):
    """Device bytes the first digest and the first export of a set ask for (transfer.cpp)."""
    tiles = max(1, (total + 1023) // 1024)
    shared = 64 + 2 * 8 * (nd + 1)  # bounds' tails, one position and one value per delta boundary
    digest = shared + 8 * (8 + tiles)
    export = shared + 8 * (8 + 4 * tiles) + 2 * 8 * (total + 1) + 16 * total + tail_used + 64
    return {"digest": int(digest), "export": int(export)}


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

    def batch():
        nonlocal now
        now += p.version_step
        b = C.ConflictBatch(cs, None)
        b.add_packed(W.c2_batch(p, rng, now))
        b.detect_conflicts(now, now - p.window)
        b.close()

    for _ in range(a.batches):
        batch()
    out = {"bench": "digest", "history": int(len(vers)), "batches": a.batches, "reps": a.reps}
    # the first digest of the set, before any export allocated anything
    t0 = time.perf_counter()
    first = cs.digest()
    out["first_digest_wall_us"] = (time.perf_counter() - t0) * 1e6
    total = cs.history_size()
    out["with_delta"] = measure(cs, a.warmup, a.reps)
    out["with_delta"]["delta_boundaries"] = int(total - len(vers))  # the base is the loaded one: no compaction ran
    out["with_delta"]["first_call_device_bytes"] = first_call_bytes(total, total - len(vers),
                                                                    out["with_delta"]["tail_bytes"])
    ok = out["with_delta"]["equal"] and first == cs.digest()
    cs.set_gc_interval(1)
    batch()  # compacts: the delta is folded into a new base
    out["after_compaction"] = measure(cs, a.warmup, a.reps)
    ok &= out["after_compaction"]["equal"]
    cs.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
