"""Device time and achieved bandwidth of the history export (fdbcs_history_export) on a C2 history.

Two states of one set: the loaded base with an empty delta, and the same base under the delta that
`--batches` C2 batches leave (no compaction in between).  Per state: 2 warm-up exports, then
`--reps` timed ones; per rep the device time of the export's kernels (events around them), the time
of the three device-to-host copies, and the host time of both calls.  The bytes the algorithm has to
move come from the shapes: 32 B read per boundary of both tiers plus the kept keys' tail bytes;
8 B (version) + 8 B (offset) + the key bytes written per kept boundary.  The yardstick is the
engine's own streaming pass over the same tiers, one compaction with GC timed per kernel (timing
level 3) at the end.

    python3 scripts/export_bench.py [--history N] [--batches B] [--reps R] [--check] [--out FILE]

--check also feeds the semantic oracle (30 batches unless --batches is given) and compares the
exported state with the canonical form of its step function; exit status 1 on a difference.
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

HBM_BYTES_PER_S = 8e12  # the project's roofline figure


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def measure(cs, warmup, reps):
    dev, d2h, host_x, host_r = [], [], [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        n, nbytes, _ = cs.export_history()
        t1 = time.perf_counter()
        kb, ko, vv = cs.read_export(n, nbytes)
        t2 = time.perf_counter()
        k_ms, c_ms = cs.export_timing()
        if r >= warmup:
            dev.append(k_ms * 1e3)
            d2h.append(c_ms * 1e3)
            host_x.append((t1 - t0) * 1e6)
            host_r.append((t2 - t1) * 1e6)
    lens = np.diff(ko)
    total = cs.history_size()
    tails = int(np.maximum(lens - 16, 0).sum())
    rd = 32 * total + tails
    wr = int(16 * n + nbytes + 8)
    med = summary(dev)["median"]
    return {
        "boundaries_in": int(total), "boundaries_out": int(n), "key_bytes": int(nbytes),
        "bytes_read": int(rd), "bytes_written": wr,
        "device_us": summary(dev), "d2h_us": summary(d2h), "host_export_us": summary(host_x),
        "host_read_us": summary(host_r),
        "achieved_GBps": (rd + wr) / (med * 1e-6) / 1e9,
        "hbm_share": (rd + wr) / (med * 1e-6) / HBM_BYTES_PER_S,
    }


def check_state(cs, o, header, what):
    from tests.export_helpers import canon, split_dump

    keys, vers = o.dump_history()
    want = canon(keys, vers, header, o.oldest_version)
    got = split_dump(cs.dump_history())
    ok = got == want
    print(f"check {what}: {len(got[1])} boundaries, oracle {len(want[1])}: {'equal' if ok else 'DIFFERENT'}",
          file=sys.stderr, flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=5_000_000)
    ap.add_argument("--batches", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = a.batches if a.batches is not None else (30 if a.check else 50)
    p = W.C2Params(history=a.history)
    start = 10_000_000
    kb, ko, vers = W.c2_history(p, seed=1, start_version=start)
    cs = C.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(8 * (batches + 2) * p.txns * p.writes)  # the delta keeps every batch: no compaction
    cs.load_history(kb, ko, vers, 0)
    o = None
    ok = True
    if a.check:
        from oracle import oracle

        oracle.build()
        o = oracle.OracleConflictSet()
        o.load_history(kb, ko, vers, 0)
        ok &= check_state(cs, o, 0, "loaded")
    out = {"bench": "export", "history": int(len(vers)), "batches": batches, "reps": a.reps,
           "empty_delta": measure(cs, a.warmup, a.reps)}
    rng = np.random.default_rng(7)
    now = start
    for _ in range(batches):
        now += p.version_step
        pb = W.c2_batch(p, rng, now)
        b = C.ConflictBatch(cs, None)
        b.add_packed(pb)
        v = b.detect_conflicts(now, now - p.window)
        b.close()
        if o is not None:
            vo, _ = o.detect(pb, now, now - p.window, gc=False)
            ok &= bool((v == vo).all())
    if o is not None:
        ok &= check_state(cs, o, 0, f"after {batches} batches")
        out["check"] = "equal" if ok else "different"
    out["with_delta"] = measure(cs, a.warmup, a.reps)
    # the yardstick: one compaction with GC over the same tiers, per kernel
    cs.set_timing(3)
    cs.reset_stats()
    cs.set_gc_interval(1)
    now += p.version_step
    b = C.ConflictBatch(cs, None)
    b.add_packed(W.c2_batch(p, rng, now))
    b.detect_conflicts(now, now - p.window)
    b.close()
    prof = cs.kernel_profile()
    print("kernels timed:", sorted(prof), file=sys.stderr)
    pick = {k: v for k, v in prof.items()
            if any(s in k for s in ("k_compact_search", "CompactSumScan", "CompactIns", "GcScan"))}
    out["yardstick_us"] = {k[:60]: v["ms"] * 1e3 / max(1, v["launches"]) for k, v in pick.items()}
    out["yardstick_sum_us"] = sum(out["yardstick_us"].values())
    cs.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
