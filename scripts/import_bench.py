"""Device time of the history import (fdbcs_history_import / fdbcs_history_import_pending) on a C2
history.

The receiver is the C2 base (`--history` boundaries) with an empty delta, or the same base under the
delta that `--batches` C2 batches leave (no compaction in between).  The sender is a second set of
the same size on another seed.  Imported: the sender's full-range export, and its export of a 1 %
key range, each through the host-array path (merge_history) and the device-to-device path
(merge_pending_export).  An import rewrites the receiver, so every repetition rebuilds the receiver
first (load, then the batches); 1 warm-up, then `--reps` timed imports per case.  Per import: the
device time of its kernels (events around its three groups of launches) and the host time of the
call.  The bytes are the algorithm's own model: the imported arrays read once (key bytes, offsets,
versions), 32 B read per boundary of the three streams, 32 B written and read again per element of
the merged stream (8 B more to zero it), 32 B plus the tail written per kept boundary; the searches'
gathers are not counted.  The yardstick is the one the export's bench uses, timed in the same run:
the engine's own compaction + GC pass over the receiver's tiers, per kernel (timing level 3).

    python3 scripts/import_bench.py [--history N] [--batches B] [--reps R] [--into base|delta|both] [--out FILE]

--into delta sends the imports through into="delta" (fdbcs_history_import_delta), --into both measures
every case through the fold and through the delta path on the same receiver in the same run; each
case then also records the path the engine took (0: fold, 1: delta; the full export passes the delta
bound and must report 0) and the delta tier's size before and after.  The default, base, is the
fold alone.

Prints one JSON line per receiver state (and appends them to FILE)."""
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
RANGE_1PCT = (b"\x40", b"\x42\x8f")  # 0x028f / 0x10000 of the key space


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


class Receiver:
    def __init__(self, p, hist, batches, start):
        self.p, self.hist, self.batches, self.start = p, hist, batches, start
        self.cs = C.ConflictSet(0)
        self.cs.set_gc_interval(0)
        self.cs.set_delta_limit(8 * (batches + 2) * p.txns * p.writes)  # the delta keeps every batch
        rng = np.random.default_rng(7)
        self.seq = [(W.c2_batch(p, rng, start + (i + 1) * p.version_step), start + (i + 1) * p.version_step)
                    for i in range(batches)]

    def rebuild(self):
        self.cs.load_history(*self.hist, 0)
        for pb, now in self.seq:
            b = C.ConflictBatch(self.cs, None)
            b.add_packed(pb)
            b.detect_conflicts(now, now - self.p.window)
            b.close()
        return self.cs.history_size()


def measure(rcv, snd, lo, hi, pending, warmup, reps, into=None):
    kw = {"into": into} if into else {}
    n, nbytes, hdr = snd.export_history(lo, hi)
    arrays = snd.read_export(n, nbytes)
    if pending:
        snd.export_history(lo, hi)  # stays pending across the imports
    dev, host = [], []
    for r in range(warmup + reps):
        before = rcv.rebuild()
        t0 = time.perf_counter()
        if pending:
            after = rcv.cs.merge_pending_export(snd, lo, hi, **kw)
        else:
            after = rcv.cs.merge_history(*arrays, hdr, lo=lo, hi=hi, **kw)
        t1 = time.perf_counter()
        k_ms, _ = rcv.cs.import_timing()
        if r >= warmup:
            dev.append(k_ms * 1e3)
            host.append((t1 - t0) * 1e6)
    m = n + (lo is not None) + (hi is not None)
    total = before + m
    rd = nbytes + 16 * n + 32 * total + 32 * total
    wr = 32 * m + 40 * total + 32 * after
    med = summary(dev)["median"]
    info = {}
    if into:
        i = rcv.cs.import_info()
        info = {"into": into, "engine_path": i["path"], "base_boundaries": i["base_boundaries"],
                "delta_before": i["delta_before"], "delta_after": i["delta_after"]}
    return {
        **info, "path": "pending" if pending else "host_arrays", "range": "full" if lo is None else "1pct",
        "imported": int(n), "imported_key_bytes": int(nbytes), "boundaries_before": int(before),
        "boundaries_after": int(after), "bytes_read": int(rd), "bytes_written": int(wr),
        "device_us": summary(dev), "host_call_us": summary(host),
        "achieved_GBps": (rd + wr) / (med * 1e-6) / 1e9, "hbm_share": (rd + wr) / (med * 1e-6) / HBM_BYTES_PER_S,
    }


def yardstick(rcv):
    """One compaction with GC over the receiver's tiers, per kernel."""
    rcv.rebuild()
    cs, p = rcv.cs, rcv.p
    cs.set_timing(3)
    cs.reset_stats()
    cs.set_gc_interval(1)
    now = rcv.start + (rcv.batches + 1) * p.version_step
    b = C.ConflictBatch(cs, None)
    b.add_packed(W.c2_batch(p, np.random.default_rng(8), now))
    b.detect_conflicts(now, now - p.window)
    b.close()
    prof = cs.kernel_profile()
    pick = {k: v for k, v in prof.items()
            if any(s in k for s in ("k_compact_search", "CompactSumScan", "CompactIns", "GcScan"))}
    us = {k[:60]: v["ms"] * 1e3 / max(1, v["launches"]) for k, v in pick.items()}
    cs.set_timing(0)
    cs.set_gc_interval(0)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=5_000_000)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--into", choices=("base", "delta", "both"), default="base")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    intos = {"base": (None,), "delta": ("delta",), "both": ("base", "delta")}[a.into]
    p = W.C2Params(history=a.history)
    start = 10_000_000
    hist = W.c2_history(p, seed=1, start_version=start)
    snd = C.ConflictSet(0)
    snd.load_history(*W.c2_history(p, seed=2, start_version=start), 0)
    for batches in (0, a.batches):
        rcv = Receiver(p, hist, batches, start)
        out = {"bench": "import", "history": int(len(hist[2])), "batches": batches, "reps": a.reps, "cases": []}
        for lo, hi in ((None, None), RANGE_1PCT):
            for pending in (False, True):
                for into in intos:
                    c = measure(rcv, snd, lo, hi, pending, a.warmup, a.reps, into)
                    print(json.dumps(c), file=sys.stderr, flush=True)
                    out["cases"].append(c)
        out["yardstick_us"] = yardstick(rcv)
        out["yardstick_sum_us"] = sum(out["yardstick_us"].values())
        rcv.cs.close()
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    snd.close()


if __name__ == "__main__":
    main()
