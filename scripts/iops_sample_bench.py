"""Device time of the resolver's iops sample of a device-routed batch (fdbcs_batch_set_iops_sample)
beside the routing kernels of the same batches.

A C2-shaped batch (5,000 transactions, 25k reads and 10k writes, 16-byte keys) is routed whole to one
resolver (one share, no bounds) and sampled with the reference's 20,000 metric units per sample:
about 200 of its 35,000 range begins.  2 warm-up batches, then `--reps` timed ones; per batch the
device time of the sample's launch (fdbcs_batch_iops_sample_timing, events around it) and of the
routing's launches (ms_route_kernels of fdbcs_get_stats, events around them).  The routing is the
yardstick: one look-back pass over the same ranges that writes all of them, where the sample writes
about 0.6 %.  Every batch is detected, so the numbers are taken with the pipeline's other streams
busy as they are in use; --check holds every sample against balancing.iops_sample_of.

    python3 scripts/iops_sample_bench.py [--reps R] [--warmup W] [--history N] [--check] [--out FILE]

Prints one JSON line (and appends it to FILE)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

torch.cuda.is_available()
from foundationdb_amd import balancing as B  # noqa: E402
from foundationdb_amd import conflict_set as C  # noqa: E402
from foundationdb_amd import workloads as W  # noqa: E402

UNITS = B.KEY_BYTES_PER_SAMPLE


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--history", type=int, default=1_000_000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = W.C2Params(history=a.history)
    start = 10_000_000
    cs = C.ConflictSet(0)
    cs.load_history(*W.c2_history(p, seed=1, start_version=start), 0)
    rng = np.random.default_rng(7)
    now = start
    sample_us, route_us, kept = [], [], []
    ok = True
    for r in range(a.warmup + a.reps):
        now += p.version_step
        pb = W.c2_batch(p, rng, now)
        share = C.share_pack(pb)
        stride = (len(share) + 255) // 256 * 256
        host = np.zeros(stride, np.uint8)
        host[: len(share)] = share
        dev = torch.from_numpy(host).cuda()
        out = torch.zeros(pb.n_txn, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = cs.stats()
        b = C.ConflictBatch(cs, None)
        b.add_routed(dev.data_ptr(), stride, 1, pb.n_txn, None, None,
                     (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes), out.data_ptr(), pb.n_txn)
        b.set_iops_sample(UNITS, seed=now)
        keys, metrics, index = b.iops_sample()
        ms = b.iops_sample_timing()
        if a.check:
            wk, wm, wi = B.iops_sample_of(pb, UNITS, now)
            ok &= keys == wk and metrics.tolist() == wm.tolist() and index.tolist() == wi.tolist()
        b.detect_async(now, now - p.window)
        b.wait()
        b.close()
        after = cs.stats()
        assert after["routed_batches"] - before["routed_batches"] == 1
        if r >= a.warmup:
            sample_us.append(ms * 1e3)
            route_us.append((after["ms_route_kernels"] - before["ms_route_kernels"]) * 1e3)
            kept.append(len(keys))
    cs.close()
    res = {"bench": "iops_sample", "txns": p.txns, "ranges": p.txns * (p.reads + p.writes), "units": UNITS,
           "reps": a.reps, "warmup": a.warmup, "sampled_keys": summary(kept),
           "sample_us": summary(sample_us), "route_us": summary(route_us)}
    if a.check:
        res["check"] = "equal" if ok else "different"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
