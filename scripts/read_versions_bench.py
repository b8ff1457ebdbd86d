"""Device time of the read-version query (fdbcs_batch_read_versions) against the read check's on the
same batch and set.

One set: a loaded base under the delta that `--batches` batches leave (no compaction in between),
and the next batch of the workload, uploaded and never detected.  In one process, after `--warmup`
rounds, `--rounds` timed ones; per round
  - the read check's isolated time on that batch (fdbcs_debug_kernel_time(b, 0, reps): the average
    of `reps` back-to-back launches), the yardstick: this code is the detect pipeline's own; and
    the same check as the query is timed, one launch between two events (reps = 1), `reps` times;
  - the query's kernel time (events around its one launch) over `reps` calls of the device form,
    and the host time of the call, both forms;
  - a sample of the result against the plain-Python model (tests/read_versions_model.py) on the
    set's own export clipped to each sampled read; exit status 1 on a difference.
Then, once: ConflictSet.read_versions over 1000 ranges against a dump_history of the same set.

    python3 scripts/read_versions_bench.py [--shape c2|c4] [--history N] [--batches B] [--out FILE]

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
from tests import read_versions_model as M  # noqa: E402


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("c2", "c4"), default="c2")
    ap.add_argument("--history", type=int, default=0, help="boundaries to load (0: the shape's own)")
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    start = 10_000_000
    if a.shape == "c2":
        p = W.C2Params(**({"history": a.history} if a.history else {}))
        kb, ko, vers = W.c2_history(p, seed=1, start_version=start)
        make = lambda rng, now: W.c2_batch(p, rng, now)
    else:
        p = W.C4Params(**({"history": a.history} if a.history else {}))
        kb, ko, vers = W.c4_history(p, seed=1, start_version=start)
        make = lambda rng, now: W.c4_batch(p, rng, now)
    cs = C.ConflictSet(0)
    cs.set_gc_interval(0)
    cs.set_delta_limit(8 * (a.batches + 2) * p.txns * p.writes)  # the delta keeps every batch: no compaction
    cs.load_history(kb, ko, vers, 0)
    rng = np.random.default_rng(7)
    now = start
    for _ in range(a.batches):
        now += p.version_step
        b = C.ConflictBatch(cs, None)
        b.add_packed(make(rng, now))
        b.detect_conflicts(now, now - p.window)
        b.close()
    now += p.version_step
    pb = make(rng, now)
    ranges = [(pb.read_range(r).begin, pb.read_range(r).end) for r in range(pb.n_reads)]
    dev = torch.zeros(pb.n_reads, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    srng = np.random.default_rng(11)
    check_us, check1_us, q_us, host_us, dev_host_us = [], [], [], [], []
    ok = True
    for r in range(a.warmup + a.rounds):
        b = C.ConflictBatch(cs, None)
        b.add_packed(pb)
        b.upload()
        ck = b.debug_kernel_time(0, a.reps)
        ck1 = sorted(b.debug_kernel_time(0, 1) for _ in range(a.reps))[a.reps // 2]
        t0 = time.perf_counter()
        V = b.read_versions()
        t1 = time.perf_counter()
        ks, hs = [], []
        for _ in range(a.reps):
            b.read_versions_device(dev.data_ptr(), pb.n_reads)
            kern, host = b.read_versions_timing()
            ks.append(kern * 1e3)
            hs.append(host * 1e3)
        ok &= bool((dev.cpu().numpy() == V).all()) and len(V) == pb.n_reads
        for i in srng.choice(pb.n_reads, size=min(a.sample, pb.n_reads), replace=False).tolist():
            lo, hi = ranges[i]
            want = M.of_dump(cs.dump_history(lo, hi), [(lo, hi)])[0] if lo < hi else None
            ok &= want is None or want == int(V[i])
        b.close()
        if r >= a.warmup:
            check_us.append(ck)
            check1_us.append(ck1)
            q_us.append(sorted(ks)[len(ks) // 2])
            dev_host_us.append(sorted(hs)[len(hs) // 2])
            host_us.append((t1 - t0) * 1e6)
    out = {"bench": "read_versions", "shape": a.shape, "history": int(len(vers)), "batches": a.batches,
           "boundaries": int(cs.history_size()), "reads": int(pb.n_reads), "rounds": a.rounds, "reps": a.reps,
           "check_kernel_us": summary(check_us), "check_single_launch_us": summary(check1_us),
           "query_kernel_us": summary(q_us),
           "query_host_form_wall_us": summary(host_us), "query_device_form_call_us": summary(dev_host_us),
           "equal": bool(ok)}
    out["query_over_check"] = out["query_kernel_us"]["median"] / out["check_kernel_us"]["median"]
    out["query_over_check_single_launch"] = out["query_kernel_us"]["median"] / out["check_single_launch_us"]["median"]
    # 1000 ranges through the set's own call, against a dump of the same set
    t0 = time.perf_counter()
    got = cs.read_versions(ranges[:1000])
    t1 = time.perf_counter()
    dump = cs.dump_history()
    t2 = time.perf_counter()
    out["set_read_versions_1000_us"] = (t1 - t0) * 1e6
    out["dump_history_us"] = (t2 - t1) * 1e6
    out["dump_bytes"] = int(sum(x.nbytes for x in dump[:3]))
    ok &= len(got) == min(1000, len(ranges))
    cs.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
