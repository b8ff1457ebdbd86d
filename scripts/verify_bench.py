"""Device time of the stored-state check (fdbcs_history_verify) on a C2 history, per check group.

Two states of one set, as scripts/export_bench.py: the loaded base with an empty delta, and the same
base under the delta that `--batches` C2 batches leave (no compaction in between).  Per state and per
check group (the pass over keys and versions, the upper levels, the directories, the dominance
searches, and everything at once): 2 warm-up calls, then `--reps` timed ones; per rep the device time
of the verify's kernels (events around them) and the host time of the whole call.  The bytes a group
has to move come from the shapes (32 B per boundary for the block pass plus the derived entries it
compares; 8 B per boundary for the upper levels; one directory word and two group starts per slot; a
binary search per boundary of both tiers for dominance, counted as its 32 B operands only).

The yardstick is the engine's own passes that build what is checked, timed per kernel (timing level 3)
in the same run: k_epilogue<false> of the last delta batches for the delta, and for the base
k_epilogue<true> plus k_directory of one compaction at the end; for DOMINANCE that compaction's search.

    python3 scripts/verify_bench.py [--history N] [--batches B] [--reps R] [--out FILE]

Prints one JSON line (and appends it to FILE); exit status 1 if a report is not clean."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.is_available()
from foundationdb_amd import conflict_set as C  # noqa: E402
from foundationdb_amd import workloads as W  # noqa: E402

GROUPS = {
    "blocks": ("order", "padding", "tails", "versions", "lvl1", "skey8", "skey"),
    "upper": ("lvl2", "lvl3"),
    "directories": ("dir", "edir"),
    "dominance": ("dominance",),
    "all": None,
}


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def group_bytes(group, rep):
    nb, nd = rep.sizes
    n = nb + nd
    slots = rep.examined(0, "dir") + rep.examined(1, "edir")
    return {"blocks": 32 * n + 8 * (n // 64) + 16 * (n // 8) + 16 * (n // 56),
            "upper": 8 * n,
            "directories": 8 * slots + 32 * slots,
            "dominance": 32 * n if nd else 0}.get(group)


def measure(cs, warmup, reps):
    out, clean = {}, True
    for name, checks in GROUPS.items():
        dev, host = [], []
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            rep = cs.verify(checks)
            t1 = time.perf_counter()
            if r >= warmup:
                dev.append(cs.verify_timing()[0] * 1e3)
                host.append((t1 - t0) * 1e6)
        clean &= rep.ok
        out[name] = {"kernels_us": summary(dev), "call_us": summary(host)}
        b = group_bytes(name, rep) if name != "all" else sum(group_bytes(g, rep) for g in GROUPS if g != "all")
        out[name]["bytes"] = int(b)
        out[name]["achieved_GBps"] = b / (summary(dev)["median"] * 1e-6) / 1e9 if summary(dev)["median"] > 0 else 0.0
    out["sizes"] = list(rep.sizes)
    out["edir_trusted"] = rep.edir_trusted
    out["clean"] = bool(clean)
    return out


def per_launch(prof, *names):
    pick = {k: v for k, v in prof.items() if any(s in k for s in names)}
    return {k[:60]: v["ms"] * 1e3 / max(1, v["launches"]) for k, v in pick.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=5_000_000)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
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
    out = {"bench": "verify", "history": int(len(vers)), "batches": a.batches, "reps": a.reps,
           "empty_delta": measure(cs, a.warmup, a.reps)}
    rng = np.random.default_rng(7)
    now = start

    def batch():
        nonlocal now
        now += p.version_step
        b = C.ConflictBatch(cs, None)
        b.add_packed(W.c2_batch(p, rng, now))
        b.detect_conflicts(now, now - p.window)
        b.close()

    for i in range(a.batches):
        if i == max(a.batches - 5, 0):  # the yardstick of the delta: the last batches' epilogues
            cs.set_timing(3)
            cs.reset_stats()
        batch()
    out["yardstick_delta_us"] = per_launch(cs.kernel_profile(), "k_epilogue<false>")
    cs.set_timing(0)
    out["with_delta"] = measure(cs, a.warmup, a.reps)
    # the yardstick of the base and of the dominance searches: one compaction, per kernel
    cs.set_timing(3)
    cs.reset_stats()
    cs.set_gc_interval(1)
    batch()
    prof = cs.kernel_profile()
    print("kernels timed:", sorted(prof), file=sys.stderr)
    out["yardstick_base_us"] = per_launch(prof, "k_epilogue<true>", "k_directory")
    out["yardstick_dominance_us"] = per_launch(prof, "k_compact_search")
    cs.set_timing(0)
    out["after_compaction_clean"] = bool(cs.verify().ok)
    yd = sum(out["yardstick_delta_us"].values()) + sum(out["yardstick_base_us"].values())
    out["ratio_all_to_builders"] = out["with_delta"]["all"]["kernels_us"]["median"] / yd if yd > 0 else None
    ok = out["empty_delta"]["clean"] and out["with_delta"]["clean"] and out["after_compaction_clean"]
    cs.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
