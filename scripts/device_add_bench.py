"""The add in the loop, from the host and from device memory: fdbcs_batch_add_packed against
fdbcs_batch_add_packed_device on the same batches, in the Resolver's order (add, then detect).

`--steps` batches of the C2 or C4 shape (workloads.py) over a prefilled history, `--window` batches
in flight, `--repeats` runs of each path, alternating in one process on two sets that see the same
sequence (the versions move on from repeat to repeat; the keys are reused).  Three paths:

  host          add_packed of the host arrays (every key read and normalized on the CPU, then H2D)
  device        add_packed_device of arrays already resident in device memory (staged before the clock)
  device+h2d    the same, with the six raw arrays copied H2D (pinned, async) inside the loop and the
                add kernels behind a ready flag the copying stream sets

The device paths issue batch i + 1's add before batch i's detect (detect blocks until the batch's
add kernels have run), as the routed path is driven.  The verdicts of every batch are compared
between the paths.  Per path: transactions per second, host milliseconds per batch inside the add
call (fdbcs_stats host_ms_add / fdbcs_batch_device_add_timing ms_host) and, for the device paths,
the add kernels' device milliseconds per batch (events around them).  --kernel-stats takes the
kernel_stats CSV of a `rocprofv3 --kernel-trace --stats` run of this script and adds the add
kernels' average durations to the record.

    python3 scripts/device_add_bench.py [--workload c2|c4] [--steps N] [--window W] [--repeats R]
                                        [--history N] [--out FILE] [--kernel-stats CSV]

Prints one JSON line (and appends it to FILE)."""
import argparse
import csv
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
from foundationdb_amd.packing import DevicePackedBatch, PackedBatch  # noqa: E402

FIELDS = ("read_snapshot", "report", "read_offsets", "write_offsets", "key_bytes", "key_offsets")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


class Slot:
    """Device tensors sized for the largest batch, and the ready flag of the copies into them."""

    def __init__(self, batches):
        self.t = {f: torch.empty(max(getattr(pb, f).nbytes for pb in batches) + 8, dtype=torch.uint8, device="cuda")
                  for f in FIELDS}
        self.flag = torch.zeros(2, dtype=torch.int32, device="cuda")

    def dpb(self, pb):
        p = {f: self.t[f].data_ptr() for f in FIELDS}
        return DevicePackedBatch(pb.n_txn, pb.n_reads, pb.n_writes, pb.key_bytes.nbytes, p["read_snapshot"], p["report"],
                                 p["read_offsets"], p["write_offsets"], p["key_bytes"], p["key_offsets"])


def resident(pb):
    """pb's arrays as device tensors of their own (kept alive by the caller) and the struct over them."""
    t = {f: torch.from_numpy(getattr(pb, f).view(np.uint8).reshape(-1).copy()).cuda() for f in FIELDS}
    p = {f: t[f].data_ptr() for f in FIELDS}
    return t, DevicePackedBatch(pb.n_txn, pb.n_reads, pb.n_writes, pb.key_bytes.nbytes, p["read_snapshot"], p["report"],
                                p["read_offsets"], p["write_offsets"], p["key_bytes"], p["key_offsets"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c2", "c4"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--history", type=int, default=0, help="prefilled boundaries; 0 = the workload's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    start = 10_000_000
    if a.workload == "c2":
        p = W.C2Params(**({"history": a.history} if a.history else {}))
        hist = W.c2_history(p, seed=1, start_version=start)
        gen = lambda rng, now: W.c2_batch(p, rng, now)
    else:
        p = W.C4Params(**({"history": a.history} if a.history else {}))
        hist = W.c4_history(p, seed=1, start_version=start)
        gen = lambda rng, now: W.c4_batch(p, rng, now)
    rng = np.random.default_rng(7)
    base = [gen(rng, start + (i + 1) * p.version_step) for i in range(a.steps)]
    T = base[0].n_txn
    sets = {k: C.ConflictSet(0) for k in ("host", "device")}
    for cs in sets.values():
        cs.load_history(*hist, 0)
    pinned = [{f: torch.from_numpy(getattr(pb, f).view(np.uint8).reshape(-1).copy()).pin_memory() for f in FIELDS}
              for pb in base]
    keep = [resident(pb) for pb in base]  # the resident path's key arrays: reused by every repeat
    slots = [Slot(base) for _ in range(3)]
    torch.cuda.synchronize()
    copy_stream = torch.cuda.Stream()

    def shifted(i, rep):
        """Batch i of repeat rep: the same ranges, snapshots and `now` moved on by the repeat."""
        d = rep * a.steps * p.version_step
        pb = base[i]
        return (PackedBatch(pb.read_snapshot + np.int64(d), pb.report, pb.read_offsets, pb.write_offsets, pb.key_bytes,
                            pb.key_offsets), start + (i + 1) * p.version_step + d)

    def run(path, cs, rep):
        """One pass over the batches; (seconds, verdicts, host ms in add per batch, kernel ms per batch)."""
        seq = [shifted(i, rep) for i in range(a.steps)]
        snaps = None
        if path == "device":  # resident arrays: this repeat's snapshots staged before the clock
            snaps = [torch.from_numpy(pb.read_snapshot).cuda() for pb, _ in seq]
            torch.cuda.synchronize()
        before = cs.stats()["host_ms_add"]
        verdicts, inflight, add_ms, kern_ms = [None] * a.steps, [], 0.0, 0.0
        pending = None

        def retire(j, b):
            nonlocal add_ms, kern_ms
            verdicts[j] = b.wait()
            if path != "host":
                k, h = b.device_add_timing()
                add_ms += h
                kern_ms += k
            b.close()

        def detect(j, b):
            b.detect_async(seq[j][1], seq[j][1] - p.window)
            inflight.append((j, b))
            while len(inflight) >= a.window:
                retire(*inflight.pop(0))

        t0 = time.perf_counter()
        for i, (pb, now) in enumerate(seq):
            b = C.ConflictBatch(cs, None)
            if path == "host":
                b.add_packed(pb)
                detect(i, b)
                continue
            if path == "device":
                d = keep[i][1]
                b.add_packed_device(DevicePackedBatch(**{**d.__dict__, "read_snapshot": snaps[i].data_ptr()}))
            else:
                sl = slots[i % len(slots)]
                with torch.cuda.stream(copy_stream):
                    for f in FIELDS:
                        src = pinned[i][f] if f != "read_snapshot" else torch.from_numpy(pb.read_snapshot.view(np.uint8))
                        sl.t[f][: src.numel()].copy_(src, non_blocking=True)
                    sl.flag.fill_(i + 1)
                b.add_packed_device(sl.dpb(pb), sl.flag.data_ptr(), i + 1)
            if pending is not None:
                detect(*pending)
            pending = (i, b)
        if pending is not None:
            detect(*pending)
        for j, b in inflight:
            retire(j, b)
        dt = time.perf_counter() - t0
        if path == "host":
            add_ms = cs.stats()["host_ms_add"] - before
        return dt, verdicts, add_ms / a.steps, kern_ms / a.steps

    paths = [("host", sets["host"]), ("device", sets["device"])]
    res = {k: {"txns_per_s": [], "host_ms_add": [], "add_kernels_ms": []} for k in ("host", "device", "device+h2d")}
    same = True
    # warm-up repeat 0 on both sets, then the timed repeats, the paths alternating; the device set
    # takes the resident and the copying pass in turn (each pass moves its versions on)
    rep = 0
    for name, cs in paths:
        run(name, cs, rep)
    for r in range(a.repeats):
        for name in ("device", "device+h2d"):
            rep += 1
            got = {}
            for pname, cs in (("host", sets["host"]), (name, sets["device"])):
                dt, v, add_ms, kern_ms = run(pname, cs, rep)
                got[pname] = v
                res[pname]["txns_per_s"].append(a.steps * T / dt)
                res[pname]["host_ms_add"].append(add_ms)
                if pname != "host":
                    res[pname]["add_kernels_ms"].append(kern_ms)
            same &= all((x == y).all() for x, y in zip(got["host"], got[name]))
    for cs in sets.values():
        cs.close()
    out = {"bench": "device_add", "workload": a.workload, "txns": T, "reads": base[0].n_reads, "writes": base[0].n_writes,
           "key_bytes": int(base[0].key_bytes.nbytes), "history": int(len(hist[2])), "steps": a.steps,
           "window": a.window, "repeats": a.repeats, "verdicts": "equal" if same else "different"}
    for k, v in res.items():
        out[k] = {m: summary(x) for m, x in v.items() if x}
        out[k]["txns_per_s_all"] = [round(x) for x in v["txns_per_s"]]
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "ingest" in r.get("Name", "") or "IngestScan" in r.get("Name", "")]
        out["rocprofv3_kernels"] = [{"name": r["Name"].split("(")[0][:80], "calls": int(r["Calls"]),
                                     "avg_us": float(r["AverageNs"]) / 1e3} for r in rows]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
