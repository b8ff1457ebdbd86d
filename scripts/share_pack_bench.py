"""A proxy's share packed by the host and by the GPU: fdbcs_share_pack from host arrays into pinned
memory plus the H2D copy of the share, against fdbcs_batch_share_pack_device from arrays already
resident in device memory, on the same batches.

`--steps` batches of the C2 or C4 shape (workloads.py), `--repeats` passes, the paths alternating
batch by batch in one process.  Per batch:

  host      host ms inside share_pack; end-to-end ms until the share is complete in device memory
            (the pack, then the asynchronous copy from pinned memory and its synchronize)
  device    host ms inside share_pack_device; device ms of its kernels (events around them);
            end-to-end ms from the call until share_pack_info has returned
  add       device ms of the kernels of fdbcs_batch_add_packed_device on the same arrays, the same
            scan with a padded store: the yardstick beside the pack's kernels

Each figure is averaged over a pass's batches; the record holds the median, minimum and maximum over
the passes.  The first pass also compares the two shares byte for byte.

On a GPU, each step under its own time limit:

    timeout -k 10 300 python3 scripts/share_pack_bench.py --workload c2 --out profiles/share_pack_bench.jsonl && \\
    timeout -k 10 300 python3 scripts/share_pack_bench.py --workload c4 --out profiles/share_pack_bench.jsonl

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
from foundationdb_amd.packing import DevicePackedBatch  # noqa: E402

FIELDS = ("read_snapshot", "report", "read_offsets", "write_offsets", "key_bytes", "key_offsets")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    start = 10_000_000
    if a.workload == "c2":
        p = W.C2Params(history=0)
        gen = lambda rng, now: W.c2_batch(p, rng, now)
    else:
        p = W.C4Params(history=0)
        gen = lambda rng, now: W.c4_batch(p, rng, now)
    rng = np.random.default_rng(7)
    base = [gen(rng, start + (i + 1) * p.version_step) for i in range(a.steps)]
    cap = max(C.share_bytes_bound(pb.n_txn, pb.n_reads, pb.n_writes, pb.key_bytes.nbytes) for pb in base)
    cs, cs_add = C.ConflictSet(0), C.ConflictSet(0)
    keep = [resident(pb) for pb in base]
    pin = torch.empty(cap, dtype=torch.uint8).pin_memory()
    pin_np = pin.numpy()
    dev_host = torch.zeros(cap, dtype=torch.uint8, device="cuda")  # the host path's share in device memory
    dev_pack = torch.zeros(cap, dtype=torch.uint8, device="cuda")  # the device path's
    assert dev_pack.data_ptr() % 64 == 0
    copy_stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    names = ("host_ms_in_call", "host_ms_end_to_end", "device_ms_in_call", "device_ms_kernels", "device_ms_end_to_end",
             "add_ms_kernels")
    res = {k: [] for k in names}
    same = True

    def one_pass(check):
        nonlocal same
        acc = dict.fromkeys(names, 0.0)
        for i, pb in enumerate(base):
            # host: pack into pinned memory, copy, wait
            if check:
                pin_np[:] = 0  # the host pack leaves the alignment gaps of its buffer as they are
            t0 = time.perf_counter()
            used = C.share_pack(pb, pin_np)
            t1 = time.perf_counter()
            with torch.cuda.stream(copy_stream):
                dev_host[: len(used)].copy_(pin[: len(used)], non_blocking=True)
            copy_stream.synchronize()
            t2 = time.perf_counter()
            acc["host_ms_in_call"] += 1e3 * (t1 - t0)
            acc["host_ms_end_to_end"] += 1e3 * (t2 - t0)
            # device: the kernels write the share where it is needed
            b = C.ConflictBatch(cs)
            t0 = time.perf_counter()
            b.share_pack_device(keep[i][1], dev_pack.data_ptr(), cap)
            n = b.share_pack_info()[0]
            t2 = time.perf_counter()
            kern, host = b.share_pack_timing()
            acc["device_ms_in_call"] += host
            acc["device_ms_kernels"] += kern
            acc["device_ms_end_to_end"] += 1e3 * (t2 - t0)
            b.close()
            if check:
                torch.cuda.synchronize()
                same &= n == len(used) and bool(torch.equal(dev_pack[:n], dev_host[:n]))
            # the device add's kernels on the same arrays
            b = C.ConflictBatch(cs_add)
            b.add_packed_device(keep[i][1])
            b.device_add_info()
            acc["add_ms_kernels"] += b.device_add_timing()[0]
            b.close()
        return {k: v / len(base) for k, v in acc.items()}

    one_pass(True)  # warm-up, and the byte comparison
    for _ in range(a.repeats):
        for k, v in one_pass(False).items():
            res[k].append(v)
    cs.close()
    cs_add.close()
    out = {"bench": "share_pack", "workload": a.workload, "txns": base[0].n_txn, "reads": base[0].n_reads,
           "writes": base[0].n_writes, "key_bytes": int(base[0].key_bytes.nbytes), "share_bytes": int(len(C.share_pack(base[0]))),
           "steps": a.steps, "repeats": a.repeats, "shares": "equal" if same else "different"}
    out.update({k: summary(v) for k, v in res.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
