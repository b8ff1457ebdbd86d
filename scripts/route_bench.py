"""Device routing alone (fdbcs_batch_add_routed) on one GPU: G proxy shares of a C2 (or C4) global
batch gathered in device memory, every resolver's split routed and timed with events (the engine's
ms_route_kernels), no collectives.  Prints one JSON line per G: routing kernels' device ms per
global batch per resolver, host ms of the call, and the routed sizes against the host routing.
--reports: every line twice in the same run, the batches created without and with report_keys (all
transactions reporting, a report output set: fdbcs_batch_set_report_output), plus the device ms of
detect (timing level 2, phases one after another) so routing + detect can be compared.
--map: routing under a keyResolvers map (fdbcs_batch_add_routed_map) against the static bounds, the
same C2 batches in one process, per resolver and repeat: (a) add_routed, (b) add_routed_map with the
equivalent one-entry-per-range map, (c) add_routed_map after resharding moves (about 4 G ranges,
histories 1-3 deep, move versions inside the snapshots' spread).  One JSON line per G with min /
median / max over the repeats of the routing kernels' device ms and of the call's host ms; (a) in
the same run is the yardstick.
Usage: python scripts/route_bench.py [--reports | --map] [c2|c4] [G ...]"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.is_available()
from foundationdb_amd import build, conflict_set as C, workloads as W  # noqa: E402
from foundationdb_amd.sharding import KeyRangeSharding, KeyResolvers  # noqa: E402

build.build()
with_map = "--map" in sys.argv
# --variants=add_routed,map_static,map_moved: the --map variants to run (all by default; one at a
# time under a kernel trace, so that the per-kernel times belong to that variant)
variants = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--variants=")]
argv = [a for a in sys.argv[1:] if a not in ("--reports", "--map") and not a.startswith("--variants=")]
with_reports = "--reports" in sys.argv
wl = argv[0] if argv else "c2"
Gs = [int(x) for x in argv[1:]] or [2, 4, 8]
NOW = 10_000_000


def moved_map(G, rng):
    """The uniform G-way map after resharding: random two-byte subranges moved to random resolvers
    at versions inside the snapshots' spread (C2: now - U[0, 100000)) until it has 4 G ranges, no
    history deeper than 3."""
    kr = KeyResolvers.from_sharding(KeyRangeSharding.uniform(G))
    k = 0
    while len(kr.bounds) < 4 * G:
        a = int(rng.integers(0, 65536))
        b = min(65535, a + int(rng.integers(1, 65536 // (2 * G))))  # narrow: the loads stay comparable
        if a == b:
            continue
        a, b = bytes([a >> 8, a & 255]), bytes([b >> 8, b & 255])
        trial = copy.deepcopy(kr)
        trial.apply_changes([(a, b, int(rng.integers(0, G)))], min(NOW - 1, NOW - 90_000 + 90_000 // (4 * G) * k))
        if max(len(h) for h in trial.hist) <= 3 and len(trial.bounds) <= 4 * G + 1:
            kr, k = trial, k + 1
    return kr


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 5), "median": round(xs[len(xs) // 2], 5), "max": round(xs[-1], 5)}


def run_map(G, repeats=7, per=10):
    rng = np.random.default_rng(G)
    p = W.C2Params(txns=5000 * G, history=0)
    sh = KeyRangeSharding.uniform(G)
    pb = W.c2_batch(p, rng, NOW)
    shares = [C.share_pack(pb.slice_txns(g * 5000, (g + 1) * 5000)) for g in range(G)]
    stride = (max(len(x) for x in shares) + 4095) // 4096 * 4096
    host = np.zeros(G * stride, np.uint8)
    for g, x in enumerate(shares):
        host[g * stride: g * stride + len(x)] = x
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(pb.n_txn, dtype=torch.uint8, device="cuda")
    ready = torch.ones(1, dtype=torch.int32, device="cuda")
    static = KeyResolvers.from_sharding(sh)
    moved = moved_map(G, np.random.default_rng(1000 + G))
    want = {"add_routed": sh.route(pb), "map_static": static.route(pb), "map_moved": moved.route(pb)}
    if variants:
        want = {v: want[v] for v in variants[0]}
    caps = (pb.n_txn, pb.n_reads, pb.n_writes, pb.tail_bytes)
    dev_ms = {v: [[] for _ in range(G)] for v in want}
    host_ms = {v: [[] for _ in range(G)] for v in want}
    now = NOW
    for r in range(G):
        cs = C.ConflictSet(0)
        lo = sh.splits[r - 1] if r > 0 else None
        hi = sh.splits[r] if r < G - 1 else None
        for k in range(repeats + 1):  # repeat 0 warms every variant up
            for v in want:
                cs.reset_stats()
                for _ in range(per):
                    b = C.ConflictBatch(cs)
                    args = (dev.data_ptr(), stride, G, 5000)
                    if v == "add_routed":
                        b.add_routed(*args, lo, hi, caps, out.data_ptr(), pb.n_txn, ready.data_ptr(), 1)
                    else:
                        b.add_routed_map(*args, static if v == "map_static" else moved, r, caps, out.data_ptr(),
                                         pb.n_txn, ready.data_ptr(), 1)
                    sub = want[v][r].batch
                    T, R, Wn, _, _ = b.routed_info()
                    assert (T, R, Wn) == (sub.n_txn, sub.n_reads, sub.n_writes), (v, r, T, R, Wn)
                    now += 1
                    b.detect_async(now, NOW // 2)
                    b.wait()
                    b.close()
                st = cs.stats()
                if k:
                    dev_ms[v][r].append(st["ms_route_kernels"] / st["routed_batches"])
                    host_ms[v][r].append(st["host_ms_route"] / st["routed_batches"])
        cs.close()
    # per repeat the slowest resolver, as the lines without --map report it
    line = {"workload": "c2", "resolvers": G, "global_txns": pb.n_txn, "share_stride": stride, "repeats": repeats,
            "batches_per_repeat": per, "moved_map_ranges": len(moved.bounds),
            "moved_map_history_depths": sorted({len(h) for h in moved.hist}), "sizes_match_host_routing": True}
    for v in want:
        line[v] = {"route_kernels_ms_per_batch": spread([max(dev_ms[v][r][k] for r in range(G)) for k in range(repeats)]),
                   "route_host_ms_per_batch": spread([max(host_ms[v][r][k] for r in range(G)) for k in range(repeats)]),
                   "routed_reads_max": max(x.batch.n_reads for x in want[v])}
    if "add_routed" in want:
        a = line["add_routed"]["route_kernels_ms_per_batch"]
        line["add_routed_spread_ms"] = round(a["max"] - a["min"], 5)
        for v in [v for v in want if v != "add_routed"]:
            line[v + "_minus_add_routed_ms"] = round(line[v]["route_kernels_ms_per_batch"]["median"] - a["median"], 5)
    print(json.dumps(line), flush=True)


if with_map:
    for G in Gs:
        run_map(G)
    sys.exit(0)
for G, reports in [(G, r) for G in Gs for r in ((False, True) if with_reports else (False,))]:
    rng = np.random.default_rng(G)
    if wl == "c4":
        p = W.C4Params(txns=5000 * G, history=0)
        sh = KeyRangeSharding([W.c4_user_split(p, g * p.users // G) for g in range(1, G)])
        pb = W.c4_batch(p, rng, 10_000_000)
    else:
        p = W.C2Params(txns=5000 * G, history=0)
        sh = KeyRangeSharding.uniform(G)
        pb = W.c2_batch(p, rng, 10_000_000)
    if reports:
        pb.report[:] = 1
    shares = [C.share_pack(pb.slice_txns(g * 5000, (g + 1) * 5000)) for g in range(G)]
    stride = (max(len(x) for x in shares) + 4095) // 4096 * 4096
    host = np.zeros(G * stride, np.uint8)
    for g, x in enumerate(shares):
        host[g * stride: g * stride + len(x)] = x
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(pb.n_txn, dtype=torch.uint8, device="cuda")
    rep_out = torch.empty(max(pb.n_reads, 1), dtype=torch.uint8, device="cuda")
    ready = torch.ones(1, dtype=torch.int32, device="cuda")  # set by torch's stream; polled by the engine
    tail = int(np.maximum(np.diff(pb.key_offsets) - 16, 0).sum())
    routes = sh.route(pb)
    res = []
    for r in range(G):
        cs = C.ConflictSet(0)
        lo = sh.splits[r - 1] if r > 0 else None
        hi = sh.splits[r] if r < G - 1 else None
        for rep in range(24 if with_reports else 12):
            if rep == 2:
                cs.reset_stats()
            if rep == 12:  # second pass: detect's device time, phase by phase
                st = cs.stats()
                cs.set_timing(2)
            if rep == 14:
                cs.reset_stats()
            b = C.ConflictBatch(cs, {} if reports else None)
            b.add_routed(dev.data_ptr(), stride, G, 5000, lo, hi, (pb.n_txn, pb.n_reads, pb.n_writes, tail),
                         out.data_ptr(), pb.n_txn, ready.data_ptr(), 1)
            if reports:
                b.set_report_output(rep_out.data_ptr(), pb.n_reads)
            T, R, Wn, _, _ = b.routed_info()
            sub = routes[r].batch
            assert (T, R, Wn) == (sub.n_txn, sub.n_reads, sub.n_writes), (T, R, Wn, sub.n_txn)
            b.detect_async(10_000_000 + rep, 5_000_000)
            b.wait()
            b.close()
        st2 = cs.stats()
        if not with_reports:
            st = st2
        res.append((st["ms_route_kernels"] / st["routed_batches"], st["host_ms_route"] / st["routed_batches"],
                    st2["ms_total"] / st2["batches"]))
        cs.close()
    extra = {"reports": reports, "detect_ms_per_batch": max(x[2] for x in res),
             "route_plus_detect_ms_per_batch": max(x[0] + x[2] for x in res)} if with_reports else {}
    print(json.dumps({**extra, "workload": wl, "resolvers": G, "global_txns": pb.n_txn, "share_stride": stride,
                      "route_kernels_ms_per_batch": max(x[0] for x in res),
                      "route_kernels_ms_mean": sum(x[0] for x in res) / G,
                      "route_host_ms_per_batch": max(x[1] for x in res), "sizes_match_host_routing": True}),
          flush=True)
