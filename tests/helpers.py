"""Shared test helpers: golden fixture loading and a uniform driver over the oracle / HIP engine."""
import json
import os

import numpy as np

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def scenario_batches(scn):
    """Yield (PackedBatch, now, new_oldest, expect, conflicting) per batch of a KAT scenario."""
    for b in scn["batches"]:
        txns = []
        for t in b["txns"]:
            txns.append(
                CommitTransaction(
                    [KeyRange(bytes.fromhex(x), bytes.fromhex(y)) for x, y in t["reads"]],
                    [KeyRange(bytes.fromhex(x), bytes.fromhex(y)) for x, y in t["writes"]],
                    t["snapshot"],
                    t["report"],
                )
            )
        conf = {int(k): v for k, v in b.get("conflicting", {}).items()}
        yield PackedBatch.from_transactions(txns), b["now"], b["new_oldest"], b["expect"], conf


def random_fixture_sequences():
    z = np.load(os.path.join(GOLDEN, "random_batches.npz"))
    seqs, nb = (int(x) for x in z["meta"])
    for s in range(seqs):
        seq = []
        for b in range(nb):
            p = f"s{s}b{b}_"
            pb = PackedBatch(z[p + "snap"], z[p + "report"], z[p + "roff"], z[p + "woff"], z[p + "kb"], z[p + "ko"])
            now, no = (int(x) for x in z[p + "now"])
            ct = z[p + "conf_txn"]
            co = z[p + "conf_off"]
            ci = z[p + "conf_idx"]
            conf = {int(ct[i]): ci[co[i] : co[i + 1]].tolist() for i in range(len(ct))}
            seq.append((pb, now, no, z[p + "verdict"], conf))
        yield s, seq


class EngineDriver:
    """Runs packed batches through the HIP engine's Python mirror of ConflictBatch."""

    def __init__(self, cs_module, device=0, gc_interval=1, delta_limit=0):
        self.C = cs_module
        self.cs = cs_module.ConflictSet(device)
        self.cs.set_gc_interval(gc_interval)
        self.cs.set_delta_limit(delta_limit)

    def clear(self, v):
        self.cs.clear(v)

    def load_history(self, kb, ko, vers, header=0):
        self.cs.load_history(kb, ko, vers, header)

    def detect(self, pb, now, new_oldest):
        m = {}
        b = self.C.ConflictBatch(self.cs, m)
        b.add_packed(pb)
        v = b.detect_conflicts(now, new_oldest)
        b.close()
        return v, {t: sorted(x) for t, x in m.items()}


def nonempty(conf):
    return {t: sorted(v) for t, v in conf.items() if v}


def list_scenarios():
    """Scenarios for the verdict-list tests (SkipList.cpp:869-876): every KAT scenario plus random
    sequences whose snapshots straddle the oldest version (TooOld transactions in most batches).
    Each scenario is a list of steps ("clear", version) or ("batch", PackedBatch, now, new_oldest)."""
    from foundationdb_amd import workloads as W

    out = []
    for scn in load_json("kat_scenarios.json"):
        steps = []
        for i, (pb, now, no, _, _) in enumerate(scenario_batches(scn)):
            if scn.get("clear_before") == i:
                steps.append(("clear", scn["clear_version"]))
            steps.append(("batch", pb, now, no))
        out.append(steps)
    rng = np.random.default_rng(869)
    for s in range(4):
        steps, now = [], 20
        for _ in range(6):
            pb = W.random_small_batch(rng, int(rng.integers(5, 40)), alphabet=3, max_len=2, now=now, staleness=25)
            steps.append(("batch", pb, now, now - 10))
            now += 4
        out.append(steps)
    return out


def write_list_file(scenarios, path):
    """The scenarios in tests/cpp/shim_driver.cpp's --lists format."""
    lines = []
    for steps in scenarios:
        lines.append("S")
        for st in steps:
            if st[0] == "clear":
                lines.append(f"C {st[1]}")
                continue
            _, pb, now, no = st
            txns = pb.to_transactions()
            lines.append(f"B {now} {no} {len(txns)}")
            for t in txns:
                keys = []
                for r in list(t.read_conflict_ranges) + list(t.write_conflict_ranges):
                    keys += [bytes(r.begin).hex() or "-", bytes(r.end).hex() or "-"]
                lines.append(f"T {t.read_snapshot} {int(bool(t.report_conflicting_keys))} "
                             f"{len(t.read_conflict_ranges)} {len(t.write_conflict_ranges)} " + " ".join(keys))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def oracle_scenario_lists(oracle_mod, scenarios):
    """Per batch: (nonConflicting, tooOld) with a tooOld list and nonConflicting without one, from
    the oracle's restatement of SkipList.cpp:869-876."""
    out = []
    for steps in scenarios:
        cs = oracle_mod.OracleConflictSet()
        res = []
        for st in steps:
            if st[0] == "clear":
                cs.clear(st[1])
                continue
            _, pb, now, no = st
            v, _ = cs.detect(pb, now, no)
            nc, to = cs.last_lists(True)
            nc2, _ = cs.last_lists(False)
            res.append((v, nc, to, nc2))
        out.append(res)
    return out


# ---- sequences shared by the verdict tests (test_gpu_parity.py) and the stored-state tests
# (test_gpu_state_paths.py): one copy, so both run the same batches


def prefixed(pb, prefix):
    """The same batch with `prefix` prepended to every key (order and overlaps unchanged)."""
    lens = np.diff(pb.key_offsets)
    parts = [np.frombuffer(prefix, np.uint8)]
    out = []
    for k in range(len(lens)):
        out.append(parts[0])
        out.append(pb.key_bytes[pb.key_offsets[k] : pb.key_offsets[k + 1]])
    kb = np.concatenate(out) if out else np.zeros(0, np.uint8)
    ko = np.concatenate([[0], np.cumsum(lens + len(prefix))]).astype(np.int64)
    return PackedBatch(pb.read_snapshot, pb.report, pb.read_offsets, pb.write_offsets, kb, ko)


# Every engine knob that selects a different kernel or submission path (DESIGN.md §5 "Engine knobs").
PIPELINE_KNOBS = [{"FDBCS_SPLIT_CHECK": "1"}, {"FDBCS_SPLIT_CHECK": "0"},
                  {"FDBCS_SORT_COLD": "1"},
                  {"FDBCS_SUBMIT_THREAD": "0", "FDBCS_SPLIT_CHECK": "1"}, {"FDBCS_SUBMIT_THREAD": "0"},
                  {"FDBCS_WRITE_GROUPS": "0"}, {"FDBCS_SERIAL": "1"},
                  {"FDBCS_DIRECTORY": "0"}, {"FDBCS_SKIP_EDGES": "0"}]

SORT_BUCKETS = [("3000", "0"), ("600", "0"), ("40", "0"), ("160", "1"), ("64", "1"), ("8", "0")]


class knob_env:
    """Engine knobs in the environment while a set is created (they are read at creation)."""

    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.knobs}
        os.environ.update(self.knobs)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def pipeline_variant_batches():
    """20 batches of (PackedBatch, now, new_oldest): keys up to 3 bytes, up to 24 (short-key lookups)
    and up to 40 (long-key lookups) in some batches."""
    from foundationdb_amd import workloads as W

    rng = np.random.default_rng(71)
    now = 10
    for i in range(20):
        pb = W.random_small_batch(rng, 250, alphabet=6 if i % 2 else 200,
                                  max_len=24 if i % 3 == 0 else (40 if i % 5 == 1 else 3), now=now, staleness=12)
        yield pb, now, now - 9
        now += 4


def sort_bucket_batches():
    """6 batches of 700 transactions; every second one behind a shared 17-byte prefix (prefix ties
    resolved by the tail bytes, warm splitters that no longer fit the keys)."""
    from foundationdb_amd import workloads as W

    rng = np.random.default_rng(31)
    seq = []
    now = 10
    for i in range(6):
        pb = W.random_small_batch(rng, 700, alphabet=3, max_len=4, now=now, staleness=10, report_frac=0.5)
        if i % 2:
            pb = prefixed(pb, b"\x02tenant\x00orders\x00\x15\x01")
        seq.append((pb, now, now - 3))
        now += 2
    return seq


def sequential_fallback_batches():
    """4 batches dense enough to overflow a candidate-edge capacity of 8 (FDBCS_EDGE_CAP)."""
    from foundationdb_amd import workloads as W

    rng = np.random.default_rng(8)
    seq = []
    now = 10
    for _ in range(4):
        seq.append((W.random_small_batch(rng, 100, alphabet=2, max_len=3, now=now, staleness=10, report_frac=1.0),
                    now, now - 3))
        now += 2
    return seq


def shift_batch(pb, D):
    """The same batch with D added to every read snapshot (the version axis moved by D)."""
    return PackedBatch(pb.read_snapshot + np.int64(D), pb.report, pb.read_offsets, pb.write_offsets, pb.key_bytes,
                       pb.key_offsets)
