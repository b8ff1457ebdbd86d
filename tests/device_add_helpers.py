"""GPU-side helpers of the device-add tests: a packed batch staged as torch device tensors, every
array between 64 bytes of 0xFF poison, and a driver that feeds one batch to a set through
add_packed, to a second set through add_packed_device and to the semantic oracle."""
import numpy as np

from foundationdb_amd.packing import DevicePackedBatch, PackedBatch, pack_keys
from tests.export_helpers import canon, split_dump

POISON = 64


def repack(pb, keys=None, **arrays):
    """pb with its keys (a list of bytes) or whole arrays replaced; nothing is validated."""
    kb, ko = (pb.key_bytes, pb.key_offsets) if keys is None else pack_keys(keys)
    f = {"read_snapshot": pb.read_snapshot, "report": pb.report, "read_offsets": pb.read_offsets,
         "write_offsets": pb.write_offsets, "key_bytes": kb, "key_offsets": ko}
    f.update(arrays)
    out = PackedBatch.__new__(PackedBatch)  # (the constructor asserts the shapes a tampered batch breaks)
    for k, v in f.items():
        setattr(out, k, np.ascontiguousarray(v))
    return out


def keys_of(pb):
    return [pb.key(k) for k in range(len(pb.key_offsets) - 1)]


class Staged:
    """pb's six arrays in device memory.  key_bytes starts `shift` bytes (0..7) into its tensor's
    payload and `base` filler bytes precede the first key (key_offsets[0] = base); the sizes default
    to the batch's own (n_reads / n_writes from the last offsets) unless given."""

    def __init__(self, torch, pb, shift=0, base=0, with_report=True, sizes=None, sync=True):
        self.tensors = []

        def put(a, lead=0):
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            host = np.full(POISON + lead + len(raw) + POISON, 0xFF, np.uint8)
            host[POISON + lead: POISON + lead + len(raw)] = raw
            t = torch.from_numpy(host).to("cuda")
            self.tensors.append(t)
            assert t.data_ptr() % 8 == 0
            return t.data_ptr() + POISON + lead

        T = len(pb.read_snapshot)
        R, W = (int(pb.read_offsets[-1]), int(pb.write_offsets[-1])) if sizes is None else sizes
        arena = np.concatenate([np.full(base, 0xFF, np.uint8), pb.key_bytes])
        self.dpb = DevicePackedBatch(
            T, R, W, len(arena),
            put(pb.read_snapshot.astype(np.int64)), put(pb.report.astype(np.uint8)) if with_report else 0,
            put(pb.read_offsets.astype(np.int32)), put(pb.write_offsets.astype(np.int32)),
            put(arena, lead=shift), put((pb.key_offsets + base).astype(np.int64)))
        if sync:
            torch.cuda.synchronize()

    def intact(self, torch):
        """The poison on both sides of every tensor is untouched."""
        return all(bool((t[:POISON] == 0xFF).all()) and bool((t[-POISON:] == 0xFF).all()) for t in self.tensors)


def batch_results(b, v):
    """Everything a detected batch reports: verdicts, conflicting reads per transaction, entries."""
    return (v.tolist(), [b.conflicting_reads(t) for t in range(len(v))], b.report_entries().tolist())


class Trio:
    """A set fed by add_packed, a set fed by add_packed_device and the oracle, step by step."""

    def __init__(self, engine, oracle_mod, torch, history=None):
        self.E, self.torch = engine, torch
        self.h, self.d = engine.ConflictSet(0), engine.ConflictSet(0)
        self.o = oracle_mod.OracleConflictSet()
        self.header = 0
        for s in (self.h, self.d):
            s.set_gc_interval(1)
        if history is not None:
            for s in (self.h, self.d, self.o):
                s.load_history(*history)
            self.header = history[3]

    def close(self):
        self.h.close()
        self.d.close()

    def host(self, pb, now, oldest, report=True):
        m = {} if report else None
        b = self.E.ConflictBatch(self.h, m)
        b.add_packed(pb)
        v = b.detect_conflicts(now, oldest)
        out = batch_results(b, v), m
        b.close()
        return out

    def device(self, pb, now, oldest, report=True, **stage):
        m = {} if report else None
        st = Staged(self.torch, pb, **stage)
        b = self.E.ConflictBatch(self.d, m)
        b.add_packed_device(st.dpb)
        v = b.detect_conflicts(now, oldest)
        out = batch_results(b, v), m
        b.close()
        assert st.intact(self.torch)
        return out

    def step(self, pb, now, oldest, report=True, what=None, **stage):
        """One batch through all three; returns the verdicts."""
        (hv, hr, he), hm = self.host(pb, now, oldest, report)
        (dv, dr, de), dm = self.device(pb, now, oldest, report, **stage)
        ov, oc = self.o.detect(pb, now, oldest)
        assert dv == hv == ov.tolist(), (what, [t for t in range(len(hv)) if dv[t] != hv[t] or dv[t] != ov[t]][:10])
        assert dr == hr and de == he and dm == hm, what
        if report:
            assert dm == oc, what
        return ov

    def check_state(self, what=None):
        """The two sets' dumps are bit-exact and equal to the canonical form of the oracle's state."""
        a, b = self.h.dump_history(), self.d.dump_history()
        for x, y in zip(a[:3], b[:3]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), what
        assert a[3] == b[3], what
        keys, vers = self.o.dump_history()
        assert split_dump(b) == canon(keys, vers, self.header, self.o.oldest_version), what
        return b


def random_batch(rng, T, reads, writes, width, now, alphabet=12, stale=6, report_frac=0.3):
    """T transactions of `reads` + `writes` ranges [k, k + 1) over keys of `width` bytes that share all
    but their last two bytes (every comparison runs to the end of the key)."""
    n = T * (reads + writes)
    mat = np.full((2 * n, width), 0x41, np.uint8)
    mat[0::2, -2:] = rng.integers(1, alphabet, size=(n, 2))
    mat[1::2] = mat[0::2]
    mat[1::2, -1] += 1
    roff = np.arange(T + 1, dtype=np.int32) * reads
    woff = np.arange(T + 1, dtype=np.int32) * writes
    snap = now - rng.integers(0, stale, size=T)
    rep = (rng.random(T) < report_frac).astype(np.uint8)
    return PackedBatch.from_key_matrix(snap, roff, woff, mat, np.full(2 * n, width), rep)
