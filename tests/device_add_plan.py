"""Directed batches for the device add (fdbcs_batch_add_packed_device): every key length at which
the normalization takes another path, with a loaded history placed so that a key mangled on its way
into the batch changes a verdict (reads) or the stored state (writes).

Key classes by length: 0, 1, 7, 8, 9, 15, 16, 17, 18, 19, 20, 23, 24, 25, 31, 32, 33, 40, 63, 64,
65, 200 and, around 16, the zero-padding ties k\\0 and k\\0\\0 of a 16-byte k (equal 16-byte
prefixes: the length decides).

Every class but the empty key has two keys, each alone in a region of the key space that its first
byte names (region i: first byte 0x10 + 2 i), with its byte-order neighbours pred < key < succ
(succ = key + \\0, the immediate successor; pred = the key without a trailing \\0, else the key with
its last byte one lower) loaded at three distinct versions, 1000 (i + 1) + ...:

  key A, read as a range's BEGIN, [kA, E) with E = the region's end marker (first byte + 1):
      pred +30, kA +20, succ +10.  The span's maximum is kA's own version.  A begin that moved down
      takes in pred's greater version (the read at the maximum now conflicts); one that moved up
      leaves kA out (the read one below the maximum now commits).
  key B, read as a range's END, ["", kB):
      pred +10, kB +20, succ +5, and every region's versions lie above all lower regions', so the
      span's maximum is pred's version.  An end that moved up takes in kB's greater version; one
      that moved down to pred or below leaves pred's segment out.

The empty key has no neighbour below: it is the first boundary (20), \\0 follows at 10, and the
set's header (15) is what the one range it can end, the empty range ["", ""), reads (an empty range
reads the segment below its key, SkipList.cpp:650-666); one \\0 appended takes in the key itself.

The four mutations (last byte dropped, last byte zeroed, one \\0 appended, bytes [16, len) rotated
by one) are undefined where there is no byte to drop or zero, and where they map the key to itself
(zeroing a trailing \\0, rotating fewer than two bytes or equal bytes): nothing could tell those
apart.  Every mutated read endpoint stays inside its range's other bound, so a mutated read batch is
always valid.  The writes are [k, k\\0) of both keys of every class; a mangled write key shows in
the stored history, and a mutation that inverts the write (a begin that moved above k\\0) is refused
outright, which is a change too.
"""
import numpy as np

from foundationdb_amd.packing import CommitTransaction, KeyRange, PackedBatch, pack_keys

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 18, 19, 20, 23, 24, 25, 31, 32, 33, 40, 63, 64, 65, 200]
TIES = [1, 2]  # trailing \0 bytes after a 16-byte key
HEADER = 15
NOW_READS, NOW_WRITES, NOW_REREADS = 100000, 100010, 100020
OLDEST_AFTER_READS = 50  # new_oldest_version of the first batch: later snapshots below it are TooOld
MUTATIONS = ("drop", "zero", "append", "rotate")


def _body(region, n):
    """n bytes starting with the region's first byte; the others in [2, 252], neighbours distinct."""
    fb = 0x10 + 2 * region
    return bytes([fb] + [(37 * j + 11 * region) % 251 + 2 for j in range(1, n)])


def pred_of(k):
    return k[:-1] if k.endswith(b"\x00") else k[:-1] + bytes([k[-1] - 1])


def mutate(k, how):
    """The mutated key, or None where the mutation is undefined or maps the key to itself."""
    if how == "drop":
        m = k[:-1] if k else None
    elif how == "zero":
        m = k[:-1] + b"\x00" if k else None
    elif how == "append":
        m = k + b"\x00"
    else:
        m = k[:16] + k[17:] + k[16:17] if len(k) > 16 else None
    return None if m is None or m == k else m


class KeyClass:
    def __init__(self, name, index, n, zeros=0):
        self.name, self.n = name, n + zeros
        self.empty = self.n == 0
        if self.empty:
            self.ra = self.rb = None
            self.ka = self.kb = b""
            self.end_a = b"\x01"
            return
        self.ra, self.rb = 2 * index, 2 * index + 1  # regions of key A and key B
        self.ka = _body(self.ra, n) + b"\x00" * zeros
        self.kb = _body(self.rb, n) + b"\x00" * zeros
        self.end_a = bytes([0x10 + 2 * self.ra + 1])

    def history(self):
        """(key, version) boundaries of this class, ascending."""
        if self.empty:
            return [(b"", 20), (b"\x00", 10)]
        out = []
        for k, r, (vp, vk, vs) in ((self.ka, self.ra, (30, 20, 10)), (self.kb, self.rb, (10, 20, 5))):
            base = 1000 * (r + 1)
            out += [(pred_of(k), base + vp), (k, base + vk), (k + b"\x00", base + vs)]
        return out

    def max_a(self):
        return 20 if self.empty else 1000 * (self.ra + 1) + 20

    def max_b(self):
        return HEADER if self.empty else 1000 * (self.rb + 1) + 10

    def reads(self, ka=None, kb=None):
        """The class's four read transactions: [kA, E) and ["", kB), each at its span's maximum
        (commits) and one below (conflicts)."""
        ka = self.ka if ka is None else ka
        kb = self.kb if kb is None else kb
        mb = self.max_b()
        return [CommitTransaction([KeyRange(ka, self.end_a)], [], self.max_a(), True),
                CommitTransaction([KeyRange(ka, self.end_a)], [], self.max_a() - 1, True),
                CommitTransaction([KeyRange(b"", kb)], [], mb, True),
                CommitTransaction([KeyRange(b"", kb)], [], mb - 1, True)]

    def want_reads(self):
        return [2, 0, 2, 0]


def classes():
    out = []
    for n in LENGTHS:
        out.append(KeyClass(f"len{n}", len(out), n))
    for z in TIES:
        out.append(KeyClass(f"tie16+{z}", len(out), 16, z))
    return out


CLASSES = classes()


def history():
    """(key_bytes, key_offsets, versions, header) of the loaded history."""
    b = sorted(x for c in CLASSES for x in c.history())
    keys = [k for k, _ in b]
    assert all(x < y for x, y in zip(keys, keys[1:]))
    kb, ko = pack_keys(keys)
    return kb, ko, np.array([v for _, v in b], np.int64), HEADER


def read_batch(override=None):
    """Every class's reads; override = (class index, "a" | "b", key) replaces one key."""
    txns = []
    for i, c in enumerate(CLASSES):
        kw = {}
        if override and override[0] == i:
            kw = {"k" + override[1]: override[2]}
        txns += c.reads(**kw)
    return PackedBatch.from_transactions(txns)


def want_read_verdicts():
    return np.array([v for c in CLASSES for v in c.want_reads()], np.uint8)


def write_keys():
    return [k for c in CLASSES for k in ((c.ka,) if c.empty else (c.ka, c.kb))]


def write_batch(ranges=None):
    """One write transaction per key, [k, k\\0), and two transactions below the oldest version:
    one with a read (TooOld; its write must never land) and one without (commits)."""
    if ranges is None:
        ranges = [(k, k + b"\x00") for k in write_keys()]
    txns = [CommitTransaction([], [KeyRange(b, e)], NOW_READS, False) for b, e in ranges]
    txns.append(CommitTransaction([KeyRange(b"\xf0", b"\xf1")], [KeyRange(b"\xf0too-old", b"\xf0too-old\x00")],
                                  OLDEST_AFTER_READS - 1, True))
    txns.append(CommitTransaction([], [KeyRange(b"\xf2", b"\xf2\x00")], OLDEST_AFTER_READS - 1, False))
    return PackedBatch.from_transactions(txns)


def reread_batch():
    """Reads of exactly the written keys, [k, k\\0): one below the writes' version (conflicts) and
    at it (commits), and of the keys right beside them, which the writes must not have touched."""
    txns = []
    for k in write_keys():
        txns.append(CommitTransaction([KeyRange(k, k + b"\x00")], [], NOW_WRITES - 1, True))
        txns.append(CommitTransaction([KeyRange(k, k + b"\x00")], [], NOW_WRITES, True))
        txns.append(CommitTransaction([KeyRange(k + b"\x00", k + b"\x00\x00")], [], NOW_READS, True))
    return PackedBatch.from_transactions(txns)


def sequence():
    """The plan: (PackedBatch, now, new_oldest_version) per batch, on a set loaded with history()."""
    return [(read_batch(), NOW_READS, OLDEST_AFTER_READS), (write_batch(), NOW_WRITES, OLDEST_AFTER_READS),
            (reread_batch(), NOW_REREADS, OLDEST_AFTER_READS)]
