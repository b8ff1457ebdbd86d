"""Reference side of the history-import tests: the pointwise max of two canonical histories over a
key range, and the array packing ConflictSet.merge_history takes."""
import numpy as np


def merge_max(own, imp, lo=None, hi=None):
    """own, imp: (header, [keys], [versions]).  The canonical form of
    H'(k) = max(own(k), imp(k)) for lo <= k < hi, own(k) elsewhere."""
    oh, ok, ov = own
    ih, ik, iv = imp
    inside = lambda k: (lo is None or k >= lo) and (hi is None or k < hi)

    def at(h, ks, vs, key):
        v = h
        for k, x in zip(ks, vs):
            if k > key:
                break
            v = x
        return v

    pts = sorted(set(ok) | {k for k in ik if inside(k)} | ({lo} - {None}) | ({hi} - {None}))
    val = lambda k: max(at(oh, ok, ov, k), at(ih, ik, iv, k)) if inside(k) else at(oh, ok, ov, k)
    hdr = max(oh, ih) if lo is None else oh
    cur, ks, vs = hdr, [], []
    for k in pts:
        v = val(k)
        if v != cur:
            ks.append(k)
            vs.append(v)
            cur = v
    return hdr, ks, vs


def merge_max_fast(own, imp, lo=None, hi=None):
    """merge_max by one sweep over both key lists (the tests' large states); test_import_cpu.py
    checks it against merge_max."""
    oh, ok, ov = own
    ih, ik, iv = imp
    inside = lambda k: (lo is None or k >= lo) and (hi is None or k < hi)
    pts = sorted(set(ok) | {k for k in ik if inside(k)} | ({lo} - {None}) | ({hi} - {None}))
    hdr = max(oh, ih) if lo is None else oh
    cur, ks, vs = hdr, [], []
    i = j = 0
    a, b = oh, ih
    for k in pts:
        while i < len(ok) and ok[i] <= k:
            a = ov[i]
            i += 1
        while j < len(ik) and ik[j] <= k:
            b = iv[j]
            j += 1
        v = max(a, b) if inside(k) else a
        if v != cur:
            ks.append(k)
            vs.append(v)
            cur = v
    return hdr, ks, vs


def pack(state):
    """(key_bytes, key_offsets, versions, header) arrays of a (header, [keys], [versions]) state."""
    hdr, ks, vs = state
    kb = np.frombuffer(b"".join(ks), np.uint8)
    ko = np.zeros(len(ks) + 1, np.int64)
    if ks:
        ko[1:] = np.cumsum([len(k) for k in ks])
    return kb, ko, np.asarray(vs, np.int64).reshape(-1), int(hdr)


def shifted(state, shift, version):
    """The state with one more boundary, the key of `shift` zero bytes (shift >= 1) at `version`: in
    the packed arrays every later key starts `shift` bytes further on, so the keys' addresses in the
    uploaded byte array take every alignment modulo 8 as shift runs over 1 .. 8."""
    import bisect

    hdr, ks, vs = state
    k = b"\x00" * shift
    assert shift >= 1 and k not in ks
    i = bisect.bisect_left(ks, k)
    return hdr, ks[:i] + [k] + ks[i:], list(vs[:i]) + [version] + list(vs[i:])
