"""The version a read is checked against, in plain Python, written from the definition in
include/fdb_conflict_set.h (fdbcs_batch_read_versions) and from nothing else: no engine, no kernel.

A history is (keys, versions, header) in the export's layout: `keys` ascending byte strings,
versions[i] the version of every key in [keys[i], keys[i + 1]), `header` the version below keys[0].
H(k) is the version of the last boundary <= k, the header if there is none.  With a floor f,
H_f(k) = H(k) if H(k) >= f, else f - 1 (NO_FLOOR: no clamp).  For a read [b, e):

    b <  e   V = max { H_f(k) : b <= k < e }: the segment containing b (the header if no boundary is
             <= b) and every boundary inside (b, e); a boundary at e does not count.
    b == e   V = H_f just below b: the greatest boundary < b, the header if there is none (so the
             empty key and a b equal to the first boundary both give the header).
"""
import bisect

NO_FLOOR = -(1 << 63)


def clamp(v, floor):
    return v if floor == NO_FLOOR or v >= floor else floor - 1


def read_version(keys, versions, header, begin, end, floor=NO_FLOOR):
    assert begin <= end
    if begin == end:
        i = bisect.bisect_left(keys, begin)  # boundaries < begin
        return clamp(int(versions[i - 1]) if i else int(header), floor)
    i = bisect.bisect_right(keys, begin)  # boundaries <= begin: the last of them holds begin
    j = bisect.bisect_left(keys, end)     # boundaries < end
    best = clamp(int(versions[i - 1]) if i else int(header), floor)
    for v in versions[i:j]:
        best = max(best, clamp(int(v), floor))
    return best


def read_versions(keys, versions, header, ranges, floor=NO_FLOOR):
    """One V per (begin, end) pair of `ranges`, in order."""
    versions = [int(v) for v in versions]
    return [read_version(keys, versions, header, b, e, floor) for b, e in ranges]


def version_at(keys, versions, header, key, floor=NO_FLOOR):
    """The read [key, key + b"\\0"): the version a point read of `key` sees."""
    return read_version(keys, versions, header, key, key + b"\x00", floor)


def of_dump(dump, ranges):
    """read_versions over ConflictSet.dump_history()'s tuple (already clamped at the dump's floor)."""
    kb, ko, vv, hdr = dump
    assert len(ko) == len(vv) + 1 and ko[0] == 0 and ko[-1] == len(kb)
    raw, ko = kb.tobytes(), ko.tolist()
    return read_versions([raw[a:b] for a, b in zip(ko, ko[1:])], vv.tolist(), int(hdr), ranges)
