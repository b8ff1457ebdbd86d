"""The partitioned history digest restated in plain Python from its definition
(include/fdb_conflict_set.h, fdbcs_history_digest_ranges and fdbcs_history_digest_arrays_ranges), on
top of the single digest's model (tests/digest_model.py).  Imports nothing from the library."""
from bisect import bisect_left, bisect_right

from tests import digest_model as M


def ranges(bounds, open_lo=False, open_hi=False):
    """The (lo, hi) pairs the ascending keys `bounds` define, None for an open end, in the order of
    the result: below bounds[0], each neighbouring pair, from bounds[-1] on."""
    bounds = [bytes(b) for b in bounds]
    assert all(a <= b for a, b in zip(bounds, bounds[1:]))
    edges = ([None] if open_lo else []) + bounds + ([None] if open_hi else [])
    assert len(edges) >= 2
    out = list(zip(edges, edges[1:]))
    if open_lo and open_hi and not bounds:
        out = [(None, None)]
    return out


def clip(header, keys, versions, lo, hi):
    """(header, keys, versions) of ascending arrays clipped to one range: the version of the last
    boundary <= lo (the given header if there is none), and the boundaries strictly inside."""
    i = bisect_right(keys, lo) if lo is not None else 0
    j = max(i, bisect_left(keys, hi)) if hi is not None else len(keys)
    return (int(versions[i - 1]) if i else header), list(keys[i:j]), [int(v) for v in versions[i:j]]


def value_at(header, keys, versions, key):
    """The step function of ascending arrays read at `key`."""
    i = bisect_right(keys, key)
    return int(versions[i - 1]) if i else header


def differing_keys(a, b):
    """The boundary keys of either of two (header, keys, versions) at which their step functions differ.
    A boundary that only one side has, with the value the other side holds there anyway (the end of a
    stretch that differs), is not among them."""
    return [k for k in sorted(set(a[1]) | set(b[1])) if value_at(*a, k) != value_at(*b, k)]


def digest_ranges(header, keys, versions, bounds, open_lo=False, open_hi=False):
    """One digest tuple (digest_model.digest) per range."""
    keys = [bytes(k) for k in keys]
    entries = [tuple(M.entry(k, v, c) for c in (0, 1)) for k, v in zip(keys, versions)]  # hashed once
    out = []
    for lo, hi in ranges(bounds, open_lo, open_hi):
        i = bisect_right(keys, lo) if lo is not None else 0
        j = max(i, bisect_left(keys, hi)) if hi is not None else len(keys)
        sums = tuple(sum(e[c] for e in entries[i:j]) & M.MASK for c in (0, 1))
        out.append((j - i, sum(len(k) for k in keys[i:j]), int(versions[i - 1]) if i else int(header), sums))
    return out


def bound_hits(keys, bounds, open_lo=False, open_hi=False):
    """Interior bounds (every bound that closes one range and opens the next; with a closed end the
    outermost bound is the span's own) that are boundaries of the arrays, each counted once."""
    bounds = [bytes(b) for b in bounds]
    interior = {b for b in bounds if (open_lo or b > bounds[0]) and (open_hi or b < bounds[-1])}
    return len(interior & {bytes(k) for k in keys})


def split_keys(keys, lo, hi, want):
    """Evenly spaced keys of an ascending list strictly inside (lo, hi): the picks of
    fdbcs_history_split_keys over a single tier."""
    inside = [bytes(k) for k in keys if (lo is None or k > lo) and (hi is None or k < hi)]
    c, n = len(inside), min(want, len(inside))
    return [inside[((2 * k + 1) * c) // (2 * n)] for k in range(n)]
