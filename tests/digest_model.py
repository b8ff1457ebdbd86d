"""The history digest restated in plain Python from its definition (include/fdb_conflict_set.h,
fdbcs_digest).  Imports nothing from the library: the tests pin the C++ and the kernel to this."""

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344)


def mix(z):
    """splitmix64's finalizer."""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def words(key):
    """ceil(L / 8) big-endian words of the key, zero-padded past its end; none for the empty key."""
    key = bytes(key)
    return [int.from_bytes(key[o:o + 8].ljust(8, b"\x00"), "big") for o in range(0, len(key), 8)]


def entry(key, version, lane):
    h = mix(SEEDS[lane] + len(key))
    for w in words(key):
        h = mix((h ^ w) + G)
    return mix((h ^ (int(version) & MASK)) + G)


def digest(header, keys, versions):
    """(n, key_bytes, header_version, (sum0, sum1)) of a canonical history given as a header, a list
    of keys and the list of their versions: the tuple ConflictSet.digest returns."""
    keys = [bytes(k) for k in keys]
    assert len(keys) == len(versions)
    sums = tuple(sum(entry(k, v, c) for k, v in zip(keys, versions)) & MASK for c in (0, 1))
    return (len(keys), sum(len(k) for k in keys), int(header), sums)
