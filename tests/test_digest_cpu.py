"""CPU tests of the history digest: the host entry (digest_arrays) against the plain-Python model
of the definition, known answers, what the digest is and is not sensitive to, the refused arrays and
the exported symbols.  No device is needed."""
import ctypes

import numpy as np
import pytest

from tests import digest_model as M
from tests.export_helpers import NO_FLOOR, canon
from tests.test_export_cpu import _states


@pytest.fixture(scope="module")
def C():
    from foundationdb_amd import build, conflict_set

    build.build()
    conflict_set.load_library()
    return conflict_set


def arrays(keys, vers):
    """The load_history / export_read layout of a list of keys and their versions."""
    kb = np.frombuffer(b"".join(keys), np.uint8)
    ko = np.concatenate([[0], np.cumsum([len(k) for k in keys], dtype=np.int64)]).astype(np.int64)
    return kb, ko, np.asarray(vers, np.int64).reshape(-1)


def lib_digest(C, header, keys, vers):
    d = C.digest_arrays(*arrays(keys, vers), header)
    assert isinstance(d, C.HistoryDigest) and isinstance(d.sum, tuple)
    return tuple(d)


# Every length meets the zero padding and the last word's mask once; the keys of 17 and 23 bytes
# share exactly 16 leading bytes, those of 25 and 100 bytes exactly 24.
LADDER_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 100)
_P = bytes((37 * i + 11) % 256 for i in range(100))
LADDER_KEYS = [_P[:L - 1] + bytes([L]) if L else b"" for L in LADDER_LENGTHS]
LADDER_VERS = [(1 << 40) + 1001 * i for i in range(len(LADDER_KEYS))]
LADDER_VERS[3] = -5                # a clamped version below zero
LADDER_VERS[7] = (1 << 62) + 12345
LADDER_HEADER = (1 << 33) + 7


def test_ladder_shape():
    assert [len(k) for k in LADDER_KEYS] == list(LADDER_LENGTHS)
    by = dict(zip(LADDER_LENGTHS, LADDER_KEYS))
    assert by[17][:16] == by[23][:16] and by[17][16] != by[23][16]
    assert by[25][:24] == by[100][:24] and by[25][24] != by[100][24]
    assert sum(v > 1 << 32 for v in LADDER_VERS) >= 10


def test_model_against_library_on_oracle_states(C, oracle_built):
    rng = np.random.default_rng(9)
    cases = 0
    for seed, header, o in _states(oracle_built, True):
        keys, vers = o.dump_history()
        probes = [b""] + keys + [k + b"\x00" for k in keys]
        for floor in (NO_FLOOR, o.oldest_version):
            clips = [(None, None)]
            for _ in range(6):
                lo, hi = sorted((probes[int(rng.integers(len(probes)))], probes[int(rng.integers(len(probes)))]))
                clips += [(lo, hi), (lo, None), (None, hi)]
            for lo, hi in clips:
                hdr, ks, vs = canon(keys, vers, header, floor, lo, hi)
                assert lib_digest(C, hdr, ks, vs) == M.digest(hdr, ks, vs), (seed, floor, lo, hi)
                cases += len(ks) > 0
    assert cases > 100  # the clipped states are not all empty


def test_model_against_library_on_the_length_ladder(C):
    assert lib_digest(C, LADDER_HEADER, LADDER_KEYS, LADDER_VERS) == M.digest(LADDER_HEADER, LADDER_KEYS, LADDER_VERS)
    for k, v in zip(LADDER_KEYS, LADDER_VERS):  # and one key at a time: which length fails
        assert lib_digest(C, 0, [k], [v]) == M.digest(0, [k], [v]), len(k)


# Computed once with tests/digest_model.py and checked against the library before they were written
# down: two independent restatements of the definition pin each other.
KNOWN = [
    ((42, [], []), (0, 0, 42, (0, 0))),
    ((0, [b""], [7]), (1, 0, 0, (0x846AEF8C3396F75E, 0xF52B318604669653))),
    ((LADDER_HEADER, LADDER_KEYS, LADDER_VERS), (12, 245, (1 << 33) + 7, (0x05FE1F12B198CD02, 0xE62447B72FE9CD0D))),
]


@pytest.mark.parametrize("i", range(len(KNOWN)))
def test_known_answers(C, i):
    (header, keys, vers), want = KNOWN[i]
    assert M.digest(header, keys, vers) == want
    assert lib_digest(C, header, keys, vers) == want


def test_sensitivity(C):
    base = lib_digest(C, LADDER_HEADER, LADDER_KEYS, LADDER_VERS)
    seen = {base}

    def differs(header, keys, vers, what, sums=True):
        d = lib_digest(C, header, keys, vers)
        assert d == M.digest(header, keys, vers), what
        assert d not in seen, what
        if sums:  # each lane alone shows it
            assert d[3][0] != base[3][0] and d[3][1] != base[3][1], what
        seen.add(d)

    v = list(LADDER_VERS)
    v[5] += 1
    differs(LADDER_HEADER, LADDER_KEYS, v, "one version by 1")
    k = list(LADDER_KEYS)
    k[-1] = k[-1][:-1] + bytes([k[-1][-1] ^ 1])
    differs(LADDER_HEADER, k, LADDER_VERS, "the last tail byte of the 100-byte key")
    for i in (1, 3, 6, 9):  # lengths 1, 8, 16, 24: the appended zero opens a new word for three of them
        k = list(LADDER_KEYS)
        k[i] += b"\x00"
        differs(LADDER_HEADER, k, LADDER_VERS, ("appending a zero byte", len(k[i])))
    v = list(LADDER_VERS)
    v[2], v[8] = v[8], v[2]
    differs(LADDER_HEADER, LADDER_KEYS, v, "exchanging two keys' versions")
    differs(LADDER_HEADER, LADDER_KEYS[:4] + LADDER_KEYS[5:], LADDER_VERS[:4] + LADDER_VERS[5:], "dropping a boundary")
    differs(LADDER_HEADER + 1, LADDER_KEYS, LADDER_VERS, "header", sums=False)
    # the order of the array does not matter
    perm = np.random.default_rng(3).permutation(len(LADDER_KEYS))
    assert lib_digest(C, LADDER_HEADER, [LADDER_KEYS[i] for i in perm], [LADDER_VERS[i] for i in perm]) == base


def test_invalid_arrays(C):
    L = C.load_library()
    kb, ko, vv = arrays([b"ab", b"c"], [1, 2])
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    d = C._CDigest()
    call = lambda n, b, o, v, out: L.fdbcs_history_digest_arrays(n, b, o, v, 0, out)
    assert call(2, vp(kb), vp(ko), vp(vv), ctypes.byref(d)) == C.FDBCS_OK and d.n == 2 and d.key_bytes == 3
    assert call(-1, vp(kb), vp(ko), vp(vv), ctypes.byref(d)) == C.FDBCS_E_INVALID
    assert call(2, vp(kb), vp(ko), vp(vv), None) == C.FDBCS_E_INVALID
    assert call(2, vp(kb), None, vp(vv), ctypes.byref(d)) == C.FDBCS_E_INVALID
    assert call(2, vp(kb), vp(ko), None, ctypes.byref(d)) == C.FDBCS_E_INVALID
    assert call(2, None, vp(ko), vp(vv), ctypes.byref(d)) == C.FDBCS_E_INVALID  # the offsets say 3 bytes are read
    bad = ko.copy()
    bad[0] = 1
    assert call(2, vp(kb), vp(bad), vp(vv), ctypes.byref(d)) == C.FDBCS_E_INVALID
    bad = np.array([0, 3, 2], np.int64)
    assert call(2, vp(kb), vp(bad), vp(vv), ctypes.byref(d)) == C.FDBCS_E_INVALID
    # nothing is read: no array is needed
    assert call(0, None, None, None, ctypes.byref(d)) == C.FDBCS_OK and (d.n, d.key_bytes) == (0, 0)
    empty = np.zeros(3, np.int64)
    assert call(2, None, vp(empty), vp(vv), ctypes.byref(d)) == C.FDBCS_OK and (d.n, d.key_bytes) == (2, 0)
    with pytest.raises(C.FdbcsError) as ei:
        C.digest_arrays(kb, np.array([0, 3, 2]), vv)
    assert ei.value.status == C.FDBCS_E_INVALID


def test_symbols(C):
    L = C.load_library()
    for name in ("fdbcs_history_digest", "fdbcs_history_digest_arrays", "fdbcs_history_digest_timing"):
        assert name in C.SIGNATURES
        assert getattr(L, name).argtypes == C.SIGNATURES[name][1]
    assert ctypes.sizeof(C._CDigest) == 40
    d = C._CDigest()
    assert L.fdbcs_history_digest(None, None, -1, None, -1, C.NO_FLOOR, ctypes.byref(d)) == C.FDBCS_E_INVALID
    a, b = ctypes.c_double(), ctypes.c_double()
    assert L.fdbcs_history_digest_timing(None, ctypes.byref(a), ctypes.byref(b)) == C.FDBCS_E_INVALID
