"""CPU tests of the partitioned history digest: the host entry (digest_arrays_ranges) against the
plain-Python model of the partition (tests/digest_ranges_model.py) and against digest_arrays of the
same arrays clipped on the host, the count identity, the refused inputs, the exported symbols, and
locate_divergence driven by two host models.  No device is needed."""
import ctypes

import numpy as np
import pytest

from tests import digest_model as M
from tests import digest_ranges_model as R
from tests.export_helpers import NO_FLOOR, canon
from tests.test_digest_cpu import LADDER_HEADER, LADDER_KEYS, LADDER_VERS, arrays
from tests.test_export_cpu import _states


@pytest.fixture(scope="module")
def C():
    from foundationdb_amd import build, conflict_set

    build.build()
    conflict_set.load_library()
    return conflict_set


def lib_ranges(C, header, keys, vers, bounds, open_lo=False, open_hi=False):
    out = C.digest_arrays_ranges(*arrays(keys, vers), header, bounds, open_lo, open_hi)
    assert all(isinstance(d, C.HistoryDigest) for d in out)
    return [tuple(d) for d in out]


def check(C, header, keys, vers, bounds, open_lo=False, open_hi=False, what=None):
    """The library against the model, every entry against digest_arrays of the clipped arrays, and
    the count identity; returns the digests."""
    got = lib_ranges(C, header, keys, vers, bounds, open_lo, open_hi)
    assert got == R.digest_ranges(header, keys, vers, bounds, open_lo, open_hi), (what, bounds, open_lo, open_hi)
    rs = R.ranges(bounds, open_lo, open_hi)
    assert len(got) == len(rs) == len(bounds) - 1 + open_lo + open_hi
    for d, (lo, hi) in zip(got, rs):
        hdr, ks, vs = R.clip(header, keys, vers, lo, hi)
        assert d == tuple(C.digest_arrays(*arrays(ks, vs), hdr)), (what, lo, hi)
    whole = R.clip(header, keys, vers, rs[0][0], rs[-1][1])
    assert len(whole[1]) == sum(d[0] for d in got) + R.bound_hits(keys, bounds, open_lo, open_hi), (what, bounds)
    return got


LADDER = sorted(zip(LADDER_KEYS, LADDER_VERS))
LKEYS, LVERS = [k for k, _ in LADDER], [v for _, v in LADDER]


def test_model_against_library_on_oracle_states(C, oracle_built):
    rng = np.random.default_rng(19)
    cases = 0
    for seed, header, o in _states(oracle_built, True):
        keys, vers = o.dump_history()
        probes = [b""] + keys + [k + b"\x00" for k in keys]
        for floor in (NO_FLOOR, o.oldest_version):
            hdr, ks, vs = canon(keys, vers, header, floor)
            for _ in range(8):
                nb = int(rng.integers(1, 9))
                bounds = sorted(probes[int(rng.integers(len(probes)))] for _ in range(nb))
                for open_lo, open_hi in ((False, False), (True, False), (False, True), (True, True)):
                    if len(bounds) - 1 + open_lo + open_hi < 1:
                        continue
                    got = check(C, hdr, ks, vs, bounds, open_lo, open_hi, what=(seed, floor))
                    cases += sum(d[0] > 0 for d in got)
    assert cases > 200  # the ranges are not all empty


def test_model_against_library_on_the_length_ladder(C):
    # every ladder key as a bound, then the keys between them (k + b"\0"), then both
    between = [k + b"\x00" for k in LKEYS]
    for bounds in (LKEYS, between, sorted(LKEYS + between)):
        for open_lo, open_hi in ((False, False), (True, True), (True, False), (False, True)):
            check(C, LADDER_HEADER, LKEYS, LVERS, bounds, open_lo, open_hi, what="ladder")
    got = check(C, LADDER_HEADER, LKEYS, LVERS, LKEYS, True, True)
    assert [d[0] for d in got] == [0] * (len(LKEYS) + 1)  # every boundary is a bound: headers only
    assert [d[2] for d in got] == [LADDER_HEADER] + LVERS


def test_named_cases(C):
    k = LKEYS
    assert k[0] == b"" and len(k[-1]) == 100
    hdr = LADDER_HEADER
    # a bound equal to a boundary key: it opens its range as the header and is counted nowhere
    got = check(C, hdr, k, LVERS, [k[3], k[6]])
    assert got[0][0] == 2 and got[0][2] == LVERS[3]
    # bounds k and k\0: the range holds nothing, its header is k's version
    for i in (0, 4, 7, 11):
        got = check(C, hdr, k, LVERS, [k[i], k[i] + b"\x00"])
        assert got[0] == (0, 0, LVERS[i], (0, 0))
    # the empty key as a bound: below it lies no key at all
    got = check(C, hdr, k, LVERS, [b""], True, True)
    assert got[0] == (0, 0, hdr, (0, 0)) and got[1][0] == len(k) - 1 and got[1][2] == LVERS[0]
    # equal neighbouring bounds: n = 0 and the header, as lo == hi
    got = check(C, hdr, k, LVERS, [k[2], k[5], k[5], k[5], k[9]])
    assert got[1] == got[2] == (0, 0, LVERS[5], (0, 0)) and got[0][0] == 2 and got[3][0] == 3
    got = check(C, hdr, k, LVERS, [k[5] + b"\x00"] * 2)
    assert got == [(0, 0, LVERS[5], (0, 0))]
    # both open ends without a bound: K = 1, the whole arrays
    got = check(C, hdr, k, LVERS, [], True, True)
    assert got == [M.digest(hdr, k, LVERS)]
    # K = 1 in its other forms
    assert check(C, hdr, k, LVERS, [k[4]], True, False)[0][0] == 4
    assert check(C, hdr, k, LVERS, [k[4]], False, True)[0][0] == len(k) - 5
    assert check(C, hdr, k, LVERS, [k[1], k[-1]])[0][0] == len(k) - 3
    # no arrays at all: headers only
    assert lib_ranges(C, 7, [], [], [b"a", b"b"], True, True) == [(0, 0, 7, (0, 0))] * 3


def test_count_identity_on_a_large_partition(C):
    rng = np.random.default_rng(23)
    keys = sorted({bytes(rng.integers(0, 256, size=int(rng.integers(1, 30)), dtype=np.uint8)) for _ in range(3000)})
    vers = [int(v) for v in rng.integers(0, 1 << 40, size=len(keys))]
    bounds = sorted([keys[int(i)] for i in rng.integers(0, len(keys), size=700)]
                    + [bytes(rng.integers(0, 256, size=3, dtype=np.uint8)) for _ in range(700)])
    got = check(C, 5, keys, vers, bounds, True, True)
    assert len(got) == 1401 and R.bound_hits(keys, bounds, True, True) > 500


def test_invalid_inputs(C):
    L = C.load_library()
    kb, ko, vv = arrays([b"ab", b"c"], [1, 2])
    bb, bo, _ = arrays([b"a", b"b", b"c"], [0, 0, 0])
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    out = (C._CDigest * 8)()
    po = ctypes.addressof(out)

    def call(n=2, b=vp(kb), o=vp(ko), v=vp(vv), nb=3, bbytes=vp(bb), boff=vp(bo), ol=0, oh=0, res=po):
        return L.fdbcs_history_digest_arrays_ranges(n, b, o, v, 0, nb, bbytes, boff, ol, oh, res)

    assert call() == C.FDBCS_OK and [out[i].n for i in range(2)] == [1, 0] and out[1].header_version == 1
    assert call(res=None) == C.FDBCS_E_INVALID
    assert call(n=-1) == C.FDBCS_E_INVALID
    assert call(o=None) == C.FDBCS_E_INVALID and call(v=None) == C.FDBCS_E_INVALID and call(b=None) == C.FDBCS_E_INVALID
    assert call(nb=-1) == C.FDBCS_E_INVALID
    assert call(boff=None) == C.FDBCS_E_INVALID and call(bbytes=None) == C.FDBCS_E_INVALID
    assert call(nb=1) == C.FDBCS_E_INVALID and call(nb=0) == C.FDBCS_E_INVALID  # K < 1
    assert call(nb=0, ol=1) == C.FDBCS_E_INVALID and call(nb=0, ol=1, oh=1) == C.FDBCS_OK
    assert call(nb=1, ol=1) == C.FDBCS_OK and call(nb=1, oh=1) == C.FDBCS_OK
    bad = bo.copy()
    bad[0] = 1
    assert call(boff=vp(bad)) == C.FDBCS_E_INVALID
    bad = np.array([0, 2, 1, 3], np.int64)
    assert call(boff=vp(bad)) == C.FDBCS_E_INVALID  # decreasing offsets
    dec, deco, _ = arrays([b"a", b"c", b"b"], [0, 0, 0])
    assert call(bbytes=vp(dec), boff=vp(deco)) == C.FDBCS_E_INVALID  # decreasing bounds
    with pytest.raises(C.FdbcsError) as ei:
        C.digest_arrays_ranges(kb, ko, vv, 0, [b"b", b"a"])
    assert ei.value.status == C.FDBCS_E_INVALID
    with pytest.raises(C.FdbcsError) as ei:
        C.digest_arrays_ranges(kb, ko, vv, 0, [b"a"])
    assert ei.value.status == C.FDBCS_E_INVALID
    # 65536 ranges are taken, 65537 are refused
    many = [(i * 65535).to_bytes(4, "big") for i in range(65537)]
    got = C.digest_arrays_ranges(kb, ko, vv, 9, many)
    assert len(got) == 65536 and sum(d.n for d in got) == 2 and got[0].header_version == 9
    with pytest.raises(C.FdbcsError) as ei:
        C.digest_arrays_ranges(kb, ko, vv, 9, many, open_hi=True)
    assert ei.value.status == C.FDBCS_E_NOMEM


def test_symbols(C):
    L = C.load_library()
    names = ("fdbcs_history_digest_ranges", "fdbcs_history_digest_arrays_ranges", "fdbcs_history_split_keys",
             "fdbcs_history_split_keys_read", "fdbcs_history_split_keys_timing")
    for name in names:
        assert name in C.SIGNATURES
        assert getattr(L, name).argtypes == C.SIGNATURES[name][1]
    out = (C._CDigest * 2)()
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    a, b = ctypes.c_double(), ctypes.c_double()
    assert L.fdbcs_history_digest_ranges(None, 0, None, None, 1, 1, C.NO_FLOOR, ctypes.addressof(out)) == C.FDBCS_E_INVALID
    assert L.fdbcs_history_split_keys(None, None, -1, None, -1, 4, ctypes.byref(n), ctypes.byref(nb)) == C.FDBCS_E_INVALID
    assert L.fdbcs_history_split_keys_read(None, None, 0, None, 0) == C.FDBCS_E_INVALID
    assert L.fdbcs_history_split_keys_timing(None, ctypes.byref(a), ctypes.byref(b)) == C.FDBCS_E_INVALID
    for f in ("digest_ranges", "split_keys", "diverging_ranges"):
        assert callable(getattr(C.ConflictSet, f))
    assert callable(C.locate_divergence)


# ---- locate_divergence on two host models

def _history(n=2000, seed=41):
    rng = np.random.default_rng(seed)
    keys = sorted({bytes(rng.integers(97, 123, size=int(rng.integers(1, 24)), dtype=np.uint8)) for _ in range(n)})
    return keys, [1000 + 7 * i for i in range(len(keys))]  # all distinct: every edit stays canonical


def _side(C, header, keys, vers, calls):
    kb, ko, vv = arrays(keys, vers)

    def digests(bounds, open_lo, open_hi):
        calls.append(len(bounds))
        return C.digest_arrays_ranges(kb, ko, vv, header, bounds, open_lo, open_hi)
    return digests


def _locate(C, a, b, lo=None, hi=None, fanout=8, leaf=4):
    """locate_divergence over two (header, keys, versions) models, with everything the result must
    satisfy checked: disjoint ascending ranges, each differing, each a leaf, every key at which the step functions differ inside one."""
    ca, cb = [], []
    da, db = _side(C, *a, ca), _side(C, *b, cb)
    got = C.locate_divergence(da, db, lambda l, h, want: R.split_keys(a[1], l, h, want), lo, hi, fanout, leaf)
    inside = lambda k, r: (r[0] is None or k >= r[0]) and (r[1] is None or k < r[1])
    for r, nxt in zip(got, got[1:]):
        assert r[1] is not None and nxt[0] is not None and r[1] <= nxt[0]
    for r in got:
        bounds = [x for x in r if x is not None]
        x, y = da(bounds, r[0] is None, r[1] is None)[0], db(bounds, r[0] is None, r[1] is None)[0]
        assert x != y, r  # nothing that is equal
        assert (x.n <= leaf and y.n <= leaf) or not R.split_keys(a[1], r[0], r[1], 1), r
    diff = [k for k in R.differing_keys(a, b) if inside(k, (lo, hi))]
    for k in diff:
        assert sum(inside(k, r) for r in got) == 1, (k, got)
    assert len(ca) == len(cb)  # both sides are asked the same questions
    return got, diff


def test_locate_divergence_on_host_models(C):
    keys, vers = _history()
    n = len(keys)
    assert n > 1500
    a = (3, keys, vers)
    assert _locate(C, a, (3, list(keys), list(vers))) == ([], [])
    # one changed version
    v = list(vers)
    v[n // 3] += 1
    got, diff = _locate(C, a, (3, keys, v))
    assert diff == [keys[n // 3]] and len(got) == 1
    # one inserted key (absent from side a's split keys), one removed key
    extra = keys[n // 2] + b"\x00"
    assert extra not in keys
    got, diff = _locate(C, a, (3, keys[:n // 2 + 1] + [extra] + keys[n // 2 + 1:], vers[:n // 2 + 1] + [5] + vers[n // 2 + 1:]))
    assert diff == [extra] and len(got) == 1
    got, diff = _locate(C, a, (3, keys[:700] + keys[701:], vers[:700] + vers[701:]))
    assert diff == [keys[700]] and len(got) == 1
    # the first and the last boundary, together with one in the middle: three separate ranges
    v = list(vers)
    v[0] -= 1
    v[-1] -= 1
    v[n // 2] += 3
    got, diff = _locate(C, a, (3, keys, v))
    assert diff == [keys[0], keys[n // 2], keys[-1]] and len(got) == 3
    assert got[-1][1] is None  # nothing lies above the last boundary: its range runs to the end
    # a different header alone: the range below the first key
    got, _ = _locate(C, a, (4, keys, vers))
    assert len(got) == 1 and got[0][0] is None and got[0][1] <= keys[4 + 1]
    # inside a closed span: differences outside it are not reported, one at lo itself is
    v = list(vers)
    v[100] += 1
    v[900] += 1
    got, diff = _locate(C, a, (3, keys, v), keys[200], keys[1000])
    assert diff == [keys[900]] and len(got) == 1
    got, diff = _locate(C, a, (3, keys, v), keys[100], keys[900])
    assert diff == [keys[100]] and len(got) == 1 and got[0][0] == keys[100]
    # the default fan-out and leaf: one level is enough here
    calls = []
    got = C.locate_divergence(_side(C, 3, keys, vers, calls), _side(C, 3, keys, v, []),
                              lambda l, h, want: R.split_keys(keys, l, h, want))
    assert len(got) == 2 and len(calls) == 2 and calls[1] == 255
