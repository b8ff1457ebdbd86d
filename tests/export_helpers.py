"""Reference side of the history-export tests: the canonical form of the oracle's step function,
and a pair driver that feeds the HIP engine and the semantic oracle the same steps."""
import numpy as np

from tests.helpers import EngineDriver

NO_FLOOR = -(1 << 63)


def canon(keys, vers, header, floor, lo=None, hi=None):
    cl = lambda v: v if (floor == NO_FLOOR or v >= floor) else floor - 1
    cur = hdr = cl(header); ks, vs = [], []
    for k, v in zip(keys, vers):
        v = cl(int(v))
        if lo is not None and k <= lo: cur = hdr = v; continue
        if hi is not None and k >= hi: break
        if v != cur: ks.append(k); vs.append(v); cur = v
    return hdr, ks, vs


def split_dump(dump):
    """(header, [key bytes], [versions]) of ConflictSet.dump_history()'s tuple."""
    kb, ko, vv, hdr = dump
    assert len(ko) == len(vv) + 1 and ko[0] == 0 and ko[-1] == len(kb)
    raw = kb.tobytes()
    return hdr, [raw[ko[i]:ko[i + 1]] for i in range(len(vv))], vv.tolist()


class Pair:
    """The engine and the semantic oracle side by side; `header` follows clear / load_history (the
    oracle's dump does not carry it)."""

    def __init__(self, engine, oracle_mod, gc_interval=1, delta_limit=0):
        self.e = EngineDriver(engine, gc_interval=gc_interval, delta_limit=delta_limit)
        self.o = oracle_mod.OracleConflictSet()
        self.header = 0

    @property
    def cs(self):
        return self.e.cs

    def clear(self, v):
        self.e.clear(v)
        self.o.clear(v)
        self.header = v

    def load_history(self, kb, ko, vers, header=0):
        self.e.load_history(kb, ko, vers, header)
        self.o.load_history(kb, ko, vers, header)
        self.header = header

    def set_oldest_version(self, v):
        self.e.cs.set_oldest_version(v)
        self.o.set_oldest_version(v)

    def detect(self, pb, now, new_oldest):
        ve, ce = self.e.detect(pb, now, new_oldest)
        vo, co = self.o.detect(pb, now, new_oldest)
        assert (ve == vo).all(), (np.nonzero(ve != vo)[0][:10],)
        assert ce == co
        return ve

    def reference(self, lo=None, hi=None, floor=None):
        keys, vers = self.o.dump_history()
        return canon(keys, vers, self.header, self.o.oldest_version if floor is None else floor, lo, hi)

    def check(self, lo=None, hi=None, floor=None, what=None):
        """The exported state equals the canonical form of the oracle's; returns it."""
        assert self.e.cs.oldest_version == self.o.oldest_version
        got = split_dump(self.e.cs.dump_history(lo, hi, floor))
        want = self.reference(lo, hi, floor)
        assert got[0] == want[0], (what, "header", got[0], want[0])
        if got[1] != want[1] or got[2] != want[2]:
            n = min(len(got[1]), len(want[1]))
            d = next((i for i in range(n) if got[1][i] != want[1][i] or got[2][i] != want[2][i]), n)
            raise AssertionError((what, "first difference at", d, len(got[1]), len(want[1]),
                                  got[1][d:d + 2], got[2][d:d + 2], want[1][d:d + 2], want[2][d:d + 2]))
        return got
