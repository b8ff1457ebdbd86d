"""Python host interface mirroring fdbserver/ConflictSet.h over the C-ABI (libfdbcs.so).

Names, argument meaning and error behaviour follow the reference:

    cs = new_conflict_set()                       # newConflictSet()       SkipList.cpp:739
    clear_conflict_set(cs, v)                     # clearConflictSet()     SkipList.cpp:742
    batch = ConflictBatch(cs, conflicting_key_range_map)   # ConflictBatch ctor SkipList.cpp:749
    batch.add_transaction(tr)                     # addTransaction         SkipList.cpp:763
    batch.detect_conflicts(now, new_oldest, non_conflicting, too_old)      SkipList.cpp:844
    destroy_conflict_set(cs)                      # destroyConflictSet()   SkipList.cpp:745

Every call goes through the HIP engine; there is no CPU fallback.  If the
extension is missing or no GPU is present, construction raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from .balancing import KEY_BYTES_PER_SAMPLE
from .packing import CommitTransaction, DevicePackedBatch, InvertedRange, PackedBatch, _CPackedBatch, _CPackedBatchDev

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FDBCS_LIB") or os.path.join(_HERE, "libfdbcs.so")

FDBCS_OK = 0
FDBCS_E_INVALID = -1
FDBCS_E_DEVICE = -2
FDBCS_E_NOMEM = -3
FDBCS_E_VERSION = -4
FDBCS_E_STATE = -5
FDBCS_E_NODEVICE = -6
FDBCS_E_TIMEOUT = -7

# dump_history(floor=NO_FLOOR): versions as stored, no clamp below the oldest version
NO_FLOOR = -(1 << 63)

TransactionConflict = 0
TransactionTooOld = 1
TransactionCommitted = 2

_lib = None


class FdbcsError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {strerror(status)} ({status})")


class Stats(ctypes.Structure):
    _fields_ = [
        ("batches", ctypes.c_int64),
        ("transactions", ctypes.c_int64),
        ("read_ranges", ctypes.c_int64),
        ("write_ranges", ctypes.c_int64),
        ("ms_upload", ctypes.c_double),
        ("ms_check_read", ctypes.c_double),
        ("ms_sort", ctypes.c_double),
        ("ms_intra", ctypes.c_double),
        ("ms_combine", ctypes.c_double),
        ("ms_merge", ctypes.c_double),
        ("ms_gc", ctypes.c_double),
        ("ms_total", ctypes.c_double),
        ("merge_bytes", ctypes.c_int64),
        ("merge_launches", ctypes.c_int64),
        ("ms_merge_kernel", ctypes.c_double),
        ("compactions", ctypes.c_int64),
        ("ms_compact", ctypes.c_double),
        ("compact_bytes", ctypes.c_int64),
        ("ms_compact_kernel", ctypes.c_double),
        ("ms_epilogue", ctypes.c_double),
        ("intra_edges", ctypes.c_int64),
        ("intra_rounds", ctypes.c_int64),
        ("intra_fallbacks", ctypes.c_int64),
        ("ms_check_kernel", ctypes.c_double),
        ("check_launches", ctypes.c_int64),
        ("check_reads", ctypes.c_int64),
        ("check_history", ctypes.c_int64),
        ("ms_sort_kernel", ctypes.c_double),
        ("sort_launches", ctypes.c_int64),
        ("sort_items", ctypes.c_int64),
        ("gc_runs", ctypes.c_int64),
        ("host_ms_prepare", ctypes.c_double),
        ("host_ms_record", ctypes.c_double),
        ("host_ms_submit", ctypes.c_double),
        ("compact_launches", ctypes.c_int64),
        ("merge_bytes_all", ctypes.c_int64),
        ("compact_bytes_all", ctypes.c_int64),
        ("delta_sum", ctypes.c_int64),
        ("base_sum", ctypes.c_int64),
        ("segments_sum", ctypes.c_int64),
        ("sort_big_buckets", ctypes.c_int64),
        ("routed_batches", ctypes.c_int64),
        ("ms_route_kernels", ctypes.c_double),
        ("host_ms_route", ctypes.c_double),
        ("host_ms_add", ctypes.c_double),
        ("added_txns", ctypes.c_int64),
        ("x_launches_skipped", ctypes.c_int64),
        ("x_edge_free_unskipped", ctypes.c_int64),
        ("x_held", ctypes.c_int64),
        ("x_forced", ctypes.c_int64),
        ("x_flushed", ctypes.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _CDigest(ctypes.Structure):
    """fdbcs_digest."""
    _fields_ = [
        ("n", ctypes.c_int64),
        ("key_bytes", ctypes.c_int64),
        ("header_version", ctypes.c_int64),
        ("sum", ctypes.c_uint64 * 2),
    ]


class HistoryDigest(NamedTuple):
    """fdbcs_digest: the digest of a canonical history (include/fdb_conflict_set.h has the
    definition).  Two histories are taken as equal iff the tuples are."""
    n: int
    key_bytes: int
    header_version: int
    sum: Tuple[int, int]

    @classmethod
    def _of(cls, d: "_CDigest") -> "HistoryDigest":
        return cls(int(d.n), int(d.key_bytes), int(d.header_version), (int(d.sum[0]), int(d.sum[1])))


# fdbcs_history_verify: check classes (bit c of `checks`, row c of a tier's report) and the arrays an
# override can name (FDBCS_VERIFY_OV_*).
VERIFY_CLASSES = ("order", "padding", "tails", "versions", "dominance", "lvl1", "lvl2", "lvl3", "skey8", "skey",
                  "dir", "edir")
VERIFY_ARRAYS = ("key", "len_tail", "version", "lvl1", "lvl2", "lvl3", "skey8", "skey", "dir", "edir", "tail_word")


class _CVerifyClass(ctypes.Structure):
    _fields_ = [("examined", ctypes.c_int64), ("violations", ctypes.c_int64), ("first", ctypes.c_int64)]


class _CVerifyTier(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("cls", _CVerifyClass * len(VERIFY_CLASSES))]


class _CVerifyReport(ctypes.Structure):
    """fdbcs_verify_report."""
    _fields_ = [("tier", _CVerifyTier * 2), ("edir_trusted", ctypes.c_int64)]


class _CVerifyOverride(ctypes.Structure):
    """fdbcs_verify_override."""
    _fields_ = [("what", ctypes.c_int32), ("tier", ctypes.c_int32), ("level", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("index", ctypes.c_int64), ("xor_lo", ctypes.c_uint64),
                ("xor_hi", ctypes.c_uint64)]


class VerifyOverride(NamedTuple):
    """One what-if element of ConflictSet.verify (a debug facility): the verifier reads element
    `index` of array `what` (a VERIFY_ARRAYS name) of `tier` (0 base, 1 delta) as its stored words
    XOR (xor_lo, xor_hi); nothing in device memory changes."""
    what: str
    tier: int
    index: int
    xor_lo: int = 0
    xor_hi: int = 0
    level: int = 0

    def c_struct(self) -> "_CVerifyOverride":
        m = (1 << 64) - 1
        return _CVerifyOverride(VERIFY_ARRAYS.index(self.what) + 1, int(self.tier), int(self.level), 0, int(self.index),
                                int(self.xor_lo) & m, int(self.xor_hi) & m)


def _cls(cls) -> int:
    return VERIFY_CLASSES.index(cls) if isinstance(cls, str) else int(cls)


class VerifyReport:
    """fdbcs_verify_report: per tier (0 base, 1 delta) its size and, per check class, the elements
    examined, the violations and the least violating index (-1: none)."""

    def __init__(self, sizes, rows, edir_trusted):
        self.sizes = tuple(int(x) for x in sizes)
        self.rows = tuple(tuple(tuple(int(x) for x in r) for r in t) for t in rows)  # [tier][class] -> 3 ints
        self.edir_trusted = int(edir_trusted)

    @classmethod
    def _of(cls, r: "_CVerifyReport") -> "VerifyReport":
        return cls([r.tier[t].n for t in range(2)],
                   [[(c.examined, c.violations, c.first) for c in r.tier[t].cls] for t in range(2)], r.edir_trusted)

    @property
    def ok(self) -> bool:
        return not any(r[1] for t in self.rows for r in t)

    def examined(self, tier: int, cls) -> int:
        return self.rows[tier][_cls(cls)][0]

    def violations(self, tier: int, cls) -> int:
        return self.rows[tier][_cls(cls)][1]

    def first(self, tier: int, cls) -> int:
        return self.rows[tier][_cls(cls)][2]

    def as_dict(self) -> dict:
        return {"edir_trusted": self.edir_trusted,
                "tiers": [{"n": self.sizes[t],
                           **{name: dict(zip(("examined", "violations", "first"), self.rows[t][c]))
                              for c, name in enumerate(VERIFY_CLASSES)}} for t in range(2)]}

    def __eq__(self, other):
        return isinstance(other, VerifyReport) and self.as_dict() == other.as_dict()

    def __repr__(self):
        bad = [(t, VERIFY_CLASSES[c], r) for t in range(2) for c, r in enumerate(self.rows[t]) if r[1]]
        return f"VerifyReport(sizes={self.sizes}, edir_trusted={self.edir_trusted}, violations={bad})"


class _CKeyResolvers(ctypes.Structure):
    """fdbcs_key_resolvers."""
    _fields_ = [
        ("n_ranges", ctypes.c_int32),
        ("bound_bytes", ctypes.c_void_p),
        ("bound_offsets", ctypes.c_void_p),
        ("hist_offsets", ctypes.c_void_p),
        ("hist_versions", ctypes.c_void_p),
        ("hist_resolvers", ctypes.c_void_p),
    ]


# C-ABI symbol table: name -> (restype, argtypes).  tests/ check that the library exports
# every function include/fdb_conflict_set.h declares.
_VP, _I32, _I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
SIGNATURES = {
    "fdbcs_new_conflict_set": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_VP)]),
    "fdbcs_clear_conflict_set": (ctypes.c_int, [_VP, _I64]),
    "fdbcs_destroy_conflict_set": (None, [_VP]),
    "fdbcs_set_oldest_version": (ctypes.c_int, [_VP, _I64]),
    "fdbcs_get_oldest_version": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "fdbcs_history_size": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "fdbcs_load_history": (ctypes.c_int, [_VP, _I64, _VP, _VP, _VP, _I64]),
    "fdbcs_history_export": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I32, _I64, ctypes.POINTER(_I64),
                                            ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fdbcs_history_export_read": (ctypes.c_int, [_VP, _VP, _I64, _VP, _VP, _I64]),
    "fdbcs_history_export_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_history_digest": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I32, _I64, ctypes.POINTER(_CDigest)]),
    "fdbcs_history_digest_arrays": (ctypes.c_int, [_I64, _VP, _VP, _VP, _I64, ctypes.POINTER(_CDigest)]),
    "fdbcs_history_digest_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_history_digest_ranges": (ctypes.c_int, [_VP, _I32, _VP, _VP, ctypes.c_int, ctypes.c_int, _I64, _VP]),
    "fdbcs_history_digest_arrays_ranges": (ctypes.c_int, [_I64, _VP, _VP, _VP, _I64, _I32, _VP, _VP, ctypes.c_int,
                                                          ctypes.c_int, _VP]),
    "fdbcs_history_verify": (ctypes.c_int, [_VP, ctypes.c_uint32, ctypes.POINTER(_CVerifyOverride),
                                            ctypes.POINTER(_CVerifyReport)]),
    "fdbcs_history_verify_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_history_verify_sizes": (ctypes.c_int, [ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fdbcs_history_split_keys": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I32, _I32, ctypes.POINTER(_I64),
                                                ctypes.POINTER(_I64)]),
    "fdbcs_history_split_keys_read": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64]),
    "fdbcs_history_split_keys_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                       ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_history_import": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I32, _I64, _VP, _VP, _VP, _I64,
                                            ctypes.POINTER(_I64)]),
    "fdbcs_history_import_pending": (ctypes.c_int, [_VP, _VP, _VP, _I32, _VP, _I32, ctypes.POINTER(_I64)]),
    "fdbcs_history_import_delta": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I32, _I64, _VP, _VP, _VP, _I64,
                                                  ctypes.POINTER(_I64)]),
    "fdbcs_history_import_delta_pending": (ctypes.c_int, [_VP, _VP, _VP, _I32, _VP, _I32, ctypes.POINTER(_I64)]),
    "fdbcs_history_import_info": (ctypes.c_int, [_VP, ctypes.POINTER(_I32), ctypes.POINTER(_I64),
                                                 ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fdbcs_history_import_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_get_stats": (ctypes.c_int, [_VP, ctypes.POINTER(Stats)]),
    "fdbcs_reset_stats": (ctypes.c_int, [_VP]),
    "fdbcs_set_gc_interval": (ctypes.c_int, [_VP, _I32]),
    "fdbcs_set_delta_limit": (ctypes.c_int, [_VP, _I64]),
    "fdbcs_set_timing": (ctypes.c_int, [_VP, _I32]),
    "fdbcs_reserve": (ctypes.c_int, [_VP, _I64, _I64, _I32, _I32, _I32]),
    "fdbcs_batch_new": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(_VP)]),
    "fdbcs_batch_destroy": (None, [_VP]),
    "fdbcs_batch_add_transaction": (
        ctypes.c_int,
        [_VP, _I64, ctypes.c_int, _I32, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP],
    ),
    "fdbcs_batch_add_packed": (ctypes.c_int, [_VP, ctypes.POINTER(_CPackedBatch)]),
    "fdbcs_batch_upload": (ctypes.c_int, [_VP]),
    "fdbcs_batch_detect_conflicts": (
        ctypes.c_int,
        [_VP, _I64, _I64, _VP, ctypes.POINTER(_I32), ctypes.POINTER(_I32)],
    ),
    "fdbcs_batch_detect_async": (ctypes.c_int, [_VP, _I64, _I64]),
    "fdbcs_batch_wait": (ctypes.c_int, [_VP, _VP, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "fdbcs_batch_conflicting_reads": (ctypes.c_int, [_VP, _I32, _VP, _I32, ctypes.POINTER(_I32)]),
    "fdbcs_batch_too_old": (ctypes.c_int, [_VP, _VP, _I32, ctypes.POINTER(_I32)]),
    "fdbcs_batch_device_verdicts": (ctypes.c_int, [_VP, ctypes.POINTER(_VP)]),
    "fdbcs_batch_set_conflict_output": (ctypes.c_int, [_VP, _VP, ctypes.c_int32, _VP]),
    "fdbcs_share_bytes": (ctypes.c_int, [ctypes.POINTER(_CPackedBatch), ctypes.POINTER(_I64)]),
    "fdbcs_share_pack": (ctypes.c_int, [ctypes.POINTER(_CPackedBatch), _VP, _I64, ctypes.POINTER(_I64)]),
    "fdbcs_batch_add_routed": (ctypes.c_int, [_VP, _VP, _I64, _I32, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _I32, _I64,
                                              _VP, _I64, _VP, ctypes.c_uint32]),
    "fdbcs_batch_routed_info": (ctypes.c_int, [_VP, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32),
                                               ctypes.POINTER(_VP), ctypes.POINTER(_VP)]),
    "fdbcs_route_map_pack": (ctypes.c_int, [ctypes.POINTER(_CKeyResolvers), _I32, _VP, _VP]),
    "fdbcs_batch_add_routed_map": (ctypes.c_int, [_VP, _VP, _I64, _I32, _I32, ctypes.POINTER(_CKeyResolvers), _I32,
                                                  _I32, _I32, _I32, _I64, _VP, _I64, _VP, ctypes.c_uint32]),
    "fdbcs_batch_set_report_output": (ctypes.c_int, [_VP, _VP, _I64]),
    "fdbcs_batch_report_entries": (ctypes.c_int, [_VP, _VP, _I32]),
    "fdbcs_batch_set_iops_sample": (ctypes.c_int, [_VP, _I32, ctypes.c_uint64]),
    "fdbcs_batch_iops_sample": (ctypes.c_int, [_VP, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fdbcs_batch_iops_sample_read": (ctypes.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _I64]),
    "fdbcs_batch_iops_sample_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_batch_add_packed_device": (ctypes.c_int, [_VP, ctypes.POINTER(_CPackedBatchDev), _VP, ctypes.c_uint32]),
    "fdbcs_batch_device_add_info": (ctypes.c_int, [_VP, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32),
                                                   ctypes.POINTER(_I64)]),
    "fdbcs_batch_device_add_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_share_bytes_bound": (ctypes.c_int, [_I32, _I32, _I32, _I64, ctypes.POINTER(_I64)]),
    "fdbcs_batch_share_pack_device": (ctypes.c_int, [_VP, ctypes.POINTER(_CPackedBatchDev), _VP, _I64, _VP,
                                                     ctypes.c_uint32]),
    "fdbcs_batch_share_pack_info": (ctypes.c_int, [_VP, ctypes.POINTER(_I64), ctypes.POINTER(_I32), ctypes.POINTER(_I32),
                                                   ctypes.POINTER(_I32), ctypes.POINTER(_I64)]),
    "fdbcs_batch_share_pack_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_batch_read_versions": (ctypes.c_int, [_VP, _I64, _VP, _I64]),
    "fdbcs_batch_read_versions_device": (ctypes.c_int, [_VP, _I64, _VP, _I64]),
    "fdbcs_batch_read_versions_timing": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double),
                                                        ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_debug_kernel_time": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_kernel_profile": (ctypes.c_int, [_VP, _I32, ctypes.c_char_p, _I32, ctypes.POINTER(_I64),
                                            ctypes.POINTER(ctypes.c_double)]),
    "fdbcs_set_timed_kernel": (ctypes.c_int, [_VP, ctypes.c_char_p]),
    "fdbcs_debug_hold": (ctypes.c_int, [_VP, _I32]),
    "fdbcs_debug_live_resources": (ctypes.c_int, [ctypes.POINTER(_I64)] * 4),
    "fdbcs_sync": (ctypes.c_int, [_VP]),
    "fdbcs_strerror": (ctypes.c_char_p, [ctypes.c_int]),
}


def load_library(path: str = LIB_PATH):
    """Load libfdbcs.so (build it first with foundationdb_amd.build.build()).  Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise RuntimeError(
                f"HIP extension {path} is missing; run `python -m foundationdb_amd.build` (no CPU fallback exists)"
            )
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib


def share_pack(pb: PackedBatch, out: Optional[np.ndarray] = None) -> np.ndarray:
    """fdbcs_share_pack: a proxy share (a packed batch) in the engine's wire layout, as uint8 (into
    `out` when given: e.g. a pinned torch buffer's numpy view; the used prefix is returned)."""
    L = load_library()
    cs = pb.c_struct()
    n = _I64()
    _check(L.fdbcs_share_bytes(ctypes.byref(cs), ctypes.byref(n)), "shareBytes")
    if out is None:
        out = np.zeros(n.value, np.uint8)
    if out.nbytes < n.value:
        raise ValueError(f"share needs {n.value} bytes, buffer has {out.nbytes}")
    used = _I64()
    _check(L.fdbcs_share_pack(ctypes.byref(cs), _VP(out.ctypes.data), out.nbytes, ctypes.byref(used)), "sharePack")
    return out[: used.value]


def share_bytes_bound(n_txn: int, n_reads: int, n_writes: int, key_bytes_len: int) -> int:
    """fdbcs_share_bytes_bound: the wire layout's size for these sizes with every key byte a tail
    byte; at least the exact size of any valid batch of those sizes (the all-gather stride of a
    caller that holds only device arrays)."""
    n = _I64()
    rc = load_library().fdbcs_share_bytes_bound(int(n_txn), int(n_reads), int(n_writes), int(key_bytes_len),
                                                ctypes.byref(n))
    if rc != FDBCS_OK:
        raise FdbcsError(rc, "shareBytesBound")
    return n.value


def _key_resolvers_struct(kr):
    """(fdbcs_key_resolvers, the arrays it points into) of a sharding.KeyResolvers, or of a dict
    holding the arrays of its flat() form."""
    f = kr.flat() if hasattr(kr, "flat") else kr
    arrs = [np.ascontiguousarray(f["bound_bytes"], np.uint8), np.ascontiguousarray(f["bound_offsets"], np.int64),
            np.ascontiguousarray(f["hist_offsets"], np.int64), np.ascontiguousarray(f["hist_versions"], np.int64),
            np.ascontiguousarray(f["hist_resolvers"], np.int32)]
    c = _CKeyResolvers(int(f.get("n_ranges", len(arrs[1]) - 1)), *[a.ctypes.data for a in arrs])
    return c, arrs


def route_map_pack(kr, resolver: int) -> Tuple[np.ndarray, np.ndarray]:
    """fdbcs_route_map_pack (host only): (own uint8[M], until int64[M]) of the keyResolvers map `kr`
    for one resolver.  own bit 0: the newest owner of the range; bit 1: in an older history entry,
    and then a read at snapshot s still goes to it iff until >= s."""
    c, keep = _key_resolvers_struct(kr)
    n = max(int(c.n_ranges), 0)
    own = np.zeros(n, np.uint8)
    until = np.zeros(n, np.int64)
    rc = load_library().fdbcs_route_map_pack(ctypes.byref(c), int(resolver), _VP(own.ctypes.data), _VP(until.ctypes.data))
    if rc != FDBCS_OK:
        raise FdbcsError(rc, "routeMapPack")
    del keep
    return own, until


def digest_arrays(key_bytes, key_offsets, versions, header_version: int = 0) -> HistoryDigest:
    """fdbcs_history_digest_arrays (host only): the digest of arrays in the layout dump_history
    returns and load_history takes, exactly as given (nothing is canonicalised, key order is not
    checked).  digest_arrays(*cs.dump_history(lo, hi, floor)) == cs.digest(lo, hi, floor)."""
    kb = np.ascontiguousarray(key_bytes, np.uint8)
    ko = np.ascontiguousarray(key_offsets, np.int64)
    vv = np.ascontiguousarray(versions, np.int64)
    d = _CDigest()
    rc = load_library().fdbcs_history_digest_arrays(len(vv), _p(kb), _p(ko), _p(vv), int(header_version),
                                                    ctypes.byref(d))
    if rc != FDBCS_OK:
        raise FdbcsError(rc, "historyDigestArrays")
    return HistoryDigest._of(d)


def _bounds_arrays(bounds, open_lo: bool, open_hi: bool):
    """The bounds of a partition in the export's key layout and the number of ranges they define."""
    bounds = [bytes(b) for b in bounds]
    kb = np.frombuffer(b"".join(bounds), np.uint8)
    ko = np.zeros(len(bounds) + 1, np.int64)
    np.cumsum([len(b) for b in bounds], out=ko[1:])
    return kb, ko, len(bounds) - 1 + bool(open_lo) + bool(open_hi)


def digest_arrays_ranges(key_bytes, key_offsets, versions, header_version: int, bounds, open_lo: bool = False,
                         open_hi: bool = False) -> List[HistoryDigest]:
    """fdbcs_history_digest_arrays_ranges (host only): one digest per range of the partition `bounds`
    define (ConflictSet.digest_ranges has the ranges' order) over arrays in the layout dump_history
    returns, read as given; the keys must ascend.  Range i's header is the version of the last
    boundary <= its lower bound, its boundaries those strictly inside.  How a checkpoint file or a
    model's canonical form is digested chunk by chunk."""
    kb = np.ascontiguousarray(key_bytes, np.uint8)
    ko = np.ascontiguousarray(key_offsets, np.int64)
    vv = np.ascontiguousarray(versions, np.int64)
    bb, bo, K = _bounds_arrays(bounds, open_lo, open_hi)
    out = (_CDigest * max(K, 1))()
    rc = load_library().fdbcs_history_digest_arrays_ranges(len(vv), _p(kb), _p(ko), _p(vv), int(header_version),
                                                           len(bo) - 1, _p(bb), _p(bo), int(bool(open_lo)),
                                                           int(bool(open_hi)), ctypes.addressof(out))
    if rc != FDBCS_OK:
        raise FdbcsError(rc, "historyDigestArraysRanges")
    return [HistoryDigest._of(out[i]) for i in range(K)]


def locate_divergence(digests_a, digests_b, split_keys_a, lo: Optional[bytes] = None, hi: Optional[bytes] = None,
                      fanout: int = 256, leaf: int = 64) -> List[Tuple[Optional[bytes], Optional[bytes]]]:
    """Where two holders of [lo, hi) differ, by a `fanout`-way bisection on digests: the ascending list
    of disjoint (lo, hi) ranges (None: an open end) whose digests differ, each refined until both
    sides report n <= `leaf` there or side a has no split key left inside it; [] when the whole-range
    digests are equal.  The sides are callables, so they may live in different processes:
    digests_x(bounds, open_lo, open_hi) returns that side's digests (ConflictSet.digest_ranges, or
    digest_arrays_ranges over a dump, under one floor), split_keys_a(lo, hi, want) keys of side a
    strictly inside (lo, hi) (ConflictSet.split_keys): both sides are digested on side a's keys.
    A range [s, t) covers a difference at s itself: H_f(s) is its header.  One digests call per side
    and level, whatever the number of ranges refined at that level."""
    if fanout < 2 or leaf < 0:
        raise ValueError("fanout must be at least 2 and leaf at least 0")

    def both(edges):
        bounds = [e for e in edges if e is not None]
        ol, oh = edges[0] is None, edges[-1] is None
        da, db = digests_a(bounds, ol, oh), digests_b(bounds, ol, oh)
        if len(da) != len(edges) - 1 or len(db) != len(edges) - 1:
            raise ValueError("a side returned a digest count other than the number of ranges")
        return da, db

    da, db = both([lo, hi])
    if tuple(da[0]) == tuple(db[0]):
        return []
    level, found = [((lo, hi), da[0], db[0])], []
    while level:
        # the edges of this level: every range still refined, cut at side a's keys
        edges, watch, nxt = [], [], []

        def flush():
            if watch:
                da, db = both(edges)
                subs = {}
                for parent, i in watch:
                    differing = subs.setdefault(parent, [])
                    if tuple(da[i]) != tuple(db[i]):
                        differing.append(((edges[i], edges[i + 1]), da[i], db[i]))
                for parent, differing in subs.items():
                    if differing:
                        nxt.extend(differing)
                    else:  # only by hash accident: the parent stands as it is
                        found.append(parent)
            edges.clear()
            watch.clear()

        for (rlo, rhi), ra, rb in level:
            keys = [] if ra.n <= leaf and rb.n <= leaf else [bytes(k) for k in split_keys_a(rlo, rhi, fanout - 1)]
            if not keys:
                found.append((rlo, rhi))
                continue
            if len(edges) + len(keys) + 2 > 60000:  # a call takes at most 65536 ranges
                flush()
            if edges and (edges[-1] is None or rlo is None or edges[-1] > rlo):
                raise ValueError("split keys out of order")
            first = len(edges)
            edges.extend([rlo] + keys + [rhi])
            watch.extend(((rlo, rhi), i) for i in range(first, first + len(keys) + 1))
        flush()
        level = nxt
    return sorted(found, key=lambda r: (r[0] is not None, r[0] or b""))


def live_resources() -> Tuple[int, int, int, int]:
    """fdbcs_debug_live_resources: (device buffers, pinned host buffers, events, streams) the engine
    holds right now, over every set and batch of the process.  Needs no device.  Diagnostics."""
    n = [_I64() for _ in range(4)]
    rc = load_library().fdbcs_debug_live_resources(*[ctypes.byref(x) for x in n])
    if rc != FDBCS_OK:
        raise FdbcsError(rc, "debugLiveResources")
    return tuple(x.value for x in n)


def strerror(status: int) -> str:
    try:
        return load_library().fdbcs_strerror(status).decode()
    except Exception:  # pragma: no cover - library missing
        return f"status {status}"


def _check(rc: int, what: str) -> None:
    if rc != FDBCS_OK:
        if rc == FDBCS_E_INVALID:
            raise InvertedRange(f"{what}: invalid argument") if "add" in what else FdbcsError(rc, what)
        raise FdbcsError(rc, what)


def _p(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data if a.size else 0)


def fill_verdict_lists(verdicts: np.ndarray, non_conflicting: Optional[List[int]],
                       too_old_transactions: Optional[List[int]]) -> None:
    """The verdict lists of detectConflicts (SkipList.cpp:869-876) from the verdict bytes.

    A TooOld transaction's conflict status is set to true (`conflict = tr.tooOld`,
    SkipList.cpp:820,830), so without a tooOld list it lands in neither list."""
    v = np.asarray(verdicts)
    if too_old_transactions is not None:
        too_old_transactions.extend(np.flatnonzero(v == TransactionTooOld).tolist())
    if non_conflicting is not None:
        non_conflicting.extend(np.flatnonzero(v == TransactionCommitted).tolist())


class ConflictSet:
    """Opaque ConflictSet handle (SkipList.cpp:730-737) living on one GPU."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = ctypes.c_void_p()
        _check(L.fdbcs_new_conflict_set(device, ctypes.byref(h)), "newConflictSet")
        self._h = h
        self.device = device

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None):
            load_library().fdbcs_destroy_conflict_set(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self, version: int) -> None:
        _check(load_library().fdbcs_clear_conflict_set(self._h, version), "clearConflictSet")

    @property
    def oldest_version(self) -> int:
        v = ctypes.c_int64()
        _check(load_library().fdbcs_get_oldest_version(self._h, ctypes.byref(v)), "oldestVersion")
        return v.value

    def set_oldest_version(self, v: int) -> None:
        _check(load_library().fdbcs_set_oldest_version(self._h, v), "setOldestVersion")

    def set_gc_interval(self, every: int) -> None:
        """Compaction (with GC) at least every `every` batches; 0 = only when the delta is full."""
        _check(load_library().fdbcs_set_gc_interval(self._h, every), "setGcInterval")

    def set_timing(self, level: int) -> None:
        """Device timing: 0 none, 1 the hot kernels on sampled batches (roofline), 2 every phase
        (stats()), 3 every kernel of every batch (kernel_profile())."""
        _check(load_library().fdbcs_set_timing(self._h, level), "setTiming")

    def kernel_profile(self) -> Dict[str, dict]:
        """Per-kernel launches and device milliseconds since reset_stats (timing levels 3 and 1)."""
        L = load_library()
        out = {}
        i = 0
        name = ctypes.create_string_buffer(512)
        n, ms = ctypes.c_int64(), ctypes.c_double()
        while L.fdbcs_kernel_profile(self._h, i, name, len(name), ctypes.byref(n), ctypes.byref(ms)) == FDBCS_OK:
            out[name.value.decode()] = {"launches": n.value, "ms": ms.value}
            i += 1
        return out

    def set_timed_kernel(self, name: Optional[str]) -> None:
        """The kernel timed on sampled batches at timing level 1 (a name kernel_profile() reported)."""
        _check(load_library().fdbcs_set_timed_kernel(self._h, (name or "").encode()), "setTimedKernel")

    def sync(self) -> None:
        """Block until every engine stream is idle (uploads and every submitted stage): the engine's
        HIP runtime is not torch's, so torch.cuda.synchronize() does not wait for it."""
        _check(load_library().fdbcs_sync(self._h), "sync")

    def debug_hold(self, on: bool) -> None:
        """Diagnostics: hold every stream (on) so batches submitted next queue up; release (off)."""
        _check(load_library().fdbcs_debug_hold(self._h, 1 if on else 0), "debugHold")

    def set_delta_limit(self, boundaries: int) -> None:
        """Delta-tier bound that triggers a compaction; 0 = automatic (~1/16 of the base)."""
        _check(load_library().fdbcs_set_delta_limit(self._h, boundaries), "setDeltaLimit")

    def reserve(self, boundaries: int, tail_bytes: int = 0, max_txns: int = 0, max_reads: int = 0,
                max_writes: int = 0) -> None:
        _check(load_library().fdbcs_reserve(self._h, boundaries, tail_bytes, max_txns, max_reads, max_writes),
               "reserve")

    def history_size(self) -> int:
        v = ctypes.c_int64()
        _check(load_library().fdbcs_history_size(self._h, ctypes.byref(v)), "historySize")
        return v.value

    def load_history(self, key_bytes, key_offsets, versions, header_version: int = 0) -> None:
        kb = np.ascontiguousarray(key_bytes, np.uint8)
        ko = np.ascontiguousarray(key_offsets, np.int64)
        vv = np.ascontiguousarray(versions, np.int64)
        _check(
            load_library().fdbcs_load_history(self._h, len(vv), _p(kb), _p(ko), _p(vv), header_version),
            "loadHistory",
        )

    def export_history(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None,
                       floor: Optional[int] = None) -> Tuple[int, int, int]:
        """fdbcs_history_export: run the export on the device and leave the result there; returns
        (boundaries, key bytes, header version).  read_export() fetches it."""
        L = load_library()
        if floor is None:
            floor = self.oldest_version
        kl = np.frombuffer(lo if lo is not None else b"", np.uint8)
        kh = np.frombuffer(hi if hi is not None else b"", np.uint8)
        n, nb, hdr = _I64(), _I64(), _I64()
        _check(L.fdbcs_history_export(self._h, _p(kl), len(kl) if lo is not None else -1, _p(kh),
                                      len(kh) if hi is not None else -1, floor, ctypes.byref(n), ctypes.byref(nb),
                                      ctypes.byref(hdr)), "historyExport")
        return n.value, nb.value, hdr.value

    def read_export(self, n: int, key_bytes: int):
        """fdbcs_history_export_read into fresh arrays of the sizes export_history returned."""
        kb = np.empty(key_bytes, np.uint8)
        ko = np.empty(n + 1, np.int64)
        vv = np.empty(n, np.int64)
        _check(load_library().fdbcs_history_export_read(self._h, _p(kb), key_bytes, _p(ko), _p(vv), n),
               "historyExportRead")
        return kb, ko, vv

    def export_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last export's kernels (device) and of the last read's copies (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _check(load_library().fdbcs_history_export_timing(self._h, ctypes.byref(a), ctypes.byref(b)), "exportTiming")
        return a.value, b.value

    def dump_history(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None, floor: Optional[int] = None):
        """The canonical history over [lo, hi): (key_bytes uint8[], key_offsets int64[n+1], versions
        int64[n], header_version), the keys where the version a read sees changes, with versions
        below `floor` (default: the oldest version; NO_FLOOR: none) read as floor - 1.  The tuple
        unpacks into load_history(*...)."""
        n, nb, hdr = self.export_history(lo, hi, floor)
        kb, ko, vv = self.read_export(n, nb)
        return kb, ko, vv, hdr

    def digest(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None,
               floor: Optional[int] = None) -> HistoryDigest:
        """fdbcs_history_digest: the digest of the canonical history over [lo, hi), what
        dump_history(lo, hi, floor) would return, computed on the device without an export (`floor`
        defaults to the oldest version, as there).  a.digest(lo, hi) == b.digest(lo, hi) checks a
        hand-over or a restore across GPUs or processes; a pending export stays readable."""
        if floor is None:
            floor = self.oldest_version
        kl, ll, kh, hl = self._bounds(lo, hi)
        d = _CDigest()
        _check(load_library().fdbcs_history_digest(self._h, _p(kl), ll, _p(kh), hl, floor, ctypes.byref(d)),
               "historyDigest")
        return HistoryDigest._of(d)

    def digest_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last digest's kernels (device) and of the whole call (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _check(load_library().fdbcs_history_digest_timing(self._h, ctypes.byref(a), ctypes.byref(b)), "digestTiming")
        return a.value, b.value

    def verify(self, checks=None, override: Optional[VerifyOverride] = None) -> VerifyReport:
        """fdbcs_history_verify: recompute on the device everything a lookup relies on (key order,
        padding, tails, the range-max levels, the samples, both directories, the delta's dominance
        over the base) where the set lies, and report per tier and class what is wrong and where.
        `checks`: an iterable of VERIFY_CLASSES names or a bit mask (default: all).  `override`: one
        what-if element (debug).  Read-only; raises FdbcsError(FDBCS_E_STATE) with batches in flight."""
        mask = 0
        if checks is not None:
            mask = int(checks) if isinstance(checks, int) else sum(1 << _cls(c) for c in checks)
        ov = override.c_struct() if override is not None else None
        out = _CVerifyReport()
        _check(load_library().fdbcs_history_verify(self._h, mask, ctypes.byref(ov) if ov is not None else None,
                                                   ctypes.byref(out)), "historyVerify")
        return VerifyReport._of(out)

    def verify_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last verify's kernels (device) and of the whole call (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _check(load_library().fdbcs_history_verify_timing(self._h, ctypes.byref(a), ctypes.byref(b)), "verifyTiming")
        return a.value, b.value

    def digest_ranges(self, bounds, floor: Optional[int] = None, open_lo: bool = False,
                      open_hi: bool = False) -> List[HistoryDigest]:
        """fdbcs_history_digest_ranges: the digests of the ranges the ascending keys `bounds` define,
        in one pass on the device: first the range below bounds[0] if `open_lo`, then
        [bounds[i], bounds[i + 1]) for each neighbouring pair, then the range from bounds[-1] on if
        `open_hi`.  Entry i equals digest(lo_i, hi_i, floor) of range i."""
        if floor is None:
            floor = self.oldest_version
        bb, bo, K = _bounds_arrays(bounds, open_lo, open_hi)
        out = (_CDigest * max(K, 1))()
        _check(load_library().fdbcs_history_digest_ranges(self._h, len(bo) - 1, _p(bb), _p(bo), int(bool(open_lo)),
                                                          int(bool(open_hi)), floor, ctypes.addressof(out)),
               "historyDigestRanges")
        return [HistoryDigest._of(out[i]) for i in range(K)]

    def split_keys(self, lo: Optional[bytes], hi: Optional[bytes], want: int) -> List[bytes]:
        """fdbcs_history_split_keys: up to `want` boundary keys strictly inside (lo, hi), ascending, at
        evenly spaced positions of the tier that holds more boundaries there.  They depend on the tier
        split and the GC cadence, not on the canonical history alone: use them as bounds only, and on
        both sides of a comparison use one side's keys."""
        L = load_library()
        kl, ll, kh, hl = self._bounds(lo, hi)
        n, nb = _I64(), _I64()
        _check(L.fdbcs_history_split_keys(self._h, _p(kl), ll, _p(kh), hl, int(want), ctypes.byref(n), ctypes.byref(nb)),
               "historySplitKeys")
        kb = np.empty(nb.value, np.uint8)
        ko = np.empty(n.value + 1, np.int64)
        _check(L.fdbcs_history_split_keys_read(self._h, _p(kb), nb.value, _p(ko), n.value), "historySplitKeysRead")
        raw = kb.tobytes()
        return [raw[ko[i]:ko[i + 1]] for i in range(n.value)]

    def split_keys_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last split_keys' kernels (device) and of its first call (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _check(load_library().fdbcs_history_split_keys_timing(self._h, ctypes.byref(a), ctypes.byref(b)),
               "splitKeysTiming")
        return a.value, b.value

    def diverging_ranges(self, other: "ConflictSet", lo: Optional[bytes] = None, hi: Optional[bytes] = None,
                         floor: Optional[int] = None, fanout: int = 256, leaf: int = 64):
        """locate_divergence for two sets of one process: the ranges of [lo, hi) in which this set's
        and `other`'s canonical histories differ under `floor` (default: this set's oldest version),
        bisected on this set's split keys."""
        if floor is None:
            floor = self.oldest_version
        return locate_divergence(lambda b, ol, oh: self.digest_ranges(b, floor, ol, oh),
                                 lambda b, ol, oh: other.digest_ranges(b, floor, ol, oh), self.split_keys, lo, hi,
                                 fanout, leaf)

    def read_versions(self, ranges, floor: Optional[int] = None) -> np.ndarray:
        """The history version each of `ranges` (a list of (begin, end) byte pairs, begin <= end) is
        checked against, int64 per range: ConflictBatch.read_versions of one throw-away batch whose
        reads they are.  `(r > V).any()` answers "did anything in these ranges change since version
        V" without spending a transaction; a.read_versions(rs) == b.read_versions(rs) checks a
        hand-over pointwise.  With no batch of the set in flight."""
        ranges = [(bytes(b), bytes(e)) for b, e in ranges]
        if not ranges:
            return np.empty(0, np.int64)
        keys = [k for r in ranges for k in r]
        ko = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([len(k) for k in keys], out=ko[1:])
        # one transaction no oldest version makes TooOld (a TooOld transaction carries no ranges)
        pb = PackedBatch(np.full(1, (1 << 63) - 1, np.int64), np.zeros(1, np.uint8), np.array([0, len(ranges)], np.int32),
                         np.zeros(2, np.int32), np.frombuffer(b"".join(keys), np.uint8), ko)
        batch = ConflictBatch(self)
        try:
            batch.add_packed(pb)
            return batch.read_versions(floor)
        finally:
            batch.close()

    def version_at(self, key: bytes, floor: Optional[int] = None) -> int:
        """The version a read of `key` sees: the read [key, key + b"\\x00")."""
        return int(self.read_versions([(key, bytes(key) + b"\x00")], floor)[0])

    @staticmethod
    def _bounds(lo: Optional[bytes], hi: Optional[bytes]):
        kl = np.frombuffer(lo if lo is not None else b"", np.uint8)
        kh = np.frombuffer(hi if hi is not None else b"", np.uint8)
        return kl, (len(kl) if lo is not None else -1), kh, (len(kh) if hi is not None else -1)

    @staticmethod
    def _into(into: str) -> bool:
        if into not in ("base", "delta"):
            raise ValueError(f"into must be 'base' or 'delta', not {into!r}")
        return into == "delta"

    def merge_history(self, key_bytes, key_offsets, versions, header_version: int = 0,
                      lo: Optional[bytes] = None, hi: Optional[bytes] = None, into: str = "base") -> int:
        """fdbcs_history_import: fold an exported history (the arrays dump_history returns) into
        this set over [lo, hi): every key there afterwards reads the greater of the version it read
        before and the imported one.  Returns the history size afterwards.
        dst.merge_history(*src.dump_history(lo, hi), lo=lo, hi=hi) hands [lo, hi) over.
        into="delta" (fdbcs_history_import_delta) writes the delta tier only, at a cost that does not
        depend on the base's size; import_info() tells which path ran."""
        delta = self._into(into)
        kb = np.ascontiguousarray(key_bytes, np.uint8)
        ko = np.ascontiguousarray(key_offsets, np.int64)
        vv = np.ascontiguousarray(versions, np.int64)
        kl, ll, kh, hl = self._bounds(lo, hi)
        out = _I64()
        L = load_library()
        f = L.fdbcs_history_import_delta if delta else L.fdbcs_history_import
        _check(f(self._h, _p(kl), ll, _p(kh), hl, len(vv), _p(kb), _p(ko), _p(vv), header_version, ctypes.byref(out)),
               "historyImportDelta" if delta else "historyImport")
        return out.value

    def merge_pending_export(self, src: "ConflictSet", lo: Optional[bytes] = None, hi: Optional[bytes] = None,
                             into: str = "base") -> int:
        """fdbcs_history_import_pending: the same import, reading the result of src.export_history()
        from src's device buffers (same device; no host copy).  src's result stays readable.
        into="delta": fdbcs_history_import_delta_pending."""
        delta = self._into(into)
        kl, ll, kh, hl = self._bounds(lo, hi)
        out = _I64()
        L = load_library()
        f = L.fdbcs_history_import_delta_pending if delta else L.fdbcs_history_import_pending
        _check(f(self._h, src._h, _p(kl), ll, _p(kh), hl, ctypes.byref(out)),
               "historyImportDeltaPending" if delta else "historyImportPending")
        return out.value

    def import_info(self) -> dict:
        """fdbcs_history_import_info: the last successful import's path (0: folded into a new base,
        1: merged into the delta), the base tier's size after it and the delta tier's around it."""
        path, base, before, after = _I32(), _I64(), _I64(), _I64()
        _check(load_library().fdbcs_history_import_info(self._h, ctypes.byref(path), ctypes.byref(base),
                                                        ctypes.byref(before), ctypes.byref(after)), "importInfo")
        return {"path": path.value, "base_boundaries": base.value, "delta_before": before.value,
                "delta_after": after.value}

    def import_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last import's kernels (device) and of the whole call (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _check(load_library().fdbcs_history_import_timing(self._h, ctypes.byref(a), ctypes.byref(b)), "importTiming")
        return a.value, b.value

    def stats(self) -> dict:
        s = Stats()
        _check(load_library().fdbcs_get_stats(self._h, ctypes.byref(s)), "stats")
        return s.as_dict()

    def reset_stats(self) -> None:
        _check(load_library().fdbcs_reset_stats(self._h), "resetStats")


def new_conflict_set(device: int = 0) -> ConflictSet:
    return ConflictSet(device)


def clear_conflict_set(cs: ConflictSet, version: int) -> None:
    cs.clear(version)


def destroy_conflict_set(cs: ConflictSet) -> None:
    cs.close()


class ConflictBatch:
    """ConflictBatch (fdbserver/ConflictSet.h:35-69) over the HIP engine."""

    TransactionConflict = TransactionConflict
    TransactionTooOld = TransactionTooOld
    TransactionCommitted = TransactionCommitted

    def __init__(self, cs: ConflictSet, conflicting_key_range_map: Optional[Dict[int, List[int]]] = None):
        L = load_library()
        h = ctypes.c_void_p()
        _check(L.fdbcs_batch_new(cs.handle, 1 if conflicting_key_range_map is not None else 0, ctypes.byref(h)),
               "ConflictBatch")
        self._h = h
        self.cs = cs
        self.conflicting_key_range_map = conflicting_key_range_map
        self.transaction_count = 0
        self._n_reads = 0  # read ranges added
        # per add call what tells the reads of each of its transactions: a count, or a packed batch's
        # read_offsets as given (only read_versions looks at them, for a batch with TooOld transactions)
        self._txn_reads: list = []
        self._report: List[bool] = []
        self._has_reads: List[bool] = []
        self._keep = []  # arrays that must outlive add calls (keys are copied by the library)
        self.verdicts: Optional[np.ndarray] = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            load_library().fdbcs_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_transaction(self, tr: CommitTransaction) -> None:
        """addTransaction (SkipList.cpp:763-794)."""
        L = load_library()

        def arrs(ranges, which):
            keys = [getattr(r, which) for r in ranges]
            bufs = [ctypes.create_string_buffer(bytes(k), max(1, len(k))) for k in keys]
            ptrs = (ctypes.c_void_p * max(1, len(keys)))(*[ctypes.addressof(b) for b in bufs])
            lens = (ctypes.c_int32 * max(1, len(keys)))(*[len(k) for k in keys])
            return bufs, ptrs, lens

        rb = arrs(tr.read_conflict_ranges, "begin")
        re = arrs(tr.read_conflict_ranges, "end")
        wb = arrs(tr.write_conflict_ranges, "begin")
        we = arrs(tr.write_conflict_ranges, "end")
        rc = L.fdbcs_batch_add_transaction(
            self._h,
            tr.read_snapshot,
            1 if tr.report_conflicting_keys else 0,
            len(tr.read_conflict_ranges),
            ctypes.cast(rb[1], ctypes.c_void_p),
            ctypes.cast(rb[2], ctypes.c_void_p),
            ctypes.cast(re[1], ctypes.c_void_p),
            ctypes.cast(re[2], ctypes.c_void_p),
            len(tr.write_conflict_ranges),
            ctypes.cast(wb[1], ctypes.c_void_p),
            ctypes.cast(wb[2], ctypes.c_void_p),
            ctypes.cast(we[1], ctypes.c_void_p),
            ctypes.cast(we[2], ctypes.c_void_p),
        )
        _check(rc, "addTransaction")
        self.transaction_count += 1
        self._n_reads += len(tr.read_conflict_ranges)
        self._txn_reads.append(len(tr.read_conflict_ranges))
        if self.conflicting_key_range_map is not None:
            self._report.append(bool(tr.report_conflicting_keys))
            self._has_reads.append(len(tr.read_conflict_ranges) > 0)

    def add_packed(self, pb: PackedBatch) -> None:
        """addTransaction for every transaction of a packed batch, in order."""
        cs = pb.c_struct()
        _check(load_library().fdbcs_batch_add_packed(self._h, ctypes.byref(cs)), "addTransaction(packed)")
        self.transaction_count += pb.n_txn
        self._n_reads += pb.n_reads
        self._txn_reads.append(pb.read_offsets)
        if self.conflicting_key_range_map is not None:  # per-transaction bookkeeping only for reports
            self._report.extend(bool(x) for x in pb.report)
            self._has_reads.extend((np.diff(pb.read_offsets) > 0).tolist())

    def add_packed_device(self, dpb: DevicePackedBatch, ready_ptr: int = 0, ready_value: int = 0) -> None:
        """fdbcs_batch_add_packed_device: addTransaction of every transaction of a packed batch whose
        arrays are in device memory, on a new batch; validated and normalized by kernels, which run
        once the uint32 at device address `ready_ptr` equals `ready_value` (0: the arrays are
        complete).  The host reads none of the arrays; they stay untouched until device_add_info()
        or detect has returned.  TooOld is judged at detect, as for a routed batch.  Any error
        status raises FdbcsError; a violation the kernels find comes from device_add_info() or
        detect (FDBCS_E_INVALID), and leaves the batch empty."""
        c = dpb.c_struct()
        rc = load_library().fdbcs_batch_add_packed_device(self._h, ctypes.byref(c), _VP(ready_ptr or None),
                                                          int(ready_value) & 0xFFFFFFFF)
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "addPackedDevice")
        self.transaction_count = int(dpb.n_txn)
        self._n_reads = int(dpb.n_reads)
        self._dev_added = True

    def device_add_info(self) -> Tuple[int, int, int, int]:
        """fdbcs_batch_device_add_info: blocks until the add kernels have run; (transactions, reads,
        writes, tail bytes) of the device-added batch, or their error (FdbcsError; the batch is then
        empty again)."""
        T, R, W, tb = _I32(), _I32(), _I32(), _I64()
        rc = load_library().fdbcs_batch_device_add_info(self._h, ctypes.byref(T), ctypes.byref(R), ctypes.byref(W),
                                                        ctypes.byref(tb))
        if rc != FDBCS_OK:
            if rc != FDBCS_E_STATE:
                self.transaction_count = 0
                self._n_reads = 0
                self._dev_added = False
            raise FdbcsError(rc, "deviceAddInfo")
        return T.value, R.value, W.value, tb.value

    def device_add_timing(self) -> Tuple[float, float]:
        """Milliseconds of the add kernels (device) and inside the add call (host), once
        device_add_info() or detect has returned."""
        a, b = ctypes.c_double(), ctypes.c_double()
        rc = load_library().fdbcs_batch_device_add_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "deviceAddTiming")
        return a.value, b.value

    def share_pack_device(self, dpb: DevicePackedBatch, out_ptr: int, cap: int, ready_ptr: int = 0,
                          ready_value: int = 0) -> None:
        """fdbcs_batch_share_pack_device: the proxy share of a packed batch whose arrays are in
        device memory, written by kernels into the `cap` bytes of device memory at `out_ptr`
        (64-byte aligned; e.g. this rank's slot of the all-gather buffer), byte for byte what
        share_pack() gives.  On a new, empty batch, which stays empty: afterwards it takes
        share_pack_info() / share_pack_timing(), add_routed() / add_routed_map(), a further pack and
        close().  The kernels run once the uint32 at `ready_ptr` equals `ready_value` (0: the arrays
        are complete).  A violation the kernels find comes from share_pack_info() or the routed add
        and leaves the empty share at `out_ptr`."""
        c = dpb.c_struct()
        rc = load_library().fdbcs_batch_share_pack_device(self._h, ctypes.byref(c), _VP(out_ptr or None), int(cap),
                                                          _VP(ready_ptr or None), int(ready_value) & 0xFFFFFFFF)
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "sharePackDevice")

    def share_pack_info(self) -> Tuple[int, int, int, int, int]:
        """fdbcs_batch_share_pack_info: blocks until the pack kernels have run; (bytes, transactions,
        reads, writes, tail bytes) of the share's header, or the pack's error (FdbcsError)."""
        n, T, R, W, tb = _I64(), _I32(), _I32(), _I32(), _I64()
        rc = load_library().fdbcs_batch_share_pack_info(self._h, ctypes.byref(n), ctypes.byref(T), ctypes.byref(R),
                                                        ctypes.byref(W), ctypes.byref(tb))
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "sharePackInfo")
        return n.value, T.value, R.value, W.value, tb.value

    def share_pack_timing(self) -> Tuple[float, float]:
        """Milliseconds of the pack kernels (device) and inside the pack call (host), once the pack
        has been waited for (share_pack_info() or a routed add)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        rc = load_library().fdbcs_batch_share_pack_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "sharePackTiming")
        return a.value, b.value

    def upload(self) -> None:
        _check(load_library().fdbcs_batch_upload(self._h), "upload")

    def add_routed(self, shares_ptr: int, stride: int, n_shares: int, max_share_txns: int, lo: Optional[bytes],
                   hi: Optional[bytes], caps: Tuple[int, int, int, int], conflict_out: int = 0, n_global: int = 0,
                   ready_ptr: int = 0, ready_value: int = 0) -> None:
        """fdbcs_batch_add_routed: this resolver's part ([lo, hi); None = unbounded) of the shares
        gathered at device address `shares_ptr` (`stride` bytes apart), routed on the device once
        the uint32 at device address `ready_ptr` equals `ready_value` (the caller's stream sets it
        after the all-gather: torch's collectives run in their own HIP runtime, whose stream
        handles this engine cannot wait on; 0 = the shares are complete already).
        caps = (txns, reads, writes, tail bytes) bounds of the routed batch."""
        lo_b = bytes(lo) if lo is not None else b""
        hi_b = bytes(hi) if hi is not None else b""
        lo_buf = ctypes.create_string_buffer(lo_b, max(1, len(lo_b)))
        hi_buf = ctypes.create_string_buffer(hi_b, max(1, len(hi_b)))
        _check(load_library().fdbcs_batch_add_routed(
            self._h, _VP(shares_ptr), int(stride), int(n_shares), int(max_share_txns), ctypes.cast(lo_buf, _VP),
            len(lo_b) if lo is not None else -1, ctypes.cast(hi_buf, _VP), len(hi_b) if hi is not None else -1,
            int(caps[0]), int(caps[1]), int(caps[2]), int(caps[3]), _VP(conflict_out or None), int(n_global),
            _VP(ready_ptr or None), int(ready_value) & 0xFFFFFFFF), "addRouted")
        self._routed = True

    def add_routed_map(self, shares_ptr: int, stride: int, n_shares: int, max_share_txns: int, key_resolvers,
                       resolver: int, caps: Tuple[int, int, int, int], conflict_out: int = 0, n_global: int = 0,
                       ready_ptr: int = 0, ready_value: int = 0) -> None:
        """fdbcs_batch_add_routed_map: add_routed under a keyResolvers map with its ownership history
        (a sharding.KeyResolvers, or the arrays of its flat() form) instead of a static [lo, hi):
        this batch is routed as resolver `resolver` of that map.  The map is read during the call
        and travels with the batch, so the next batch may pass another one.  Any error status,
        FDBCS_E_INVALID of an invalid map included, raises FdbcsError."""
        c, keep = _key_resolvers_struct(key_resolvers)
        rc = load_library().fdbcs_batch_add_routed_map(
            self._h, _VP(shares_ptr), int(stride), int(n_shares), int(max_share_txns), ctypes.byref(c), int(resolver),
            int(caps[0]), int(caps[1]), int(caps[2]), int(caps[3]), _VP(conflict_out or None), int(n_global),
            _VP(ready_ptr or None), int(ready_value) & 0xFFFFFFFF)
        del keep
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "routedMap")
        self._routed = True

    def routed_info(self) -> Tuple[int, int, int, int, int]:
        """(transactions, reads, writes, device address of the global -> batch map, of the read ids)."""
        T, R, W = _I32(), _I32(), _I32()
        inv, rid = _VP(), _VP()
        _check(load_library().fdbcs_batch_routed_info(self._h, ctypes.byref(T), ctypes.byref(R), ctypes.byref(W),
                                                      ctypes.byref(inv), ctypes.byref(rid)), "routedInfo")
        return T.value, R.value, W.value, inv.value or 0, rid.value or 0

    def detect_async(self, now: int, new_oldest_version: int) -> None:
        _check(load_library().fdbcs_batch_detect_async(self._h, now, new_oldest_version), "detectConflicts")

    def wait(self) -> np.ndarray:
        if getattr(self, "_routed", False):
            self.transaction_count = self.routed_info()[0]
        v = np.zeros(self.transaction_count, np.uint8)
        _check(load_library().fdbcs_batch_wait(self._h, _p(v), None, None), "wait")
        self.verdicts = v
        self._collect_conflicting_keys()
        return v

    def detect_conflicts(
        self,
        now: int,
        new_oldest_version: int,
        non_conflicting: Optional[List[int]] = None,
        too_old_transactions: Optional[List[int]] = None,
    ) -> np.ndarray:
        """detectConflicts (SkipList.cpp:844-890).  Appends to the lists exactly as the reference
        does (SkipList.cpp:869-876) and returns the per-transaction verdict bytes
        (Resolver.actor.cpp:196-204 encoding)."""
        v = np.zeros(self.transaction_count, np.uint8)
        rc = load_library().fdbcs_batch_detect_conflicts(self._h, now, new_oldest_version, _p(v), None, None)
        _check(rc, "detectConflicts")
        self.verdicts = v
        fill_verdict_lists(v, non_conflicting, too_old_transactions)
        self._collect_conflicting_keys()
        return v

    def debug_kernel_time(self, which: int = 0, reps: int = 50) -> float:
        """Average device microseconds of one launch of a pipeline kernel on this (uploaded, not
        yet detected) batch against the current history: 0 = the read check.  Tuning only."""
        us = ctypes.c_double()
        _check(load_library().fdbcs_debug_kernel_time(self._h, which, reps, ctypes.byref(us)), "debugKernelTime")
        return us.value

    def _floor(self, floor: Optional[int]) -> int:
        return self.cs.oldest_version if floor is None else int(floor)

    def _read_versions_failed(self, rc: int, what: str):
        # a violation the add kernels found surfaces here as it does from device_add_info()
        if getattr(self, "_dev_added", False) and rc not in (FDBCS_E_STATE, FDBCS_E_NOMEM):
            self.transaction_count = 0
            self._n_reads = 0
            self._dev_added = False
        raise FdbcsError(rc, what)

    def _held_reads(self) -> int:
        """Reads the batch holds: a transaction that was TooOld when added carries no ranges
        (SkipList.cpp:770-790); a device-added batch is judged at detect and holds them all."""
        if getattr(self, "_dev_added", False) or not self._txn_reads:
            return self._n_reads
        too_old: List[int] = []
        self.get_too_old_transactions(too_old)
        if not too_old:
            return self._n_reads
        per_txn = np.concatenate([np.diff(x) if isinstance(x, np.ndarray) else [x] for x in self._txn_reads])
        return self._n_reads - int(per_txn[too_old].sum())

    def read_versions(self, floor: Optional[int] = None) -> np.ndarray:
        """fdbcs_batch_read_versions: int64 per read of this batch (in read order), the history
        version the read is checked against: the greatest version any key of [begin, end) reads (for
        an empty read [k, k): the version just below k), with versions below `floor` (default: the
        oldest version; NO_FLOOR: none) read as floor - 1.  A read that is not TooOld conflicts with
        the history iff its entry is above its snapshot; the reads of a transaction that was TooOld
        when added are not held by the batch and have no entry.  On a batch that is being added or
        is uploaded, with no batch of the set in flight; the batch is uploaded and can be detected
        afterwards as if it had not been queried."""
        out = np.empty(self._held_reads(), np.int64)
        rc = load_library().fdbcs_batch_read_versions(self._h, self._floor(floor), _p(out), len(out))
        if rc != FDBCS_OK:
            self._read_versions_failed(rc, "readVersions")
        return out

    def read_versions_device(self, dev_out_ptr: int, cap: int, floor: Optional[int] = None) -> None:
        """fdbcs_batch_read_versions_device: the same, written as int64 to the `cap` entries of
        device memory at `dev_out_ptr` (the set's GPU; e.g. a torch tensor's data_ptr()); complete
        when the call returns."""
        rc = load_library().fdbcs_batch_read_versions_device(self._h, self._floor(floor), _VP(dev_out_ptr or None),
                                                             int(cap))
        if rc != FDBCS_OK:
            self._read_versions_failed(rc, "readVersionsDevice")

    def read_versions_timing(self) -> Tuple[float, float]:
        """Milliseconds of the last read_versions kernel on this batch's set (device) and of the whole
        call (host)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        rc = load_library().fdbcs_batch_read_versions_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        if rc != FDBCS_OK:
            raise FdbcsError(rc, "readVersionsTiming")
        return a.value, b.value

    def device_verdicts_ptr(self) -> int:
        p = ctypes.c_void_p()
        _check(load_library().fdbcs_batch_device_verdicts(self._h, ctypes.byref(p)), "deviceVerdicts")
        return p.value or 0

    def set_conflict_output(self, txn_ids: np.ndarray, n_global: int, dev_out: int) -> None:
        """fdbcs_batch_set_conflict_output: detect also writes the multi-resolver conflict bytes of
        this batch's transactions (global indices `txn_ids`) into device memory `dev_out` (an
        address, e.g. a torch tensor's data_ptr())."""
        ids = np.ascontiguousarray(txn_ids, dtype=np.int32)
        _check(load_library().fdbcs_batch_set_conflict_output(self._h, _VP(ids.ctypes.data if ids.size else 0),
                                                              int(n_global), _VP(dev_out)), "setConflictOutput")

    def set_report_output(self, dev_out: int, n_global_reads: int) -> None:
        """fdbcs_batch_set_report_output: on a routed batch created with a
        conflicting_key_range_map, detect also writes the report bytes, one per read of the
        concatenated shares (`n_global_reads` of them), into device memory `dev_out` (an address):
        1 where this resolver's conflictingKeyRangeMap holds the read, for sharding.
        combine_report_bytes / an all-reduce MAX."""
        _check(load_library().fdbcs_batch_set_report_output(self._h, _VP(dev_out or None), int(n_global_reads)),
               "setReportOutput")

    def set_iops_sample(self, units: int = KEY_BYTES_PER_SAMPLE, seed: int = 0) -> None:
        """fdbcs_batch_set_iops_sample: on a routed batch, before detect, take the resolver's iops
        sample (Resolver.actor.cpp:178-192) of the batch on the device, with `units` metric units
        per sample under the counter-based roll balancing.iops_roll restates, seeded with `seed`
        (64 bits).  iops_sample() fetches it."""
        _check(load_library().fdbcs_batch_set_iops_sample(self._h, int(units), int(seed) & 0xFFFFFFFFFFFFFFFF),
               "setIopsSample")

    def iops_sample_raw(self):
        """fdbcs_batch_iops_sample + _read: (key_bytes uint8[], key_offsets int64[n + 1], metrics
        int32[n], index int32[n]) of the sampled range begins, in range order.  Waits for the
        routing and the sample only, not for detect; may be called again until the batch is closed."""
        L = load_library()
        n, nb = _I64(), _I64()
        _check(L.fdbcs_batch_iops_sample(self._h, ctypes.byref(n), ctypes.byref(nb)), "iopsSample")
        kb = np.empty(nb.value, np.uint8)
        ko = np.empty(n.value + 1, np.int64)
        met = np.empty(n.value, np.int32)
        idx = np.empty(n.value, np.int32)
        _check(L.fdbcs_batch_iops_sample_read(self._h, _p(kb), nb.value, _p(ko), _p(met), _p(idx), n.value),
               "iopsSampleRead")
        return kb, ko, met, idx

    def iops_sample(self) -> Tuple[List[bytes], np.ndarray, np.ndarray]:
        """(keys, metrics, index) of the sampled range begins: what ResolverLoad.add_sampled takes."""
        kb, ko, met, idx = self.iops_sample_raw()
        raw = kb.tobytes()
        return [raw[ko[i]:ko[i + 1]] for i in range(len(met))], met, idx

    def iops_sample_timing(self) -> float:
        """Milliseconds of the sample's kernels on the device (after iops_sample())."""
        ms = ctypes.c_double()
        _check(load_library().fdbcs_batch_iops_sample_timing(self._h, ctypes.byref(ms)), "iopsSampleTiming")
        return ms.value

    def report_entries(self) -> np.ndarray:
        """fdbcs_batch_report_entries: uint8 per transaction, 1 where the reference would have
        created conflictingKeyRangeMap[t] (SkipList.cpp:770-784).  Valid after detect."""
        n = len(self.verdicts) if self.verdicts is not None else self.transaction_count
        out = np.zeros(n, np.uint8)
        _check(load_library().fdbcs_batch_report_entries(self._h, _p(out), n), "reportEntries")
        return out

    def get_too_old_transactions(self, too_old_transactions: List[int]) -> None:
        """GetTooOldTransactions (SkipList.cpp:836-842): appends the transactions whose add-time
        TooOld test held (SkipList.cpp:770); valid right after addTransaction, before detect."""
        L = load_library()
        n = _I32(0)
        _check(L.fdbcs_batch_too_old(self._h, None, 0, ctypes.byref(n)), "GetTooOldTransactions")
        out = np.zeros(max(n.value, 1), np.int32)
        _check(L.fdbcs_batch_too_old(self._h, _p(out), n.value, ctypes.byref(n)), "GetTooOldTransactions")
        too_old_transactions.extend(out[: n.value].tolist())

    def conflicting_reads(self, t: int) -> List[int]:
        L = load_library()
        n = ctypes.c_int32()
        _check(L.fdbcs_batch_conflicting_reads(self._h, t, None, 0, ctypes.byref(n)), "conflictingReads")
        out = np.zeros(max(1, n.value), np.int32)
        _check(L.fdbcs_batch_conflicting_reads(self._h, t, _p(out), n.value, ctypes.byref(n)), "conflictingReads")
        return out[: n.value].tolist()

    def _collect_conflicting_keys(self) -> None:
        m = self.conflicting_key_range_map
        if m is None:
            return
        if getattr(self, "_routed", False) or getattr(self, "_dev_added", False):
            # a routed batch's sub-transactions were placed on the device: the engine says which
            # have an entry; the indices are the sub-transaction's own (this resolver's map).  A
            # device-added batch's flags and offsets were never on the host either
            for t in np.flatnonzero(self.report_entries()).tolist():
                entry = m.setdefault(t, [])
                if self.verdicts[t] == TransactionConflict:
                    entry.extend(self.conflicting_reads(t))
            return
        # the reference creates (*conflictingKeyRangeMap)[t] while registering the read ranges of a
        # reporting, admitted transaction (SkipList.cpp:777-784): only transactions with reads get
        # an entry; conflicting read indices are appended to it
        for t, rep in enumerate(self._report):
            if rep and self._has_reads[t] and self.verdicts[t] != TransactionTooOld:
                entry = m.setdefault(t, [])
                if self.verdicts[t] == TransactionConflict:
                    entry.extend(self.conflicting_reads(t))
