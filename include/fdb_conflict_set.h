/*
 * fdb_conflict_set.h — C-ABI of the MI355X-native MVCC conflict-resolution engine.
 *
 * Drop-in boundary for the FoundationDB resolver hot path.  Each entry point
 * replaces one member of the reference interface `fdbserver/ConflictSet.h`
 * (implemented by `fdbserver/SkipList.cpp`); the citation on every
 * declaration names the reference line it stands in for.  Plain C types only:
 * pointers, sizes, int64 versions.  No entry point throws; every fallible call
 * returns an `int` status (FDBCS_OK == 0, negative on error).
 *
 * Semantics are those of the reference:
 *   - keys are unsigned byte strings, compared memcmp-then-length
 *     (SkipList.cpp:53-60, flow/Arena.h:692-697);
 *   - a transaction is TooOld iff read_snapshot < oldestVersion and it has at
 *     least one read range (SkipList.cpp:770);
 *   - history conflict: some read range [b,e) overlaps history written at a
 *     version > read_snapshot (SkipList.cpp:619-706);
 *   - intra-batch conflict: in batch order, a read range overlaps a write range
 *     of an earlier committed transaction of the same batch (SkipList.cpp:812-834);
 *   - committed write ranges are recorded at version `now` (SkipList.cpp:899-939);
 *   - verdict bytes use the reference enum: 0 = TransactionConflict,
 *     1 = TransactionTooOld, 2 = TransactionCommitted (ConflictSet.h:40-44).
 *
 * Threading: like the reference (single flow thread, Resolver.actor.cpp:179-194)
 * a conflict set handle is not thread-safe; one handle per GPU.
 * Precondition the reference relies on implicitly (Resolver orders batches by
 * version, Resolver.actor.cpp:139-150): `now` never decreases below a version
 * already written; violating it returns FDBCS_E_VERSION.
 */
#ifndef FDB_CONFLICT_SET_H
#define FDB_CONFLICT_SET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes. */
#define FDBCS_OK 0
#define FDBCS_E_INVALID (-1)   /* bad argument: NULL handle, inverted range (KeyRangeRef throws inverted_range, FDBTypes.h:288-291), ... */
#define FDBCS_E_DEVICE (-2)    /* HIP runtime error */
#define FDBCS_E_NOMEM (-3)     /* host or device allocation failed / capacity exceeded */
#define FDBCS_E_VERSION (-4)   /* `now` below a version already present in the history */
#define FDBCS_E_STATE (-5)     /* call out of order (e.g. add after detect) */
#define FDBCS_E_NODEVICE (-6)  /* no HIP device / extension unusable: the product never falls back to the CPU */
#define FDBCS_E_TIMEOUT (-7)   /* a routed batch's shares never became ready (fdbcs_batch_add_routed) */

/* Verdict bytes: ConflictBatch::TransactionCommitResult (ConflictSet.h:40-44). */
#define FDBCS_TRANSACTION_CONFLICT 0
#define FDBCS_TRANSACTION_TOO_OLD 1
#define FDBCS_TRANSACTION_COMMITTED 2

typedef struct fdbcs_conflict_set fdbcs_conflict_set; /* ConflictSet (SkipList.cpp:730-737) */
typedef struct fdbcs_batch fdbcs_batch;               /* ConflictBatch (ConflictSet.h:35-69) */

/*
 * Packed, structure-of-arrays form of a commit batch: the CommitTransactionRef
 * fields the conflict set reads (CommitTransaction.h:184-188), flattened.
 * R = read_offsets[n_txn], W = write_offsets[n_txn].
 * Key k occupies key_bytes[key_offsets[k] .. key_offsets[k+1]).
 * Read range r (0 <= r < R): begin key 2r, end key 2r+1.
 * Write range w (0 <= w < W): begin key 2(R+w), end key 2(R+w)+1.
 * Ranges of transaction t: reads [read_offsets[t], read_offsets[t+1]),
 * writes [write_offsets[t], write_offsets[t+1]), in the transaction's order
 * (that order defines indexInTx for conflicting-key reports, SkipList.cpp:781).
 */
typedef struct fdbcs_packed_batch {
    int32_t n_txn;
    const int64_t* read_snapshot;           /* [n_txn] CommitTransactionRef::read_snapshot */
    const uint8_t* report_conflicting_keys; /* [n_txn] or NULL (= all false) */
    const int32_t* read_offsets;            /* [n_txn+1] */
    const int32_t* write_offsets;           /* [n_txn+1] */
    const uint8_t* key_bytes;               /* key arena */
    const int64_t* key_offsets;             /* [2*(R+W)+1] */
} fdbcs_packed_batch;

/* Per-phase device time (HIP events on the engine's stream, see fdbcs_set_timing), accumulated
 * since the last reset.  Phase names mirror the reference PerfDoubleCounters
 * D.CheckRead / D.Sort / D.CheckIntraBatch / D.Combine / D.MergeWrite /
 * D.RemoveBefore (SkipList.cpp:49-51). */
typedef struct fdbcs_stats {
    int64_t batches;
    int64_t transactions;
    int64_t read_ranges;
    int64_t write_ranges;
    double ms_upload;       /* H2D of packed batches */
    double ms_check_read;   /* history check (search + range max over both tiers; overlaps the sort) */
    double ms_sort;         /* endpoint sort */
    double ms_intra;        /* intra-batch candidate edges + batch-order resolution */
    double ms_combine;      /* union of committed writes */
    double ms_merge;        /* merge into the delta tier */
    double ms_gc;           /* removeBefore equivalent (runs with compactions) */
    double ms_total;        /* whole detect pipeline, device time */
    int64_t merge_bytes;    /* algorithmic bytes moved by the delta-merge copy kernel */
    int64_t merge_launches;
    double ms_merge_kernel; /* device time of the delta-merge copy kernel alone */
    int64_t compactions;    /* delta tier folded into the base tier */
    double ms_compact;      /* compaction phase (search + scan + copy) */
    int64_t compact_bytes;  /* algorithmic bytes moved by the compaction copy kernel */
    double ms_compact_kernel; /* device time of the compaction copy kernel alone */
    double ms_epilogue;     /* range-max rebuild + verdicts */
    int64_t intra_edges;    /* candidate intra-batch edges (sum over batches) */
    int64_t intra_rounds;   /* batch-order resolution rounds (sum over batches) */
    int64_t intra_fallbacks;/* batches resolved by the sequential MiniConflictSet replay */
    /* Roofline inputs of the other hot kernels (timing level >= 1), see roofline.py. */
    double ms_check_kernel; /* device time of the read-check kernel (D.CheckRead) */
    int64_t check_launches;
    int64_t check_reads;    /* read ranges checked (sum over launches) */
    int64_t check_history;  /* boundaries searched: base + delta tier size at check time (sum) */
    double ms_sort_kernel;  /* device time of the per-bucket sort kernel (D.Sort) */
    int64_t sort_launches;
    int64_t sort_items;     /* endpoints sorted (sum over launches) */
    int64_t gc_runs;        /* removeBefore passes (full, over the base tier after a compaction) */
    /* Host time inside fdbcs_batch_detect_async (milliseconds, summed): capacity checks and result
     * buffers, the host part of the upload, recording both stages, submitting them. */
    double host_ms_prepare;
    double host_ms_record;
    double host_ms_submit;
    int64_t compact_launches; /* compactions whose copy kernel was timed (compact_bytes counts these only) */
    /* Shapes of every batch, whatever the timing level (the roofline's byte models, roofline.py). */
    int64_t merge_bytes_all;   /* algorithmic bytes of every delta-merge copy */
    int64_t compact_bytes_all; /* algorithmic bytes of every compaction copy */
    int64_t delta_sum;         /* delta-tier boundaries at the start of each batch's merge, summed */
    int64_t base_sum;          /* base-tier boundaries after each batch, summed */
    int64_t segments_sum;      /* union segments of committed writes, summed */
    int64_t sort_big_buckets;  /* sort buckets past the per-wave capacity (ranked by their workgroup) */
    /* Device routing (fdbcs_batch_add_routed): batches, device time of their routing kernels
     * (events around them, every routed batch) and host time inside the call. */
    int64_t routed_batches;
    double ms_route_kernels;
    double host_ms_route;
    /* addTransaction of whole batches (fdbcs_batch_add_packed): host time inside the
     * calls (validation, normalization into pinned staging) and the calls' transactions. */
    double host_ms_add;
    int64_t added_txns;
    /* Launches of batch-order resolution left out of a batch's X half because the host had seen
     * its stage A find no candidate intra-batch edge (k_resolve, k_combine, k_intra_report). */
    int64_t x_launches_skipped;
    /* Edge-free batches whose X half was issued with those launches in it: the host issued it
     * before stage A's edge count had arrived (too early to skip).  Counted at the batch's wait; a
     * batch closed without a wait is never counted. */
    int64_t x_edge_free_unskipped;
    /* The held stage-B lists ("The held X half"): batches held right now (a gauge, at
     * most 2), X halves issued at their second call because two were held, and batches issued by a
     * flush from the calling thread (a wait, sync or close reached them, or two went out at one
     * call and the older one took this path). */
    int64_t x_held;
    int64_t x_forced;
    int64_t x_flushed;
} fdbcs_stats;

/* newConflictSet() — SkipList.cpp:739-741.  `device` = HIP ordinal. */
int fdbcs_new_conflict_set(int device, fdbcs_conflict_set** out);
/* clearConflictSet(cs, v) — SkipList.cpp:742-744: history reset to all-v, oldestVersion kept. */
int fdbcs_clear_conflict_set(fdbcs_conflict_set* cs, int64_t version);
/* destroyConflictSet(cs) — SkipList.cpp:745-747. */
void fdbcs_destroy_conflict_set(fdbcs_conflict_set* cs);

/* Raise-only oldestVersion (the effect of SkipList.cpp:880-882 without GC);
 * affects the next batch's TooOld test (SkipList.cpp:770). */
int fdbcs_set_oldest_version(fdbcs_conflict_set* cs, int64_t version);
int fdbcs_get_oldest_version(const fdbcs_conflict_set* cs, int64_t* out);
/* Boundaries held on the device, both tiers (SkipList::count, SkipList.cpp:386-394; equal to the
 * reference's count right after a compaction with GC, an upper bound otherwise). */
int fdbcs_history_size(fdbcs_conflict_set* cs, int64_t* out);
/* Bulk-load a history: boundaries sorted strictly ascending, boundary i holds
 * version versions[i] for keys in [key_i, key_{i+1}); keys below the first
 * boundary read `header_version`.  Used by benchmarks to prefill an MVCC window. */
int fdbcs_load_history(fdbcs_conflict_set* cs, int64_t n, const uint8_t* key_bytes,
                       const int64_t* key_offsets, const int64_t* versions, int64_t header_version);
/* Canonical export of the history over [lo, hi), computed on the device; the set is not modified.
 * No reference counterpart (the reference never serialises its skip list).
 * With H(k) the version a read of key k sees and H_f(k) = H(k) if H(k) >= floor_version, else
 * floor_version - 1 (INT64_MIN: no clamp; with the oldest version as floor the result does not
 * depend on whether or when GC ran): *header_version_out = H_f(lo) (no lower bound: the clamped
 * header of the set), and the boundaries are the keys lo < k < hi where H_f changes, ascending,
 * each with its new value, adjacent equal values coalesced; keys are the original bytes.  The
 * result stays in device buffers owned by the set (allocated by the first export) until it is read;
 * *n_out and *key_bytes_out are the capacities fdbcs_history_export_read needs.  lo > hi is
 * FDBCS_E_INVALID; with batches in flight FDBCS_E_STATE, and nothing is touched.
 * Key-byte offsets are exact 64-bit values (the byte scan cannot wrap); a set of 2^29 boundaries or
 * one whose keys could pass 32 GiB is refused with FDBCS_E_NOMEM. */
int fdbcs_history_export(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, /* lo_len < 0: no lower bound */
                         const uint8_t* hi_key, int32_t hi_len,                       /* hi_len < 0: no upper bound */
                         int64_t floor_version, int64_t* n_out, int64_t* key_bytes_out,
                         int64_t* header_version_out);
/* Copy the pending export out, in the layout fdbcs_load_history takes (key_offsets [n+1], versions
 * [n]), and release it.  FDBCS_E_NOMEM when a capacity is too small (the result stays available);
 * FDBCS_E_STATE when no result is pending or the set changed since the export (a detect, a load,
 * a clear; another export replaces the result). */
int fdbcs_history_export_read(fdbcs_conflict_set* cs, uint8_t* key_bytes, int64_t key_bytes_cap,
                              int64_t* key_offsets, int64_t* versions, int64_t cap);
/* Diagnostics: device time of the last export's kernels and host time of the last read's copies (ms). */
int fdbcs_history_export_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_d2h);
/* Digest of the canonical history over [lo, hi): 40 bytes that two holders of a range compare
 * instead of two exports (a restored checkpoint against the set it was taken from, the two sides of
 * a hand-over, two resolvers on different GPUs or in different processes, the device state against
 * a host model).  No reference counterpart.  All integer, mod 2^64, restatable bit for bit on a host.
 * The canonical history is exactly what fdbcs_history_export defines for the same arguments: the
 * header H_f(lo) and the keys lo < k < hi where H_f changes, each with its new value v, equal
 * neighbours coalesced (same clamp, same open bounds, INT64_MIN as floor: no clamp).
 *   M(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *          z = z ^ (z >> 31)                 (splitmix64's finalizer, as the iops roll below)
 *   G = 0x9E3779B97F4A7C15,  S_0 = 0x243F6A8885A308D3,  S_1 = 0x13198A2E03707344
 * A key of L bytes is read as m = ceil(L / 8) words, w_j = bytes [8j, 8j + 8) big-endian, zero past
 * L (the empty key has none).  For lane c in {0, 1}:
 *   h = M(S_c + L);  for j in 0 .. m - 1: h = M((h ^ w_j) + G);  e_c(k, v) = M((h ^ (uint64)v) + G)
 * and sum[c] is the sum of e_c over the canonical boundaries.  The length enters before any word, so
 * "a" and "a\0" differ; the sums commute, so no order of keys, tiles or atomics matters.  Two digests
 * are equal iff all five fields are.  Equal canonical histories always give equal digests; unequal
 * ones collide only by hash accident (two independent 64-bit sums).  Not cryptographic: it detects
 * divergence, it does not resist someone constructing a collision. */
typedef struct fdbcs_digest {
    int64_t n;              /* canonical boundaries */
    int64_t key_bytes;      /* sum of their lengths */
    int64_t header_version; /* H_f(lo) */
    uint64_t sum[2];        /* sum[c] = sum of e_c(k_i, v_i) mod 2^64 */
} fdbcs_digest;
/* The digest of this set's canonical history over [lo, hi) under floor_version, computed on the
 * device; the set is not modified.  n, key_bytes and header_version equal what fdbcs_history_export
 * reports for the same arguments.  Status as the export's: FDBCS_E_STATE with batches in flight,
 * FDBCS_E_INVALID for lo > hi or a NULL handle or out; lo == hi gives n = 0 and the header.  Unlike
 * the export it stores no key: it allocates only one scratch pair per delta boundary, one word per
 * 1024 boundaries and a word block (a set that was never exported is fine), it has no 2^29-boundary
 * or 32 GiB limit, and a pending export result of the set stays pending and readable. */
int fdbcs_history_digest(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, /* lo_len < 0: no lower bound */
                         const uint8_t* hi_key, int32_t hi_len,                       /* hi_len < 0: no upper bound */
                         int64_t floor_version, fdbcs_digest* out);
/* Host only (no device is touched): the digest of arrays in the layout of fdbcs_load_history and
 * fdbcs_history_export_read, exactly as given: nothing is canonicalised and key order is not
 * checked.  How a checkpoint file, a host-side dump or a model's state is digested.
 * FDBCS_E_INVALID for n < 0, a NULL array that n or the offsets say is read, key_offsets[0] != 0 or
 * decreasing offsets. */
int fdbcs_history_digest_arrays(int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                                const int64_t* versions, int64_t header_version, fdbcs_digest* out);
/* Diagnostics: device time of the last digest's kernels and host time of the whole call (ms). */
int fdbcs_history_digest_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host);
/* The digests of many key ranges of this set's canonical history in one pass on the device: what two
 * holders whose digests differ exchange to find out where (one call per level of a K-way bisection
 * instead of K), and the digest of a checkpoint chunk by chunk.  No reference counterpart.
 * The bounds s_0 <= s_1 <= ... <= s_{n_bounds-1} are host bytes in the export's key layout
 * (bound_offsets [n_bounds + 1], bound_offsets[0] = 0).  They define, in this order, the range from
 * below every key to s_0 if open_lo is set, [s_i, s_{i+1}) for each neighbouring pair, and the range
 * from the last bound to the end if open_hi is set: K = n_bounds - 1 + open_lo + open_hi ranges
 * (n_bounds = 0 with both ends open is the whole history).  out[i] equals, field for field, what
 * fdbcs_history_digest returns for range i under the same floor_version (n, key_bytes, header_version
 * = H_f at the range's lower bound, both sums); equal neighbouring bounds give n = 0 and the header,
 * as lo == hi does there.  A canonical boundary equal to an interior bound belongs to no range (it
 * is the header of the range it opens), so the whole span's n is the sum of the ranges' n plus the
 * interior bounds that are canonical boundaries.
 * One pass over the stream of both tiers whatever K is: the bounds' stream positions are found by one
 * launch (long bounds included), the tiles are the single digest's.  Scratch grows with K and the
 * tile count only, in buffers the set owns.  The set is not modified and a pending export result
 * stays pending and readable.  FDBCS_E_STATE with batches in flight; FDBCS_E_INVALID for a NULL
 * handle or out, n_bounds < 0, K < 1, bound_offsets[0] != 0, decreasing offsets or decreasing
 * bounds; FDBCS_E_NOMEM for K > 65536 (the bound of the routing map's ranges).
 * fdbcs_history_digest_timing reports the last call of either kind. */
int fdbcs_history_digest_ranges(fdbcs_conflict_set* cs, int32_t n_bounds, const uint8_t* bound_bytes,
                                const int64_t* bound_offsets /* [n_bounds + 1] */, int open_lo, int open_hi,
                                int64_t floor_version, fdbcs_digest* out /* [K] */);
/* Host only (no device is touched): the same partition over arrays in the layout of
 * fdbcs_load_history, read as given (nothing is canonicalised).  The arrays' keys must ascend, as a
 * canonical history's do; this is not checked.  Range i's header_version is the version of the last
 * boundary <= its lower bound (header_version if there is none, or below an open low end), its
 * boundaries are those strictly between its bounds.  On the arrays fdbcs_history_export_read returns
 * for a span it gives what fdbcs_history_digest_ranges gives for the set over the same bounds: how a
 * checkpoint file or a model's canonical form is digested chunk by chunk.  Validation as
 * fdbcs_history_digest_arrays and, for the bounds, as fdbcs_history_digest_ranges. */
int fdbcs_history_digest_arrays_ranges(int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                                       const int64_t* versions, int64_t header_version, int32_t n_bounds,
                                       const uint8_t* bound_bytes, const int64_t* bound_offsets, int open_lo,
                                       int open_hi, fdbcs_digest* out /* [K] */);
/* Verify the stored state: one read-only pass over both tiers, on the device, that recomputes
 * everything a lookup relies on, independently of the kernels that build it and of the lookups, and
 * says what is wrong and where.  No reference counterpart.  The digest compares the canonical history
 * and goes through the lookups; this checks what the lookups stand on.  After a restore or a
 * hand-over: digest equal and verify clean.
 * Tier 0 is the base (its size: the device scalar n), tier 1 the current delta buffer (ndb[current]);
 * the non-current buffers are scratch and are not read.  A tier of n boundaries holds keys (a
 * zero-padded 16-byte prefix as two big-endian words, a length, and for a key over 16 bytes the 8-byte
 * unit of its tail in the tail arena) and versions (INT64_MIN in the delta: a hole, the base shows
 * through).  Check classes, each per tier, each with three counts (examined, violations, least
 * violating index or -1):
 *   ORDER      key[i] < key[i+1] in the full order (prefix words, tail bytes, length), i + 1 < n;
 *              index i.  A pair that needs a tail TAILS flags is examined and not judged.
 *   PADDING    the prefix bytes at and past len are zero (every key).  The bytes between the end of a
 *              tail and its 8-byte pad are NOT checked: the merge copies whole words from a batch's
 *              packed tails, and every comparison masks them off.
 *   TAILS      for len > 16: 8 * unit + 8 * ceil((len - 16) / 8) <= tail_used (only long keys are
 *              examined: the unit of a shorter key is never read by anything).
 *   VERSIONS   no base version is a hole (base only).
 *   DOMINANCE  (reported under the delta) a delta boundary j with a version v covers [d_j, d_j+1): no
 *              base version that holds inside that span exceeds v.  Examined pair by pair: (j, the base
 *              boundary at or below d_j, the set's header version if there is none) and (j, every base
 *              boundary strictly inside the span); each pair with a greater base version is one
 *              violation at index j.  This is what makes "the maximum of the two tiers' maxima" the
 *              version a read is checked against.
 *   LVL1/LVL2  lvl1[b] (lvl2[c]) equals the maximum of the versions [64 b, 64 b + 64) ([4096 c, ...))
 *              clipped to n, for every entry that covers a boundary; index b (c).
 *   LVL3       for entry j < ceil(n / 262144): the maximum of its eight replica words equals the
 *              span's true maximum (so none exceeds it; a replica below it is allowed); index j.
 *   SKEY8      skey8[e] == prefix of key[8 e], e < ceil(n / 8); index e.
 *   SKEY       skey[L][d] == prefix of key[64 * 8^L * d] for every level L < 12 and every d whose
 *              boundary is below n; index L << 48 | d.
 *   DIR        (base, when the set has a directory) for every slot v in [0, dir_top + 1]: dir[v] is the
 *              number of group starts (key[8 e]) whose directory slot is below v: it lies in
 *              [0, ceil(n / 8)], start dir[v] - 1 has a slot below v and start dir[v] has not; index
 *              v, examined dir_top + 2.  Beside it, the slots of the group starts never decrease: a
 *              start whose slot is below its predecessor's is a violation at that slot.
 *   EDIR       (delta) the same for every entry whose epoch tag is the current one; the others are
 *              left alone (edir_trusted counts the current ones).  Without a current epoch nothing is
 *              examined.
 * An empty tier is clean with nothing examined.  checks: a bit per class (FDBCS_VERIFY_*), 0 = all.
 * The verifier survives the states it looks for: sizes are clamped to the allocated capacities, and no
 * stored value (a tail unit, a directory count) is used as an index before it is checked; what
 * depends on a value out of range is skipped.  Counts are atomic sums and firsts atomic minima, so a
 * report is deterministic.
 * Override (ov, or NULL: the set as stored), a debug facility: every kernel reads the one element it
 * names as its stored words XOR the masks; nothing in device memory changes, so a what-if needs no
 * restore and no other entry point ever sees a damaged set.  index counts elements of the array
 * (LVL3: replica word 8 j + r; TAIL_WORD: 8-byte word of the arena, tier ignored; SKEY: entry d of
 * `level`).  A 16-byte element takes xor_hi on its first word and xor_lo on its second; (len, tail)
 * takes xor_lo on len and xor_hi on the unit; smaller elements take xor_lo.
 * Returns FDBCS_OK whether or not violations were found; FDBCS_E_STATE with batches in flight;
 * FDBCS_E_INVALID for a NULL handle or out, an unknown check bit, or an override that names no
 * element of the set as it stands.  The set is not modified, a pending export or split-keys result
 * stays pending, scratch is a few hundred bytes the set owns from the first call on. */
#define FDBCS_VERIFY_CLASSES 12
enum {
    FDBCS_VERIFY_ORDER = 1 << 0, FDBCS_VERIFY_PADDING = 1 << 1, FDBCS_VERIFY_TAILS = 1 << 2,
    FDBCS_VERIFY_VERSIONS = 1 << 3, FDBCS_VERIFY_DOMINANCE = 1 << 4, FDBCS_VERIFY_LVL1 = 1 << 5,
    FDBCS_VERIFY_LVL2 = 1 << 6, FDBCS_VERIFY_LVL3 = 1 << 7, FDBCS_VERIFY_SKEY8 = 1 << 8,
    FDBCS_VERIFY_SKEY = 1 << 9, FDBCS_VERIFY_DIR = 1 << 10, FDBCS_VERIFY_EDIR = 1 << 11
};
enum {
    FDBCS_VERIFY_OV_KEY = 1, FDBCS_VERIFY_OV_LEN_TAIL = 2, FDBCS_VERIFY_OV_VERSION = 3, FDBCS_VERIFY_OV_LVL1 = 4,
    FDBCS_VERIFY_OV_LVL2 = 5, FDBCS_VERIFY_OV_LVL3 = 6, FDBCS_VERIFY_OV_SKEY8 = 7, FDBCS_VERIFY_OV_SKEY = 8,
    FDBCS_VERIFY_OV_DIR = 9, FDBCS_VERIFY_OV_EDIR = 10, FDBCS_VERIFY_OV_TAIL_WORD = 11
};
typedef struct fdbcs_verify_class {
    int64_t examined, violations, first; /* first: least violating index, -1 when none */
} fdbcs_verify_class;
typedef struct fdbcs_verify_tier {
    int64_t n; /* the tier's size as the device scalar gives it */
    fdbcs_verify_class cls[FDBCS_VERIFY_CLASSES];
} fdbcs_verify_tier;
typedef struct fdbcs_verify_report {
    fdbcs_verify_tier tier[2]; /* 0 base, 1 delta */
    int64_t edir_trusted;      /* delta-directory entries of the current epoch */
} fdbcs_verify_report;
typedef struct fdbcs_verify_override {
    int32_t what, tier, level, reserved; /* FDBCS_VERIFY_OV_*; level: SKEY only */
    int64_t index;
    uint64_t xor_lo, xor_hi;
} fdbcs_verify_override;
int fdbcs_history_verify(fdbcs_conflict_set* cs, uint32_t checks /* bit per class, 0 = all */,
                         const fdbcs_verify_override* ov /* NULL: the set as stored */, fdbcs_verify_report* out);
/* Diagnostics: device time of the last verify's kernels and host time of the whole call (ms). */
int fdbcs_history_verify_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host);
/* sizeof(fdbcs_verify_report) and sizeof(fdbcs_verify_override) as the library was built (600, 40):
 * what a binding checks its own layout against. */
int fdbcs_history_verify_sizes(int64_t* report_bytes, int64_t* override_bytes);
/* Up to `want` boundary keys strictly inside (lo, hi), strictly ascending, in original bytes: bounds
 * to bisect a range on without an export.  They are taken at evenly spaced positions among the
 * boundaries inside the range of whichever tier (base or delta) holds more of them there: fewer than
 * `want` when that tier holds fewer, none when the range holds no boundary.
 * The keys depend on how the history is split between the tiers and on when GC ran: they are NOT
 * canonical, and two sets with equal canonical histories may return different keys.  They serve only
 * as bounds (fdbcs_history_digest_ranges accepts any ascending keys); both sides of a comparison use
 * the keys of one side.
 * Two calls, as the export: this one runs on the device and reports the sizes, the read copies the
 * result out (key_offsets [n + 1]) and releases it; FDBCS_E_NOMEM from the read for a capacity too
 * small (the result stays), FDBCS_E_STATE when none is pending.  The result is a copy: it stays
 * readable whatever the set does next, until it is read or another call replaces it.  The set is
 * not modified and a pending export result stays pending and readable.  FDBCS_E_STATE with batches
 * in flight, FDBCS_E_INVALID for lo > hi, want < 0 or a NULL argument, FDBCS_E_NOMEM for
 * want > 65536. */
int fdbcs_history_split_keys(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, /* lo_len < 0: no lower bound */
                             const uint8_t* hi_key, int32_t hi_len,                       /* hi_len < 0: no upper bound */
                             int32_t want, int64_t* n_out, int64_t* key_bytes_out);
int fdbcs_history_split_keys_read(fdbcs_conflict_set* cs, uint8_t* key_bytes, int64_t key_bytes_cap,
                                  int64_t* key_offsets, int64_t cap);
/* Diagnostics: device time of the last fdbcs_history_split_keys' kernels and host time of the call (ms). */
int fdbcs_history_split_keys_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host);
/* Merge an exported history range into a live set, on the device: the receiving half of a range
 * hand-over.  No reference counterpart.  The arrays are in the layout of fdbcs_load_history and the
 * export and describe a step function I: I(k) is the version of the last imported boundary <= k,
 * header_version if there is none.  With H(k) the version a read of k sees in this set, afterwards
 *   H'(k) = max(H(k), I(k)) for lo <= k < hi,  H'(k) = H(k) elsewhere
 * (lo_len < 0: from below every key, and the set's header becomes max(header, header_version);
 * hi_len < 0: to the end).  Imported boundaries need not lie inside the range: one <= lo only
 * determines I(lo), one >= hi is ignored.  lo == hi changes nothing but still validates the arrays;
 * lo > hi is FDBCS_E_INVALID.  INT64_MIN is not a version.
 * Both tiers are folded into a new base (O(set), like a compaction) and the delta becomes empty;
 * *boundaries_out is the history size afterwards.  The oldest version does not move and no floor is
 * applied; a later detect with `now` below the greatest version the import left in the history is
 * FDBCS_E_VERSION.  A pending export result of this set is dropped.  Capacity grows as for
 * fdbcs_load_history; the directory code fixed at the last load / clear is kept.
 * Atomic: FDBCS_E_STATE with batches in flight, FDBCS_E_INVALID for keys not strictly ascending, a
 * negative key length, key_offsets[0] != 0 or offsets outside the bytes, FDBCS_E_NOMEM for a
 * capacity failure; in each case the set is exactly as before.  The host does no per-boundary work:
 * the three arrays are uploaded as they are and validated, normalized, searched and folded by
 * kernels. */
int fdbcs_history_import(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, /* lo_len < 0: no lower bound */
                         const uint8_t* hi_key, int32_t hi_len,                       /* hi_len < 0: no upper bound */
                         int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                         const int64_t* versions, int64_t header_version, int64_t* boundaries_out);
/* The same import, reading src's pending export result (fdbcs_history_export) straight from src's
 * device buffers: no host copy of keys, offsets or versions.  src must be another set on the same
 * device (else FDBCS_E_INVALID) with a pending export (else FDBCS_E_STATE), which stays pending and
 * readable. */
int fdbcs_history_import_pending(fdbcs_conflict_set* dst, fdbcs_conflict_set* src, const uint8_t* lo_key,
                                 int32_t lo_len, const uint8_t* hi_key, int32_t hi_len, int64_t* boundaries_out);
/* The same import (same H', same validation, error codes and atomicity: on any error the set is
 * exactly as before), written into the delta tier only: device work is O(boundaries of the base,
 * the delta and the import inside [lo, hi) + size of the delta), whatever the base holds.
 * Inside [lo, hi) the new delta carries H' at every key where H' changes, base boundaries included,
 * equal neighbours coalesced, so every delta version is still a hole or at least every base version
 * it covers (no delta entry at an imported version spans a base boundary of a greater one).  With a
 * lower bound, a delta boundary at lo carries H'(lo); with an upper bound, a delta boundary at hi
 * carries what the delta held there before (the version of its last boundary <= hi, a hole if
 * none), unless the delta already has a boundary at hi.  Outside the range the delta is unchanged.
 * Without a lower bound the set's header becomes max(header, header_version); the delta has no
 * header of its own.  Kept base and delta boundaries keep their tails; only kept imported keys
 * longer than 16 bytes append tails to the arena (FDBCS_E_NOMEM at its 32 GiB limit).
 * When the delta afterwards could pass its bound (delta boundaries + base boundaries in the range +
 * imported boundaries + 2 over the delta limit) or its capacity cannot grow, the call runs
 * fdbcs_history_import instead (fdbcs_history_import_info reports path 0): never an error for a
 * range that call accepts.
 * *boundaries_out is what fdbcs_history_size returns afterwards: both tiers, an upper bound of the
 * reference's count as between compactions, not the canonical count (base boundaries in the range
 * are now also present in the delta, until the next compaction folds them).
 * A later detect with `now` below the greatest version left in the new delta is FDBCS_E_VERSION (a
 * great version the range clipped away does not count).  FDBCS_E_STATE with batches in flight.  The
 * oldest version does not move, no floor is applied, the directory code is kept, and a pending export
 * of the set is dropped. */
int fdbcs_history_import_delta(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, /* lo_len < 0: no lower bound */
                               const uint8_t* hi_key, int32_t hi_len,                       /* hi_len < 0: no upper bound */
                               int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                               const int64_t* versions, int64_t header_version, int64_t* boundaries_out);
/* fdbcs_history_import_delta reading src's pending export, as fdbcs_history_import_pending does. */
int fdbcs_history_import_delta_pending(fdbcs_conflict_set* dst, fdbcs_conflict_set* src, const uint8_t* lo_key,
                                       int32_t lo_len, const uint8_t* hi_key, int32_t hi_len,
                                       int64_t* boundaries_out);
/* Diagnostics: the last successful import of either kind.  *path: 0 = folded into a new base, 1 =
 * merged into the delta; *base_boundaries: the base tier afterwards; *delta_before / *delta_after:
 * the delta tier around it.  All zero before the first import. */
int fdbcs_history_import_info(fdbcs_conflict_set* cs, int32_t* path, int64_t* base_boundaries,
                              int64_t* delta_before, int64_t* delta_after);
/* Diagnostics: device time of the last import's kernels and host time of the whole call (ms), for
 * the imports of both kinds. */
int fdbcs_history_import_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host);
int fdbcs_get_stats(fdbcs_conflict_set* cs, fdbcs_stats* out);
int fdbcs_reset_stats(fdbcs_conflict_set* cs);
/* Pre-size device capacity (history boundaries, history tail bytes, and the largest batch
 * shape) so later batches never reallocate; sizes are upper bounds, 0 keeps the current. */
int fdbcs_reserve(fdbcs_conflict_set* cs, int64_t boundaries, int64_t tail_bytes, int32_t max_txns,
                  int32_t max_reads, int32_t max_writes);
/* The history is two-tiered: every batch merges into a small delta tier; a
 * compaction folds the delta into the base tier, and removeBefore (GC) runs
 * with it when the oldest version moved.  Compaction happens when the delta may
 * exceed its limit (set_delta_limit; 0 = automatic, ~1/16 of the base) and, if
 * `every` > 0, at least every `every` batches (default 0).  Both knobs are
 * verdict-neutral: they only trade memory for speed. */
int fdbcs_set_gc_interval(fdbcs_conflict_set* cs, int32_t every);
int fdbcs_set_delta_limit(fdbcs_conflict_set* cs, int64_t boundaries);
/* Device timing of the pipeline (HIP events; each recorded event costs a few microseconds of
 * queue time, so production runs keep them off): 0 = none (default), 1 = the hot kernels only
 * (read check, bucket sort, the two history copy kernels: ms_*_kernel), 2 = every phase of
 * fdbcs_stats. */
int fdbcs_set_timing(fdbcs_conflict_set* cs, int32_t level);

/* ConflictBatch(cs, conflictingKeyRangeMap, arena) — SkipList.cpp:749-752.
 * report_keys != 0 enables conflictingKeyRangeMap collection for transactions
 * that set report_conflicting_keys. */
int fdbcs_batch_new(fdbcs_conflict_set* cs, int report_keys, fdbcs_batch** out);
void fdbcs_batch_destroy(fdbcs_batch* b);
/* ConflictBatch::addTransaction(tr) — SkipList.cpp:763-794.  Keys are copied. */
int fdbcs_batch_add_transaction(fdbcs_batch* b, int64_t read_snapshot, int report_conflicting_keys,
                                int32_t n_reads, const uint8_t* const* read_begin,
                                const int32_t* read_begin_len, const uint8_t* const* read_end,
                                const int32_t* read_end_len, int32_t n_writes,
                                const uint8_t* const* write_begin, const int32_t* write_begin_len,
                                const uint8_t* const* write_end, const int32_t* write_end_len);
/* addTransaction for every transaction of a packed batch, in order. */
int fdbcs_batch_add_packed(fdbcs_batch* b, const fdbcs_packed_batch* pb);
/* Stage the batch in HBM now (async H2D on the engine stream).  Optional:
 * detect uploads implicitly.  Lets callers keep PCIe out of a timed region. */
int fdbcs_batch_upload(fdbcs_batch* b);
/* Block until every stream of the conflict set is idle: uploads issued by fdbcs_batch_upload,
 * and every stage of every batch already submitted.  The engine's HIP runtime is not torch's
 * (INTEGRATION.md), so a caller timing HBM-resident batches calls this before starting its
 * clock.  No reference counterpart (the reference is synchronous, Resolver.actor.cpp:179-194). */
int fdbcs_sync(fdbcs_conflict_set* cs);
/* ConflictBatch::detectConflicts(now, newOldestVersion, nonConflicting, tooOld)
 * — SkipList.cpp:844-890.  verdicts[t] receives 0/1/2 per transaction
 * (Resolver.actor.cpp:196-204 encoding); counts are optional (NULL). */
int fdbcs_batch_detect_conflicts(fdbcs_batch* b, int64_t now, int64_t new_oldest_version,
                                 uint8_t* verdicts, int32_t* n_committed, int32_t* n_too_old);
/* Asynchronous form: enqueue the pipeline, return immediately; the verdicts of
 * the batch are fetched with fdbcs_batch_wait.  Batches must be waited in
 * submission order before the set is used for anything else. */
int fdbcs_batch_detect_async(fdbcs_batch* b, int64_t now, int64_t new_oldest_version);
int fdbcs_batch_wait(fdbcs_batch* b, uint8_t* verdicts, int32_t* n_committed, int32_t* n_too_old);
/* conflictingKeyRangeMap[txn] (SkipList.cpp:641-645, 822-825): read-range
 * indices (indexInTx) that conflicted, ascending.  Valid after detect.  On a routed batch
 * (fdbcs_batch_add_routed, created with report_keys) txn is the sub-transaction and the indices
 * are its own, as this resolver's map holds them. */
int fdbcs_batch_conflicting_reads(fdbcs_batch* b, int32_t txn, int32_t* idx_out, int32_t cap,
                                  int32_t* n_out);
/* ConflictBatch::GetTooOldTransactions (SkipList.cpp:836-842): indices of the transactions added
 * so far whose add-time TooOld test held (read_snapshot < oldestVersion with at least one read,
 * SkipList.cpp:770), ascending; valid right after the adds, before detect, as in the reference.
 * Writes at most cap indices (idx_out may be NULL to count).  A routed batch
 * (fdbcs_batch_add_routed) or a device-added one (fdbcs_batch_add_packed_device) is judged at
 * detect on the device: FDBCS_E_STATE (read its verdict bytes instead). */
int fdbcs_batch_too_old(fdbcs_batch* b, int32_t* idx_out, int32_t cap, int32_t* n_out);
/* Device pointer to the batch's per-transaction verdict bytes (valid after
 * detect until the batch is destroyed) for on-device combine (RCCL). */
int fdbcs_batch_device_verdicts(fdbcs_batch* b, void** dptr);

/* On-device combine for key-range sharded resolvers (one per GPU).  Call after the batch's
 * transactions are added and before detect: txn_ids[t] in [0, n_global) is the global index (in
 * the proxy's batch) of the batch's transaction t.  Detect then also writes dev_out[0, n_global)
 * (device memory of this GPU, any allocator) with the conflict byte 2 - verdict of each routed
 * transaction and 0 elsewhere, complete when the batch is (fdbcs_batch_wait returns).  An
 * element-wise MAX all-reduce of dev_out over the resolvers holds 2 - min(verdict), the proxy's
 * combine (CommitProxyServer.actor.cpp:764-780). */
int fdbcs_batch_set_conflict_output(fdbcs_batch* b, const int32_t* txn_ids, int32_t n_global, uint8_t* dev_out);

/* Multi-resolver routing on the device: the commit proxy's split of a batch across resolvers
 * (CommitProxyServer.actor.cpp:118-187 with a static keyResolvers map; fdbrpc/RangeMap.h:126-129).
 * Each GPU is the proxy of one share of the global batch and the resolver of one key range.
 *   fdbcs_share_bytes / fdbcs_share_pack: the share in the engine's wire layout (host memory; no
 *     TooOld test, which stays with the resolvers).  The shares of all ranks are then gathered
 *     into one device buffer, `stride` bytes apart in rank order (an RCCL all-gather).
 *   fdbcs_batch_add_routed: on a new batch (the addTransaction step, SkipList.cpp:763-794): once
 *     the device word *ready_flag equals ready_value (the caller's stream sets it after the
 *     all-gather; NULL: the shares are already complete), the engine keeps, on the
 *     device, every range of the gathered shares that meets [lo_key, hi_key) (lo_len < 0: no lower
 *     bound, hi_len < 0: none above), unclipped, reads and writes alike; a transaction gets a
 *     sub-transaction iff one of its ranges is kept (:107-116), its snapshot copied.  Its TooOld
 *     test (SkipList.cpp:770) is made when the batch is detected, against the oldest version every
 *     earlier detect of this set left: the value addTransaction sees in the Resolver's order
 *     (Resolver.actor.cpp:139-150, 179-194), whether the routing was issued before or after the
 *     previous batch's detect.  Sub-transactions keep the global order.  cap_*: bounds on the
 *     routed batch, TooOld sub-transactions' ranges included (FDBCS_E_NOMEM at detect if passed).
 *     conflict_out (optional, n_global bytes of device memory, n_global = the transactions of all
 *     shares, FDBCS_E_INVALID at detect otherwise): as fdbcs_batch_set_conflict_output, with the
 *     global index of a sub-transaction = its position in the concatenated shares.  A batch
 *     created with report_keys copies each share's report flag to its sub-transaction (:181-186);
 *     after detect, fdbcs_batch_conflicting_reads returns the sub-transaction's own indexInTx (what
 *     this resolver's conflictingKeyRangeMap holds; the read-id view below maps it back to the
 *     transaction's index), fdbcs_batch_report_entries which sub-transactions have a map entry, and
 *     fdbcs_batch_set_report_output makes detect write the reports as device bytes.  A batch
 *     created without report_keys collects none and pays nothing.  Detect and wait as for any batch; detect
 *     blocks until the routing kernels have run (issue the next batch's routing first).  The wait
 *     for the ready flag is bounded by FDBCS_ROUTE_TIMEOUT_MS (default 60000): past it detect
 *     returns FDBCS_E_TIMEOUT and the batch is empty again, to be routed anew.  The capacity
 *     (FDBCS_E_NOMEM) and n_global (FDBCS_E_INVALID) errors leave it empty the same way.
 *   fdbcs_batch_routed_info: the routed batch's sizes and device views of its global -> batch
 *     transaction map (int32[n_shares * max_share_txns], -1 where not routed) and of each kept
 *     read's index in its transaction (txReadConflictRangeIndexMap, :144-165). */
int fdbcs_share_bytes(const fdbcs_packed_batch* pb, int64_t* bytes);
int fdbcs_share_pack(const fdbcs_packed_batch* pb, void* out, int64_t cap, int64_t* used);
int fdbcs_batch_add_routed(fdbcs_batch* b, const void* shares, int64_t stride, int32_t n_shares, int32_t max_share_txns,
                           const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key, int32_t hi_len,
                           int32_t cap_txns, int32_t cap_reads, int32_t cap_writes, int64_t cap_tail,
                           uint8_t* conflict_out, int64_t n_global, const uint32_t* ready_flag,
                           uint32_t ready_value);
int fdbcs_batch_routed_info(fdbcs_batch* b, int32_t* n_txn, int32_t* n_reads, int32_t* n_writes, void** inv_dev,
                            void** read_ids_dev);

/* Device routing under a keyResolvers map with its ownership history (ProxyCommitData::keyResolvers,
 * CommitProxyServer.actor.cpp:147-174, 622-626): a key range may move between resolvers while the
 * batches are routed on the GPUs.  The map has n_ranges ranges [bound m, bound m+1): bound m is
 * bound_bytes[bound_offsets[m], bound_offsets[m+1]), bound 0 is the empty key and the last range is
 * unbounded.  Range m's history is entries [hist_offsets[m], hist_offsets[m+1]) of hist_versions /
 * hist_resolvers, oldest first.  A conflict range [b, e) meets the ranges m0 = rangeContaining(b)
 * to m1 = max(m0, the last m with bound m < e) (an empty range: rangeContaining(b)).  A write goes
 * to resolver g iff g is the newest owner of one of them; a read at snapshot s iff, for one of them,
 * walking its history from the newest entry and stopping after the first entry whose version is
 * < s, g is met.
 * A map is invalid (FDBCS_E_INVALID) with n_ranges < 1 or > 65536, a non-empty first bound, bounds
 * not strictly ascending, a range without a history entry, versions decreasing within a range, or
 * a negative resolver id (the argument or an entry). */
typedef struct fdbcs_key_resolvers {
    int32_t n_ranges;
    const uint8_t* bound_bytes;
    const int64_t* bound_offsets; /* [n_ranges + 1] */
    const int64_t* hist_offsets;  /* [n_ranges + 1] */
    const int64_t* hist_versions;
    const int32_t* hist_resolvers;
} fdbcs_key_resolvers;
/* Host only (no device needed, like fdbcs_share_pack): checks the map and writes what the routing
 * kernel reads of it for one resolver.  own_out[m] bit 0: the resolver is range m's newest owner;
 * bit 1: it appears in an older entry.  until_out[m]: the largest version of an entry that follows
 * one of its older entries (INT64_MIN without bit 1).  A read at snapshot s is kept iff some range
 * it meets has bit 0, or bit 1 and until >= s; a write iff some range it meets has bit 0. */
int fdbcs_route_map_pack(const fdbcs_key_resolvers* map, int32_t resolver, uint8_t* own_out, int64_t* until_out);
/* fdbcs_batch_add_routed with the key range [lo_key, hi_key) replaced by (map, resolver): the same
 * states, capacities, conflict_out, ready flag and error codes, and the same calls afterwards
 * (fdbcs_batch_routed_info, fdbcs_batch_set_report_output, fdbcs_batch_conflicting_reads,
 * fdbcs_batch_report_entries).  An invalid map is FDBCS_E_INVALID at the call and leaves the batch
 * untouched.  The map is read during the call and travels with the batch: its derived form is
 * copied to device memory of the batch ahead of the routing kernels, so every batch may pass a
 * different map at no extra synchronisation, and batches in flight keep the map they were routed
 * under. */
int fdbcs_batch_add_routed_map(fdbcs_batch* b, const void* shares, int64_t stride, int32_t n_shares,
                               int32_t max_share_txns, const fdbcs_key_resolvers* map, int32_t resolver,
                               int32_t cap_txns, int32_t cap_reads, int32_t cap_writes, int64_t cap_tail,
                               uint8_t* conflict_out, int64_t n_global, const uint32_t* ready_flag,
                               uint32_t ready_value);
/* Routed batches only, after fdbcs_batch_add_routed and before detect.  Detect then also writes
 * dev_out[0, n_global_reads) (device memory of this GPU, any allocator): 1 at the global read
 * index of every read this resolver's conflictingKeyRangeMap would hold (every conflicting read
 * of a history conflict, SkipList.cpp:641-645; the first of an intra-batch conflict, :821-828)
 * for a reporting sub-transaction whose verdict here is Conflict, 0 everywhere else, complete
 * when the batch is.  The global read index of read j of share p is its position among the reads
 * of the concatenated shares, sum of the earlier shares' reads + j.  An element-wise MAX
 * all-reduce over the resolvers is the set of the proxy's conflictingKRIndices
 * (CommitProxyServer.actor.cpp:1243-1261): the proxy's list holds an index twice when a read spans
 * a split key and both owners report it; the bytes are the sorted set of that list.  A resolver
 * writes ones only for sub-transactions it judged Conflict, so after the MAX a transaction has
 * ones iff some resolver conflicted, which is when the proxy reports it.
 * FDBCS_E_STATE on a batch that is not routed, was created without report_keys, or has been
 * detected; FDBCS_E_INVALID for a NULL handle or pointer or a negative size.  n_global_reads
 * differing from the reads of all shares is found at detect: FDBCS_E_INVALID, and the batch is
 * empty again, to be routed anew. */
int fdbcs_batch_set_report_output(fdbcs_batch* b, uint8_t* dev_out, int64_t n_global_reads);
/* Valid after detect, for any batch: entry_out[t] = 1 iff the reference would have created
 * conflictingKeyRangeMap[t] (report flag set, at least one read range, not TooOld:
 * SkipList.cpp:770-784), for the first min(cap, transactions) transactions.  A routed batch's
 * caller never saw its sub-transactions and learns the map's keys here. */
int fdbcs_batch_report_entries(fdbcs_batch* b, uint8_t* entry_out, int32_t cap);

/* The resolver's iops sample (Resolver.actor.cpp:178-192) of a routed batch, taken on the device:
 * what the master's resolutionBalancing asks a resolver for (ResolutionMetricsRequest /
 * ResolutionSplitRequest, :318-342) is fed by the begin key of every range of every transaction
 * the resolver was sent, which for a routed batch only the device holds.  The begin key of range i
 * of the routed batch (read r: i = r, write w: i = n_reads + w, the order of
 * fdbcs_batch_routed_info's views; TooOld sub-transactions' ranges included, the roll does not
 * depend on the verdicts) has metric = 100 + its length (SAMPLE_OFFSET_PER_KEY) and is sampled by
 * TransientStorageMetricSample::add's rule (StorageMetrics.actor.h) under a counter-based roll:
 *   z = seed + 0x9E3779B97F4A7C15 * (i + 1)                      (mod 2^64)
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   z = z ^ (z >> 31);  u = z >> 32
 *   sampled = metric >= units  or  u * units < (metric << 32)    (unsigned 64-bit)
 *   value   = metric if metric >= units else units               (what addMetric is given)
 * All integer: a host restatement gives the same sample bit for bit.
 *   fdbcs_batch_set_iops_sample: after fdbcs_batch_add_routed / _map and before detect; enqueues
 *     the sample behind the routing, off the detect pipeline's path (detect does not wait for it).
 *     units = metricUnitsPerSample (KEY_BYTES_PER_SAMPLE, 20000 in the reference).  FDBCS_E_STATE on
 *     a batch that is not routed or is already detected, FDBCS_E_INVALID for a NULL handle or
 *     units < 1, FDBCS_E_NOMEM when 16 * (cap_reads + cap_writes) + cap_tail of the routing call
 *     could pass 2^32 bytes of keys.  A second call before detect replaces the request.  A batch
 *     that never asks launches and allocates nothing.
 *   fdbcs_batch_iops_sample: blocks until the routing and the sample have run (it neither needs
 *     nor waits for detect) and returns the sampled ranges and their key bytes.  A routing error
 *     comes first (FDBCS_E_TIMEOUT / NOMEM / INVALID as from fdbcs_batch_routed_info: the batch is
 *     empty again and the request is dropped with it); FDBCS_E_STATE when no sample was requested.
 *   fdbcs_batch_iops_sample_read: the sampled keys in ascending i, in the layout of
 *     fdbcs_history_export_read (key_offsets[n + 1]), metrics[n] the values above, index[n] (may be
 *     NULL) the ranges i.  FDBCS_E_NOMEM when a capacity is too small (the result stays
 *     available); the result can be read any number of times until the batch is destroyed.
 *   fdbcs_batch_iops_sample_timing: device time of the sample's kernels (valid once
 *     fdbcs_batch_iops_sample returned). */
int fdbcs_batch_set_iops_sample(fdbcs_batch* b, int32_t units, uint64_t seed);
int fdbcs_batch_iops_sample(fdbcs_batch* b, int64_t* n_out, int64_t* key_bytes_out);
int fdbcs_batch_iops_sample_read(fdbcs_batch* b, uint8_t* key_bytes, int64_t key_bytes_cap, int64_t* key_offsets,
                                 int32_t* metrics, int32_t* index /* may be NULL */, int64_t cap);
int fdbcs_batch_iops_sample_timing(fdbcs_batch* b, double* ms_kernels);

/* A whole batch from device memory, normalized on the GPU.  The six arrays of fdbcs_packed_batch,
 * same meaning and layout, in DEVICE memory of the set's GPU (any allocator), with the sizes the
 * host knows anyway (they are message sizes): T = n_txn, R = n_reads, W = n_writes and the bytes of
 * key_bytes.  key_bytes may start at any byte and needs no slack after its last byte;
 * report_conflicting_keys may be NULL (= all false). */
typedef struct fdbcs_packed_batch_dev {
    int32_t n_txn, n_reads, n_writes;
    int64_t key_bytes_len;
    const int64_t* read_snapshot;           /* [n_txn] */
    const uint8_t* report_conflicting_keys; /* [n_txn] or NULL */
    const int32_t* read_offsets;            /* [n_txn+1] */
    const int32_t* write_offsets;           /* [n_txn+1] */
    const uint8_t* key_bytes;               /* [key_bytes_len] */
    const int64_t* key_offsets;             /* [2*(R+W)+1] */
} fdbcs_packed_batch_dev;
/* fdbcs_batch_add_packed_device: on a new, empty batch, addTransaction (SkipList.cpp:763-794) of
 *     every transaction of the arrays, in order.  FDBCS_E_STATE on a batch that holds anything, is
 *     routed or is detected, and from every add call made after it on the same batch; n_txn == 0 is
 *     FDBCS_OK and the batch stays empty.  The host does no work per transaction, range or key and
 *     reads none of the arrays: it sizes the batch's buffers from T, R, W and key_bytes_len,
 *     enqueues the add kernels and returns.  They run once the device word *ready_flag equals
 *     ready_value (as for fdbcs_batch_add_routed; NULL: the arrays are complete), on the stream the
 *     routing kernels use, off the detect pipeline's chains; the wait is bounded by
 *     FDBCS_ROUTE_TIMEOUT_MS (FDBCS_E_TIMEOUT past it).  The arrays must stay unchanged until
 *     fdbcs_batch_device_add_info or detect has returned (both block until the add kernels have
 *     run); after that they may be reused: keys are copied.
 *     Every range is kept, in input order: read r of the arrays is the batch's read r, write w its
 *     write w.  The TooOld test (SkipList.cpp:770) is made when the batch is detected, by the routed
 *     batch's rule, against the oldest version every earlier detect of the set left: the value
 *     addTransaction sees in the Resolver's order (Resolver.actor.cpp:139-150, 179-194).  A TooOld
 *     transaction keeps its ranges, which are inert.  This differs from fdbcs_batch_add_packed,
 *     which tests at the call, only for a batch added ahead of an earlier batch's detect;
 *     fdbcs_batch_too_old is FDBCS_E_STATE (read the verdict bytes), as for a routed batch.
 *     Refused by the host before anything is enqueued: FDBCS_E_INVALID for a NULL pointer where a
 *     size says the array is read, a negative size or n_txn over the engine's batch limit (49152);
 *     FDBCS_E_NOMEM for key_bytes_len >= 2^32, R + W >= 2^28 or a capacity failure.  Everything else
 *     is validated on the device: read_offsets[0] == write_offsets[0] == 0, both non-decreasing,
 *     read_offsets[T] == n_reads, write_offsets[T] == n_writes, key_offsets non-decreasing inside
 *     [0, key_bytes_len], and no inverted range (FDBTypes.h:288-291) in the full byte order, tails
 *     and the ranges of TooOld transactions included.  No address is formed from a value of the
 *     arrays before it is checked.  A violation surfaces as FDBCS_E_INVALID from
 *     fdbcs_batch_device_add_info or detect; the batch is then empty again and can be added anew,
 *     and the set is exactly as before.
 *     Afterwards fdbcs_batch_set_conflict_output (with its host txn_ids), sync and async detect,
 *     fdbcs_batch_conflicting_reads, fdbcs_batch_report_entries and fdbcs_batch_device_verdicts work
 *     as after fdbcs_batch_add_packed (the report flags count only on a batch created with
 *     report_keys), and fdbcs_batch_upload is a no-op.  fdbcs_batch_routed_info,
 *     fdbcs_batch_set_report_output and fdbcs_batch_set_iops_sample stay with routed batches:
 *     FDBCS_E_STATE.  Host-mapped pinned input pointers are not supported.
 *   fdbcs_batch_device_add_info: blocks until the add kernels have run; their error, or the batch's
 *     sizes and the bytes its key tails take (each padded to 8).  Outputs may be NULL.
 *     FDBCS_E_STATE on a batch that is not device-added.
 *   fdbcs_batch_device_add_timing: device time of the add kernels and host time inside the add call
 *     (ms), valid once fdbcs_batch_device_add_info or detect returned FDBCS_OK. */
int fdbcs_batch_add_packed_device(fdbcs_batch* b, const fdbcs_packed_batch_dev* pb, const uint32_t* ready_flag,
                                  uint32_t ready_value);
int fdbcs_batch_device_add_info(fdbcs_batch* b, int32_t* n_txn, int32_t* n_reads, int32_t* n_writes,
                                int64_t* tail_bytes);
int fdbcs_batch_device_add_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host);

/* A proxy's share packed on the GPU from device-resident arrays: fdbcs_share_pack's output, byte
 * for byte, written by kernels straight into the caller's gather buffer, so a rank whose batch
 * arrived in device memory (fdbcs_packed_batch_dev) routes it without the host reading a key.
 *   fdbcs_share_bytes_bound: host only (no device needed, like fdbcs_share_bytes).  The size of the
 *     wire layout of a share of T transactions, R reads and W writes whose key tails take
 *     key_bytes_len bytes: at least fdbcs_share_bytes of every valid batch of those sizes (a key's
 *     tail is shorter than the key), and what a caller that holds only device arrays sizes its
 *     all-gather stride with (the exact size needs key_offsets).  (0, 0, 0, 0) gives the empty
 *     share's 320 bytes.  FDBCS_E_INVALID for a negative size or a NULL `bytes`.
 *   fdbcs_batch_share_pack_device: on a new, empty batch of the set whose GPU holds the arrays and
 *     out_dev.  FDBCS_E_STATE on a batch that holds anything, is routed, device-added or detected, or
 *     whose previous pack has not been waited for.  The host reads none of the arrays and does no
 *     work per transaction, range or key: it enqueues the pack kernels on the stream the routing
 *     kernels use (off the detect pipeline's chains) and returns.  They run once the device word
 *     *ready_flag equals ready_value (NULL: the arrays are complete), the wait bounded by
 *     FDBCS_ROUTE_TIMEOUT_MS, exactly as for fdbcs_batch_add_packed_device.  out_dev: device memory
 *     of the set's GPU (any allocator), 64-byte aligned, cap bytes.  The batch stays empty and the
 *     set is never touched.  The only calls accepted on the batch afterwards are
 *     fdbcs_batch_share_pack_info / _timing, fdbcs_batch_add_routed / _add_routed_map (they first
 *     block for a pending pack and return its error if it had one, routing nothing; an error that
 *     fdbcs_batch_share_pack_info has already returned is not returned again by them: the buffer
 *     then holds the empty share, and they route what the gather buffer holds.  The typical use
 *     packs the rank's share into its slot of the gather buffer, all-gathers after _info and
 *     routes with the same handle), a further pack once _info has returned, and destroy; every other add is
 *     FDBCS_E_STATE.
 *     Refused by the host before anything is enqueued or written: FDBCS_E_INVALID for the NULL and
 *     negative-size cases of the device add, n_txn over the batch limit (49152), out_dev NULL or
 *     not 64-byte aligned; FDBCS_E_NOMEM for key_bytes_len >= 2^32, R + W >= 2^28, or cap below the
 *     layout of (T, R, W) without tails (fdbcs_share_bytes_bound(T, R, W, 0); never below the empty
 *     share's 320 bytes).  n_txn == 0 is FDBCS_OK and packs the empty share (no array is read).
 *     Validated on the device, as by the device add: read_offsets[0] == write_offsets[0] == 0, both
 *     non-decreasing, read_offsets[T] == n_reads, write_offsets[T] == n_writes, key_offsets
 *     non-decreasing inside [0, key_bytes_len], no inverted range in the full byte order (tails
 *     included); no address is formed from a value of the arrays before it is checked.  The exact
 *     size is checked there too: the layout for the tail total the kernels found must fit cap.
 *     On success out_dev[0, bytes) equals what fdbcs_share_pack writes into a zeroed buffer for the
 *     same batch: the header (pads zero), the endpoint records (tail = the byte offset in the
 *     share's tail region; tails byte-packed in key order, not padded), snapshots, offsets, the
 *     report flags (zeros for a NULL array; copied whether or not the batch was created with
 *     report_keys), owners, the tail bytes and 64 zero bytes after them; every alignment gap is
 *     zero.  [bytes, cap) is unspecified, and nothing outside [out_dev, out_dev + cap) is written.
 *     On any error found by the kernels nothing but out_dev[0, 320) is written, and it holds the
 *     empty share (T = R = W = 0, bytes = 320): a gather buffer is always well formed, and a failed
 *     pack routes as no transactions.
 *   fdbcs_batch_share_pack_info: blocks until the pack kernels have run.  The header's bytes, T, R,
 *     W and tail_bytes (outputs may be NULL), or FDBCS_E_INVALID for a violation, FDBCS_E_NOMEM when
 *     the exact size passes cap, FDBCS_E_TIMEOUT for a ready flag never set; the same status again
 *     on every later call until the next pack.  The arrays may be reused once it has returned.
 *     FDBCS_E_STATE on a batch that never packed.
 *   fdbcs_batch_share_pack_timing: device time of the pack kernels and host time inside the pack
 *     call (ms), valid once the pack has been waited for.
 * Not provided: a device-side completion signal for the caller's stream (the handshake is the
 * blocking _info, as for fdbcs_batch_device_add_info), and host-mapped pinned input pointers. */
int fdbcs_share_bytes_bound(int32_t n_txn, int32_t n_reads, int32_t n_writes, int64_t key_bytes_len, int64_t* bytes);
int fdbcs_batch_share_pack_device(fdbcs_batch* b, const fdbcs_packed_batch_dev* pb, void* out_dev, int64_t cap,
                                  const uint32_t* ready_flag, uint32_t ready_value);
int fdbcs_batch_share_pack_info(fdbcs_batch* b, int64_t* bytes, int32_t* n_txn, int32_t* n_reads, int32_t* n_writes,
                                int64_t* tail_bytes);
int fdbcs_batch_share_pack_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host);

/* The history version each read of a batch is checked against, computed on the device against an
 * idle set; neither the set nor the batch's outcome is modified.  No reference counterpart (the
 * reference's CheckMax answers only "above the snapshot or not").
 * With H(k) the version a read of key k sees and a floor f, H_f is exactly the export's clamp:
 *   H_f(k) = H(k) if H(k) >= f, otherwise f - 1;  f = INT64_MIN: no clamp.
 * For read r of the batch, with range [b, e), the result V_r is
 *   b <  e:  V_r = max { H_f(k) : b <= k < e }: the segment containing b (the header if no
 *            boundary is <= b) and every boundary inside (b, e); a boundary at e does not count.
 *   b == e:  V_r = H_f just below b: the version of the greatest boundary < b, or the set's header
 *            if there is none.  The empty key and a b equal to the first boundary both give the
 *            header.  This is the reference's finger rule for empty reads (SkipList.cpp:650-666),
 *            the rule the read check follows.
 * Across the tiers V is the greater of the base tier's value and the delta tier's (a hole is
 * INT64_MIN, and the delta has no header): a delta version that is not a hole is at least every base
 * version it covers, which the two-tier read check already rests on.  Consequences:
 *   1. At f <= the oldest version, a read that is not TooOld conflicts with the history iff
 *      V_r > its snapshot.
 *   2. At f = the oldest version the result does not depend on how the history is split between the
 *      tiers, on when compaction or GC ran, or on which GPU or process holds the set.
 * Snapshots, TooOld, report flags and the batch's writes play no part.
 *
 * The batch: one that is being added or is uploaded (a batch still being added is uploaded, as by
 * fdbcs_batch_upload), built by fdbcs_batch_add_transaction, fdbcs_batch_add_packed or
 * fdbcs_batch_add_packed_device; for a device-added batch the call first waits for its add kernels,
 * and a malformed one gives FDBCS_E_INVALID and is left as a failed detect leaves it (empty again).
 * Entry r of the output is V_r, in the order of the reads the batch holds (R of them): a
 * transaction that was TooOld when the host added it carries no ranges (SkipList.cpp:770-790), so
 * its reads are not held and have no entry; a device-added batch is judged at detect and holds
 * them all.  A batch without reads writes nothing and is FDBCS_OK.  Both forms are complete when the call returns; the device form (dev_out: device
 * memory of the set's GPU) copies nothing to the host but its error word.  The host form's result
 * passes through a grow-only buffer owned by the set.
 * The batch stays an uploaded, undetected batch: a later detect gives exactly the verdicts and
 * conflicting reads it would have given without the query, nothing the pipeline expects zeroed is
 * dirtied, and a pending export result of the set stays pending and readable.
 * FDBCS_E_STATE: batches are in flight on the set; the batch is submitted or done; it was routed or
 * packed a share; its set is gone.  FDBCS_E_NOMEM: cap < R, or the result buffer cannot grow.
 * FDBCS_E_INVALID: a NULL handle, or a NULL output with R > 0.
 * fdbcs_batch_read_versions_timing: device time of the last query's kernel on the batch's set and
 * host time of the whole call (ms).  Every query's launch also counts in fdbcs_kernel_profile of the
 * set under its kernel's name, k_read_versions<false> or, for a batch with a key over 24 bytes (the
 * read check's rule for its long-key lookups), k_read_versions<true>. */
int fdbcs_batch_read_versions(fdbcs_batch* b, int64_t floor_version, int64_t* versions_out, int64_t cap); /* host [R] */
int fdbcs_batch_read_versions_device(fdbcs_batch* b, int64_t floor_version, int64_t* dev_out, int64_t cap);
int fdbcs_batch_read_versions_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host);

/* Diagnostics (tuning, not part of the ConflictSet contract): average device time of one launch
 * of a pipeline kernel over `reps` back-to-back launches on the uploaded batch `b` against the
 * current history, with no batch in flight.  which: 0 = the read check (D.CheckRead); 1-2 = the
 * endpoint sort's kernels (partition, per-bucket sort; splitters of the last batch detected); 3-4 =
 * the split check's base / delta tier launch alone. */
int fdbcs_debug_kernel_time(fdbcs_batch* b, int which, int reps, double* us_per_launch);
/* Per-kernel device time accumulated since fdbcs_reset_stats: timing level 3 brackets every kernel
 * of every batch with events, level 1 the kernel named by fdbcs_set_timed_kernel on the sampled
 * batches, and the kernel of every fdbcs_batch_read_versions call at any level.  Entry `index` (0-based; FDBCS_E_INVALID past the last): demangled kernel name (without
 * namespace and parameters) into name[cap], its timed launches and their total milliseconds. */
int fdbcs_kernel_profile(fdbcs_conflict_set* cs, int32_t index, char* name, int32_t cap, int64_t* launches,
                         double* ms);
/* The kernel timed at level 1 (a name fdbcs_kernel_profile reported; NULL or "" = none). */
int fdbcs_set_timed_kernel(fdbcs_conflict_set* cs, const char* name);
/* Diagnostics: on != 0 queues a bounded hold kernel on every stream of the set, so batches
 * submitted next wait behind it; on == 0 releases them, and they run back to back at the device's
 * own rate (the device-bound throughput, free of the submitting thread). */
int fdbcs_debug_hold(fdbcs_conflict_set* cs, int32_t on);
/* Diagnostics: what the engine holds of the HIP runtime right now, over every set and batch of the
 * process: device allocations, pinned host allocations, events and streams.  Each count goes up
 * where the runtime handed one out and down where it took one back, so the four are back at their
 * earlier values once the sets and batches created since are destroyed (a leak check for tests).
 * Needs no device and no set; FDBCS_E_INVALID on a NULL pointer. */
int fdbcs_debug_live_resources(int64_t* device_buffers, int64_t* host_buffers, int64_t* events, int64_t* streams);

const char* fdbcs_strerror(int status);

#ifdef __cplusplus
}
#endif
#endif /* FDB_CONFLICT_SET_H */
