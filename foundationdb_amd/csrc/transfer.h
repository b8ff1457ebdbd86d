// transfer.h — internal interface between the maintenance entry points (transfer.cpp) and their
// gfx950 kernels (transfer.hip): history export, the history digests, split keys, the two history
// imports, the resolver's iops sample and the read versions of a batch.  Not part of the public
// C-ABI; the detect pipeline's interface is engine.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

namespace fdbcs {

// ---- canonical history export (fdbcs_history_export): reads both tiers, writes only the arrays below.
// Device words of one export (zeroed before its launches).
enum ExportWord { kXwLo, kXwHi, kXwHeader, kXwN, kXwBytes, kXwScan /* int counter, int error */, kXwWords = 8 };
struct ExportArgs {
    Hist base, delta;
    const uint8_t* htail;
    int64_t nb, nd;        // exact tier sizes (the set is idle)
    int64_t hdr;           // the set's header version
    int64_t floor;         // versions below it read floor - 1 (kHole: no clamp)
    int32_t has_lo, has_hi;  // export (lo, hi) of the merged stream, header H(lo)
    DKey lo, hi;
    const uint8_t* btail;  // their tails
    // scratch, one entry per delta boundary j: its position in the merged stream of both tiers' boundaries
    // (j + base boundaries below it: on equal keys the delta's comes first) and the version at its key
    int64_t* d_pos;
    int64_t* d_val;
    int64_t* words;        // [kXwWords] ExportWord
    int64_t* tile_tb;      // [export_tiles] delta boundaries below each scan tile's first element
    // result: the layout fdbcs_load_history takes
    int64_t* versions;     // [n]
    int64_t* offsets;      // [n + 1]
    uint8_t* bytes;
    int64_t bytes_cap;     // bytes the key buffer holds
};
// Tiles (scan granule triples) of an export over nb + nd boundaries.
int64_t export_tiles(int64_t n);
// mode: the compaction search's (1: lane_lower_bound, 2: the long-key form).
void launch_export(hipStream_t s, const ExportArgs& a, const MaxLevels& basem, uint64_t* granules, int mode);

// ---- history digest (fdbcs_history_digest): the export's searches, then one pass that hashes the
// kept boundaries where they lie.  Takes an ExportArgs whose result pointers (versions, offsets,
// bytes) are unused; its word block is the digest's own, zeroed before the launches: the export's
// kXwLo, kXwHi and kXwHeader, kXwN and kXwBytes as sums over the kept boundaries, the error word of
// kXwScan (bit 4 only: there is no scan) and the two lanes' sums below.
enum DigestWord { kDwSum0 = 6, kDwSum1 = 7 };
static_assert((int)kDwSum1 < (int)kXwWords && (int)kDwSum0 > (int)kXwScan, "the digest's sums lie in the export's spare words");
void launch_export_digest(hipStream_t s, const ExportArgs& a, const MaxLevels& basem, int mode);

// ---- partitioned digest (fdbcs_history_digest_ranges): K ranges between ascending bounds in one pass
// over the span they cover.  Edge e of the partition is a bound, or with an open end "below every
// key" (edge 0) or "past every key" (edge K); range i lies between edges i and i + 1.  The ExportArgs
// are the digest's, with lo / hi the first / last bound (absent at an open end); of its words only
// kXwLo, kXwHi, kXwHeader and the error word are used.
enum DigestRangeWord { kDrN, kDrBytes, kDrHeader, kDrSum0, kDrSum1, kDrWords };
struct DigestRangesArgs {
    int32_t n_bounds, open_lo, open_hi;
    int64_t K;               // ranges: n_bounds - 1 + open_lo + open_hi
    const uint8_t* bytes;    // the bounds' bytes as given (8-byte aligned, kTailSlack readable bytes past them)
    const int64_t* offsets;  // [n_bounds + 1]
    int64_t* lt;             // [K + 1] per edge: stream elements below it
    int64_t* le;             // [K + 1] per edge: stream elements at or below it
    int64_t* out;            // [K][kDrWords], zeroed before the launches
};
// k_digest_ranges_bounds, the export's first three launches, k_export_digest_ranges.
void launch_export_digest_ranges(hipStream_t s, const ExportArgs& a, const DigestRangesArgs& r, const MaxLevels& basem,
                                 int mode);

// ---- split keys (fdbcs_history_split_keys): boundary keys of one tier at evenly spaced positions
// inside (lo, hi).  Reads both tiers, writes only the arrays below.
enum SplitWord { kSwN, kSwBytes, kSwTier, kSwFirst, kSwCount, kSwError /* int */, kSwWords = 8 };
struct SplitArgs {
    Hist base, delta;
    const uint8_t* htail;
    int64_t nb, nd;
    int32_t has_lo, has_hi;
    DKey lo, hi;
    const uint8_t* btail;  // their tails
    int64_t want;          // keys asked for
    int64_t* words;        // [kSwWords] SplitWord, zeroed before the launches
    int64_t* offsets;      // [want + 1]
    uint8_t* bytes;        // sized by the host from kSwBytes, between the two launches
    int64_t bytes_cap;
};
void launch_split_plan(hipStream_t s, const SplitArgs& a);
void launch_split_gather(hipStream_t s, const SplitArgs& a, int64_t n);

// ---- history import (fdbcs_history_import / fdbcs_history_import_pending): folds an exported range
// into both tiers, H'(k) = max(H(k), I(k)) over [lo, hi).  Reads the current buffers, writes only
// scratch and the non-current base buffer and tail arena; the host switches to them on success.
// Device words of one import (zeroed before its launches).
enum ImportWord {
    kIwError,      // int: 1 invalid input, 4 a merged position out of range, 8 a capacity bound
    kIwJlo,        // imported boundaries <= lo
    kIwM,          // overlay boundaries: lo, the imported ones inside (lo, hi), hi
    kIwKept,       // boundaries of the new base
    kIwTailUnits,  // 8-byte units used in the new tail arena
    kIwMaxVer,     // greatest version of the new base (k_import_max, after its levels are rebuilt)
    kIwScan,       // int counter, int error of the fold's scan
    kIwWords = 8
};
struct ImportArgs {
    Hist base, delta;      // the receiving set's tiers
    const uint8_t* htail;  // their tail arena
    int64_t nb, nd;        // exact tier sizes (the set is idle)
    int64_t hdr;           // the set's header version
    // the imported arrays, on the device, in the layout fdbcs_load_history takes
    int64_t n;
    const uint8_t* bytes;  // 8-byte aligned, >= 16 readable bytes past nbytes
    int64_t nbytes;
    const int64_t* offsets;
    const int64_t* versions;
    int64_t ihdr;
    int32_t has_lo, has_hi;
    int32_t lo_len, hi_len;
    const uint8_t* bnd;    // lo's bytes at 0, hi's at bnd_hi (8-byte aligned, >= 16 readable bytes past each)
    int64_t bnd_hi;
    // the overlay: a third stream shaped like the delta tier (kHole outside [lo, hi), I inside)
    Hist ov;
    uint8_t* otail;        // its tails: imported boundary j at unit (offsets[j] >> 3) + j, then lo's and hi's
    int64_t otail_lo, otail_hi;  // units of lo's and hi's tails
    int64_t ovhdr;         // version below the first overlay boundary (kHole with a lower bound, else ihdr)
    int64_t* words;        // [kIwWords] ImportWord
    // the merged stream of the three (on equal keys: delta, overlay, base): per position the
    // version H' at the element's key, its prefix words and (len | bit 31: tail in otail, tail unit)
    int64_t* m_val;
    ulonglong2* m_key;
    uint2* m_lt;       // zeroed before the launches: a position nobody wrote reads as an empty key
    int64_t* d_blt;    // [nd] base boundaries below delta boundary j
    int64_t* v_blt;    // [m] base boundaries below overlay boundary e
    // result: the non-current base buffer and tail arena
    Hist dst;
    uint8_t* tdst;
    int64_t dst_cap, tdst_units;
    int64_t new_hdr;       // the set's header after the import
};
// What k_import_rank<S> merges: a window of each stream, by value.  Counts and values are taken over
// the whole streams, positions in the merged arrays from the windows' start.
struct ImportWindow {
    int64_t p_lo, p_hi;    // the delta's boundaries: [p_lo, p_hi)
    int64_t q_lo, q_hi;    // the base's: [q_lo, q_hi)
    int64_t mr;            // the overlay's: [0, mr)
    int64_t R;             // boundaries of the three windows: the merged positions are [0, R)
    int64_t e_ver;         // with a closing boundary: its version
    int32_t closing;       // overlay boundary mr closes the range: it takes position R as it is
    int* error;            // the word that gets bit 4 for a merged position out of range
};
// Validate the imported arrays, place lo / hi in them and normalize the overlay (phase 1 of both
// imports: k_import_check, k_import_bounds, k_import_normalize); the host reads the words (error,
// overlay size) before phase 2.
void launch_import_overlay(hipStream_t s, const ImportArgs& a);
// Merge the three streams and write the new base (phase 2: k_import_rank<1>, <2>, <0> over the whole
// streams, then k_scan<ImportFold>).  m: the overlay size phase 1 reported.
void launch_import_fold(hipStream_t s, const ImportArgs& a, int64_t m, uint64_t* granules);
// The greatest version of the tier whose levels `m` were just rebuilt, into *out (device, atomicMax).
void launch_import_max(hipStream_t s, const MaxLevels& m, int64_t lvl3_n, int64_t* out);

// ---- history import into the delta tier (fdbcs_history_import_delta / _delta_pending): the same
// definition, written as delta boundaries over [lo, hi) only.  Reads the current buffers, writes only
// scratch, the non-current delta buffer and arena bytes past tail_used; the host switches on success.
// Device words of one delta import (zeroed before its launches).
enum ImportDeltaWord {
    kIdError,      // int: 4 a merged position out of range, 8 a capacity bound
    kIdPlo,        // delta boundaries below lo
    kIdPhi,        // delta boundaries below hi
    kIdQlo,        // base boundaries below lo
    kIdQhi,        // base boundaries below hi
    kIdEver,       // the delta's value at hi: the version of its last boundary <= hi, kHole if none
    kIdEskip,      // the delta has a boundary at hi (no closing boundary is written)
    kIdKept,       // boundaries the fold wrote at the delta position of lo
    kIdTailUnits,  // 8-byte units it appended to the arena
    kIdScan,       // int counter, int error of the fold's scan
    kIdWords = 12
};
struct ImportDeltaArgs {
    // the tiers, the imported arrays, the overlay and the merged arrays as for the fold; dst is the
    // non-current delta buffer (dst_cap its capacity), tdst the current arena (tdst_units its capacity)
    ImportArgs a;
    int64_t* dwords;       // [kIdWords] ImportDeltaWord
    // what k_impd_bounds found, read back by the host and passed to the later launches by value:
    // the boundaries inside the range (mr: all of the overlay's but the closing one, which stands
    // with an upper bound and carries kIdEver); w.error is the launcher's to set
    ImportWindow w;
    int32_t e_skip;        // kIdEskip
    int64_t tail_base;     // first free unit of the arena (tail_used / 8)
};
// Positions of lo and hi in both tiers and the delta's value at hi (k_impd_bounds); after
// launch_import_overlay, in phase 1 (the host reads both word blocks in one go).
void launch_import_delta_bounds(hipStream_t s, const ImportDeltaArgs& d);
// Rank the three streams' boundaries inside the range (k_import_rank<1>, <2>, <0> over d.w), fold
// them into the non-current delta buffer at p_lo (k_scan<ImportDeltaFold>) and copy the delta's
// prefix and suffix around them (k_impd_copy) (phase 2).
void launch_import_delta_merge(hipStream_t s, const ImportDeltaArgs& d, uint64_t* granules);

// ---- the resolver's iops sample of a routed batch (fdbcs_batch_set_iops_sample; Resolver.actor.cpp:
// 178-192): the begin keys the roll keeps, in range order, in the layout of a history export.
constexpr uint32_t kIopsOffsetPerKey = 100;  // SAMPLE_OFFSET_PER_KEY (fdbserver/Knobs.cpp)
constexpr int kIopsScanP = 1;                // elements per thread of the sample's scan
constexpr int kIopsTile = kScanThreads * kIopsScanP;
// Totals of one sample (host-mapped).
struct IopsTotals {
    int64_t n, key_bytes;
};
struct IopsArgs {
    const DKey* keys;          // the routed batch's endpoints (range i's begin at 2i: reads, then writes)
    const uint8_t* tail;       // its tail arena
    const RouteResult* dres;   // the routing's device result: R, W and its error
    uint32_t units;            // metricUnitsPerSample, 1 .. 2^31 - 1
    uint64_t seed;
    int64_t cap;               // ranges the result arrays hold (the routing's read + write capacities)
    int64_t bytes_cap;         // bytes the key buffer holds
    int32_t* metrics;          // [n] what addMetric takes: max(metric, units)
    int32_t* index;            // [n] the range
    int64_t* key_offsets;      // [n + 1]
    uint8_t* bytes;
    IopsTotals* totals;        // host-mapped
};
// 8-byte words of the sample's scan state: counter and error words, then its granules.
int64_t iops_scan_words(int64_t cap);
// One launch on `s`, after the routing's; the scan state is zeroed by the caller.
void launch_iops_sample(hipStream_t s, const IopsArgs& a, ScanState st);

// ---- the version each read of a batch is checked against (fdbcs_batch_read_versions): per read r of
// an uploaded batch, out[r] = the greatest H_f(k) over the read's keys (a degenerate read: H_f just
// below its key), against an idle set.  Reads the batch's endpoint keys and both tiers; writes out
// and, for a position no consistent tier can give, bit 0 of *error.
struct ReadVersionsArgs {
    BatchDev b;            // the uploaded batch: keys [2R] and tail are read, nothing else
    Tier base, delta;      // the set's tiers as the read check sees them (sizes read on the device)
    const uint8_t* htail;  // their tail arena
    int64_t floor;         // versions below it read floor - 1 (kHole: no clamp)
    int64_t* out;          // [R] device memory
    int* error;            // one word, zeroed before the launch
};
// One launch on `s` (none for a batch without reads).  long_keys: as launch_check's.  Returns the
// kernel launched (the instantiation's host function, as fdbcs_kernel_profile names kernels).
const void* launch_read_versions(hipStream_t s, const ReadVersionsArgs& a, bool long_keys);

}  // namespace fdbcs
