// ingest.h — internal interface between the device-add entry points (ingest.cpp) and their gfx950
// kernels (ingest.hip): a whole batch in the plain fdbcs_packed_batch form, already in device
// memory, validated and normalized into the upload layout by kernels (fdbcs_batch_add_packed_device),
// or validated and packed as a proxy's share (fdbcs_batch_share_pack_device).
// Not part of the public C-ABI; the detect pipeline's interface is engine.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "engine.h"

namespace fdbcs {

constexpr int kIngestScanP = 1;  // one key per thread: every visit of the scan is a gather
constexpr int kIngestScanK = 5;  // tail units, keys > 19 bytes, keys > 24 bytes, reporting transactions, violations
constexpr int kIngestTile = kScanThreads * kIngestScanP;

// Totals of a device-added batch (host-mapped copy for the host, device copy for k_ingest_write).
struct IngestResult {
    int32_t reports;         // transactions whose report flag is set (0 unless the batch collects reports)
    int32_t n_gt19, n_gt24;  // keys longer than 19 / 24 bytes (sort tail windows, long-key probes)
    int32_t error;           // 0; 1: the arrays violate the layout or hold an inverted range; 2: the
                             // ready flag was never set; 4: the scan's look-back gave up
    int64_t tail_bytes;      // bytes of the batch's tail region in use (every tail padded to 8)
};

struct IngestArgs {
    int32_t T, R, W;
    int32_t report_enabled;   // the batch was created with report_keys
    int64_t nk;               // 2 (R + W) keys
    int64_t nbytes;           // bytes of kbytes, < 2^32
    // the caller's arrays (device memory, read only; kbytes at any byte alignment, no slack)
    const int64_t* snap;
    const uint8_t* report;    // or null
    const int32_t* roff;
    const int32_t* woff;
    const uint8_t* kbytes;
    const int64_t* koff;
    // the batch in the upload layout: key k of the input is key k of the batch
    DKey* keys;
    int32_t *rown, *wown, *oroff, *owoff;
    int64_t* osnap;
    uint8_t* flags;
    uint8_t* tail;            // 8-byte aligned; key k's tail at 8 * (the units before it)
    IngestResult* res;        // host-mapped
    IngestResult* dres;       // device copy
    const uint32_t* ready;    // device word the caller's stream sets to ready_value once the arrays
    uint32_t ready_value;     // are complete (null: already complete); k_ingest_wait spins on it
    uint32_t* wait_err;       // set when that wait timed out
    uint64_t wait_ticks;      // bound of that wait, in 100 MHz wall-clock ticks
};

// ---- fdbcs_batch_share_pack_device: the same arrays packed as a proxy share (engine.h ShareHeader)

constexpr int kShareScanK = 2;  // tail bytes, violations

// Outcome of a share pack (host-mapped copy for the host, device copy for k_share_write).
struct ShareResult {
    int64_t tail_bytes;  // bytes of the share's tail region in use (byte-packed)
    int64_t bytes;       // the share, header included (the empty share's on an error)
    int32_t error;       // 0; 1: the arrays violate the layout or hold an inverted range; 2: the ready
                         // flag was never set; 3: the exact size passes cap; 4: the scan's look-back gave up
    int32_t pad;
};

struct ShareArgs {
    IngestArgs in;        // sizes, the caller's arrays, the ready flag and its wait (nothing of the batch)
    uint8_t* out;         // the share: 64-byte aligned, cap bytes, cap >= the layout without tails
    int64_t cap;
    uint64_t hdr[16];     // ShareHeader of (T, R, W) without tails: every offset is final
    uint64_t empty[16];   // ShareHeader of the empty share, written on an error
    uint32_t* toff;       // [nk] scratch: each key's byte offset in the tail region (the scan's store)
    ShareResult* res;     // host-mapped
    ShareResult* dres;    // device copy
};
// 8-byte words of ShareHeader
constexpr int kShareHdrBytes = 2, kShareHdrOffKeys = 3, kShareHdrOffSnap = 4, kShareHdrOffRoff = 5, kShareHdrOffWoff = 6,
              kShareHdrOffReport = 7, kShareHdrOffTail = 8, kShareHdrTail = 9, kShareHdrOffOwner = 10;
static_assert(offsetof(ShareHeader, bytes) == 8 * kShareHdrBytes && offsetof(ShareHeader, off_keys) == 8 * kShareHdrOffKeys &&
                  offsetof(ShareHeader, off_snap) == 8 * kShareHdrOffSnap &&
                  offsetof(ShareHeader, off_roff) == 8 * kShareHdrOffRoff &&
                  offsetof(ShareHeader, off_woff) == 8 * kShareHdrOffWoff &&
                  offsetof(ShareHeader, off_report) == 8 * kShareHdrOffReport &&
                  offsetof(ShareHeader, off_tail) == 8 * kShareHdrOffTail &&
                  offsetof(ShareHeader, tail_bytes) == 8 * kShareHdrTail &&
                  offsetof(ShareHeader, off_owner) == 8 * kShareHdrOffOwner && sizeof(DKey) == 24,
              "ShareArgs::hdr indexes ShareHeader by 8-byte words");
constexpr int64_t kShareEmptyBytes = 320;             // the empty share: header, roff[0], woff[0], tail slack

// 8-byte words of the add's scan state: counter, error and wait words, then its granules.
int64_t ingest_scan_words(int64_t n_elems);
int64_t share_scan_words(int64_t n_elems);
// The wait, the scan and the write launch of a share pack on `s`; the scan state is zeroed by the caller.
void launch_share_pack(hipStream_t s, const ShareArgs& a, ScanState st);
// Elements of the add's scan and lanes of its write launch: one per key and one per offset entry.
inline int64_t ingest_elems(int32_t T, int64_t nk) { return nk > (int64_t)T + 1 ? nk : (int64_t)T + 1; }
// The wait, the scan and the write launch on `s`; the scan state is zeroed by the caller.
void launch_ingest(hipStream_t s, const IngestArgs& a, ScanState st);

}  // namespace fdbcs
