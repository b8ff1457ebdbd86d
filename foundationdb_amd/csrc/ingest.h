// ingest.h — internal interface between the device-add entry points (ingest.cpp) and their gfx950
// kernels (ingest.hip): a whole batch in the plain fdbcs_packed_batch form, already in device
// memory, validated and normalized into the upload layout by kernels (fdbcs_batch_add_packed_device).
// Not part of the public C-ABI; the detect pipeline's interface is engine.h.
#pragma once
#include <hip/hip_runtime.h>
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

// 8-byte words of the add's scan state: counter, error and wait words, then its granules.
int64_t ingest_scan_words(int64_t n_elems);
// Elements of the add's scan and lanes of its write launch: one per key and one per offset entry.
inline int64_t ingest_elems(int32_t T, int64_t nk) { return nk > (int64_t)T + 1 ? nk : (int64_t)T + 1; }
// The wait, the scan and the write launch on `s`; the scan state is zeroed by the caller.
void launch_ingest(hipStream_t s, const IngestArgs& a, ScanState st);

}  // namespace fdbcs
