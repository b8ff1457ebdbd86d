// verify.h — internal interface between fdbcs_history_verify (verify.cpp) and its gfx950 kernels
// (verify.hip): a read-only check of both stored tiers and of every derived array a lookup relies
// on.  Not part of the public C-ABI (the definition of each check class is the comment of
// fdbcs_history_verify in include/fdb_conflict_set.h); the detect pipeline's interface is engine.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

namespace fdbcs {

// Check classes, in the bit order of the public FDBCS_VERIFY_* masks.
enum VerifyClass {
    kVcOrder, kVcPadding, kVcTails, kVcVersions, kVcDominance, kVcLvl1, kVcLvl2, kVcLvl3, kVcSkey8, kVcSkey,
    kVcDir, kVcEdir, kVcCount
};
// Arrays an override can name, in the order of the public FDBCS_VERIFY_OV_* values (0: none).
enum VerifyWhat {
    kVwNone, kVwKey, kVwLenTail, kVwVersion, kVwLvl1, kVwLvl2, kVwLvl3, kVwSkey8, kVwSkey, kVwDir, kVwEdir,
    kVwTailWord, kVwCount
};
// One what-if element: every verifier kernel reads it as its stored words XOR (lo, hi).  A 16-byte
// element takes hi on its first word (the key prefix's high word) and lo on its second; (len,
// tail) takes lo on len and hi on the tail unit; 8- and 4-byte elements take lo alone.
struct VerifyOv {
    int32_t what, tier, level, pad;
    int64_t index;  // element of the array; lvl3: replica word j * kL3Rep + r; tail: 8-byte word of the arena
    uint64_t lo, hi;
};

// Device words of one verify, zeroed (counts) and set to all ones (firsts) before its launches.
// Counts: [tier][class][examined, violations], then the trusted delta-directory entries.
constexpr int kVfCounts = 2 * kVcCount * 2 + 2;
constexpr int kVfFirsts = 2 * kVcCount;  // [tier][class], atomicMin over unsigned indices
__host__ __device__ constexpr int vf_count(int tier, int cls, int k) { return (tier * kVcCount + cls) * 2 + k; }
constexpr int kVfTrusted = 2 * kVcCount * 2;
__host__ __device__ constexpr int vf_first(int tier, int cls) { return kVfCounts + tier * kVcCount + cls; }
constexpr int kVfWords = kVfCounts + kVfFirsts;

// One tier as the verifier reads it.  n is clamped by the host to the capacity of every array
// below, so an index below a count derived from n is always inside its array.
struct VerifyTier {
    Hist h;
    MaxLevels m;    // levels, samples and directories of the current buffer; dir / edir null: none
    int64_t n;
    int32_t has_dir, has_edir;
};
struct VerifyArgs {
    VerifyTier t[2];       // 0 base, 1 delta
    const uint64_t* tail;  // the tail arena as 8-byte words
    int64_t tail_used;     // clamped to the arena's capacity
    int64_t hdr;           // the set's header version (covers keys below the first base boundary)
    uint32_t checks;       // bit per VerifyClass
    VerifyOv ov;
    unsigned long long* words;  // [kVfWords]
};

// All launches of one verify on `s` (none for an empty tier's passes).
void launch_verify(hipStream_t s, const VerifyArgs& a);

}  // namespace fdbcs
