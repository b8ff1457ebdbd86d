// ingest.hip — gfx950 kernels of fdbcs_batch_add_packed_device: a batch in the plain
// fdbcs_packed_batch form that already lives in device memory becomes a batch in the upload layout
// (engine.cpp upload_layout) without the host reading any of it.  The detect pipeline's kernels are
// in kernels.hip and call nothing here; the look-back scan is scan.h, first_false search.h.
//
//   k_ingest_wait       one wave polls the caller's ready flag (bounded), as the routing's wait does
//   k_scan<IngestScan>  one element per key and per offset entry, one element per thread (every
//                       visit is a gather).  A lane checks its own two key offsets before it forms an
//                       address from them; the lane of a range's begin key also compares the range's
//                       two keys in the full byte order (TooOld transactions' ranges too: the verdict
//                       is not known yet, and KeyRangeRef refuses the range whatever becomes of it).
//                       Lanes t <= T check the read / write offsets at t.  The scan carries the tail
//                       units (8 bytes each) before each key, the keys longer than 19 and 24 bytes,
//                       the reporting transactions and the violations; its store leaves (len, tail)
//                       in the key's record and its last tile publishes the IngestResult.
//   k_ingest_write      returns at once on an error.  Lane k builds key k's prefix words and copies
//                       its tail, zero-padded to whole 8-byte words; lane g < R + W derives range g's
//                       owner by a search of the offsets; lane t <= T copies offsets, snapshot, flags.
//
// fdbcs_batch_share_pack_device runs the same wait and the same per-lane checks (ingest_check) and
// writes the arrays as the proxy share fdbcs_share_pack would, into the caller's buffer:
//   k_scan<ShareScan>   carries the tail bytes before each key (byte-packed, not units of 8) and the
//                       violations; its store leaves each key's tail offset in the slot's scratch,
//                       so nothing of the share is written before the outcome is known.  The last
//                       tile checks the exact size against cap, publishes the ShareResult and writes
//                       the header: the real one, or on an error the whole empty share.
//   k_share_write       returns at once on an error.  Lane k writes key k's record and copies its
//                       tail to its byte-packed place: both ends of the copy are at any byte, and
//                       neighbouring tails share 8-byte words, so the ragged head and end go out as
//                       byte stores and only the aligned words between them as words; lane g < R + W
//                       derives owner[g]; lane t <= T copies offsets, snapshot and report flag;
//                       workgroup 0 zeroes the alignment gaps and the 64 bytes of slack.
//
// Loads of key bytes.  The caller's arena has no slack and starts at any byte, so dkey.h tail_word
// (always two aligned words) is not used here: ingest_load reads the second aligned word only when
// the bytes asked for reach into it.  Every word loaded therefore holds at least one byte of the
// key, and a key lies inside [kbytes, kbytes + nbytes) once its offsets are checked.  An aligned
// 8-byte word never crosses a page, so the bytes of it outside the arena are readable.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ingest.h"
#include "launch.h"
#include "scan.h"
#include "search.h"

namespace fdbcs {

// Bytes p[0, n), 1 <= n <= 8, with p[0] lowest and zero past n.
__device__ __forceinline__ uint64_t ingest_load(const uint8_t* p, uint32_t n) {
    const uintptr_t a = (uintptr_t)p;
    const uint64_t* w = (const uint64_t*)(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7u) * 8u;
    uint64_t v = w[0] >> sh;
    if (sh + 8u * n > 64u) v |= w[1] << (64u - sh);  // (sh > 0 here)
    if (n < 8u) v &= (1ull << (8u * n)) - 1ull;
    return v;
}

// memcmp-then-length order of two keys of the arena, 8 bytes per step.
__device__ __forceinline__ int ingest_cmp(const uint8_t* a, uint32_t al, const uint8_t* b, uint32_t bl) {
    const uint32_t n = al < bl ? al : bl;
    for (uint32_t i = 0; i < n; i += 8u) {
        const uint32_t m = n - i < 8u ? n - i : 8u;
        const uint64_t x = __builtin_bswap64(ingest_load(a + i, m)), y = __builtin_bswap64(ingest_load(b + i, m));
        if (x != y) return x < y ? -1 : 1;
    }
    return (al > bl) - (al < bl);
}

// Key k's bytes; false (and an empty key) unless its two offsets lie inside the arena in order.
__device__ __forceinline__ bool ingest_key(const IngestArgs& a, int64_t k, const uint8_t*& p, uint32_t& len) {
    const int64_t o0 = a.koff[k], o1 = a.koff[k + 1];
    p = a.kbytes;
    len = 0;
    if (o0 < 0 || o1 < o0 || o1 > a.nbytes) return false;
    p = a.kbytes + o0;
    len = (uint32_t)(o1 - o0);  // nbytes < 2^32
    return true;
}

// The arrays are written by another HIP runtime (or another stream of the caller's), which this
// engine cannot wait on: the caller's stream sets a device word once they are complete, and one
// wave polls it (agent scope), bounded by `timeout_ticks` of the 100 MHz constant clock.
__global__ void k_ingest_wait(const uint32_t* ready, uint32_t value, uint32_t* err, uint64_t timeout_ticks) {
    if (threadIdx.x != 0) return;
    if (ready) {
        const uint64_t t0 = wall_clock64();
        for (;;) {
            if (__hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == value) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                *err = 0;
                return;
            }
            if (wall_clock64() - t0 > timeout_ticks) break;
            __builtin_amdgcn_s_sleep(16);
        }
        *err = 1;
        return;
    }
    *err = 0;
}

// The checks of scan element i, shared by the add and the share pack: key i's two offsets (before
// an address is formed from them) and, on a begin key, the order of its range's keys; the read /
// write offsets at i <= T.  Returns 1 on a violation; len is key i's length (0 without a valid key).
__device__ __forceinline__ uint32_t ingest_check(const IngestArgs& a, int64_t i, uint32_t& len) {
    uint32_t bad = 0;
    len = 0;
    if (i < a.nk) {
        const uint8_t *p, *q;
        uint32_t ql;
        if (!ingest_key(a, i, p, len)) {
            bad = 1;
        } else if (!(i & 1) && ingest_key(a, i + 1, q, ql) && ingest_cmp(p, len, q, ql) > 0) {
            // a begin key (nk is even, so its end key exists): begin <= end; an end key whose
            // offsets are wrong is reported by its own lane
            bad = 1;
        }
    }
    if (i <= a.T) {
        const int32_t r = a.roff[i], w = a.woff[i];
        if (i == 0 && (r != 0 || w != 0)) bad = 1;
        if (i == a.T) {
            if (r != a.R || w != a.W) bad = 1;
        } else if (a.roff[i + 1] < r || a.woff[i + 1] < w) {
            bad = 1;
        }
    }
    return bad;
}

struct IngestScan {
    IngestArgs a;
    const int* scan_err;
    __device__ void load(int64_t i, uint32_t (&v)[kIngestScanK]) const {
        if (*a.wait_err) return;  // the arrays never became ready: read nothing of them
        uint32_t len;
        v[4] = ingest_check(a, i, len);
        v[0] = len > 16u ? (len - 16u + 7u) >> 3 : 0u;
        v[1] = len > 19u ? 1u : 0u;
        v[2] = len > 24u ? 1u : 0u;
        if (i < a.T && a.report_enabled && a.report && a.report[i]) v[3] = 1;
    }
    __device__ void store(int64_t i, const uint32_t (&ex)[kIngestScanK]) const {
        if (i >= a.nk || *a.wait_err) return;
        const uint8_t* p;
        uint32_t len;
        if (!ingest_key(a, i, p, len)) return;
        // (len, tail) of the record: one 8-byte store at its 8-aligned offset 16
        *(uint2*)&a.keys[i].len = make_uint2(len, len > 16u ? 8u * ex[0] : 0u);
    }
    __device__ void finish(const uint32_t (&tot)[kIngestScanK]) const {
        IngestResult r{};
        r.reports = (int32_t)tot[3];
        r.n_gt19 = (int32_t)tot[1];
        r.n_gt24 = (int32_t)tot[2];
        r.tail_bytes = 8ll * (int64_t)tot[0];
        r.error = *a.wait_err ? 2 : tot[4] ? 1 : 0;
        if (!r.error && __hip_atomic_load(scan_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) r.error = 4;
        *a.dres = r;
        *a.res = r;
    }
};

__global__ __launch_bounds__(kBlock) void k_ingest_write(IngestArgs a) {
    if (a.dres->error) return;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.nk) {
        // offsets the scan checked; (len, tail) as its store left them
        const uint8_t* p = a.kbytes + a.koff[g];
        const uint2 lt = *(const uint2*)&a.keys[g].len;
        const uint32_t len = lt.x;
        const uint64_t w0 = len ? ingest_load(p, len < 8u ? len : 8u) : 0ull;
        const uint64_t w1 = len > 8u ? ingest_load(p + 8, len < 16u ? len - 8u : 8u) : 0ull;
        // the first key byte is the lowest of the loaded word and the highest of the prefix word
        a.keys[g].hi = __builtin_bswap64(w0);
        a.keys[g].lo = __builtin_bswap64(w1);
        if (len > 16u) {
            const uint32_t nt = len - 16u;
            uint64_t* d = (uint64_t*)(a.tail + lt.y);
            for (uint32_t q = 0; 8u * q < nt; q++) d[q] = ingest_load(p + 16 + 8u * q, nt - 8u * q < 8u ? nt - 8u * q : 8u);
        }
    }
    if (g < (int64_t)a.R + a.W) {
        // the transaction t with off[t] <= j < off[t + 1]: the last of a run of equal offsets (the
        // empty transactions before it own nothing)
        const bool is_read = g < a.R;
        const int32_t j = (int32_t)(is_read ? g : g - a.R);
        const int32_t* off = is_read ? a.roff : a.woff;
        const int32_t t = first_false<int32_t>(0, a.T + 1, [&](int32_t q) { return off[q] <= j; }) - 1;
        (is_read ? a.rown : a.wown)[j] = t;
    }
    if (g <= a.T) {
        a.oroff[g] = a.roff[g];
        a.owoff[g] = a.woff[g];
        if (g < a.T) {
            a.osnap[g] = a.snap[g];
            // TooOld is decided when the batch is detected (k_route_too_old ORs it in)
            a.flags[g] = (a.report_enabled && a.report && a.report[g]) ? kFlagReport : 0;
        }
    }
}

// ---- the share pack (fdbcs_batch_share_pack_device): the same arrays, the same checks, written as
// the proxy share fdbcs_share_pack writes.  Nothing of the share is written before the scan's last
// tile knows the outcome: the scan's store goes to the slot's scratch.

struct ShareScan {
    ShareArgs s;
    const int* scan_err;
    __device__ void load(int64_t i, uint32_t (&v)[kShareScanK]) const {
        const IngestArgs& a = s.in;
        if (*a.wait_err || a.T == 0) return;  // never ready, or the empty share: read nothing
        uint32_t len;
        v[1] = ingest_check(a, i, len);
        v[0] = len > 16u ? len - 16u : 0u;  // < 2^32 in all: the tails are bytes of the arena
    }
    __device__ void store(int64_t i, const uint32_t (&ex)[kShareScanK]) const {
        if (i < s.in.nk) s.toff[i] = ex[0];
    }
    __device__ void finish(const uint32_t (&tot)[kShareScanK]) const {
        const IngestArgs& a = s.in;
        ShareResult r{};
        r.tail_bytes = (int64_t)tot[0];
        // share_layout's last step: the tail region, its 64 bytes of slack, rounded up to 64
        r.bytes = ((int64_t)s.hdr[kShareHdrOffTail] + r.tail_bytes + 64 + 63) / 64 * 64;
        r.error = *a.wait_err ? 2 : tot[1] ? 1 : 0;
        if (!r.error && __hip_atomic_load(scan_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) r.error = 4;
        if (!r.error && r.bytes > s.cap) r.error = 3;
        uint64_t* o = (uint64_t*)s.out;
        if (r.error) {
            r.tail_bytes = 0;
            r.bytes = kShareEmptyBytes;
#pragma unroll
            for (int j = 0; j < 16; j++) o[j] = s.empty[j];
            for (int j = 16; j < (int)(kShareEmptyBytes / 8); j++) o[j] = 0;
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++)
                o[j] = j == kShareHdrBytes ? (uint64_t)r.bytes : j == kShareHdrTail ? (uint64_t)r.tail_bytes : s.hdr[j];
        }
        *s.dres = r;
        *s.res = r;
    }
};

// Bytes [0, n) of v, lowest first, to d: the ragged ends of a tail (n <= 7).
__device__ __forceinline__ void share_put_bytes(uint8_t* d, uint64_t v, uint32_t n) {
    for (uint32_t j = 0; j < n; j++) d[j] = (uint8_t)(v >> (8u * j));
}

// Zero [from, to) of the share, spread over one workgroup (an alignment gap: under 128 bytes).
__device__ __forceinline__ void share_zero_gap(uint8_t* out, int64_t from, int64_t to) {
    for (int64_t j = from + threadIdx.x; j < to; j += blockDim.x) out[j] = 0;
}

__global__ __launch_bounds__(kBlock) void k_share_write(ShareArgs s) {
    if (s.dres->error) return;
    const IngestArgs& a = s.in;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t off_keys = (int64_t)s.hdr[kShareHdrOffKeys], off_snap = (int64_t)s.hdr[kShareHdrOffSnap],
                  off_roff = (int64_t)s.hdr[kShareHdrOffRoff], off_woff = (int64_t)s.hdr[kShareHdrOffWoff],
                  off_report = (int64_t)s.hdr[kShareHdrOffReport], off_tail = (int64_t)s.hdr[kShareHdrOffTail],
                  off_owner = (int64_t)s.hdr[kShareHdrOffOwner];
    const int64_t nr = (int64_t)a.R + a.W;
    if (g < a.nk) {
        // offsets the scan checked; the tail's place as its store left it
        const int64_t o0 = a.koff[g];
        const uint8_t* p = a.kbytes + o0;
        const uint32_t len = (uint32_t)(a.koff[g + 1] - o0);
        const uint64_t w0 = len ? ingest_load(p, len < 8u ? len : 8u) : 0ull;
        const uint64_t w1 = len > 8u ? ingest_load(p + 8, len < 16u ? len - 8u : 8u) : 0ull;
        const uint32_t to = len > 16u ? s.toff[g] : 0u;
        uint64_t* k = (uint64_t*)(s.out + off_keys + 24 * g);  // DKey {hi, lo, len, tail}
        k[0] = __builtin_bswap64(w0);
        k[1] = __builtin_bswap64(w1);
        *(uint2*)&k[2] = make_uint2(len, to);
        if (len > 16u) {
            // source and destination at any byte; a neighbour's tail may share the destination's
            // first and last 8-byte word, so the ragged ends go out as bytes and only the aligned
            // words between them, which this lane owns whole, as words
            const uint8_t* src = p + 16;
            uint8_t* d = s.out + off_tail + to;
            const uint32_t n = len - 16u;
            uint32_t h = (8u - (uint32_t)((uintptr_t)d & 7u)) & 7u;
            if (h > n) h = n;
            if (h) share_put_bytes(d, ingest_load(src, h), h);
            uint32_t q = h;
            for (; q + 8u <= n; q += 8u) *(uint64_t*)(d + q) = ingest_load(src + q, 8u);
            if (q < n) share_put_bytes(d + q, ingest_load(src + q, n - q), n - q);
        }
    }
    if (g < nr) {
        // the transaction t with off[t] <= j < off[t + 1]: the last of a run of equal offsets
        const bool is_read = g < a.R;
        const int32_t j = (int32_t)(is_read ? g : g - a.R);
        const int32_t* off = is_read ? a.roff : a.woff;
        const int32_t t = first_false<int32_t>(0, a.T + 1, [&](int32_t q) { return off[q] <= j; }) - 1;
        ((int32_t*)(s.out + off_owner))[g] = t;
    }
    if (g <= a.T) {
        // (the empty share reads no array: its two offsets are zero)
        ((int32_t*)(s.out + off_roff))[g] = a.T ? a.roff[g] : 0;
        ((int32_t*)(s.out + off_woff))[g] = a.T ? a.woff[g] : 0;
        if (g < a.T) {
            ((int64_t*)(s.out + off_snap))[g] = a.snap[g];
            s.out[off_report + g] = a.report ? a.report[g] : (uint8_t)0;
        }
    }
    if (blockIdx.x == 0) {
        // what fdbcs_share_pack leaves of its zeroed buffer: the gap after each region up to the
        // next one, and after the tail bytes their 64 bytes of slack and the rounding of the size
        const int64_t T = a.T;
        share_zero_gap(s.out, off_keys + 24 * a.nk, off_snap);
        share_zero_gap(s.out, off_snap + 8 * T, off_roff);
        share_zero_gap(s.out, off_roff + 4 * (T + 1), off_woff);
        share_zero_gap(s.out, off_woff + 4 * (T + 1), off_report);
        share_zero_gap(s.out, off_report + T, off_owner);
        share_zero_gap(s.out, off_owner + 4 * nr, off_tail);
        share_zero_gap(s.out, off_tail + s.dres->tail_bytes, s.dres->bytes);
    }
}

int64_t ingest_scan_words(int64_t n_elems) { return 8 + scan_granules(n_elems, kIngestScanK, kIngestScanP); }
int64_t share_scan_words(int64_t n_elems) { return 8 + scan_granules(n_elems, kShareScanK, kIngestScanP); }

void launch_share_pack(hipStream_t s, const ShareArgs& a, ScanState st) {
    const int64_t n = ingest_elems(a.in.T, a.in.nk);
    fdb_launch(k_ingest_wait, dim3(1), dim3(64), 0, s, a.in.ready, a.in.ready_value, a.in.wait_err, a.in.wait_ticks);
    launch_scan<kShareScanK, kIngestScanP>(s, ShareScan{a, st.error}, nullptr, n, st);
    fdb_launch(k_share_write, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
}

void launch_ingest(hipStream_t s, const IngestArgs& a, ScanState st) {
    const int64_t n = ingest_elems(a.T, a.nk);
    fdb_launch(k_ingest_wait, dim3(1), dim3(64), 0, s, a.ready, a.ready_value, a.wait_err, a.wait_ticks);
    launch_scan<kIngestScanK, kIngestScanP>(s, IngestScan{a, st.error}, nullptr, n, st);
    fdb_launch(k_ingest_write, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
}

}  // namespace fdbcs
