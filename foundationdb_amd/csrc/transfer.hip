// transfer.hip — gfx950 kernels of the maintenance side of the engine: history export, the history
// digest and its partitioned form, split keys, the two history imports, the resolver's iops sample
// and the read versions of a batch.  They run on an idle set or off the detect stream
// (transfer.cpp); the detect pipeline's kernels are in kernels.hip and call nothing here.  The
// searches both sides use are in search.h, the look-back scan in scan.h.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>

#include "transfer.h"
#include "launch.h"
#include "scan.h"
#include "search.h"

namespace fdbcs {

// ------------------------------------------------------------------ history export
//
// The canonical description of H_f(k) = the version a read of k sees (delta entry unless kHole, else
// base entry, else the header), clamped to floor - 1 below the floor, over (lo, hi): the keys where
// it changes, with their new values, in the layout fdbcs_load_history takes.  Read-only: nothing of
// the set, its levels, index, directories, Scalars or batch workspaces is written.
//
// Both tiers' boundaries in key order form one merged stream (on equal keys the delta's first).  H at
// every stream element is known from the element and the delta boundary covering it, and an element
// is kept when its clamped value differs from its predecessor's: base boundaries hidden under a
// written delta segment, the second of two equal keys and runs the floor made equal all repeat their
// predecessor's value, so no case is special.
//   k_export_search  one lane per delta boundary j: lower bound lb in the base (the compaction's
//                    search, without its side effects) -> stream position j + lb, and H(d_j)
//   k_export_bounds  stream positions of lo and hi by plain binary searches, and the header H_f(lo)
//   k_export_tile_starts  per scan tile, the delta boundaries below its first element (one thread each)
//   k_export_scan    per 1024-element tile of the stream: the delta positions the tile can meet are
//                    staged in LDS (consecutive elements meet consecutive delta boundaries), every
//                    element is resolved to its source and clamped value there, then flagged and
//                    scanned (scan.h look-back) and the kept ones written.
// Key bytes are scanned as three 32-bit components, kept count c, bytes mod 2^32 a, and sum of
// (len >> 3) b: a prefix P lies in [8 b, 8 b + 7 c] and is congruent to a, which determines it while
// 7 c < 2^32 and b < 2^32: exact 64-bit offsets below 2^29 boundaries and 32 GiB of key bytes (the
// host refuses an export that could pass either).

__device__ __forceinline__ int64_t export_prefix64(uint32_t a, uint32_t b) {
    const uint64_t lower = 8ull * b;
    return (int64_t)(lower + (uint32_t)(a - (uint32_t)lower));
}

__device__ __forceinline__ int64_t export_clamp(int64_t v, int64_t floor) {
    return (floor == kHole || v >= floor) ? v : floor - 1;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_export_search(Hist base, MaxLevels basem, Hist delta,
                                                          const uint8_t* htail, int64_t nb, int64_t nd, int64_t hdr,
                                                          int64_t* d_pos, int64_t* d_val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd) return;
    DKey q;
    const uint8_t* qtail;
    tier_query(delta, j, htail, q, qtail);
    bool exact;
    int64_t lb;
    if constexpr (MODE == 1) {
        lb = lane_lower_bound(base, basem, nb, q, htail, qtail, exact);
    } else {
        QTail qt;
        load_qtail(qt, q, qtail);
        lb = lane_lower_bound_long(base, basem, nb, q, qt, htail, qtail, exact);
    }
    const int64_t dv = delta.ver[j];
    d_pos[j] = j + lb;
    // a hole takes the base value at its key: the base boundary there, or the one covering it
    d_val[j] = dv != kHole ? dv : exact ? base.ver[lb] : lb > 0 ? base.ver[lb - 1] : hdr;
}

__global__ __launch_bounds__(64) void k_export_bounds(ExportArgs a) {
    __shared__ int64_t r[4];  // boundaries <= lo in base, delta; boundaries < hi in base, delta
    const int t = threadIdx.x;
    if (t < 4)
        r[t] = tier_bounds_lane(t, a.base, a.nb, a.delta, a.nd, a.htail, a.has_lo, a.has_hi, true,
                                [&](bool is_hi, DKey& q, const uint8_t*& qtail) {
                                    q = is_hi ? a.hi : a.lo;
                                    qtail = a.btail;
                                });
    __syncthreads();
    if (t != 0) return;
    int64_t h = a.hdr;
    if (r[0] > 0) h = a.base.ver[r[0] - 1];
    if (r[1] > 0) {
        const int64_t dv = a.delta.ver[r[1] - 1];
        if (dv != kHole) h = dv;
    }
    const int64_t m_lo = r[0] + r[1], m_hi = r[2] + r[3];
    a.words[kXwLo] = m_lo;
    a.words[kXwHi] = m_hi > m_lo ? m_hi : m_lo;
    a.words[kXwHeader] = export_clamp(h, a.floor);
}

// Write the n bytes of a key, given as little-endian 8-byte words get(0 .. nw - 1) in key order, to
// d (any alignment): bytes up to d's next 8-byte line, whole words, then the rest.
template <class G>
__device__ __forceinline__ void export_put_key(uint8_t* d, uint32_t n, uint32_t nw, const G& get) {
    uint32_t head = (uint32_t)((8u - ((uintptr_t)d & 7u)) & 7u);
    if (head > n) head = n;
    uint64_t cur = nw ? get(0u) : 0ull;
    for (uint32_t b = 0; b < head; b++) d[b] = (uint8_t)(cur >> (8u * b));
    const uint32_t sh = 8u * head, nfull = (n - head) >> 3;
    uint64_t* dw = (uint64_t*)(d + head);
    for (uint32_t q = 0; q < nfull; q++) {
        const uint64_t next = q + 1u < nw ? get(q + 1u) : 0ull;
        dw[q] = sh ? (cur >> sh) | (next << (64u - sh)) : cur;
        cur = next;
    }
    for (uint32_t b = head + 8u * nfull; b < n; b++) d[b] = (uint8_t)(get(b >> 3) >> (8u * (b & 7u)));
}

// Per scan tile: the delta boundaries below the first stream element the tile resolves (its
// predecessor; tile 0: its first element).  One thread per tile, so the binary searches of all tiles
// run side by side instead of one per workgroup at the head of its tile.
__global__ __launch_bounds__(kBlock) void k_export_tile_starts(ExportArgs a) {
    const int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m_lo = a.words[kXwLo], n = a.words[kXwHi] - m_lo;
    const int64_t ntiles = n > 0 ? (n + kScanTile - 1) / kScanTile : 1;
    if (tile >= ntiles) return;
    const int64_t mfirst = m_lo + tile * kScanTile - (tile > 0 ? 1 : 0);
    a.tile_tb[tile] = first_false<int64_t>(0, a.nd, [&](int64_t j) { return a.d_pos[j] < mfirst; });
}

constexpr int kExpWin = kScanTile + 2;  // delta boundaries a tile and its predecessor can meet, and one past

struct ExportScan {
    ExportArgs a;
    const int64_t* s_val;  // LDS: clamped value of the tile's predecessor, then of its elements
    const int64_t* s_src;  // LDS: source of each element: base boundary i, or ~j for delta boundary j
    int64_t tile0;         // the tile's first element
    int* err;              // the export's error word
    __device__ bool keep(int e) const { return s_val[e + 1] != s_val[e]; }
    __device__ void load(int64_t i, uint32_t (&v)[3]) const {
        const int e = (int)(i - tile0);
        uint32_t len = 0;
        const bool kp = keep(e);
        if (kp) {
            const int64_t src = s_src[e];
            len = src >= 0 ? a.base.lt[src].x : a.delta.lt[~src].x;
        }
        v[0] = kp ? 1u : 0u;
        v[1] = len;
        v[2] = len >> 3;
    }
    __device__ void store(int64_t i, const uint32_t (&ex)[3]) const {
        const int e = (int)(i - tile0);
        if (!keep(e)) return;
        const int64_t o = ex[0], P = export_prefix64(ex[1], ex[2]);
        const int64_t src = s_src[e];
        const Hist& h = src >= 0 ? a.base : a.delta;
        const int64_t p = src >= 0 ? src : ~src;
        const ulonglong2 k = h.key[p];
        const uint2 lt = h.lt[p];
        a.versions[o] = s_val[e + 1];
        a.offsets[o] = P;
        if (P + (int64_t)lt.x > a.bytes_cap) {  // never past the result buffer (the host sized it for every key)
            atomicOr(err, 8);
            return;
        }
        // the prefix words are big-endian: swapped back, the key's first byte is the lowest
        const uint64_t w0 = __builtin_bswap64(k.x), w1 = __builtin_bswap64(k.y);
        const uint64_t* tw = (const uint64_t*)hist_tail(a.htail, lt.x > 16u ? lt.y : 0u);
        export_put_key(a.bytes + P, lt.x, (lt.x + 7u) >> 3,
                       [&](uint32_t q) { return q == 0u ? w0 : q == 1u ? w1 : tw[q - 2u]; });
    }
    __device__ void finish(const uint32_t (&tot)[3]) const {
        const int64_t P = export_prefix64(tot[1], tot[2]);
        a.words[kXwN] = tot[0];
        a.words[kXwBytes] = P;
        a.offsets[tot[0]] = P;
    }
};

// The resolve step of one tile (k_export_scan, k_export_digest; the whole workgroup calls it): the
// clamped value of the tile's predecessor and of each of its elements into s_val[0 .. cnt], each
// element's source into s_src.  Ends with a barrier.
__device__ __forceinline__ void export_resolve_tile(const ExportArgs& a, int64_t tile, int64_t m_lo, int64_t n,
                                                    int64_t (&s_pos)[kExpWin], int64_t (&s_val)[kScanTile + 1],
                                                    int64_t (&s_src)[kScanTile], int* err) {
    const int64_t tile0 = tile * kScanTile;
    // stream elements resolved here: the tile's, and before them its predecessor (tile 0: the header)
    const int pre = tile > 0 ? 1 : 0;
    const int64_t mfirst = m_lo + tile0 - pre;
    int64_t rest = n - tile0;
    const int cnt = (int)(rest < kScanTile ? rest : kScanTile) + pre;
    // delta boundaries below the first element (k_export_tile_starts); the next kExpWin positions cover
    // every element's search: positions ascend strictly, so window entry q lies at mfirst + q or later
    const int64_t tb = a.tile_tb[tile];
    for (int q = threadIdx.x; q < kExpWin; q += kScanThreads) s_pos[q] = tb + q < a.nd ? a.d_pos[tb + q] : LLONG_MAX;
    __syncthreads();
    for (int k = threadIdx.x; k < cnt; k += kScanThreads) {
        const int64_t m = mfirst + k;
        const int l = first_false<int>(0, kExpWin, [&](int q) { return s_pos[q] <= m; });  // window entries at or below m
        const int64_t t = tb + l;  // delta boundaries at or below element m: t - 1 covers it
        int64_t v, src;
        if (l > 0 && s_pos[l - 1] == m) {
            src = ~(t - 1);
            v = a.d_val[t - 1];
        } else {
            src = m - t;
            if (src < 0 || src >= a.nb) {  // positions out of order: never index past the tier
                atomicOr(err, 4);
                src = a.nb > 0 ? 0 : ~(int64_t)0;
            }
            const int64_t dv = t > 0 ? a.delta.ver[t - 1] : kHole;
            v = dv != kHole ? dv : src >= 0 ? a.base.ver[src] : a.hdr;
        }
        const int slot = k + 1 - pre;
        s_val[slot] = export_clamp(v, a.floor);
        if (slot > 0) s_src[slot - 1] = src;
    }
    if (tile == 0 && threadIdx.x == 0) s_val[0] = a.words[kXwHeader];
    __syncthreads();
}

__global__ __launch_bounds__(kScanThreads) void k_export_scan(ExportArgs a, ScanState st) {
    __shared__ uint32_t sv[3][kScanPad];
    __shared__ uint32_t swave[3][kScanThreads / 64];
    __shared__ uint32_t sbase[3];
    __shared__ int s_tile;
    __shared__ int64_t s_pos[kExpWin];
    __shared__ int64_t s_val[kScanTile + 1];
    __shared__ int64_t s_src[kScanTile];
    const int64_t m_lo = a.words[kXwLo], n = a.words[kXwHi] - m_lo;
    if (threadIdx.x == 0) s_tile = atomicAdd(st.counter, 1);
    __syncthreads();
    const int tile = s_tile;
    const int64_t ntiles = n > 0 ? (n + kScanTile - 1) / kScanTile : 1;
    if (tile >= ntiles) return;
    export_resolve_tile(a, tile, m_lo, n, s_pos, s_val, s_src, st.error);
    const ExportScan f{a, s_val, s_src, (int64_t)tile * kScanTile, st.error};
    scan_tile<3>(f, n, tile, ntiles, st, sv, swave, sbase);
}

// ---- history digest (fdbcs_history_digest; the definition is in include/fdb_conflict_set.h)
//
// The export's first three launches as they stand, then k_export_digest instead of k_export_scan: the
// same tiles, resolved by the same helper, but a kept element's key is hashed where it lies instead of
// being copied.  The four totals (kept boundaries, their key bytes, the two lanes' sums) are sums mod
// 2^64 of per-element terms, so they need no scan, no tile order and no look-back: every workgroup
// reduces its own and adds them to the digest's words (kXwN, kXwBytes, kDwSum0, kDwSum1).

__device__ __forceinline__ uint64_t digest_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t kDigestG = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kDigestS0 = 0x243F6A8885A308D3ull, kDigestS1 = 0x13198A2E03707344ull;

// One kept element's terms (k_export_digest, k_export_digest_ranges): e is the element's index in the
// tile export_resolve_tile resolved; acc counts kept, key bytes, sum[0], sum[1].
__device__ __forceinline__ void digest_element(const ExportArgs& a, const int64_t* s_val, const int64_t* s_src, int e,
                                               uint64_t (&acc)[4]) {
    const int64_t src = s_src[e];
    const Hist& h = src >= 0 ? a.base : a.delta;
    const int64_t p = src >= 0 ? src : ~src;
    const ulonglong2 key = h.key[p];
    const uint2 lt = h.lt[p];
    const uint32_t len = lt.x, nw = (len + 7u) >> 3;
    uint64_t h0 = digest_mix(kDigestS0 + len), h1 = digest_mix(kDigestS1 + len);
    // the prefix words are the big-endian words of the definition, zero past the key
    if (nw > 0u) h0 = digest_mix((h0 ^ key.x) + kDigestG), h1 = digest_mix((h1 ^ key.x) + kDigestG);
    if (nw > 1u) h0 = digest_mix((h0 ^ key.y) + kDigestG), h1 = digest_mix((h1 ^ key.y) + kDigestG);
    if (nw > 2u) {
        // tail words hold the key's bytes lowest first; what the last one holds past the key is not read
        const uint64_t* tw = (const uint64_t*)hist_tail(a.htail, lt.y);
        const uint32_t last = nw - 3u, used = len & 7u;
        for (uint32_t q = 0; q <= last; q++) {
            uint64_t w = __builtin_bswap64(tw[q]);
            if (q == last && used) w &= ~0ull << (64u - 8u * used);
            h0 = digest_mix((h0 ^ w) + kDigestG);
            h1 = digest_mix((h1 ^ w) + kDigestG);
        }
    }
    const uint64_t v = (uint64_t)s_val[e + 1];
    acc[0] += 1;
    acc[1] += len;
    acc[2] += digest_mix((h0 ^ v) + kDigestG);
    acc[3] += digest_mix((h1 ^ v) + kDigestG);
}

// A wave's totals of four terms, in every lane.
__device__ __forceinline__ void digest_wave_sum(uint64_t (&acc)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        unsigned long long x = acc[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        acc[c] = x;
    }
}

// The workgroup's totals added to words[w0 .. w3] (kept, key bytes, sum[0], sum[1]): wave, then
// workgroup, then one atomic per total.  The whole workgroup calls it.
__device__ __forceinline__ void digest_tile_add(uint64_t (&acc)[4], uint64_t (&s_part)[kScanThreads / 64][4],
                                                int64_t* words, int w0, int w1, int w2, int w3) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    digest_wave_sum(acc);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) s_part[wid][c] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t x = 0, kept = 0;
#pragma unroll
        for (int q = 0; q < kScanThreads / 64; q++) x += s_part[q][threadIdx.x], kept += s_part[q][0];
        if (kept != 0) {  // a tile that kept nothing adds nothing
            const int word = threadIdx.x == 0 ? w0 : threadIdx.x == 1 ? w1 : threadIdx.x == 2 ? w2 : w3;
            atomicAdd((unsigned long long*)&words[word], (unsigned long long)x);
        }
    }
}

__global__ __launch_bounds__(kScanThreads) void k_export_digest(ExportArgs a) {
    __shared__ int64_t s_pos[kExpWin];
    __shared__ int64_t s_val[kScanTile + 1];
    __shared__ int64_t s_src[kScanTile];
    __shared__ uint64_t s_part[kScanThreads / 64][4];
    const int64_t m_lo = a.words[kXwLo], n = a.words[kXwHi] - m_lo;
    const int64_t tile = blockIdx.x;
    const int64_t ntiles = n > 0 ? (n + kScanTile - 1) / kScanTile : 1;
    if (tile >= ntiles) return;  // spare tile of the launch sized by both tiers
    export_resolve_tile(a, tile, m_lo, n, s_pos, s_val, s_src, (int*)&a.words[kXwScan] + 1);
    const int64_t rest = n - tile * kScanTile;
    const int cnt = (int)(rest < kScanTile ? rest : kScanTile);
    uint64_t acc[4] = {0, 0, 0, 0};  // kept, key bytes, sum[0], sum[1]
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
        const int e = k * kScanThreads + threadIdx.x;
        if (e >= cnt || s_val[e + 1] == s_val[e]) continue;
        digest_element(a, s_val, s_src, e, acc);
    }
    digest_tile_add(acc, s_part, a.words, kXwN, kXwBytes, kDwSum0, kDwSum1);
}

// ---- partitioned digest (fdbcs_history_digest_ranges; the definition is in include/fdb_conflict_set.h)
//
// K ranges between ascending bounds, digested in one pass over the span they cover.  The canonical
// elements of range i are the canonical elements of the whole span that lie strictly between its two
// bounds, and "H_f changes here" is a property of an element and its predecessor in the stream, so the
// tiles, their resolve step and the keep rule are the single digest's; only where a kept element's
// terms are added differs.  With edge e the e-th bound (edge 0 below every key with an open low end,
// edge K past every key with an open high end):
//   k_digest_ranges_bounds  two lanes per bound (base, delta): the bound is normalized from its bytes
//                    where it is searched, lt[e] / le[e] = stream elements below / at or below it
//                    (plain binary searches over full keys), and range e's header, the clamped value
//                    of element le[e] - 1 (k_export_bounds' rule), goes into its result block.
//   launch_export_head      as it stands, over (first bound, last bound): the span's words, d_pos /
//                    d_val and the tile starts.
//   k_export_digest_ranges  range i owns the stream positions [le[i], lt[i + 1]); elements in
//                    [lt[i], le[i]) equal a bound and belong to no range.  A workgroup looks up the
//                    bins of its first and last element once; when they agree it reduces as
//                    k_export_digest does, into the bin's block.  Otherwise every element finds its
//                    bin among the tile's (positions ascend, so bins do), a wave whose elements share
//                    one reduces by shuffles and adds once, and only a wave that straddles a bound
//                    adds per element.

__device__ __forceinline__ void ranges_bound_key(const DigestRangesArgs& r, int64_t j, DKey& q) {
    const int64_t o = r.offsets[j];
    const uint32_t len = (uint32_t)(r.offsets[j + 1] - o);
    const uint8_t* p = r.bytes + o;
    uint64_t w0 = len ? load8_unaligned(p) : 0ull, w1 = len > 8u ? load8_unaligned(p + 8) : 0ull;
    if (len < 8u) w0 &= (1ull << (8u * len)) - 1ull;
    if (len < 16u) w1 &= len > 8u ? (1ull << (8u * (len - 8u))) - 1ull : 0ull;
    // the first key byte is the lowest of the loaded word and the highest of the prefix word
    q.hi = __builtin_bswap64(w0);
    q.lo = __builtin_bswap64(w1);
    q.len = len;
    q.tail = (uint32_t)(o + 16);  // bytes [16, len) where they lie (tail_cmp reads at any alignment)
}

__global__ __launch_bounds__(kBlock) void k_digest_ranges_bounds(ExportArgs a, DigestRangesArgs r) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = g >> 1;
    const int tier = (int)(g & 1);  // 0 base, 1 delta
    const bool live = j < r.n_bounds;
    int64_t lt = 0, le = 0;
    if (live) {
        DKey q;
        ranges_bound_key(r, j, q);
        const Hist& h = tier ? a.delta : a.base;
        const int64_t n = tier ? a.nd : a.nb;
        lt = tier_bounds_lane(tier, a.base, a.nb, a.delta, a.nd, a.htail, true, true, false,
                              [&](bool, DKey& k, const uint8_t*& t) {
                                  k = q;
                                  t = r.bytes;
                              });
        // a tier's keys ascend strictly: at most one equals the bound
        le = lt + (lt < n && hist_cmp(h, lt, a.htail, q, r.bytes) == 0 ? 1 : 0);
    }
    const int64_t dlt = __shfl_xor(lt, 1, 64), dle = __shfl_xor(le, 1, 64);  // the delta lane's to the base lane
    if (live && tier == 0) {
        const int64_t e = j + r.open_lo;
        r.lt[e] = lt + dlt;
        r.le[e] = le + dle;
        if (e < r.K) {  // H_f at the bound: the last boundary at or below it, the delta's unless a hole
            int64_t h = a.hdr;
            if (le > 0) h = a.base.ver[le - 1];
            if (dle > 0) {
                const int64_t dv = a.delta.ver[dle - 1];
                if (dv != kHole) h = dv;
            }
            r.out[e * kDrWords + kDrHeader] = export_clamp(h, a.floor);
        }
    }
    if (g == 0) {
        if (r.open_lo) {
            r.lt[0] = r.le[0] = 0;
            r.out[kDrHeader] = export_clamp(a.hdr, a.floor);
        }
        if (r.open_hi) r.lt[r.K] = r.le[r.K] = a.nb + a.nd;
    }
}

// The range that owns stream position p among edges [e_lo, e_hi): the last whose le is at or below p
// (e_lo - 1 if none).
__device__ __forceinline__ int64_t ranges_bin(const DigestRangesArgs& r, int64_t e_lo, int64_t e_hi, int64_t p) {
    return first_false<int64_t>(e_lo, e_hi, [&](int64_t e) { return r.le[e] <= p; }) - 1;
}

__global__ __launch_bounds__(kScanThreads) void k_export_digest_ranges(ExportArgs a, DigestRangesArgs r) {
    __shared__ int64_t s_pos[kExpWin];
    __shared__ int64_t s_val[kScanTile + 1];
    __shared__ int64_t s_src[kScanTile];
    __shared__ uint64_t s_part[kScanThreads / 64][4];
    __shared__ int64_t s_bin[2];
    const int64_t m_lo = a.words[kXwLo], n = a.words[kXwHi] - m_lo;
    const int64_t tile = blockIdx.x;
    const int64_t ntiles = n > 0 ? (n + kScanTile - 1) / kScanTile : 1;
    if (tile >= ntiles) return;  // spare tile of the launch sized by both tiers
    export_resolve_tile(a, tile, m_lo, n, s_pos, s_val, s_src, (int*)&a.words[kXwScan] + 1);
    const int64_t rest = n - tile * kScanTile;
    const int cnt = (int)(rest < kScanTile ? rest : kScanTile);
    if (cnt <= 0) return;  // an empty span: the headers are all there is
    const int64_t p0 = m_lo + tile * kScanTile;  // the tile's first stream position
    if (threadIdx.x < 2) s_bin[threadIdx.x] = ranges_bin(r, 0, r.K, threadIdx.x ? p0 + cnt - 1 : p0);
    __syncthreads();
    const int64_t b0 = s_bin[0], b1 = s_bin[1];
    if (b0 < 0 || b1 < b0) {  // the span starts below the first range: the two bound searches disagree
        if (threadIdx.x == 0) atomicOr((int*)&a.words[kXwScan] + 1, 4);
        return;
    }
    if (b0 == b1) {  // one range's tile: the single digest's reduction into that range's block
        const int64_t end = r.lt[b0 + 1] - p0;  // elements from here on equal the next bound
        uint64_t acc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kScanPer; k++) {
            const int e = k * kScanThreads + threadIdx.x;
            if (e >= cnt || e >= end || s_val[e + 1] == s_val[e]) continue;
            digest_element(a, s_val, s_src, e, acc);
        }
        digest_tile_add(acc, s_part, r.out + b0 * kDrWords, kDrN, kDrBytes, kDrSum0, kDrSum1);
        return;
    }
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < kScanPer; k++) {  // every lane takes every round: the shuffles need whole waves
        const int e = k * kScanThreads + threadIdx.x;
        const bool in = e < cnt;
        const int64_t bin = in ? ranges_bin(r, b0, b1 + 1, p0 + e) : -1;
        uint64_t t[4] = {0, 0, 0, 0};
        const bool adds = in && bin >= b0 && s_val[e + 1] != s_val[e] && p0 + e < r.lt[bin + 1];
        if (adds) digest_element(a, s_val, s_src, e, t);
        const int64_t wb = __shfl(bin, 0, 64);  // elements ascend with the lane: lane 0 is outside only if all are
        if (__all(!in || bin == wb)) {
            digest_wave_sum(t);
            if (lane == 0 && t[0] != 0) {
                unsigned long long* o = (unsigned long long*)(r.out + wb * kDrWords);
                atomicAdd(&o[kDrN], (unsigned long long)t[0]);
                atomicAdd(&o[kDrBytes], (unsigned long long)t[1]);
                atomicAdd(&o[kDrSum0], (unsigned long long)t[2]);
                atomicAdd(&o[kDrSum1], (unsigned long long)t[3]);
            }
        } else if (adds) {
            unsigned long long* o = (unsigned long long*)(r.out + bin * kDrWords);
            atomicAdd(&o[kDrN], (unsigned long long)t[0]);
            atomicAdd(&o[kDrBytes], (unsigned long long)t[1]);
            atomicAdd(&o[kDrSum0], (unsigned long long)t[2]);
            atomicAdd(&o[kDrSum1], (unsigned long long)t[3]);
        }
    }
}

int64_t export_tiles(int64_t n) { return n > 0 ? (n + kScanTile - 1) / kScanTile : 1; }

// The launches the export and the digest share: every delta boundary's stream position and value, the
// stream positions of lo and hi with the header, and every tile's first delta boundary.
static int64_t launch_export_head(hipStream_t s, const ExportArgs& a, const MaxLevels& basem, int mode) {
    if (a.nd > 0) {
        const dim3 grid((unsigned)((a.nd + kBlock - 1) / kBlock));
        fdb_launch(search_mode_kernel(mode, k_export_search<1>, k_export_search<2>), grid, dim3(kBlock), 0, s, a.base,
                   basem, a.delta, a.htail, a.nb, a.nd, a.hdr, a.d_pos, a.d_val);
    }
    fdb_launch(k_export_bounds, dim3(1), dim3(64), 0, s, a);
    const int64_t tiles = export_tiles(a.nb + a.nd);
    fdb_launch(k_export_tile_starts, dim3((unsigned)((tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    return tiles;
}

void launch_export(hipStream_t s, const ExportArgs& a, const MaxLevels& basem, uint64_t* granules, int mode) {
    const int64_t tiles = launch_export_head(s, a, basem, mode);
    ScanState st;
    st.granules = granules;
    st.counter = (int*)&a.words[kXwScan];
    st.error = st.counter + 1;
    fdb_launch(k_export_scan, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, a, st);
}

void launch_export_digest(hipStream_t s, const ExportArgs& a, const MaxLevels& basem, int mode) {
    const int64_t tiles = launch_export_head(s, a, basem, mode);
    fdb_launch(k_export_digest, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, a);
}

void launch_export_digest_ranges(hipStream_t s, const ExportArgs& a, const DigestRangesArgs& r, const MaxLevels& basem,
                                 int mode) {
    const int64_t lanes = std::max<int64_t>(1, 2 * (int64_t)r.n_bounds);
    fdb_launch(k_digest_ranges_bounds, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, r);
    const int64_t tiles = launch_export_head(s, a, basem, mode);
    fdb_launch(k_export_digest_ranges, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, a, r);
}

// ---- split keys (fdbcs_history_split_keys; the definition is in include/fdb_conflict_set.h)
//
// Up to `want` boundary keys strictly inside (lo, hi), taken at evenly spaced positions of the tier
// that holds more boundaries there.  Read-only; two launches with a host read between them, which
// sizes the key buffer:
//   k_split_plan    one workgroup: the bounds' positions in both tiers (k_export_bounds' searches), the
//                   tier, the count n and the picked boundaries' byte offsets (each thread sums the
//                   lengths of a contiguous share of the picks, the shares are scanned in LDS)
//   k_split_gather  one lane per picked boundary: its original bytes by export_put_key

// Pick k of n among c boundaries: the middle of the k-th of n equal shares (strictly ascending for n <= c).
__device__ __forceinline__ int64_t split_pick(int64_t k, int64_t n, int64_t c) { return ((2 * k + 1) * c) / (2 * n); }

__global__ __launch_bounds__(kBlock) void k_split_plan(SplitArgs a) {
    __shared__ int64_t r[4];  // boundaries <= lo in base, delta; boundaries < hi in base, delta
    __shared__ int64_t s_sum[kBlock];
    const int t = threadIdx.x;
    if (t < 4)
        r[t] = tier_bounds_lane(t, a.base, a.nb, a.delta, a.nd, a.htail, a.has_lo, a.has_hi, true,
                                [&](bool is_hi, DKey& q, const uint8_t*& qtail) {
                                    q = is_hi ? a.hi : a.lo;
                                    qtail = a.btail;
                                });
    __syncthreads();
    const int64_t cb = r[2] > r[0] ? r[2] - r[0] : 0, cd = r[3] > r[1] ? r[3] - r[1] : 0;
    const int tier = cd > cb ? 1 : 0;
    const int64_t first = tier ? r[1] : r[0], c = tier ? cd : cb;
    const int64_t n = a.want < c ? a.want : c;
    const Hist& h = tier ? a.delta : a.base;
    // thread t owns picks [k0, k1)
    const int64_t per = (n + kBlock - 1) / kBlock;
    const int64_t k0 = t * per < n ? t * per : n, k1 = k0 + per < n ? k0 + per : n;
    int64_t sum = 0;
    for (int64_t k = k0; k < k1; k++) sum += h.lt[first + split_pick(k, n, c)].x;
    s_sum[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int q = 0; q < kBlock; q++) {
            const int64_t x = s_sum[q];
            s_sum[q] = run;
            run += x;
        }
        a.words[kSwN] = n;
        a.words[kSwBytes] = run;
        a.words[kSwTier] = tier;
        a.words[kSwFirst] = first;
        a.words[kSwCount] = c;
        a.offsets[n] = run;
    }
    __syncthreads();
    int64_t off = s_sum[t];
    for (int64_t k = k0; k < k1; k++) {
        a.offsets[k] = off;
        off += h.lt[first + split_pick(k, n, c)].x;
    }
}

__global__ __launch_bounds__(kBlock) void k_split_gather(SplitArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = a.words[kSwN], c = a.words[kSwCount];
    if (k >= n || k >= a.want) return;
    const Hist& h = a.words[kSwTier] ? a.delta : a.base;
    const int64_t p = a.words[kSwFirst] + split_pick(k, n, c);
    const ulonglong2 key = h.key[p];
    const uint2 lt = h.lt[p];
    const int64_t P = a.offsets[k];
    if (P < 0 || P + (int64_t)lt.x > a.bytes_cap) {  // never past the buffer the host sized from the plan
        atomicOr((int*)&a.words[kSwError], 8);
        return;
    }
    // the prefix words are big-endian: swapped back, the key's first byte is the lowest
    const uint64_t w0 = __builtin_bswap64(key.x), w1 = __builtin_bswap64(key.y);
    const uint64_t* tw = (const uint64_t*)hist_tail(a.htail, lt.x > 16u ? lt.y : 0u);
    export_put_key(a.bytes + P, lt.x, (lt.x + 7u) >> 3,
                   [&](uint32_t q) { return q == 0u ? w0 : q == 1u ? w1 : tw[q - 2u]; });
}

void launch_split_plan(hipStream_t s, const SplitArgs& a) { fdb_launch(k_split_plan, dim3(1), dim3(kBlock), 0, s, a); }

void launch_split_gather(hipStream_t s, const SplitArgs& a, int64_t n) {
    if (n > 0) fdb_launch(k_split_gather, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
}

// ------------------------------------------------------------------ iops sample
//
// The resolver's iopsSample (Resolver.actor.cpp:178-192) of a routed batch: the begin key of every
// range the resolver kept, TooOld sub-transactions' included, is rolled with
// TransientStorageMetricSample::add's odds (StorageMetrics.actor.h: metric / metricUnitsPerSample,
// a metric at or above the unit always) and the sampled ones are handed to the host.  The roll is a
// counter-based one, so that the host can restate it bit for bit (balancing.iops_roll): range i
// (read r: r, write w: R + w) under the caller's seed takes the top 32 bits u of splitmix64's
// finalizer over seed + 0x9E3779B97F4A7C15 (i + 1) and is sampled iff u * units < metric << 32.
// One launch: a look-back scan with one element per thread (a kept element's store is a chain of
// dependent loads, as the other gather scans') over two counters, the kept ranges and their key
// bytes (32-bit: the host refuses capacities whose keys could pass 2^32 bytes).  R and W come from
// the routing's device result; the grid is sized by the capacities, spare tiles leave at once.

__device__ __forceinline__ uint32_t iops_mix(uint64_t seed, uint64_t i) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}

struct IopsScan {
    IopsArgs a;
    int* err;
    static constexpr bool kOwn = true;
    // [0] sampled ranges, [1] their begin keys' bytes
    __device__ void load(int64_t i, uint32_t (&v)[2]) const {
        const uint32_t len = a.keys[2 * i].len;
        const uint64_t metric = kIopsOffsetPerKey + (uint64_t)len;
        const bool hit = metric >= a.units || (uint64_t)iops_mix(a.seed, (uint64_t)i) * a.units < (metric << 32);
        v[0] = hit ? 1u : 0u;
        v[1] = hit ? len : 0u;
    }
    __device__ void store(int64_t i, const uint32_t (&ex)[2], const uint32_t (&own)[2]) const {
        if (!own[0]) return;
        const int64_t o = ex[0], P = ex[1];
        const DKey k = a.keys[2 * i];
        const uint64_t metric = kIopsOffsetPerKey + (uint64_t)k.len;
        a.metrics[o] = (int32_t)(metric >= a.units ? metric : a.units);
        a.index[o] = (int32_t)i;
        a.key_offsets[o] = P;
        if (P + (int64_t)k.len > a.bytes_cap) {  // never past the result buffer (the host sized it for every key)
            atomicOr(err, 8);
            return;
        }
        // the prefix words are big-endian: swapped back, the key's first byte is the lowest; the
        // tail starts at any byte of the batch's arena (k_route_write packs them), so a tail word is
        // an unaligned load (the arena's slack covers its second word)
        const uint64_t w0 = __builtin_bswap64(k.hi), w1 = __builtin_bswap64(k.lo);
        const uint8_t* tp = a.tail + (k.len > 16u ? k.tail : 0u);
        export_put_key(a.bytes + P, k.len, (k.len + 7u) >> 3, [&](uint32_t q) {
            return q == 0u ? w0 : q == 1u ? w1 : load8_unaligned(tp + 8u * (q - 2u));
        });
    }
    __device__ void finish(const uint32_t (&tot)[2]) const {
        a.key_offsets[tot[0]] = tot[1];
        a.totals->n = tot[0];
        a.totals->key_bytes = tot[1];
    }
};

__global__ __launch_bounds__(kScanThreads) void k_iops_sample(IopsArgs a, ScanState st) {
    __shared__ uint32_t sv[2][scan_pad(kIopsScanP)];
    __shared__ uint32_t swave[2][kScanThreads / 64];
    __shared__ uint32_t sbase[2];
    __shared__ int s_tile;
    // a routing that reported an error placed nothing usable: an empty sample
    const RouteResult res = *a.dres;
    int64_t n = res.error ? 0 : (int64_t)res.R + res.W;
    if (n > a.cap) n = a.cap;  // (the routing reports an error past the capacities: never taken)
    if (threadIdx.x == 0) s_tile = atomicAdd(st.counter, 1);
    __syncthreads();
    const int tile = s_tile;
    const int64_t ntiles = n > 0 ? (n + kIopsTile - 1) / kIopsTile : 1;
    if (tile >= ntiles) return;  // spare tile of the capacity-sized launch: nobody waits on it
    const IopsScan f{a, st.error};
    scan_tile<2, IopsScan, kIopsScanP>(f, n, tile, ntiles, st, sv, swave, sbase);
}

int64_t iops_scan_words(int64_t cap) { return 8 + scan_granules(cap, 2, kIopsScanP); }

void launch_iops_sample(hipStream_t s, const IopsArgs& a, ScanState st) {
    const int64_t tiles = std::max<int64_t>(1, (a.cap + kIopsTile - 1) / kIopsTile);
    fdb_launch(k_iops_sample, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, a, st);
}

// ------------------------------------------------------------------ history import
//
// H'(k) = max(H(k), I(k)) for lo <= k < hi and H(k) elsewhere, I the step function of the imported
// arrays (the export's layout).  The import becomes a third stream shaped like the delta tier, the
// overlay: a boundary at lo carrying I(lo), the imported boundaries inside (lo, hi), a boundary at
// hi carrying kHole (no lo: the overlay's header is the imported header; no hi: no closing hole).
// With H the two tiers' value, H' = overlay == kHole ? H : max(H, overlay) at every key.
//   k_import_check      one lane per imported boundary: offsets inside the byte array, lengths not
//                       negative, neighbours strictly ascending (full byte compare) -> error word
//   k_import_bounds     imported boundaries <= lo and < hi (plain binary searches), overlay size
//   k_import_normalize  one lane per overlay boundary: big-endian prefix words, (len, tail unit),
//                       version, and the bytes past 16 as zero-padded 8-byte words (the inverse of
//                       export_put_key; source keys start at any byte).  Tail units need no scan:
//                       imported boundary j owns unit (offsets[j] >> 3) + j, which never overlaps
//                       its neighbours' and wastes at most 15 bytes per key of scratch.
//   k_import_rank<S>    one lane per element of stream S inside an ImportWindow (this import: the
//                       whole streams, no closing boundary): its lower bounds in the other two's
//                       windows give its position in the merged order (on equal keys delta,
//                       overlay, base) and all three streams' values at its key, hence H'.  Values
//                       come from the whole tiers (the boundary covering a window's first key may
//                       lie before it); the searches are plain binary searches over the windows.
//                       Later elements of a tie repeat their predecessor's value, so no case is
//                       special.  The element's prefix words, (len, tail unit) and H' go to its
//                       merged position.  Base boundaries (S = 0, launched last) search no keys:
//                       their ranks follow from the lower bounds the other two streams' elements
//                       found in the base.
//   k_scan<ImportFold>  flags value changes along the merged stream, scans (kept, tail units) with
//                       the look-back and writes the kept boundaries into the non-current base
//                       buffer, their tails packed into the non-current arena; every read of the
//                       merged stream is coalesced.
// Nothing current is written: the host switches buffers after reading the result words.

// memcmp-then-length order of two byte strings at any alignment, 8 bytes per step.
__device__ __forceinline__ int import_cmp(const uint8_t* a, uint32_t al, const uint8_t* b, uint32_t bl) {
    const uint32_t n = al < bl ? al : bl;
    uint32_t i = 0;
    for (; i + 8u <= n; i += 8u) {
        const uint64_t x = tail_word(a + i), y = tail_word(b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    if (i < n) {
        const uint64_t msk = ~0ull << (64u - 8u * (n - i));
        const uint64_t x = tail_word(a + i) & msk, y = tail_word(b + i) & msk;
        if (x != y) return x < y ? -1 : 1;
    }
    return (al > bl) - (al < bl);
}

// Imported boundary j's bytes; false (and an empty key) unless its offsets lie inside the byte array.
__device__ __forceinline__ bool import_key(const ImportArgs& a, int64_t j, const uint8_t*& p, uint32_t& len) {
    const int64_t o0 = a.offsets[j], o1 = a.offsets[j + 1];
    p = a.bytes;
    len = 0;
    if (o0 < 0 || o1 < o0 || o1 > a.nbytes || o1 - o0 > (int64_t)INT32_MAX) return false;
    p = a.bytes + o0;
    len = (uint32_t)(o1 - o0);
    return true;
}

__global__ __launch_bounds__(kBlock) void k_import_check(ImportArgs a) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    const uint8_t *p, *q;
    uint32_t pl, ql;
    bool ok = import_key(a, j, p, pl);
    if (j == 0) {
        ok = ok && a.offsets[0] == 0;
    } else if (ok) {
        ok = import_key(a, j - 1, q, ql) && import_cmp(q, ql, p, pl) < 0;
    }
    if (!ok) atomicOr((int*)&a.words[kIwError], 1);
}

__global__ __launch_bounds__(64) void k_import_bounds(ImportArgs a) {
    __shared__ int64_t r[2];  // imported boundaries <= lo, < hi
    const int t = threadIdx.x;
    if (t < 2) {
        const bool is_hi = t == 1;
        if (!(is_hi ? a.has_hi : a.has_lo)) {
            r[t] = is_hi ? a.n : 0;
        } else {
            const uint8_t* b = a.bnd + (is_hi ? a.bnd_hi : 0);
            const uint32_t bl = (uint32_t)(is_hi ? a.hi_len : a.lo_len);
            r[t] = first_false<int64_t>(0, a.n, [&](int64_t j) {
                const uint8_t* p;
                uint32_t pl;
                import_key(a, j, p, pl);
                const int c = import_cmp(p, pl, b, bl);
                return c < 0 || (!is_hi && c == 0);
            });
        }
    }
    __syncthreads();
    if (t != 0) return;
    const int64_t inner = r[1] > r[0] ? r[1] - r[0] : 0;
    a.words[kIwJlo] = r[0];
    a.words[kIwM] = (a.has_lo ? 1 : 0) + inner + (a.has_hi ? 1 : 0);
}

__global__ __launch_bounds__(kBlock) void k_import_normalize(ImportArgs a) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = a.words[kIwM], jlo = a.words[kIwJlo];
    if (e >= m || e >= a.n + 2) return;
    const uint8_t* p;
    uint32_t len;
    int64_t ver, unit;
    if (a.has_lo && e == 0) {  // the range's first boundary carries I(lo)
        p = a.bnd;
        len = (uint32_t)a.lo_len;
        ver = jlo > 0 ? a.versions[jlo - 1] : a.ihdr;
        unit = a.otail_lo;
    } else if (a.has_hi && e == m - 1) {  // the synthetic boundary that closes the range
        p = a.bnd + a.bnd_hi;
        len = (uint32_t)a.hi_len;
        ver = kHole;
        unit = a.otail_hi;
    } else {
        const int64_t j = jlo + e - (a.has_lo ? 1 : 0);
        if (j < 0 || j >= a.n || !import_key(a, j, p, len)) {
            atomicOr((int*)&a.words[kIwError], 1);
            return;
        }
        ver = a.versions[j];
        unit = (a.offsets[j] >> 3) + j;
    }
    uint64_t w0 = len ? load8_unaligned(p) : 0ull, w1 = len > 8u ? load8_unaligned(p + 8) : 0ull;
    if (len < 8u) w0 &= (1ull << (8u * len)) - 1ull;
    if (len < 16u) w1 &= len > 8u ? (1ull << (8u * (len - 8u))) - 1ull : 0ull;
    // the first key byte is the lowest of the loaded word and the highest of the prefix word
    a.ov.key[e] = make_ulonglong2(__builtin_bswap64(w0), __builtin_bswap64(w1));
    a.ov.lt[e] = make_uint2(len, len > 16u ? (uint32_t)unit : 0u);
    a.ov.ver[e] = ver;
    if (len > 16u) {
        const uint32_t nt = len - 16u, nu = (nt + 7u) >> 3;
        uint64_t* d = (uint64_t*)hist_tail(a.otail, (uint32_t)unit);
        for (uint32_t u = 0; u < nu; u++) {
            uint64_t w = load8_unaligned(p + 16u + 8u * u);
            const uint32_t left = nt - 8u * u;
            if (left < 8u) w &= (1ull << (8u * left)) - 1ull;  // zero padded
            d[u] = w;
        }
    }
}

// Boundaries of h[lo, hi) below q counted from 0 (the answer lies in [lo, hi]), and whether the
// next one equals it.
__device__ __forceinline__ int64_t impd_lower(const Hist& h, int64_t lo, int64_t hi, const uint8_t* arena,
                                              const DKey& q, const uint8_t* qtail, bool& exact) {
    const int64_t lb = first_false(lo, hi, [&](int64_t i) { return hist_cmp(h, i, arena, q, qtail) < 0; });
    exact = lb < hi && hist_cmp(h, lb, arena, q, qtail) == 0;
    return lb;
}

constexpr uint32_t kImportOvTail = 1u << 31;  // ImportArgs::m_lt len bit: the tail is in the overlay's arena

// S: the stream of this launch's elements (0 base, 1 delta, 2 overlay), one lane per boundary inside
// the window; with a closing boundary the overlay's launch has one more lane for it.
template <int S>
__global__ __launch_bounds__(kBlock) void k_import_rank(ImportArgs a, ImportWindow w) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ndr = w.p_hi - w.p_lo, nbr = w.q_hi - w.q_lo;
    if (i0 >= (S == 0 ? nbr : S == 1 ? ndr : w.mr + w.closing)) return;
    if (S == 2 && i0 == w.mr) {  // the closing boundary: hi's key, the delta's old value there
        const uint2 lt = a.ov.lt[i0];
        a.m_val[w.R] = w.e_ver;
        a.m_key[w.R] = a.ov.key[i0];
        a.m_lt[w.R] = make_uint2(lt.x | kImportOvTail, lt.x > 16u ? lt.y : 0u);
        return;
    }
    const int64_t i = i0 + (S == 0 ? w.q_lo : S == 1 ? w.p_lo : 0);
    const Hist& h = S == 0 ? a.base : S == 1 ? a.delta : a.ov;
    const ulonglong2 k = h.key[i];
    const uint2 lt = h.lt[i];
    DKey q;
    const uint8_t* qtail;
    tier_query(h, i, S == 2 ? a.otail : a.htail, q, qtail);
    // boundaries below the key (lt) and at or below it (le) in each stream, counted over the whole stream
    int64_t b_lt = i, b_le = i + 1, d_lt = i, d_le = i + 1, v_lt = i, v_le = i + 1;
    [[maybe_unused]] bool ex;
    if constexpr (S == 0) {
        // a base boundary's ranks in the other two streams follow from their elements' lower bounds
        // in the base (k_import_rank<1>, <2> ran first): the in-window delta boundaries at or below
        // base key i are those with at most i base boundaries below them.  A search over a dense
        // ascending array of integers, no key compares.
        d_le = first_false(w.p_lo, w.p_hi, [&](int64_t j) { return a.d_blt[j] <= i; });
        v_le = first_false<int64_t>(0, w.mr, [&](int64_t e) { return a.v_blt[e] <= i; });
    } else {
        b_lt = impd_lower(a.base, w.q_lo, w.q_hi, a.htail, q, qtail, ex);
        b_le = b_lt + (ex ? 1 : 0);
        (S == 1 ? a.d_blt : a.v_blt)[i] = b_lt;
    }
    if constexpr (S == 2) {
        d_lt = impd_lower(a.delta, w.p_lo, w.p_hi, a.htail, q, qtail, ex);
        d_le = d_lt + (ex ? 1 : 0);
    }
    if constexpr (S == 1) {
        v_lt = impd_lower(a.ov, 0, w.mr, a.otail, q, qtail, ex);
        v_le = v_lt + (ex ? 1 : 0);
    }
    // on equal keys: delta, then overlay, then base; positions count from the window's start
    const int64_t pos = S == 1   ? (d_lt - w.p_lo) + v_lt + (b_lt - w.q_lo)
                        : S == 2 ? v_lt + (d_le - w.p_lo) + (b_lt - w.q_lo)
                                 : (b_lt - w.q_lo) + (d_le - w.p_lo) + v_le;
    const int64_t dv = d_le > 0 ? a.delta.ver[d_le - 1] : kHole;
    const int64_t bv = b_le > 0 ? a.base.ver[b_le - 1] : a.hdr;
    const int64_t ov = v_le > 0 ? a.ov.ver[v_le - 1] : a.ovhdr;
    int64_t v = dv != kHole ? dv : bv;
    if (ov != kHole && ov > v) v = ov;
    if (pos < 0 || pos >= w.R) {  // streams out of order: never index past the merged arrays
        atomicOr(w.error, 4);
        return;
    }
    a.m_val[pos] = v;
    a.m_key[pos] = k;
    a.m_lt[pos] = make_uint2(lt.x | (S == 2 ? kImportOvTail : 0u), lt.x > 16u ? lt.y : 0u);
}

struct ImportFold {
    ImportArgs a;
    __device__ bool keep(int64_t p) const { return a.m_val[p] != (p ? a.m_val[p - 1] : a.new_hdr); }
    // [0] kept boundaries, [1] their tail units (offsets in the new arena)
    __device__ void load(int64_t p, uint32_t (&x)[2]) const {
        const bool kp = keep(p);
        x[0] = kp ? 1u : 0u;
        x[1] = kp ? tail_units(a.m_lt[p].x & ~kImportOvTail) : 0u;
    }
    __device__ void store(int64_t p, const uint32_t (&ex)[2]) const {
        if (!keep(p)) return;
        uint2 lt = a.m_lt[p];
        const bool ovt = (lt.x & kImportOvTail) != 0;
        lt.x &= ~kImportOvTail;
        const int64_t o = ex[0], v = a.m_val[p];
        const uint32_t nu = tail_units(lt.x);
        if (o >= a.dst_cap || (int64_t)ex[1] + nu > a.tdst_units) {  // never past the buffers the host sized
            atomicOr((int*)&a.words[kIwError], 8);
            return;
        }
        if (nu) {
            const uint8_t* arena = a.htail;
            if (ovt) arena = a.otail;
            const uint64_t* src = (const uint64_t*)hist_tail(arena, lt.y);
            uint64_t* d = (uint64_t*)hist_tail(a.tdst, ex[1]);
            for (uint32_t u = 0; u < nu; u++) d[u] = src[u];
        }
        lt.y = nu ? ex[1] : 0u;
        a.dst.key[o] = a.m_key[p];
        a.dst.lt[o] = lt;
        a.dst.ver[o] = v;
    }
    __device__ void finish(const uint32_t (&tot)[2]) const {
        a.words[kIwKept] = tot[0];
        a.words[kIwTailUnits] = tot[1];
    }
};

// The greatest version of a tier from the top level of its range-max hierarchy (every wave of the
// rebuild raised one of its words; unused words hold LLONG_MIN), into *out by atomicMax.
__global__ __launch_bounds__(kBlock) void k_import_max(const int64_t* lvl3, int64_t words, int64_t* out) {
    long long x = LLONG_MIN;
    for (int64_t i = threadIdx.x; i < words; i += blockDim.x) {
        const long long y = lvl3[i * kL3Pad];
        x = y > x ? y : x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    if ((threadIdx.x & 63) == 0 && x != LLONG_MIN) atomicMax((long long*)out, x);
}

void launch_import_max(hipStream_t s, const MaxLevels& m, int64_t lvl3_n, int64_t* out) {
    fdb_launch(k_import_max, dim3(1), dim3(kBlock), 0, s, (const int64_t*)m.lvl[3], lvl3_n * kL3Rep, out);
}

void launch_import_overlay(hipStream_t s, const ImportArgs& a) {
    if (a.n > 0) fdb_launch(k_import_check, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    fdb_launch(k_import_bounds, dim3(1), dim3(64), 0, s, a);
    fdb_launch(k_import_normalize, dim3((unsigned)((a.n + 2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
}

// The rank launches of either import: delta, overlay, then base (it reads d_blt, v_blt).
static void launch_import_rank(hipStream_t s, const ImportArgs& a, const ImportWindow& w) {
    auto grid = [](int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); };
    const int64_t ndr = w.p_hi - w.p_lo, nv = w.mr + w.closing, nbr = w.q_hi - w.q_lo;
    if (ndr > 0) fdb_launch(k_import_rank<1>, grid(ndr), dim3(kBlock), 0, s, a, w);
    if (nv > 0) fdb_launch(k_import_rank<2>, grid(nv), dim3(kBlock), 0, s, a, w);
    if (nbr > 0) fdb_launch(k_import_rank<0>, grid(nbr), dim3(kBlock), 0, s, a, w);
}

void launch_import_fold(hipStream_t s, const ImportArgs& a, int64_t m, uint64_t* granules) {
    ImportWindow w{};  // the whole streams, no closing boundary
    w.p_hi = a.nd;
    w.q_hi = a.nb;
    w.mr = m;
    w.R = a.nb + a.nd + m;
    w.error = (int*)&a.words[kIwError];
    launch_import_rank(s, a, w);
    ScanState st;
    st.granules = granules;
    st.counter = (int*)&a.words[kIwScan];
    st.error = st.counter + 1;
    launch_scan<2>(s, ImportFold{a}, (const int64_t*)nullptr, a.nb + a.nd + m, st);
}

// ------------------------------------------------------------------ history import into the delta tier
//
// The same H' as above, written as delta boundaries over [lo, hi) instead of a new base: the work is
// O(boundaries of the three streams inside the range + size of the delta), whatever the base holds.
// Inside the range the new delta carries H' at every key where a stream has a boundary, base
// boundaries included (equal neighbours coalesced), so no delta entry at an imported version spans a
// base boundary of a greater one (the delta invariant: a delta version is kHole or at least every
// base version it covers).  The boundary at lo is always written; at hi a closing boundary carries
// what the delta held there before (as the E of a batch merge), unless the delta has a boundary at
// hi.  Outside the range the delta is copied as it is.
//   k_impd_bounds     positions of lo and hi in the base and in the delta (plain binary searches,
//                     full key compare), the delta's value at hi
//   k_import_rank<S>  the fold's kernel over the windows k_impd_bounds found: one lane per boundary of
//                     stream S inside the range, log2(range) search steps instead of log2(tier)
//                     (the base's directory, lane_lower_bound, is not used: an in-range search is
//                     already short).  The overlay's launch has one more lane, which puts the
//                     closing boundary at position R.
//   k_scan<ImportDeltaFold>  flags value changes along the in-range stream, scans (kept, tail units
//                     of kept overlay keys) on granules of the import's own and writes the kept
//                     boundaries into the non-current delta buffer from p_lo on, one lane each.
//                     Base and delta boundaries keep their tail offsets (the arena is shared);
//                     kept overlay keys longer than 16 bytes append theirs past tail_used.
//   k_impd_copy       the delta's prefix [0, p_lo) as it is and its suffix [p_hi, nd) shifted behind
//                     the kept boundaries, grid-stride.
// The greatest version is read off the rebuilt delta's top level (k_import_max), never per element.

__global__ __launch_bounds__(64) void k_impd_bounds(ImportDeltaArgs d) {
    const ImportArgs& a = d.a;
    __shared__ int64_t r[4];  // boundaries below lo in base, delta; below hi in base, delta
    const int t = threadIdx.x;
    const int64_t m = a.words[kIwM];
    // an invalid import leaves nothing to place (the host refuses it after reading the words)
    const bool ok = a.words[kIwError] == 0 && m >= (a.has_lo ? 1 : 0) + (a.has_hi ? 1 : 0) && m <= a.n + 2;
    if (t < 4)
        r[t] = tier_bounds_lane(t, a.base, a.nb, a.delta, a.nd, a.htail, ok && a.has_lo, ok && a.has_hi, false,
                                [&](bool is_hi, DKey& q, const uint8_t*& qtail) {
                                    tier_query(a.ov, is_hi ? m - 1 : 0, a.otail, q, qtail);
                                });
    __syncthreads();
    if (t != 0) return;
    const int64_t q_lo = r[0], p_lo = r[1], q_hi = r[2] > r[0] ? r[2] : r[0], p_hi = r[3] > r[1] ? r[3] : r[1];
    int64_t skip = 0;
    if (ok && a.has_hi && p_hi < a.nd) {
        DKey q;
        const uint8_t* qtail;
        tier_query(a.ov, m - 1, a.otail, q, qtail);
        skip = hist_cmp(a.delta, p_hi, a.htail, q, qtail) == 0 ? 1 : 0;
    }
    d.dwords[kIdPlo] = p_lo;
    d.dwords[kIdPhi] = p_hi;
    d.dwords[kIdQlo] = q_lo;
    d.dwords[kIdQhi] = q_hi;
    d.dwords[kIdEver] = p_hi > 0 ? a.delta.ver[p_hi - 1] : kHole;
    d.dwords[kIdEskip] = skip;
}

struct ImportDeltaFold {
    ImportDeltaArgs d;
    __device__ bool keep(int64_t p) const {
        const ImportArgs& a = d.a;
        if (p == d.w.R && d.e_skip) return false;  // the delta's own boundary at hi follows
        // the boundary at lo always stands; without a lower bound the delta's implicit header is a hole
        if (p == 0) return a.has_lo || a.m_val[0] != kHole;
        return a.m_val[p] != a.m_val[p - 1];
    }
    // [0] kept boundaries, [1] tail units appended to the arena (kept overlay keys only)
    __device__ void load(int64_t p, uint32_t (&x)[2]) const {
        const bool kp = keep(p);
        const uint32_t len = d.a.m_lt[p].x;
        x[0] = kp ? 1u : 0u;
        x[1] = kp && (len & kImportOvTail) ? tail_units(len & ~kImportOvTail) : 0u;
    }
    __device__ void store(int64_t p, const uint32_t (&ex)[2]) const {
        if (!keep(p)) return;
        const ImportArgs& a = d.a;
        uint2 lt = a.m_lt[p];
        const bool ovt = (lt.x & kImportOvTail) != 0;
        lt.x &= ~kImportOvTail;
        const int64_t o = d.w.p_lo + (int64_t)ex[0];
        const uint32_t nu = ovt ? tail_units(lt.x) : 0u;
        const int64_t unit = d.tail_base + (int64_t)ex[1];
        if (o >= a.dst_cap || unit + nu > a.tdst_units) {  // never past the buffers the host sized
            atomicOr((int*)&d.dwords[kIdError], 8);
            return;
        }
        if (nu) {  // past tail_used: invisible until the host raises it
            const uint64_t* src = (const uint64_t*)hist_tail(a.otail, lt.y);
            uint64_t* dst = (uint64_t*)(a.tdst + 8 * (size_t)unit);
            for (uint32_t u = 0; u < nu; u++) dst[u] = src[u];
            lt.y = (uint32_t)unit;
        }
        a.dst.key[o] = a.m_key[p];
        a.dst.lt[o] = lt;
        a.dst.ver[o] = a.m_val[p];
    }
    __device__ void finish(const uint32_t (&tot)[2]) const {
        d.dwords[kIdKept] = tot[0];
        d.dwords[kIdTailUnits] = tot[1];
    }
};

__global__ __launch_bounds__(kBlock) void k_impd_copy(ImportDeltaArgs d) {
    const ImportArgs& a = d.a;
    const int64_t kept = d.dwords[kIdKept];
    const int64_t n = a.nd - (d.w.p_hi - d.w.p_lo);  // boundaries outside the range
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool pre = i < d.w.p_lo;
        const int64_t src = pre ? i : d.w.p_hi + (i - d.w.p_lo), dst = pre ? i : i + kept;
        if (dst < 0 || dst >= a.dst_cap) {
            atomicOr((int*)&d.dwords[kIdError], 8);
            continue;
        }
        a.dst.key[dst] = a.delta.key[src];
        a.dst.lt[dst] = a.delta.lt[src];
        a.dst.ver[dst] = a.delta.ver[src];
    }
}

void launch_import_delta_bounds(hipStream_t s, const ImportDeltaArgs& d) {
    fdb_launch(k_impd_bounds, dim3(1), dim3(64), 0, s, d);
}

void launch_import_delta_merge(hipStream_t s, const ImportDeltaArgs& d, uint64_t* granules) {
    ImportWindow w = d.w;
    w.error = (int*)&d.dwords[kIdError];
    launch_import_rank(s, d.a, w);
    ScanState st;
    st.granules = granules;
    st.counter = (int*)&d.dwords[kIdScan];
    st.error = st.counter + 1;
    const int64_t total = w.R + w.closing;
    if (total > 0) launch_scan<2>(s, ImportDeltaFold{d}, (const int64_t*)nullptr, total, st);
    const int64_t outside = d.a.nd - (w.p_hi - w.p_lo);
    if (outside > 0) {
        const int64_t g = (outside + kBlock - 1) / kBlock;
        fdb_launch(k_impd_copy, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(kBlock), 0, s, d);
    }
}

// ------------------------------------------------------------------ read versions
//
// V_r of every read of an uploaded batch against an idle set (fdbcs_batch_read_versions; the
// definition is in include/fdb_conflict_set.h): the greatest clamped version H_f(k) over the read's
// keys, or for a degenerate read [b, b) the version just below b.  The lookups are the read check's
// (kernels.hip check_read_lanes: four lanes per read, begin and end key in the base and the delta
// tier, the begin lane taking the end's position by a shuffle); what follows them is not: a range
// maximum with no snapshot to stop at, so every level entry the span touches is read and a stale or
// missed one shows as a wrong number.  Reads the batch's keys and the tiers, writes one word per
// read; no snapshot, flag, write or workspace of the batch plays a part.

// Entry i of a tier's top level: the max over its kL3Rep replicas (kernels.hip l3_at).
__device__ __forceinline__ int64_t l3_entry(const int64_t* a, int64_t i) {
    int64_t v[kL3Rep];
#pragma unroll
    for (int r = 0; r < kL3Rep; r++) v[r] = a[(i * kL3Rep + r) * kL3Pad];
    int64_t best = v[0];
#pragma unroll
    for (int r = 1; r < kL3Rep; r++) best = v[r] > best ? v[r] : best;
    return best;
}

// max(best, a[lo, hi)), four independent loads per round.
__device__ __forceinline__ int64_t span_max(const int64_t* a, int64_t lo, int64_t hi, int64_t best) {
    int64_t i = lo;
    for (; i + 4 <= hi; i += 4) {
        const int64_t v0 = a[i], v1 = a[i + 1], v2 = a[i + 2], v3 = a[i + 3];
        const int64_t m0 = v0 > v1 ? v0 : v1, m1 = v2 > v3 ? v2 : v3;
        const int64_t m = m0 > m1 ? m0 : m1;
        best = m > best ? m : best;
    }
    for (; i < hi; i++) {
        const int64_t v = a[i];
        best = v > best ? v : best;
    }
    return best;
}

// The exact max of lvl[0][lo, hi) through the 64-ary hierarchy (LLONG_MIN for an empty span): per
// level the entries before the first and after the last whole block, the whole blocks one level up;
// a span of at most two blocks, or what reaches the top level, entry by entry.
__device__ __forceinline__ int64_t range_max_full(const MaxLevels& m, int64_t lo, int64_t hi) {
    int64_t best = LLONG_MIN;
    for (int L = 0; L < kMaxLevels - 1; L++) {
        const int64_t* a = m.lvl[L];
        if (hi - lo <= 2 * kFan) return span_max(a, lo, hi, best);
        const int64_t lo2 = (lo + kFan - 1) / kFan, hi2 = hi / kFan;
        best = span_max(a, lo, lo2 * kFan, best);
        best = span_max(a, hi2 * kFan, hi, best);
        lo = lo2;
        hi = hi2;
    }
    const int64_t* a = m.lvl[kMaxLevels - 1];
    for (int64_t i = lo; i < hi; i++) {
        const int64_t v = l3_entry(a, i);
        best = v > best ? v : best;
    }
    return best;
}

template <bool LONG>
__global__ __launch_bounds__(kBlock) void k_read_versions(ReadVersionsArgs a) {
    const BatchDev& b = a.b;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 2;
    const int k = (int)(t & 3);
    const bool live = r < b.R;
    const int64_t rr = live ? r : 0;
    const DKey kb = b.keys[2 * rr], ke = b.keys[2 * rr + 1];
    const bool degenerate = dkey_cmp(kb, b.tail, ke, b.tail) == 0;
    const bool is_delta = k >= 2;
    const Tier& tier = is_delta ? a.delta : a.base;
    const int64_t n = *tier.n;
    const bool active = live && (!is_delta || n > 0);
    int64_t lb = 0;
    bool eq = false;
    if (active && !((k & 1) && degenerate)) {
        const DKey& q = (k & 1) ? ke : kb;
        if constexpr (LONG) {
            QTail qt;
            load_qtail(qt, q, b.tail);
            lb = lane_lower_bound_long(tier.h, tier.m, n, q, qt, a.htail, b.tail, eq);
        } else {
            lb = lane_lower_bound(tier.h, tier.m, n, q, a.htail, b.tail, eq);
        }
    }
    const int64_t j = __shfl_xor(lb, 1, 64);  // the begin lane takes the end key's position
    int64_t v = kHole;
    if (active && !(k & 1)) {
        const int64_t hdr = is_delta ? kHole : tier.hdr;
        const int64_t ub = lb + (eq ? 1 : 0);
        if (lb < 0 || lb > n || (!degenerate && (j < ub || j > n))) {
            atomicOr(a.error, 1);  // a position outside the tier, or the end's below the begin's
        } else if (degenerate) {
            v = lb > 0 ? tier.h.ver[lb - 1] : hdr;  // the greatest boundary < b
        } else {
            // segments [ub - 1, j): the one containing b (the header if ub == 0) and the boundaries in (b, e)
            v = range_max_full(tier.m, ub > 0 ? ub - 1 : 0, j);
            if (ub == 0) v = hdr > v ? hdr : v;
        }
    }
    const int64_t o = __shfl_xor(v, 2, 64);  // the delta tier's value to the quad's first lane
    v = o > v ? o : v;
    if (live && k == 0) a.out[r] = export_clamp(v, a.floor);
}

const void* launch_read_versions(hipStream_t s, const ReadVersionsArgs& a, bool long_keys) {
    if (a.b.R == 0) return nullptr;
    const int grid = (int)(((int64_t)a.b.R * 4 + kBlock - 1) / kBlock);
    const auto k = long_keys ? k_read_versions<true> : k_read_versions<false>;
    fdb_launch(k, dim3(grid), dim3(kBlock), 0, s, a);
    return (const void*)k;
}

}  // namespace fdbcs
