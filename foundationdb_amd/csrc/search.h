// search.h — device-side searches of a history tier, shared by the detect pipeline (kernels.hip)
// and the maintenance kernels (transfer.hip): key comparisons against a boundary, the cooperative
// and per-lane lower bounds over a tier's sample index, and the small helpers both sides build on
// (tier_query, first_false, tier_bounds_lane).  Everything is __forceinline__:
// each translation unit compiles its own copies, no device call crosses a unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

namespace fdbcs {

// ------------------------------------------------------------------ helpers

// History tails are 8-byte aligned and Hist::lt.y counts 8-byte units (32 GiB of tail arena per
// conflict set with a 32-bit offset).
__device__ __forceinline__ const uint8_t* hist_tail(const uint8_t* htail, uint32_t unit) {
    return htail + 8 * (size_t)unit;
}
__device__ __forceinline__ uint32_t tail_units(uint32_t len) { return len > 16u ? (len - 16u + 7u) / 8u : 0u; }

// Copy the n tail bytes at src (any alignment; the arena has >= 16 bytes of slack past them) to the
// 8-aligned dst as whole words; the bytes past n in the last word are never compared (tail_cmp).
__device__ __forceinline__ void copy_tail_words(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const uintptr_t a = (uintptr_t)src;
    const uint64_t* w = (const uint64_t*)(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7u) * 8u;
    uint64_t* d = (uint64_t*)dst;
    for (uint32_t i = 0; i < (n + 7u) / 8u; i++) d[i] = sh ? (w[i] >> sh) | (w[i + 1] << (64u - sh)) : w[i];
}

__device__ __forceinline__ int hist_cmp(const Hist& h, int64_t i, const uint8_t* htail, const DKey& q,
                                        const uint8_t* qtail) {
    ulonglong2 k = h.key[i];
    if (k.x != q.hi) return k.x < q.hi ? -1 : 1;
    if (k.y != q.lo) return k.y < q.lo ? -1 : 1;
    uint2 lt = h.lt[i];
    if (lt.x > 16u && q.len > 16u) return tail_cmp(hist_tail(htail, lt.y), lt.x, qtail + q.tail, q.len);
    return (lt.x > q.len) - (lt.x < q.len);
}

__device__ __forceinline__ bool prefix_less(const ulonglong2& k, const DKey& q) {
    return k.x < q.hi || (k.x == q.hi && k.y < q.lo);
}

// Full key comparison of boundary i with q, given its prefix already loaded.
__device__ __forceinline__ int probe_cmp(const Hist& h, int64_t i, const ulonglong2& k, const uint8_t* htail,
                                         const DKey& q, const uint8_t* qtail) {
    if (k.x != q.hi) return k.x < q.hi ? -1 : 1;
    if (k.y != q.lo) return k.y < q.lo ? -1 : 1;
    return hist_cmp(h, i, htail, q, qtail);  // equal prefixes: length / tail
}
// The same with a word-at-a-time tail comparison (one pair of 8-byte words live, not four): keeps
// the read check's register footprint low; equal 16-byte prefixes are the rare path.
__device__ __forceinline__ int probe_cmp_lean(const Hist& h, int64_t i, const ulonglong2& k, const uint8_t* htail,
                                              const DKey& q, const uint8_t* qtail) {
    if (k.x != q.hi) return k.x < q.hi ? -1 : 1;
    if (k.y != q.lo) return k.y < q.lo ? -1 : 1;
    const uint2 lt = h.lt[i];
#if defined(__HIP_DEVICE_COMPILE__)
    if (lt.x > 16u && q.len > 16u) {
        const uint8_t* ta = hist_tail(htail, lt.y);
        const uint8_t* tb = qtail + q.tail;
        const uint32_t nb = (lt.x < q.len ? lt.x : q.len) - 16u;
        for (uint32_t o = 0; o < nb; o += 8) {
            const int vb = (int)(nb - o);
            const uint64_t msk = vb >= 8 ? ~0ull : ~0ull << (64 - 8 * vb);
            const uint64_t x = tail_word(ta + o) & msk, y = tail_word(tb + o) & msk;
            if (x != y) return x < y ? -1 : 1;
        }
    }
#endif
    return (lt.x > q.len) - (lt.x < q.len);
}

// ---- long-key probes (batches with keys over 16 bytes: C4 tuple keys)
//
// Keys of one tuple subspace/user share their 16-byte prefix, so the last rounds of a lookup tie
// on the prefix and compare tails.  The generic probe loads the boundary's (len, tail) only after
// its prefix tied, then the two tails 32 bytes per dependent round, each tail word through two
// unaligned loads.  The long-key probe instead holds the query's tail words in registers for the
// whole lookup (kQW words), loads the boundary's (len, tail) beside its prefix, and reads the
// history tail (8-byte aligned in its arena) as whole words, kHW per round: one dependent round
// after the prefix for tails up to 48 bytes, two up to 96.
constexpr int kQW = 12;  // query tail words in registers: keys up to 112 bytes compare without reloads
[[maybe_unused]] constexpr int kHW = 6;  // history tail words per load round
struct QTail {
    uint64_t w[kQW];  // big-endian words of query bytes [16, 16 + 8 kQW), garbage past the key's end
};

__device__ __forceinline__ void load_qtail(QTail& qt, const DKey& q, const uint8_t* qtail) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t n = q.len > 16u ? q.len - 16u : 0u;
    const uintptr_t a = (uintptr_t)(qtail + q.tail);
    const uint64_t* w = (const uint64_t*)(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7u) * 8u;
    const uint32_t cnt = ((uint32_t)(a & 7u) + n + 7u) / 8u;  // aligned words holding the tail
    uint64_t raw[kQW + 1];
#pragma unroll
    for (int j = 0; j <= kQW; j++) raw[j] = (uint32_t)j < cnt ? w[j] : 0ull;
#pragma unroll
    for (int j = 0; j < kQW; j++) qt.w[j] = __builtin_bswap64(sh ? (raw[j] >> sh) | (raw[j + 1] << (64u - sh)) : raw[j]);
#endif
}

// probe_cmp with the boundary's (len, tail) already loaded and the query tail in registers.
__device__ __forceinline__ int probe_cmp_long(const ulonglong2& k, const uint2& lt, const uint8_t* htail, const DKey& q,
                                              const QTail& qt, const uint8_t* qtail) {
    if (k.x != q.hi) return k.x < q.hi ? -1 : 1;
    if (k.y != q.lo) return k.y < q.lo ? -1 : 1;
#if defined(__HIP_DEVICE_COMPILE__)
    if (lt.x > 16u && q.len > 16u) {
        const uint64_t* ha = (const uint64_t*)hist_tail(htail, lt.y);
        const uint32_t n = (lt.x < q.len ? lt.x : q.len) - 16u;  // common tail bytes
        const int nw = (int)((n + 7u) / 8u);
#pragma unroll
        for (int j0 = 0; j0 < kQW; j0 += kHW) {
            if (j0 >= nw) break;
            uint64_t x[kHW];
#pragma unroll
            for (int u = 0; u < kHW; u++) x[u] = j0 + u < nw ? ha[j0 + u] : 0ull;
#pragma unroll
            for (int u = 0; u < kHW; u++) {
                const int j = j0 + u;
                const int vb = (int)n - 8 * j;  // bytes of word j inside the shorter tail
                if (vb <= 0) break;
                const uint64_t msk = vb >= 8 ? ~0ull : ~0ull << (64 - 8 * vb);
                const uint64_t hx = __builtin_bswap64(x[u]) & msk, qy = qt.w[j] & msk;
                if (hx != qy) return hx < qy ? -1 : 1;
            }
        }
        if (nw > kQW)  // both tails run past the registers: the rest from memory
            return tail_cmp(hist_tail(htail, lt.y) + 8 * kQW, lt.x - 8 * kQW, qtail + q.tail + 8 * kQW,
                            q.len - 8 * kQW);
    }
#endif
    return (lt.x > q.len) - (lt.x < q.len);
}

// ---- cooperative search: kArity lanes per query, one kArity-entry tree node per level
//
// Each lane of an aligned kArity-lane group loads one entry of the node, so a level is one
// coalesced kArity*16-byte access (one 128-byte line at kArity 8).  All lanes of a group call with
// the same query and get the same result.  gmask(): the group's bits of a wave ballot.
__device__ __forceinline__ uint32_t gmask(bool pred) {
    const uint64_t m = __ballot(pred);
    return (uint32_t)(m >> (threadIdx.x & 63 & ~(kArity - 1))) & ((1u << kArity) - 1u);
}

// Directory slot of a 16-byte prefix (MaxLevels::dir_p .. dir_w), monotone over all keys: keys
// below the loaded keys' common prefix take slot 0, keys above it dir_top, keys under it 1 + the
// mixed-radix code of the next dir_e bytes (each byte's offset in its position's value range; the
// code ends at the first byte outside its range).  ALU only.  Both tiers' directories
// (k_directory, the epilogue's delta fill) and every lookup use it.
__device__ __forceinline__ uint32_t dir_slot(const MaxLevels& m, uint64_t hi, uint64_t lo) {
    const uint32_t p = m.dir_p;
    if (p) {
        const uint64_t mh = p >= 8 ? ~0ull : ~0ull << (64 - 8 * p);
        const uint64_t ml = p <= 8 ? 0ull : ~0ull << (128 - 8 * p);
        const uint64_t xh = hi & mh, xl = lo & ml;
        if (xh != m.dir_phi || xl != m.dir_plo)
            return (xh < m.dir_phi || (xh == m.dir_phi && xl < m.dir_plo)) ? 0u : m.dir_top;
    }
    // the bytes after the prefix, left-aligned: position p + i is byte i of h
    const uint64_t h = p == 0 ? hi : (p < 8 ? (hi << (8 * p)) | (lo >> (64 - 8 * p)) : lo << (8 * (p - 8)));
    uint32_t code = 1;
    bool live = true;
#pragma unroll
    for (int i = 0; i < kDirPos; i++) {
        const uint32_t b = (uint32_t)(h >> (56 - 8 * i)) & 255u;
        const uint32_t pos = m.dir_pos[i];
        const uint32_t l = pos & 255u, d = (pos >> 8) & 511u, s = pos >> 17;
        const uint32_t r = b < l ? 0u : (b - l < d ? b - l : d);
        if (live && (uint32_t)i < m.dir_e) code += (r >> s) * m.dir_w[i];
        live = live && b >= l && b - l < d;
    }
    return code;
}

// The directory range of q's slot, in skey8 entries (every 8th boundary): entries [d8a, d8b) share
// q's slot, every entry before d8a lies below q and every entry from d8b on above it (dir_slot is
// monotone over the 16-byte prefix).  Both tiers' directories count skey8 entries (base:
// k_directory, exact; delta: the epilogue's fill, entries of the current epoch only).  false: no
// directory, or a delta slot of another epoch.
__device__ __forceinline__ bool dir_range8(const MaxLevels& m, const DKey& q, int64_t& d8a, int64_t& d8b) {
    if (!m.dir && !m.edir_epoch) return false;
    const uint32_t dv = dir_slot(m, q.hi, q.lo);
    if (m.dir) {
        d8a = m.dir[dv];
        d8b = m.dir[dv + 1];
        return true;
    }
    const uint64_t x0 = m.edir[dv], x1 = m.edir[dv + 1];
    d8a = (uint32_t)x0;
    d8b = (uint32_t)x1;
    return (uint32_t)(x0 >> 32) == m.edir_epoch && (uint32_t)(x1 >> 32) == m.edir_epoch;
}

// LONG: the long-key probes above (the batch has keys over 16 bytes); same result.
template <bool LONG = false>
__device__ __forceinline__ int64_t group_lower_bound(const Hist& h, const MaxLevels& m, int64_t n, const DKey& q,
                                                     const uint8_t* htail, const uint8_t* qtail, bool& eq) {
    const int gl = threadIdx.x & (kArity - 1);
    const int g0 = threadIdx.x & 63 & ~(kArity - 1);  // first lane of the group
    eq = false;
    if (n <= 0) return 0;
    QTail qt;
    if constexpr (LONG) load_qtail(qt, q, qtail);  // in flight during the descent
    // one probe of boundary p (prefix k): the long-key form loads (len, tail) beside the prefix
    auto probe = [&](int64_t p, const ulonglong2* kp) -> int {
        if constexpr (LONG) {
            const ulonglong2 k = *kp;
            const uint2 lt = h.lt[p];
            return probe_cmp_long(k, lt, htail, q, qt, qtail);
        } else {
            return probe_cmp(h, p, *kp, htail, q, qtail);
        }
    };
    int64_t sz[kIdxLevels];
    sz[0] = (n + kFan - 1) / kFan;
#pragma unroll
    for (int L = 1; L < kIdxLevels; L++) sz[L] = (sz[L - 1] + kArity - 1) / kArity;
    int top = 0;
    while (top + 1 < kIdxLevels && sz[top] > kArity) top++;
    // c = number of entries of level `top` whose prefix is < q.  When level 0 is probed, also learn
    // whether the first sample not below q shares q's prefix (`bknown`: it does not).
    auto prefix_eq = [&](const ulonglong2& k) { return k.x == q.hi && k.y == q.lo; };
    int64_t c = 0;
    bool bknown = false;
    // the top level's first group is loaded beside the directory slot (no added round trip when
    // the slot is crowded and the tree is taken)
    const bool v_top = gl < sz[top];
    const ulonglong2 e_top = m.skey[top][v_top ? gl : 0];
    bool direct = false;
    int64_t d8a, d8b;
    if (dir_range8(m, q, d8a, d8b)) {
        // radix directory: the level-0 samples (every 8th skey8 entry) sharing q's directory bits
        // are [d0, d1); a slot of at most two groups is counted directly at level 0
        const int64_t d0 = (d8a + 7) >> 3, d1 = (d8b + 7) >> 3;
        if (d1 - d0 <= 2 * kArity && d1 <= sz[0]) {
            direct = true;
            c = d0;
            bknown = true;  // all of the slot below q: the next sample's first two bytes are greater
            for (int64_t j0 = d0; j0 < d1; j0 += kArity) {
                const bool v = j0 + gl < d1;
                const ulonglong2 e = m.skey[0][v ? j0 + gl : 0];
                const int k = __popc(gmask(v && prefix_less(e, q)));
                c += k;
                if (k < __popc(gmask(v))) {
                    bknown = !((gmask(v && prefix_eq(e)) >> k) & 1u);
                    break;
                }
            }
        }
    }
    if (!direct) {
        for (int64_t j0 = 0; j0 < sz[top]; j0 += kArity) {
            const bool v = j0 == 0 ? v_top : j0 + gl < sz[top];
            const ulonglong2 e = j0 == 0 ? e_top : m.skey[top][v ? j0 + gl : 0];
            const int k = __popc(gmask(v && prefix_less(e, q)));
            if (top == 0 && k < __popc(gmask(v))) bknown = !((gmask(v && prefix_eq(e)) >> k) & 1u);
            c += k;
            if (k < kArity) break;
        }
        for (int L = top; L > 0; L--) {
            if (c == 0) continue;  // nothing below q at this level: nothing below it underneath either
            // entries of level L-1 below q: [0, c') with c' in [A(c-1)+1, Ac]
            const int64_t base = (int64_t)kArity * (c - 1) + 1;
            const int64_t end = min((int64_t)kArity * c, sz[L - 1]);
            const bool v = base + gl < end;
            const ulonglong2 e = m.skey[L - 1][v ? base + gl : 0];
            const int k = __popc(gmask(v && prefix_less(e, q)));
            if (L == 1 && k < __popc(gmask(v))) bknown = !((gmask(v && prefix_eq(e)) >> k) & 1u);
            c = base + k;
        }
    }
    // c = #samples below q; samples equal to q's prefix (shared prefixes) widen the block
    int64_t b = c;
    for (; !bknown;) {
        const bool v = b + gl < sz[0];
        const ulonglong2 k = m.skey[0][v ? b + gl : 0];
        const uint32_t same = gmask(v && k.x == q.hi && k.y == q.lo);
        const int run = __ffs(~same) - 1;  // leading lanes equal to q's prefix
        b += run;
        if (run < kArity) break;
    }
    int64_t lo = c > 0 ? kFan * (c - 1) + 1 : 0;
    const int64_t hi = min(n, kFan * b);
    if (b == c && m.skey8) {
        // Boundary 64(c-1) < q < boundary 64c (sample c's prefix is greater): the answer lies in one
        // 64-boundary block.  Round one probes the starts of its eight 8-groups through skey8 (one
        // 128-byte line, not eight); round two the seven keys after the last start below q (one
        // line).  Prefix ties compare lengths / tails against the boundary itself (probe_cmp).
        const int64_t B = c > 0 ? kFan * (c - 1) : 0;
        const int64_t p8 = B + 8 * gl;
        const bool v8 = p8 < hi;
        int r8 = 1;
        if (v8) r8 = probe(p8, &m.skey8[p8 / 8]);
        const int k8 = __popc(gmask(v8 && r8 < 0));  // group starts below q
        const int r_first = __shfl(r8, g0, 64);
        if (k8 == 0) {  // c == 0 and q <= boundary 0
            eq = hi > 0 && r_first == 0;
            return 0;
        }
        const int64_t g = B + 8 * (k8 - 1);  // boundary g < q; the answer is in (g, min(g + 8, hi)]
        const int64_t gend = min(g + 8, hi);
        const int64_t pk = g + 1 + gl;
        const bool vk = gl < 7 && pk < gend;
        int rk = 1;
        if (vk) rk = probe(pk, &h.key[pk]);
        const int k1 = __popc(gmask(vk && rk < 0));
        const int64_t lb = g + 1 + k1;
        const int r_stop = __shfl(rk, g0 + (k1 < 7 ? k1 : 6), 64);
        const int r_next = __shfl(r8, g0 + (k8 < kArity ? k8 : kArity - 1), 64);
        if (lb < gend)
            eq = r_stop == 0;  // the probe that stopped the count
        else if (lb < hi)
            eq = r_next == 0;  // lb = g + 8: the next group's start, probed in round one
        return lb;
    }
    // lower_bound in [lo, lo + span]: rounds of kArity probes at a shrinking stride.  span <= 64
    // normally; a long run of boundaries sharing q's 16-byte prefix (tuple keys) only starts the
    // stride higher, so the lanes still compare tails side by side.
    int64_t span = hi - lo;
    int64_t stride0 = kFan / kArity;
    while (stride0 * kArity < span) stride0 *= kArity;
    bool eq_cand = false;  // cmp == 0 at the last probe that stopped a count (the answer, if < hi)
    for (int64_t stride = stride0; span > 0; stride = stride > kArity ? stride / kArity : 1) {
        const int64_t p = lo + stride * (gl + 1) - 1;
        const bool v = stride * (gl + 1) <= span && p < hi;
        int r = 1;
        if (v) r = probe(p, &h.key[p]);
        const uint32_t valid = gmask(v);
        const int cnt = __popc(gmask(v && r < 0));
        const int stop = __shfl(r, g0 + (cnt < kArity ? cnt : kArity - 1), 64);
        if (cnt < __popc(valid)) eq_cand = stop == 0;  // lane cnt probed a key >= q
        lo += stride * cnt;
        span = cnt < __popc(valid) ? stride - 1 : span - stride * cnt;
        if (stride == 1) break;
    }
    if (lo < hi) eq = eq_cand;
    return lo;
}

// ---- per-lane lookups (SkipList.cpp:426-458 + CheckMax :619-706, as the step-function rule of
// SURVEY A.2)
//
// The history is the base tier overlaid by the delta tier; every delta version is >= the base
// versions it covers (versions only grow), so the max over the overlay equals the max of the two
// tiers' maxima, and holes (kHole) never conflict.
//
// One lane per lookup.  Round 3's cooperative lookups (group_lower_bound, still used by the
// segment search of small batches) gave each lookup kArity lanes that load one node entry each,
// so a wave served kArity lookups and the wave's instruction stream (ballots, shuffles, 64-bit
// compares) was paid per kArity lookups: at C2 12,500 waves of ~350 VALU + ~260 SALU instructions
// each, 77 % of their life waiting on loads (rocprofv3 SQ counters), the chip never holding all
// of them at once.  Here a lane issues a whole node's (or directory slot's)
// entries itself, up to kLaneProbe independent 16-byte loads in flight, and counts them in
// registers: the same dependent rounds per lookup, 64 lookups per wave, every wave of a C2 batch
// resident at once.
constexpr int kLaneProbe = 16;  // entries one lane loads per round (a directory slot of two groups)

// Number of the first cnt (<= N) entries of a[base, ...) whose 16-byte prefix is below q's, and
// whether the first entry not below it has q's prefix (eq_next; false if all are below).
template <int N>
__device__ __forceinline__ int lane_count(const ulonglong2* a, int64_t base, int cnt, const DKey& q, bool& eq_next) {
    ulonglong2 k[N];
#pragma unroll
    for (int i = 0; i < N; i++)
        if (i < cnt) k[i] = a[base + i];
    int c = 0;
    eq_next = false;
    bool stop = false;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < cnt && !stop) {
            if (prefix_less(k[i], q)) {
                c++;
            } else {
                stop = true;
                eq_next = k[i].x == q.hi && k[i].y == q.lo;
            }
        }
    }
    return c;
}

// The level-0 samples of a tier below q's 16-byte prefix (c) and the end of the run of samples
// sharing that prefix (b >= c), by one lane: the radix directory slot (at most kLaneProbe level-0
// samples) or the kArity-ary sample tree, each node's entries loaded by the lane as independent
// 16-byte loads.  Boundary 64(c-1) lies below q and boundary 64b (if any) above it.
__device__ __forceinline__ void lane_sample_range(const MaxLevels& m, int64_t n, const DKey& q, int64_t& c_out,
                                                  int64_t& b_out) {
    int64_t sz[kIdxLevels];
    sz[0] = (n + kFan - 1) / kFan;
#pragma unroll
    for (int L = 1; L < kIdxLevels; L++) sz[L] = (sz[L - 1] + kArity - 1) / kArity;
    int top = 0;
    while (top + 1 < kIdxLevels && sz[top] > kArity) top++;
    int64_t c = 0;      // level-0 samples whose prefix is below q
    bool bknown = false;  // the sample at c (if any) is known not to share q's prefix
    bool direct = false;
    int64_t w0 = -1, w1 = -1;  // a directory slot too wide to count at level 0
    int64_t d8a, d8b;
    if (dir_range8(m, q, d8a, d8b)) {
        // the level-0 samples (every 8th skey8 entry) in q's slot: [d0, d1)
        const int64_t d0 = (d8a + 7) >> 3, d1 = (d8b + 7) >> 3;
        if (d1 - d0 <= kLaneProbe && d1 <= sz[0]) {
            direct = true;
            bool eqn;
            const int cnt = (int)(d1 - d0);
            const int k = lane_count<kLaneProbe>(m.skey[0], d0, cnt, q, eqn);
            c = d0 + k;
            // all of the slot below q: the next sample's first two bytes are greater
            bknown = k < cnt ? !eqn : true;
        } else if (d1 <= sz[0]) {
            w0 = d0;
            w1 = d1;
        }
    }
    if (!direct) {
        // A wide slot (keys whose directory bits take few values: C4's decimal digits after the
        // shared prefix) still bounds q: samples before w0 lie below it and from w1 on above it, so
        // the descent starts at the lowest level whose entries over [w0, w1) fit one probe round
        // (entry j of level L is sample j A^L) instead of at the top.
        int lv = top;
        bool started = false;
        if (w0 >= 0) {
            int64_t span = 1;
            for (int L = 1; L < top; L++) {
                span *= kArity;
                const int64_t a = w0 / span, z = (w1 - 1) / span;
                if (z - a + 1 <= kLaneProbe) {
                    bool eqn;
                    c = a + lane_count<kLaneProbe>(m.skey[L], a, (int)(z - a + 1), q, eqn);
                    lv = L;
                    started = true;
                    break;
                }
            }
        }
        for (int64_t j0 = 0; !started && j0 < sz[top]; j0 += kArity) {
            const int cnt = (int)min((int64_t)kArity, sz[top] - j0);
            bool eqn;
            const int k = lane_count<kArity>(m.skey[top], j0, cnt, q, eqn);
            if (top == 0 && k < cnt) bknown = !eqn;
            c += k;
            if (k < cnt) break;
        }
        for (int L = lv; L > 0; L--) {
            if (c == 0) continue;  // nothing below q at this level: nothing below it underneath either
            const int64_t base = (int64_t)kArity * (c - 1) + 1;
            const int64_t end = min((int64_t)kArity * c, sz[L - 1]);
            bool eqn;
            const int cnt = (int)(end - base);
            const int k = lane_count<kArity>(m.skey[L - 1], base, cnt, q, eqn);
            if (L == 1 && k < cnt) bknown = !eqn;
            c = base + k;
        }
    }
    // samples sharing q's prefix widen the block
    int64_t b = c;
    while (!bknown && b < sz[0]) {
        const ulonglong2 k = m.skey[0][b];
        if (k.x != q.hi || k.y != q.lo) break;
        b++;
    }
    c_out = c;
    b_out = b;
}

// std::lower_bound of q over the n boundaries of a tier by one lane (the result and eq as
// group_lower_bound's): lane_sample_range down to one 64-boundary block, then the block's eight
// group starts (skey8) and the seven boundaries after the last start below q; prefix ties compare
// lengths and tails against the boundary itself (probe_cmp_lean).  A run of boundaries sharing q's
// 16-byte prefix over more than one block (tuple subspaces) falls back to a binary search.
__device__ __forceinline__ int64_t lane_lower_bound(const Hist& h, const MaxLevels& m, int64_t n, const DKey& q,
                                                    const uint8_t* htail, const uint8_t* qtail, bool& eq) {
    eq = false;
    if (n <= 0) return 0;
    // Directory slot of at most kLaneProbe skey8 entries (C2: ~10 per slot of the base, ~2 of the
    // delta): the group starts of q's slot are probed at once, so the lookup takes three dependent
    // rounds (directory, group starts, the seven boundaries after the last start below q) instead
    // of four (the level-0 samples first).  Entries before the slot lie below q, entries past it
    // above q (dir_range8); prefix ties compare against the boundary itself (probe_cmp_lean).
    int64_t d8a, d8b;
    const int64_t n8 = (n + 7) >> 3;
    if (dir_range8(m, q, d8a, d8b) && d8b - d8a <= kLaneProbe && d8b <= n8) {
        const int cnt = (int)(d8b - d8a);
        ulonglong2 s8[kLaneProbe];
#pragma unroll
        for (int i = 0; i < kLaneProbe; i++)
            if (i < cnt) s8[i] = m.skey8[d8a + i];
        int r8[kLaneProbe];
        int k8 = 0;
        bool stop = false;
#pragma unroll
        for (int i = 0; i < kLaneProbe; i++) {
            r8[i] = 1;
            if (i < cnt && !stop) {
                r8[i] = probe_cmp_lean(h, 8 * (d8a + i), s8[i], htail, q, qtail);
                if (r8[i] < 0) k8++; else stop = true;
            }
        }
        const int64_t g = d8a + k8 - 1;  // the last group start below q (-1: none)
        if (g < 0) {                     // q <= boundary 0 (probed when the slot holds entry 0)
            eq = cnt > 0 && r8[0] == 0;
            return 0;
        }
        const int64_t B = 8 * g, gend = min(B + 8, n);
        const int nk = (int)(gend - B - 1);
        ulonglong2 kk[7];
#pragma unroll
        for (int i = 0; i < 7; i++)
            if (i < nk) kk[i] = h.key[B + 1 + i];
        int k1 = 0, r_stop = 1;
        stop = false;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            if (i < nk && !stop) {
                const int r = probe_cmp_lean(h, B + 1 + i, kk[i], htail, q, qtail);
                if (r < 0) {
                    k1++;
                } else {
                    stop = true;
                    r_stop = r;
                }
            }
        }
        const int64_t lb = B + 1 + k1;
        if (lb < gend)
            eq = r_stop == 0;
        else if (lb < n)  // lb = 8(g + 1): the next group start, probed above unless past the slot
            eq = k8 < cnt && r8[k8] == 0;
        return lb;
    }
    int64_t c, b;
    lane_sample_range(m, n, q, c, b);
    const int64_t hi = min(n, kFan * b);
    if (b == c) {
        // boundary 64(c-1) < q < boundary 64c: one 64-boundary block; its group starts, then the
        // boundaries after the last start below q
        const int64_t B = c > 0 ? kFan * (c - 1) : 0;
        const int n8 = (int)min((int64_t)8, (hi - B + 7) / 8);  // group starts below hi
        ulonglong2 s8[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i < n8) s8[i] = m.skey8[B / 8 + i];
        int r8[8];
        int k8 = 0;
        bool stop = false;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            r8[i] = 1;
            if (i < n8 && !stop) {
                r8[i] = probe_cmp_lean(h, B + 8 * i, s8[i], htail, q, qtail);
                if (r8[i] < 0) k8++; else stop = true;
            }
        }
        if (k8 == 0) {  // c == 0 and q <= boundary 0
            eq = hi > 0 && r8[0] == 0;
            return 0;
        }
        const int64_t g = B + 8 * (k8 - 1);  // boundary g < q; the answer lies in (g, min(g + 8, hi)]
        const int64_t gend = min(g + 8, hi);
        const int nk = (int)(gend - g - 1);
        ulonglong2 kk[7];
#pragma unroll
        for (int i = 0; i < 7; i++)
            if (i < nk) kk[i] = h.key[g + 1 + i];
        int k1 = 0;
        int r_stop = 1;
        stop = false;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            if (i < nk && !stop) {
                const int r = probe_cmp_lean(h, g + 1 + i, kk[i], htail, q, qtail);
                if (r < 0) {
                    k1++;
                } else {
                    stop = true;
                    r_stop = r;
                }
            }
        }
        const int64_t lb = g + 1 + k1;
        if (lb < gend)
            eq = r_stop == 0;
        else if (lb < hi)
            eq = k8 < 8 && r8[k8] == 0;  // lb = g + 8: the next group's start, probed above
        return lb;
    }
    // a run of boundaries sharing q's prefix across blocks: binary search with full compares
    int64_t lo = c > 0 ? kFan * (c - 1) + 1 : 0, hh = hi;
    while (lo < hh) {
        const int64_t mid = (lo + hh) >> 1;
        const int r = hist_cmp(h, mid, htail, q, qtail);
        if (r < 0) {
            lo = mid + 1;
        } else {
            hh = mid;
            eq = r == 0;
        }
    }
    if (lo >= hi) eq = false;
    return lo;
}

// ---- per-lane lookups of long keys (batches with keys over 24 bytes: C4 tuple keys)
//
// Keys of one tuple subspace / user share their 16-byte prefix, so a lookup that reaches their run
// compares tails.  One lane per lookup, in three steps: lane_sample_range; the run [s, e) of
// boundaries sharing q's prefix, by prefix-only counts (the group starts of skey8, then the seven
// boundaries after a start: no tails); inside the run a (kRunProbes + 1)-ary search by full
// compares, whose probes' (len, tail offset) and then tails are loaded together against the query
// tail held in registers (QTail): two dependent loads per round.  Keys between two probes share
// with q at least the tail words both probes share with it, so later rounds load and compare only
// the words from there on (C4: the item bytes after a user's ~20-85 shared bytes).
#ifndef FDBCS_RUN_PROBES
#define FDBCS_RUN_PROBES 3
#endif
[[maybe_unused]] constexpr int kRunProbes = FDBCS_RUN_PROBES;

// Boundaries of [lo1, hi) whose prefix is below q's, counted among the n <= N from `base` (sorted).
template <int N>
__device__ __forceinline__ int lane_count_below(const ulonglong2* a, int64_t base, int n, const DKey& q, bool not_above) {
    ulonglong2 k[N];
#pragma unroll
    for (int i = 0; i < N; i++)
        if (i < n) k[i] = a[base + i];
    int c = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
        if (i < n) c += (not_above ? !(q.hi < k[i].x || (q.hi == k[i].x && q.lo < k[i].y)) : prefix_less(k[i], q)) ? 1 : 0;
    return c;
}

// The run of boundaries of [lo1, hi) sharing q's 16-byte prefix: s = the first whose prefix is not
// below q's, e = the first whose prefix is above it (hi if none).  Boundaries before lo1 lie below
// q's prefix, hi and after it above.
__device__ __forceinline__ void lane_prefix_run(const Hist& h, const MaxLevels& m, int64_t lo1, int64_t hi,
                                                const DKey& q, int64_t& s, int64_t& e) {
    const int64_t G0 = (lo1 + 7) / 8;                           // group starts 8g in [lo1, hi)
    const int64_t NG = hi > 8 * G0 ? (hi - 1) / 8 - G0 + 1 : 0;
    if (NG > kLaneProbe) {  // a run over several blocks (a hot subspace): binary searches on prefixes
        int64_t lo = lo1, hh = hi;
        while (lo < hh) {
            const int64_t mid = (lo + hh) >> 1;
            if (prefix_less(h.key[mid], q)) lo = mid + 1; else hh = mid;
        }
        s = lo;
        hh = hi;
        while (lo < hh) {
            const int64_t mid = (lo + hh) >> 1;
            const ulonglong2 k = h.key[mid];
            if (!(q.hi < k.x || (q.hi == k.x && q.lo < k.y))) lo = mid + 1; else hh = mid;
        }
        e = lo;
        return;
    }
    ulonglong2 g[kLaneProbe];
#pragma unroll
    for (int i = 0; i < kLaneProbe; i++)
        if (i < NG) g[i] = m.skey8[G0 + i];
    int kl = 0, kle = 0;
#pragma unroll
    for (int i = 0; i < kLaneProbe; i++) {
        if (i < NG) {
            kl += prefix_less(g[i], q) ? 1 : 0;
            kle += (q.hi < g[i].x || (q.hi == g[i].x && q.lo < g[i].y)) ? 0 : 1;
        }
    }
    // s lies in [as, bs], e in [ae, be]: at most seven boundaries after a group start each
    const int64_t as = kl > 0 ? 8 * (G0 + kl - 1) + 1 : lo1, bs = kl < NG ? 8 * (G0 + kl) : hi;
    const int64_t ae = kle > 0 ? 8 * (G0 + kle - 1) + 1 : lo1, be = kle < NG ? 8 * (G0 + kle) : hi;
    ulonglong2 ks[7], ke[7];
    const int ns = (int)(bs - as), ne = (int)(be - ae);
#pragma unroll
    for (int i = 0; i < 7; i++) {
        if (i < ns) ks[i] = h.key[as + i];
        if (i < ne) ke[i] = h.key[ae + i];
    }
    int cs = 0, ce = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        if (i < ns) cs += prefix_less(ks[i], q) ? 1 : 0;
        if (i < ne) ce += (q.hi < ke[i].x || (q.hi == ke[i].x && q.lo < ke[i].y)) ? 0 : 1;
    }
    s = as + cs;
    e = ae + ce;
}

// lane_lower_bound for long keys (same result and eq); qt: q's tail words (load_qtail).  RP: probes
// per round inside a prefix run (more per round made k_seg_prep's few, latency-bound lookups slower
// at C4: 37.7 / 41.4 / 42.9 us at 3 / 5 / 7).
template <int RP = kRunProbes>
__device__ __forceinline__ int64_t lane_lower_bound_long(const Hist& h, const MaxLevels& m, int64_t n, const DKey& q,
                                                         const QTail& qt, const uint8_t* htail, const uint8_t* qtail,
                                                         bool& eq) {
    eq = false;
    if (n <= 0) return 0;
    int64_t c, b;
    lane_sample_range(m, n, q, c, b);
    int64_t lo, hh;
    lane_prefix_run(h, m, c > 0 ? kFan * (c - 1) + 1 : 0, min(n, kFan * b), q, lo, hh);
#if defined(__HIP_DEVICE_COMPILE__)
    // [lo, hh): boundaries sharing q's prefix, lower_bound among them by full compares.  dlo / dhi:
    // tail words known equal to q's in the boundaries just below lo and at hh (none at first: their
    // prefixes differ from q's).
    int dlo = 0, dhi = 0;
    bool eq_hh = false;  // the boundary at hh equals q (hh was set by a probe)
    const bool qlong = q.len > 16u;
    while (lo < hh) {
        const int64_t span = hh - lo;
        const int w0 = dlo < dhi ? dlo : dhi;  // tail words every boundary in [lo, hh) shares with q
        int64_t p[RP];
        bool v[RP];
        uint2 lt[RP];
#pragma unroll
        for (int j = 0; j < RP; j++) {
            p[j] = lo + (span * (j + 1)) / (RP + 1);
            v[j] = p[j] < hh && (j == 0 || p[j] != p[j - 1]);
            if (v[j]) lt[j] = h.lt[p[j]];
        }
        uint64_t x[RP][kQW];
        uint32_t nb[RP];
#pragma unroll
        for (int j = 0; j < RP; j++) {
            nb[j] = v[j] && qlong && lt[j].x > 16u ? (lt[j].x < q.len ? lt[j].x : q.len) - 16u : 0u;
            const uint64_t* ha = (const uint64_t*)hist_tail(htail, v[j] ? lt[j].y : 0u);
            const int nw = (int)((nb[j] + 7u) / 8u);
#pragma unroll
            for (int u = 0; u < kQW; u++)
                if (u >= w0 && u < nw) x[j][u] = ha[u];
        }
        int r[RP], d[RP];
#pragma unroll
        for (int j = 0; j < RP; j++) {
            r[j] = 1;
            d[j] = 0;
            if (!v[j]) continue;
            const int nw = (int)((nb[j] + 7u) / 8u);
            bool found = false;
#pragma unroll
            for (int u = 0; u < kQW; u++) {
                if (!found && u >= w0 && u < nw) {
                    const int vb = (int)nb[j] - 8 * u;
                    const uint64_t msk = vb >= 8 ? ~0ull : ~0ull << (64 - 8 * vb);
                    const uint64_t hx = __builtin_bswap64(x[j][u]) & msk, qy = qt.w[u] & msk;
                    if (hx != qy) {
                        r[j] = hx < qy ? -1 : 1;
                        d[j] = u;
                        found = true;
                    }
                }
            }
            if (!found) {
                if (nw > kQW) {  // both tails run past the registers: the rest from memory
                    r[j] = tail_cmp(hist_tail(htail, lt[j].y) + 8 * kQW, lt[j].x - 8 * kQW, qtail + q.tail + 8 * kQW,
                                    q.len - 8 * kQW);
                    d[j] = kQW;
                } else {
                    r[j] = (lt[j].x > q.len) - (lt[j].x < q.len);
                    d[j] = (int)(nb[j] / 8u);
                }
            }
        }
        // the probes below q form a prefix of the valid ones
        int64_t nlo = lo, nhh = hh;
        int ndlo = dlo, ndhi = dhi;
        bool neq = eq_hh, hit = false;
#pragma unroll
        for (int j = 0; j < RP; j++) {
            if (!v[j] || hit) continue;
            if (r[j] < 0) {
                nlo = p[j] + 1;
                ndlo = d[j];
            } else {
                nhh = p[j];
                ndhi = d[j];
                neq = r[j] == 0;
                hit = true;
            }
        }
        lo = nlo;
        hh = nhh;
        dlo = ndlo;
        dhi = ndhi;
        eq_hh = neq;
    }
    eq = eq_hh;
#endif
    return lo;
}

// ---- one tier searched by another's boundaries, and plain searches

// Boundary i of a tier as a search key whose tail starts at qtail (q.tail = 0).  lt.y goes into
// hist_tail unguarded: every writer of a tier's lt stores y = 0 for keys of at most 16 bytes
// (fdbcs_load_history, BatchIns, CompactIns and the merge copies, GcScan, k_import_normalize,
// k_import_rank, ImportFold, ImportDeltaFold, k_impd_copy), and no comparison reads qtail unless
// the key is longer than that.
__device__ __forceinline__ void tier_query(const Hist& h, int64_t i, const uint8_t* arena, DKey& q,
                                           const uint8_t*& qtail) {
    const ulonglong2 k = h.key[i];
    const uint2 lt = h.lt[i];
    q.hi = k.x;
    q.lo = k.y;
    q.len = lt.x;
    q.tail = 0;
    qtail = hist_tail(arena, lt.y);
}

// The host's pick between the two MODE instantiations of a kernel that searches the base for
// delta boundaries (k_compact_search, k_export_search): 1 lane_lower_bound, 2 the long-key form.
template <class K>
inline K search_mode_kernel(int mode, K mode1, K mode2) {
    return mode == 1 ? mode1 : mode2;
}

// The first index of [lo, hi) at which an ascending predicate (true up to some index, false from
// it on) stops holding; hi if it holds throughout.
template <class I, class Pred>
__device__ __forceinline__ I first_false(I lo, I hi, const Pred& pred) {
    while (lo < hi) {
        const I mid = lo + (hi - lo) / 2;
        if (pred(mid))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The positions of a key range's bounds in both tiers, one count per lane t < 4 (0: lo in the
// base, 1: lo in the delta, 2: hi in the base, 3: hi in the delta): the tier's boundaries below
// the bound (lo with upper_lo: or equal to it) by a plain binary search over full keys; without
// the bound, none for lo and all for hi.  key(is_hi, q, qtail) supplies the bound as a query.
template <class Key>
__device__ __forceinline__ int64_t tier_bounds_lane(int t, const Hist& base, int64_t nb, const Hist& delta, int64_t nd,
                                                    const uint8_t* htail, bool has_lo, bool has_hi, bool upper_lo,
                                                    const Key& key) {
    const bool is_hi = t >= 2, is_delta = t & 1;
    const int64_t n = is_delta ? nd : nb;
    if (!(is_hi ? has_hi : has_lo)) return is_hi ? n : 0;
    DKey q;
    const uint8_t* qtail;
    key(is_hi, q, qtail);
    const Hist& h = is_delta ? delta : base;
    const bool upper = upper_lo && !is_hi;
    return first_false<int64_t>(0, n, [&](int64_t i) {
        const int c = hist_cmp(h, i, htail, q, qtail);
        return c < 0 || (upper && c == 0);
    });
}

}  // namespace fdbcs
