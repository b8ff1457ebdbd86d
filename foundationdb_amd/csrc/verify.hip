// verify.hip — gfx950 kernels of fdbcs_history_verify (include/fdb_conflict_set.h has the
// definition of every check class): streaming, read-only passes over both stored tiers that
// recompute what a lookup relies on, independently of the kernels that build it (k_epilogue,
// k_directory, the compaction, the GC, the imports) and of the lookups of search.h.
//
// Rules of this unit:
//  - every load of a stored array goes through Rd, which applies the caller's what-if override to
//    the one element it names, so a what-if takes exactly the path of a real read;
//  - no address is formed from a stored value before that value is checked against the array it
//    indexes (a tail unit against tail_used, a directory count against the group starts); an
//    out-of-range value is a violation of its own class and the check that depends on it is skipped;
//  - sizes come from the host, clamped to the capacities it allocated; every loop is bounded by them;
//  - no kernel waits, spins or scans: counts by atomicAdd, first indices by atomicMin, the level-3
//    spans' true maxima by atomicMax, all commutative, so a report is deterministic.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>

#include "verify.h"
#include "launch.h"
#include "search.h"

namespace fdbcs {

namespace {

constexpr int kVfThreads = 256;
constexpr int kVfWaves = kVfThreads / 64;
constexpr int kVfMaxGrid = 2048;
constexpr int kSearchSteps = 48;  // binary-search rounds: tiers hold far fewer than 2^48 boundaries

struct Rd {
    const VerifyArgs& a;
    __device__ __forceinline__ bool hit(int what, int tier, int64_t i) const {
        return a.ov.what == what && a.ov.tier == tier && a.ov.index == i;
    }
    __device__ __forceinline__ ulonglong2 key(int t, int64_t i) const {
        ulonglong2 k = a.t[t].h.key[i];
        if (hit(kVwKey, t, i)) k.x ^= a.ov.hi, k.y ^= a.ov.lo;
        return k;
    }
    __device__ __forceinline__ uint2 lt(int t, int64_t i) const {
        uint2 v = a.t[t].h.lt[i];
        if (hit(kVwLenTail, t, i)) v.x ^= (uint32_t)a.ov.lo, v.y ^= (uint32_t)a.ov.hi;
        return v;
    }
    __device__ __forceinline__ int64_t ver(int t, int64_t i) const {
        int64_t v = a.t[t].h.ver[i];
        if (hit(kVwVersion, t, i)) v ^= (int64_t)a.ov.lo;
        return v;
    }
    // L = 1, 2: entry i; L = 3: replica word i = j * kL3Rep + r
    __device__ __forceinline__ int64_t lvl(int t, int L, int64_t i) const {
        int64_t v = a.t[t].m.lvl[L][L == 3 ? i * kL3Pad : i];
        if (hit(kVwLvl1 + L - 1, t, i)) v ^= (int64_t)a.ov.lo;
        return v;
    }
    __device__ __forceinline__ ulonglong2 skey8(int t, int64_t e) const {
        ulonglong2 k = a.t[t].m.skey8[e];
        if (hit(kVwSkey8, t, e)) k.x ^= a.ov.hi, k.y ^= a.ov.lo;
        return k;
    }
    __device__ __forceinline__ ulonglong2 skey(int t, int L, int64_t d) const {
        int64_t off = 0;
        for (int l = 0; l < L; l++) off += idx_level_cap(a.t[t].m.idx_cap, l);
        ulonglong2 k = a.t[t].m.skey[0][off + d];
        if (hit(kVwSkey, t, d) && a.ov.level == L) k.x ^= a.ov.hi, k.y ^= a.ov.lo;
        return k;
    }
    __device__ __forceinline__ int64_t dir(int64_t v) const {
        int32_t c = a.t[0].m.dir[v];
        if (hit(kVwDir, 0, v)) c ^= (int32_t)a.ov.lo;
        return c;
    }
    __device__ __forceinline__ uint64_t edir(int64_t v) const {
        uint64_t x = a.t[1].m.edir[v];
        if (hit(kVwEdir, 1, v)) x ^= a.ov.lo;
        return x;
    }
    __device__ __forceinline__ uint64_t tailw(int64_t w) const {
        uint64_t x = a.tail[w];
        if (a.ov.what == kVwTailWord && a.ov.index == w) x ^= a.ov.lo;
        return x;
    }
    // The tail of a key longer than 16 bytes lies inside the used arena.
    __device__ __forceinline__ bool tail_ok(const uint2& l) const {
        return 8 * (int64_t)l.y + 8 * (int64_t)tail_units(l.x) <= a.tail_used;
    }
};

// The full key order (dkey.h key_cmp) over two stored keys, the tails read word by word through
// the accessor (history tails are 8-byte aligned; bytes past the shorter tail are masked off, as
// tail_cmp does).  ok = false: a tail that is needed lies outside the arena, nothing was read.
__device__ __forceinline__ int stored_cmp(const Rd& r, const ulonglong2& ka, const uint2& la, const ulonglong2& kb,
                                          const uint2& lb, bool& ok) {
    ok = true;
    if (ka.x != kb.x) return ka.x < kb.x ? -1 : 1;
    if (ka.y != kb.y) return ka.y < kb.y ? -1 : 1;
    if (la.x > 16u && lb.x > 16u) {
        if (!r.tail_ok(la) || !r.tail_ok(lb)) {
            ok = false;
            return 0;
        }
        const int64_t nb = (int64_t)(la.x < lb.x ? la.x : lb.x) - 16;  // <= tail_used: both tails are inside
        for (int64_t o = 0; o < nb; o += 8) {
            const int64_t vb = nb - o;
            const uint64_t msk = vb >= 8 ? ~0ull : ~0ull << (64 - 8 * vb);
            const uint64_t x = __builtin_bswap64(r.tailw((int64_t)la.y + o / 8)) & msk;
            const uint64_t y = __builtin_bswap64(r.tailw((int64_t)lb.y + o / 8)) & msk;
            if (x != y) return x < y ? -1 : 1;
        }
    }
    return (la.x > lb.x) - (la.x < lb.x);
}

// Per-lane tallies of the classes one kernel checks, flushed once per workgroup: LDS atomics, then
// one global atomic per word that is not zero.
template <int N>
struct Tally {
    uint32_t ex[N] = {}, vi[N] = {};
    unsigned long long first[N];
    __device__ __forceinline__ Tally() {
        for (int c = 0; c < N; c++) first[c] = ~0ull;
    }
    __device__ __forceinline__ void note(int c, bool on, bool bad, int64_t idx) {
        if (!on) return;
        ex[c]++;
        if (bad) {
            vi[c]++;
            if ((unsigned long long)idx < first[c]) first[c] = (unsigned long long)idx;
        }
    }
    // cls[c]: the VerifyClass of local class c.  Every thread of the workgroup calls it.
    __device__ __forceinline__ void flush(const VerifyArgs& a, int tier, const int (&cls)[N]) {
        __shared__ unsigned long long s_cnt[2 * N], s_first[N];
        for (int i = threadIdx.x; i < 2 * N; i += blockDim.x) s_cnt[i] = 0;
        for (int i = threadIdx.x; i < N; i += blockDim.x) s_first[i] = ~0ull;
        __syncthreads();
        for (int c = 0; c < N; c++) {
            if (ex[c]) atomicAdd(&s_cnt[2 * c], (unsigned long long)ex[c]);
            if (vi[c]) {
                atomicAdd(&s_cnt[2 * c + 1], (unsigned long long)vi[c]);
                atomicMin(&s_first[c], first[c]);
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * N; i += blockDim.x)
            if (s_cnt[i]) atomicAdd(&a.words[vf_count(tier, cls[i / 2], i & 1)], s_cnt[i]);
        for (int i = threadIdx.x; i < N; i += blockDim.x)
            if (s_first[i] != ~0ull) atomicMin(&a.words[vf_first(tier, cls[i])], s_first[i]);
    }
};

__device__ __forceinline__ bool on(const VerifyArgs& a, int cls) { return (a.checks >> cls) & 1u; }

// ---- pass 1: keys, (len, tail) and versions, one wave per 64-boundary block (the epilogue's
// geometry): ORDER, PADDING, TAILS, VERSIONS, LVL1, SKEY8 and the sample tree SKEY.
__global__ __launch_bounds__(kVfThreads) void k_verify_blocks(VerifyArgs a, int tier) {
    enum { cOrder, cPadding, cTails, cVersions, cLvl1, cSkey8, cSkey, cN };
    const int cls[cN] = {kVcOrder, kVcPadding, kVcTails, kVcVersions, kVcLvl1, kVcSkey8, kVcSkey};
    const Rd r{a};
    Tally<cN> t;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t n = a.t[tier].n, n1 = (n + kFan - 1) / kFan;
    for (int64_t b = (int64_t)blockIdx.x * kVfWaves + wid; b < n1; b += (int64_t)gridDim.x * kVfWaves) {
        const int64_t i = b * kFan + lane;
        const bool live = i < n;
        ulonglong2 k = make_ulonglong2(0, 0);
        uint2 l = make_uint2(0, 0);
        int64_t v = LLONG_MIN;
        if (live) k = r.key(tier, i), l = r.lt(tier, i), v = r.ver(tier, i);
        // PADDING: prefix bytes at and past len are zero
        if (live) {
            const uint64_t mh = l.x >= 8u ? 0ull : ~0ull >> (8 * l.x);
            const uint64_t ml = l.x >= 16u ? 0ull : (l.x <= 8u ? ~0ull : ~0ull >> (8 * (l.x - 8u)));
            t.note(cPadding, on(a, kVcPadding), (k.x & mh) != 0 || (k.y & ml) != 0, i);
        }
        // TAILS: a long key's tail lies inside the used arena (a short key's tail unit is never read)
        if (live && l.x > 16u) t.note(cTails, on(a, kVcTails), !r.tail_ok(l), i);
        // VERSIONS: the base has no hole
        if (live && tier == 0) t.note(cVersions, on(a, kVcVersions), v == kHole, i);
        // ORDER: key[i] < key[i + 1]; the next lane's key, the next block's first for lane 63
        {
            ulonglong2 kn;
            uint2 ln;
            kn.x = __shfl_down(k.x, 1, 64), kn.y = __shfl_down(k.y, 1, 64);
            ln.x = __shfl_down(l.x, 1, 64), ln.y = __shfl_down(l.y, 1, 64);
            const bool pair = i + 1 < n && on(a, kVcOrder);
            if (pair && lane == 63) kn = r.key(tier, i + 1), ln = r.lt(tier, i + 1);
            if (pair) {
                bool ok;
                const int c = stored_cmp(r, k, l, kn, ln, ok);
                t.note(cOrder, true, ok && c >= 0, i);
            }
        }
        // LVL1: the block's maximum
        int64_t x = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t y = __shfl_xor(x, o, 64);
            x = y > x ? y : x;
        }
        if (lane == 0) t.note(cLvl1, on(a, kVcLvl1), r.lvl(tier, 1, b) != x, b);
        // SKEY8: every 8th boundary's prefix
        if (live && (lane & 7) == 0) {
            const ulonglong2 s = r.skey8(tier, i / 8);
            t.note(cSkey8, on(a, kVcSkey8), s.x != k.x || s.y != k.y, i / 8);
        }
        // SKEY: block b is entry b / 8^L of level L when divisible; lane L checks level L
        {
            const uint64_t k0x = __shfl(k.x, 0, 64), k0y = __shfl(k.y, 0, 64);
            if (lane < kIdxLevels && on(a, kVcSkey)) {
                int64_t d = b;
                bool mine = true;
                for (int L = 0; L < lane; L++) {
                    mine = mine && d % kArity == 0;
                    d /= kArity;
                }
                if (mine) {
                    const ulonglong2 s = r.skey(tier, lane, d);
                    t.note(cSkey, true, s.x != k0x || s.y != k0y, (int64_t)lane << 48 | d);
                }
            }
        }
    }
    t.flush(a, tier, cls);
}

// Level-3 spans' true maxima, order-preserved as unsigned words (0: LLONG_MIN, what a memset gives).
__device__ __forceinline__ unsigned long long ord(int64_t v) { return (unsigned long long)v ^ (1ull << 63); }

// ---- pass 2: one wave per level-2 entry: the true maximum of its 4096 versions against lvl[2],
// and into its level-3 span's true maximum (true3).
__global__ __launch_bounds__(kVfThreads) void k_verify_lvl2(VerifyArgs a, int tier, unsigned long long* true3) {
    enum { cLvl2, cN };
    const int cls[cN] = {kVcLvl2};
    const Rd r{a};
    Tally<cN> t;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t n = a.t[tier].n, span = (int64_t)kFan * kFan, n2 = (n + span - 1) / span;
    for (int64_t c = (int64_t)blockIdx.x * kVfWaves + wid; c < n2; c += (int64_t)gridDim.x * kVfWaves) {
        int64_t x = LLONG_MIN;
        for (int q = 0; q < kFan; q++) {
            const int64_t i = c * span + q * kFan + lane;
            if (i < n) {
                const int64_t v = r.ver(tier, i);
                x = v > x ? v : x;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t y = __shfl_xor(x, o, 64);
            x = y > x ? y : x;
        }
        if (lane == 0) {
            t.note(cLvl2, on(a, kVcLvl2), r.lvl(tier, 2, c) != x, c);
            atomicMax(&true3[c / kFan], ord(x));
        }
    }
    t.flush(a, tier, cls);
}

// ---- pass 3: one lane per level-3 entry: every replica at most the span's maximum, one equal to it.
__global__ __launch_bounds__(kVfThreads) void k_verify_lvl3(VerifyArgs a, int tier, const unsigned long long* true3) {
    enum { cLvl3, cN };
    const int cls[cN] = {kVcLvl3};
    const Rd r{a};
    Tally<cN> t;
    const int64_t n = a.t[tier].n, span = (int64_t)kFan * kFan * kFan, n3 = (n + span - 1) / span;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n3; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long want = true3[j];
        unsigned long long top = 0;
        for (int q = 0; q < kL3Rep; q++) {
            const unsigned long long x = ord(r.lvl(tier, 3, j * kL3Rep + q));
            top = x > top ? x : top;
        }
        t.note(cLvl3, on(a, kVcLvl3), top != want, j);
    }
    t.flush(a, tier, cls);
}

// ---- pass 4: one lane per directory slot v in [0, dir_top + 1]: the entry's count c is the number
// of group starts (keys[8 e], e < S) whose slot is below v iff c lies in [0, S], start c - 1 has a
// slot below v and start c has not (the starts' slots do not decrease: checked beside it, one lane
// per start, reported at the slot of the start that stands too low).  The delta's entries carry an
// epoch tag: those of the current epoch are counted (trusted) and checked, the others skipped.
__global__ __launch_bounds__(kVfThreads) void k_verify_dir(VerifyArgs a, int tier) {
    enum { cDir, cN };
    const int cls[cN] = {tier ? kVcEdir : kVcDir};
    const Rd r{a};
    Tally<cN> t;
    const MaxLevels& m = a.t[tier].m;
    const int64_t n = a.t[tier].n, S = (n + 7) / 8, slots = (int64_t)m.dir_top + 2;
    const bool check = on(a, cls[0]);
    uint32_t trusted = 0;
    const int64_t work = slots > S ? slots : S;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < work; v += (int64_t)gridDim.x * blockDim.x) {
        if (v < slots) {
            int64_t c;
            bool mine = true;
            if (tier) {
                const uint64_t x = r.edir(v);
                mine = (uint32_t)(x >> 32) == m.edir_epoch;
                trusted += mine;
                c = (int64_t)(uint32_t)x;
            } else {
                c = r.dir(v);
            }
            if (mine && check) {
                bool bad = c < 0 || c > S;
                if (!bad && c > 0) {
                    const ulonglong2 k = r.key(tier, 8 * (c - 1));
                    bad = (int64_t)dir_slot(m, k.x, k.y) >= v;
                }
                if (!bad && c < S) {
                    const ulonglong2 k = r.key(tier, 8 * c);
                    bad = (int64_t)dir_slot(m, k.x, k.y) < v;
                }
                t.note(cDir, true, bad, v);
            }
        }
        if (check && v >= 1 && v < S) {
            const ulonglong2 k0 = r.key(tier, 8 * (v - 1)), k1 = r.key(tier, 8 * v);
            const uint32_t s0 = dir_slot(m, k0.x, k0.y), s1 = dir_slot(m, k1.x, k1.y);
            if (s1 < s0) {
                t.vi[cDir]++;
                if (s1 < t.first[cDir]) t.first[cDir] = s1;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) trusted += __shfl_xor(trusted, o, 64);
    if (tier && trusted && (threadIdx.x & 63) == 0) atomicAdd(&a.words[kVfTrusted], (unsigned long long)trusted);
    t.flush(a, tier, cls);
}

// Boundaries of tier `ts` at or below key (k, l): one plain binary search over its keys with the
// full comparison.  eq: the last of them equals the key.  ok = false: a needed tail lies outside
// the arena.
__device__ __forceinline__ int64_t count_le(const Rd& r, int ts, const ulonglong2& k, const uint2& l, bool& eq, bool& ok) {
    int64_t lo = 0, hi = r.a.t[ts].n;
    eq = false;
    ok = true;
    for (int it = 0; it < kSearchSteps && lo < hi; it++) {
        const int64_t mid = (lo + hi) >> 1;
        bool ok1;
        const int c = stored_cmp(r, r.key(ts, mid), r.lt(ts, mid), k, l, ok1);
        if (!ok1) {
            ok = false;
            return 0;
        }
        if (c <= 0) {
            lo = mid + 1;
            eq = eq || c == 0;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// ---- pass 5: DOMINANCE, one lane per boundary of each tier.  A delta boundary j with a version v
// looks up the base boundary at or below its key (the header if none); a base boundary looks up the
// delta boundary below its key (an equal key is the delta lane's pair).  Each pair whose base
// version exceeds v is one violation, reported at j.
__global__ __launch_bounds__(kVfThreads) void k_verify_dominance(VerifyArgs a) {
    enum { cDom, cN };
    const int cls[cN] = {kVcDominance};
    const Rd r{a};
    Tally<cN> t;
    const int64_t nb = a.t[0].n, nd = a.t[1].n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nb + nd; e += (int64_t)gridDim.x * blockDim.x) {
        bool eq, ok;
        if (e < nd) {
            const int64_t v = r.ver(1, e);
            if (v == kHole) continue;
            const int64_t p = count_le(r, 0, r.key(1, e), r.lt(1, e), eq, ok);
            if (!ok) continue;
            t.note(cDom, true, (p > 0 ? r.ver(0, p - 1) : a.hdr) > v, e);
        } else {
            const int64_t i = e - nd;
            const int64_t q = count_le(r, 1, r.key(0, i), r.lt(0, i), eq, ok);
            if (!ok || q == 0 || eq) continue;
            const int64_t v = r.ver(1, q - 1);
            if (v == kHole) continue;
            t.note(cDom, true, r.ver(0, i) > v, q - 1);
        }
    }
    t.flush(a, 1, cls);
}

unsigned grid_for(int64_t items, int per_group) {
    const int64_t g = (items + per_group - 1) / per_group;
    return (unsigned)std::min<int64_t>(std::max<int64_t>(g, 1), kVfMaxGrid);
}

}  // namespace

void launch_verify(hipStream_t s, const VerifyArgs& a) {
    constexpr uint32_t kBlocks = 1u << kVcOrder | 1u << kVcPadding | 1u << kVcTails | 1u << kVcVersions |
                                 1u << kVcLvl1 | 1u << kVcSkey8 | 1u << kVcSkey;
    unsigned long long* true3 = a.words + kVfWords;  // per tier: its level-3 entries, zeroed by the caller
    for (int t = 0; t < 2; t++) {
        const int64_t n = a.t[t].n;
        const int64_t n2 = (n + (int64_t)kFan * kFan - 1) / ((int64_t)kFan * kFan), n3 = (n2 + kFan - 1) / kFan;
        if (n > 0 && (a.checks & kBlocks))
            fdb_launch(k_verify_blocks, dim3(grid_for((n + kFan - 1) / kFan, kVfWaves)), dim3(kVfThreads), 0, s, a, t);
        if (n > 0 && (a.checks & (1u << kVcLvl2 | 1u << kVcLvl3))) {
            fdb_launch(k_verify_lvl2, dim3(grid_for(n2, kVfWaves)), dim3(kVfThreads), 0, s, a, t, true3);
            if (a.checks & (1u << kVcLvl3))
                fdb_launch(k_verify_lvl3, dim3(grid_for(n3, kVfThreads)), dim3(kVfThreads), 0, s, a, t,
                           (const unsigned long long*)true3);
        }
        true3 += n3;
        const bool has = t ? a.t[1].has_edir && a.t[1].m.edir_epoch != 0 : a.t[0].has_dir != 0;
        if (n > 0 && has && (a.checks & (1u << (t ? kVcEdir : kVcDir))))
            fdb_launch(k_verify_dir, dim3(grid_for(std::max<int64_t>((int64_t)a.t[t].m.dir_top + 2, (n + 7) / 8), kVfThreads)),
                       dim3(kVfThreads), 0, s, a, t);
    }
    if (a.t[1].n > 0 && (a.checks & (1u << kVcDominance)))
        fdb_launch(k_verify_dominance, dim3(grid_for(a.t[0].n + a.t[1].n, kVfThreads)), dim3(kVfThreads), 0, s, a);
}

}  // namespace fdbcs
