// engine.cpp — host side of the MI355X conflict-resolution engine and its C-ABI
// (include/fdb_conflict_set.h).
//
// Mirrors the reference ConflictSet / ConflictBatch lifecycle (fdbserver/SkipList.cpp:730-890):
// addTransaction packs each transaction's conflict ranges into flat SoA buffers of normalized
// key prefixes plus a tail arena; detectConflicts uploads the batch with one pinned H2D copy,
// enqueues the kernel pipeline on the set's stream, and copies back one verdict byte per
// transaction.  No CPU fallback exists: without a usable HIP device every entry point fails.
// The entry points of the maintenance side (history export and import, the iops sample) are in
// transfer.cpp; the set's state both files work on is in engine_impl.h.
#include "engine_impl.h"

// Base-tier size from which the read check splits by default (FDBCS_SPLIT_CHECK=2).
constexpr int64_t kSplitCheckMinBase = 16 << 20;

namespace fdbcs::impl {

void add_key(fdbcs_batch* b, std::vector<DKey>& out, const uint8_t* p, int32_t len) {
    DKey k;
    dkey_prefix(p, (uint32_t)len, &k.hi, &k.lo);
    k.len = (uint32_t)len;
    k.tail = 0;
    if (len > b->max_len) b->max_len = len;
    if (len > 16) {
        k.tail = (uint32_t)b->tail.size();
        b->tail.insert(b->tail.end(), p + 16, p + len);
    }
    out.push_back(k);
}

int cmp_bytes(const uint8_t* a, int32_t al, const uint8_t* b, int32_t bl) {
    int c = memcmp(a, b, (size_t)std::min(al, bl));
    if (c) return c;
    return (al > bl) - (al < bl);
}

// Scan arena for the current workspace shape and history capacity (zeroed per batch by k_prepare).
int ensure_scan_arena(fdbcs_conflict_set* cs) {
    if (cs->ws_T < 0 || cs->hist_cap <= 0) return FDBCS_OK;
    if (cs->delta_cap <= 0) return FDBCS_OK;
    const int64_t words = scan_arena_words(cs->ws_T, cs->ws_R, cs->ws_W, cs->hist_cap, cs->delta_cap);
    for (int k = 0; k < kNumWork; k++) {
        Work& w = cs->work[k];
        int rc = cs->ws[k][kWsArenaSlot].ensure(8 * words + 64);
        if (rc) return rc;
        w.scan_arena = (uint64_t*)cs->ws[k][kWsArenaSlot].p;
        if ((rc = cs->ws[k][kWsTileSlot].ensure(4 * (std::max(cs->hist_cap, cs->delta_cap) / 256 + 8)))) return rc;
        w.tile_first = (int32_t*)cs->ws[k][kWsTileSlot].p;
        carve_scans(w, cs->ws_T, cs->ws_R, cs->ws_W, cs->hist_cap, cs->delta_cap);
        HIPOK(hipMemsetAsync(w.scan_arena, 0, 8 * w.scan_words, cs->stream));
        for (int q = 0; q < kNumScans; q++) w.scan[q].error = &w.bsc->debug_error;
    }
    HIPOK(hipStreamSynchronize(cs->stream));
    return FDBCS_OK;
}

int flush_pending(fdbcs_conflict_set* cs, const fdbcs_batch* upto = nullptr);

// Both streams idle (before reallocating anything either stage uses).
int sync_all(fdbcs_conflict_set* cs) {
    if (int rc = flush_pending(cs)) return rc;
    HIPOK(hipStreamSynchronize(cs->ustream));
    HIPOK(hipStreamSynchronize(cs->cstream));
    HIPOK(hipStreamSynchronize(cs->astream));
    HIPOK(hipStreamSynchronize(cs->stream));
    HIPOK(hipStreamSynchronize(cs->ystream));
    cs->prev_segs = false;  // everything submitted is merged: the next check reads the current delta
    return FDBCS_OK;
}

// Each workspace's copy of a batch tail region (Work::btail) for `bytes`.
int ensure_btail(fdbcs_conflict_set* cs, int64_t bytes) {
    const size_t need = (size_t)bytes + 64;
    if (cs->wbtail[0].p && need <= cs->wbtail[0].cap) return FDBCS_OK;
    if (int rc = sync_all(cs)) return rc;
    for (int k = 0; k < kNumWork; k++) {
        if (int rc = cs->wbtail[k].ensure(std::max<size_t>(need, 1 << 16))) return rc;
        cs->work[k].btail = (uint8_t*)cs->wbtail[k].p;
    }
    return FDBCS_OK;
}

// Workspace sized for (T, R, W); edge capacity grows with R.
int ensure_workspace(fdbcs_conflict_set* cs, int64_t T, int64_t R, int64_t W) {
    if (T <= cs->ws_T && R <= cs->ws_R && W <= cs->ws_W) return FDBCS_OK;
    T = std::max<int64_t>(T, std::max<int64_t>(cs->ws_T, 1024));
    R = std::max<int64_t>(R, std::max<int64_t>(cs->ws_R, 4096));
    W = std::max<int64_t>(W, std::max<int64_t>(cs->ws_W, 4096));
    if (int rc = sync_all(cs)) return rc;
    const int64_t E = 2 * (R + W);
    int64_t edge_cap = std::max<int64_t>(16 * R, 1 << 22);
    if (const char* env = getenv("FDBCS_EDGE_CAP")) edge_cap = std::max<int64_t>(1, atoll(env));  // testing knob
    for (int k = 0; k < kNumWork; k++) {
    Work& w = cs->work[k];
    // One arena per workspace (slot 0), its size a multiple of 2 MiB: the ~50 scratch arrays of a
    // batch share a few large pages instead of one small allocation each (every kernel touches a
    // dozen of them; a single-workgroup kernel's first loads otherwise wait on address
    // translation misses).  Two passes: sizes, then the carve.
    size_t off = 0;
    char* arena = nullptr;
    auto take = [&](size_t bytes, void** ptr) -> int {
        off = align_up(off, 256);
        if (arena) *ptr = arena + off;
        off += bytes + 64;
        return FDBCS_OK;
    };
    for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
        if (int rc = cs->ws[k][0].ensure(align_up(off, (size_t)2 << 20))) return rc;
        arena = (char*)cs->ws[k][0].p;
        off = 0;
    }
#define TAKE(field, bytes) \
    if (int rc = take((bytes), (void**)&w.field)) return rc
    TAKE(hist_conf, T);
    TAKE(rconf, R);
    TAKE(status, T);
    TAKE(first_conf, 4 * T);
    // the sort's slab holds kSlab endpoints per bucket for the buckets a batch of E endpoints
    // takes at the default target (sort_bucket_count clamps smaller targets to it)
    const int64_t slab_buckets = std::min<int64_t>(kSortMaxBuckets, (E + kSortTarget - 1) / kSortTarget + 1);
    TAKE(items, sizeof(SortItem) * E);
    TAKE(scnt, 8 * kCntStride * (size_t)kSortMaxBuckets);
    TAKE(slab, sizeof(SortItem) * kSlab * slab_buckets);
    TAKE(ovf, sizeof(SortItem) * E);
    TAKE(ovf_b, 4 * E);
    TAKE(big, sizeof(SortItem) * E);
    TAKE(big_p, 4 * E);
    TAKE(samples, sizeof(SortItem) * kMaxSample);
    TAKE(srank, 4 * (kMaxSample + 64));
    w.slab_buckets = (int32_t)slab_buckets;
    TAKE(erec, sizeof(int4) * E);
    TAKE(wends, 8 * (2 * W + 1));
    TAKE(wkeys, sizeof(DKey) * (2 * W + 1));
    TAKE(segk, sizeof(DKey) * (2 * W + 2));
    TAKE(cflag, 2 * W + 2);
    TAKE(wbrange, 4 * W);
    TAKE(wlead, 4 * (W + 1));
    TAKE(wtxn, 4 * (W + 1));
    TAKE(gminc, 4 * (W + 1));
    TAKE(rbrange, 4 * R);
    TAKE(eoff, 4 * (R + 1));
    TAKE(poff, 4 * (R + W + 1));
    TAKE(pcg, 4 * (R + W + 1));
    TAKE(pcoff, 4 * (R + W + 1));
    TAKE(pcbase, 4 * (R + W + 1));
    TAKE(pca, 4 * (R + W + 1));
    TAKE(ecur, 4 * R);
    TAKE(edges, 4 * edge_cap);
    TAKE(eptr, 4 * T);
    TAKE(pre_st, T);
    TAKE(pre_ep, 4 * T);
    TAKE(pre_end, 4 * T);
    TAKE(ulist, 32 * T);
    TAKE(wpk, 4 * (W + 1));
    TAKE(tedges, 4 * edge_cap);
    TAKE(mcs_bits, 8 * (E / 64 + 2));
    TAKE(seg_lo, 8 * (W + 1));
    TAKE(seg_hi, 8 * (W + 1));
    TAKE(seg_rem, 8 * (W + 1));
    TAKE(seg_ins, 8 * (W + 1));
    TAKE(seg_tlen, 8 * (W + 1));
    TAKE(seg_endins, W + 1);
    TAKE(seg_vend, 8 * (W + 1));
    TAKE(verdict, T);
    TAKE(bsc, sizeof(BatchScalars));
    }
#undef TAKE
    w.edge_cap = edge_cap;
    w.cap_T = T;
    w.cap_R = R;
    // the epilogue of every batch re-zeroes these for the batch after next; start them zeroed
    HIPOK(hipMemsetAsync(w.hist_conf, 0, T, cs->stream));
    HIPOK(hipMemsetAsync(w.rconf, 0, R, cs->stream));
    HIPOK(hipMemsetAsync(w.ecur, 0, 4 * R, cs->stream));
    HIPOK(hipMemsetAsync(w.scnt, 0, 8 * kCntStride * (size_t)kSortMaxBuckets, cs->stream));
    HIPOK(hipMemsetAsync(w.srank, 0, 4 * (kMaxSample + 64), cs->stream));
    HIPOK(hipMemsetAsync(w.bsc, 0, sizeof(BatchScalars), cs->stream));
    // compaction arrays are shared (stage B only)
    if (k >= 1) {
        Work& w0 = cs->work[0];
        w.c_lo = w0.c_lo, w.c_hi = w0.c_hi, w.c_rem = w0.c_rem, w.c_ins = w0.c_ins, w.c_val = w0.c_val;
        w.c_exact = w0.c_exact;
    }
    }
    cs->edge_cap = edge_cap;
    cs->prev_segs = false;  // the last batch's segments were in the old arrays (and are merged: synced)
    cs->ws_T = T;
    cs->ws_R = R;
    cs->ws_W = W;
    return ensure_scan_arena(cs);
}

// Automatic delta bound: about 1/16 of the base, so a batch's merge touches a small tier and a
// compaction (a full rewrite of the base) is amortised over many batches.
// The delta tier's bound: N/16, raised towards N/4 up to kDeltaFloor boundaries.  A compaction
// rewrites the whole base on Y and the next check waits for it, so on a 5M-boundary base fewer,
// larger deltas pay although every merge copies more: C2 54.6 -> 56.7M, C3 45.9 -> 50.4M, C2 at
// 32768-txn batches 91.1 -> 92.9M over 150-400-batch windows with a 1.25M bound
// (scripts/gpu_r05_dl*.sh); a 50M base (C4) keeps N/16 = 3.1M.
constexpr int64_t kDeltaFloor = 1250000;
constexpr int kTimingEvery = 4;  // timing level 1 times the hot kernels of 1 batch in kTimingEvery
int64_t delta_limit_for(const fdbcs_conflict_set* cs, int64_t n_base) {
    if (cs->delta_limit > 0) return cs->delta_limit;
    return std::max<int64_t>({(int64_t)1 << 16, n_base / 16, std::min<int64_t>(n_base / 4, kDeltaFloor)});
}


Hist hist_of(fdbcs_conflict_set* cs, int k) {
    Hist h;
    h.key = (ulonglong2*)cs->hkey[k].p;
    h.lt = (uint2*)cs->hlt[k].p;
    h.ver = (int64_t*)cs->hver[k].p;
    return h;
}

// Search-tree levels laid out back to back in one allocation sized for `cap` boundaries.
void carve_index(MaxLevels& m, ulonglong2* base, int64_t cap) {
    for (int L = 0; L < kIdxLevels; L++) {
        m.skey[L] = base;
        base += idx_level_cap(cap, L);
    }
    m.skey8 = base;  // cap / 8 + 2 entries
    m.idx_cap = cap;
}

int64_t index_bytes(int64_t cap) {
    int64_t n = 0;
    for (int L = 0; L < kIdxLevels; L++) n += idx_level_cap(cap, L);
    return 16 * (n + cap / 8 + 2);
}

static void set_dir_fields(const fdbcs_conflict_set* cs, MaxLevels& m) {
    m.dir_p = cs->dir_p;
    m.dir_phi = cs->dir_phi;
    m.dir_plo = cs->dir_plo;
    m.dir_e = cs->dir_e;
    m.dir_top = cs->dir_top;
    for (int i = 0; i < kDirPos; i++) m.dir_pos[i] = cs->dir_pos[i], m.dir_w[i] = cs->dir_w[i];
}

// The directory code of the keys k[0..n) (sorted): their common prefix and, after it, the range
// of byte values at each position while the product of the ranges fits the slot budget (the last
// position coarsened by a shift).  See MaxLevels::dir_p.  Large loads are sampled (at most ~2M
// keys); values outside a position's range get the range's end codes.
static int set_dir_map(fdbcs_conflict_set* cs, const ulonglong2* k, int64_t n) {
    auto byte_at = [](const ulonglong2& x, int i) -> uint32_t {
        return i < 8 ? (uint32_t)(x.x >> (56 - 8 * i)) & 255u : (uint32_t)(x.y >> (56 - 8 * (i - 8))) & 255u;
    };
    const bool rank = n >= 2;
    uint32_t p = 0;
    if (rank) {
        const uint64_t xh = k[0].x ^ k[n - 1].x, xl = k[0].y ^ k[n - 1].y;
        const uint32_t lcp = xh ? (uint32_t)__builtin_clzll(xh) / 8 : (xl ? 8 + (uint32_t)__builtin_clzll(xl) / 8 : 16);
        p = std::min<uint32_t>(lcp, 15);
    }
    const uint64_t mh = p >= 8 ? ~0ull : (p ? ~0ull << (64 - 8 * p) : 0ull);
    const uint64_t ml = p <= 8 ? 0ull : ~0ull << (128 - 8 * p);
    cs->dir_p = p;
    cs->dir_phi = n ? k[0].x & mh : 0;
    cs->dir_plo = n ? k[0].y & ml : 0;
    const int npos = std::min<int>(kDirPos, 16 - (int)p);
    uint32_t lo[kDirPos], hi[kDirPos];
    for (int i = 0; i < kDirPos; i++) lo[i] = rank ? 255 : 0, hi[i] = 255;
    if (rank) {
        for (int i = 0; i < kDirPos; i++) hi[i] = 0;
        const int64_t stride = std::max<int64_t>(1, n / (1 << 21));
        auto mark = [&](const ulonglong2& x) {
            for (int i = 0; i < npos; i++) {
                const uint32_t b = byte_at(x, (int)p + i);
                lo[i] = std::min(lo[i], b);
                hi[i] = std::max(hi[i], b);
            }
        };
        for (int64_t j = 0; j < n; j += stride) mark(k[j]);
        mark(k[n - 1]);
    }
    const int64_t samples = (n + kFan - 1) / kFan;
    uint64_t budget = 1ull << 16;
    if (cs->dir_bits)
        budget = 1ull << cs->dir_bits;
    else
        while (budget < (1ull << kDirMaxBits) && 8 * budget < (uint64_t)samples) budget <<= 1;
    uint32_t radix[kDirPos], shift[kDirPos];
    uint64_t prod = 1;
    int e = 0;
    for (int i = 0; i < npos; i++) {
        const uint32_t d = hi[i] - lo[i] + 1;
        shift[i] = 0;
        if (prod * d <= budget) {
            radix[i] = d;
            prod *= d;
            if (d > 1) e = i + 1;  // trailing single-value positions add nothing
            continue;
        }
        uint32_t s = 0;  // coarsen: digit >> s, radix ((d - 1) >> s) + 1
        while (prod * (((d - 1) >> s) + 1) > budget) s++;
        if (((d - 1) >> s) + 1 > 1) {
            radix[i] = ((d - 1) >> s) + 1;
            shift[i] = s;
            e = i + 1;
        }
        break;
    }
    prod = 1;
    for (int i = 0; i < e; i++) prod *= radix[i];
    uint64_t w = 1;
    for (int i = kDirPos - 1; i >= 0; i--) {
        if (i >= e) {
            cs->dir_pos[i] = cs->dir_w[i] = 0;
            continue;
        }
        cs->dir_pos[i] = lo[i] | (hi[i] - lo[i] + 1) << 8 | shift[i] << 17;
        cs->dir_w[i] = (uint32_t)w;
        w *= radix[i];
    }
    cs->dir_e = (uint32_t)e;
    // codes run over [0, prod] (prod: above the range at the first position), slots are code + 1,
    // 0 below the common prefix and prod + 2 above it
    cs->dir_top = (uint32_t)prod + 2;
    return FDBCS_OK;
}

MaxLevels levels_of(fdbcs_conflict_set* cs, int k) {
    MaxLevels m;
    m.lvl[0] = (int64_t*)cs->hver[k].p;
    for (int L = 1; L < kMaxLevels; L++) m.lvl[L] = (int64_t*)cs->lvl[L].p;
    m.keys = (const ulonglong2*)cs->hkey[k].p;
    carve_index(m, (ulonglong2*)cs->lvl[0].p, cs->hist_cap);
    m.dir = cs->directory ? (const int32_t*)cs->dir.p : nullptr;
    set_dir_fields(cs, m);
    return m;
}

Hist delta_of(fdbcs_conflict_set* cs, int k) {
    Hist h;
    h.key = (ulonglong2*)cs->dkey[k].p;
    h.lt = (uint2*)cs->dlt[k].p;
    h.ver = (int64_t*)cs->dver[k].p;
    return h;
}

MaxLevels dlevels_of(fdbcs_conflict_set* cs, int k) {
    MaxLevels m;
    m.lvl[0] = (int64_t*)cs->dver[k].p;
    for (int L = 1; L < kMaxLevels; L++) m.lvl[L] = (int64_t*)cs->dlvl[k][L].p;
    m.keys = (const ulonglong2*)cs->dkey[k].p;
    carve_index(m, (ulonglong2*)cs->dlvl[k][0].p, cs->delta_cap);
    m.edir = (uint64_t*)cs->edir[k].p;
    m.edir_epoch = cs->edir[k].p ? cs->ddir_epoch[k] : 0;
    set_dir_fields(cs, m);  // the delta's directory slots too (the epilogue's fill)
    return m;
}

// Read the exact history size/tail usage back (synchronizes the stream).
int sync_sizes(fdbcs_conflict_set* cs) {
    if (int rc = sync_all(cs)) return rc;  // both halves of stage B
    Scalars s;
    HIPOK(hipMemcpyAsync(&s, cs->scal.p, sizeof(s), hipMemcpyDeviceToHost, cs->stream));
    HIPOK(hipStreamSynchronize(cs->stream));
    cs->n_ub = s.n;
    cs->nd_ub = s.nd;
    cs->tail_ub = s.tail_used;
    return FDBCS_OK;
}

// Range-max hierarchy buffers (and the sampled key index in lv[0]) for `cap` elements; returns the
// top level's length.
int alloc_levels(DBuf* lv, int64_t cap, int64_t* top_n, int64_t* l2_n) {
    lv[0].release();
    if (int rc = lv[0].ensure(index_bytes(cap))) return rc;
    int64_t m = cap;
    for (int L = 1; L < kMaxLevels; L++) {
        m = (m + kFan - 1) / kFan + 1;
        lv[L].release();
        if (int rc = lv[L].ensure(8 * (L == kMaxLevels - 1 ? l3_words(m) : m))) return rc;
        if (L == 2) *l2_n = m;
    }
    *top_n = m;
    return FDBCS_OK;
}

// Grow one ping-pong buffer set pair to `cap` elements, keeping the live `n` of set `live`.
int grow_sets(fdbcs_conflict_set* cs, DBuf* key, DBuf* lt, DBuf* ver, int live, int64_t n, int64_t cap) {
    int rc;
    for (int k = 0; k < 2; k++) {
        DBuf nk, nl, nv;
        if ((rc = nk.ensure(16 * cap)) || (rc = nl.ensure(8 * cap)) || (rc = nv.ensure(8 * cap))) return rc;
        if (k == live && n) {
            HIPOK(hipMemcpyAsync(nk.p, key[k].p, 16 * n, hipMemcpyDeviceToDevice, cs->stream));
            HIPOK(hipMemcpyAsync(nl.p, lt[k].p, 8 * n, hipMemcpyDeviceToDevice, cs->stream));
            HIPOK(hipMemcpyAsync(nv.p, ver[k].p, 8 * n, hipMemcpyDeviceToDevice, cs->stream));
        }
        HIPOK(hipStreamSynchronize(cs->stream));
        key[k] = std::move(nk);
        lt[k] = std::move(nl);
        ver[k] = std::move(nv);
    }
    return FDBCS_OK;
}

// Delta-tier capacity for `need` boundaries (plus the compaction arrays sized to match).
int ensure_delta(fdbcs_conflict_set* cs, int64_t need) {
    if (need <= cs->delta_cap) return FDBCS_OK;
    int rc = sync_sizes(cs);
    if (rc) return rc;
    int64_t cap = std::max<int64_t>(need, cs->delta_cap);
    cap = std::max<int64_t>(cap + cap / 2, 1 << 14);
    if ((rc = grow_sets(cs, cs->dkey, cs->dlt, cs->dver, cs->dcur, cs->nd_ub, cap))) return rc;
    for (int k = 0; k < 5; k++) {
        cs->cws[k].release();
        if ((rc = cs->cws[k].ensure(8 * (cap + 2)))) return rc;
    }
    cs->cws[5].release();
    if ((rc = cs->cws[5].ensure(cap + 2))) return rc;
    for (Work& w : cs->work) {  // compaction runs on stage B only: both workspaces share the arrays
        int64_t** c64[5] = {&w.c_lo, &w.c_hi, &w.c_rem, &w.c_ins, &w.c_val};
        for (int k = 0; k < 5; k++) *c64[k] = (int64_t*)cs->cws[k].p;
        w.c_exact = (uint8_t*)cs->cws[5].p;
    }
    for (int k = 0; k < 2; k++)
        if ((rc = alloc_levels(cs->dlvl[k], cap, &cs->dlvl3_n, &cs->dlvl2_n))) return rc;
    cs->delta_cap = cap;
    cs->ddir_epoch[0] = cs->ddir_epoch[1] = 0;  // the current delta's levels are rebuilt, its directory not
    cs->prev_segs = false;                      // (sync_sizes drained every stream)
    launch_rangemax(cs->stream, dlevels_of(cs, cs->dcur), (Scalars*)cs->scal.p, &((Scalars*)cs->scal.p)->ndb[cs->dcur],
                    cs->dlvl3_n, cs->dlvl2_n, std::max<int64_t>(cs->nd_ub, 1));
    HIPOK(take_launch_error());
    HIPOK(hipStreamSynchronize(cs->stream));
    return ensure_scan_arena(cs);
}

// Base-tier capacity for `need` boundaries (copies the live history when growing).
int ensure_history(fdbcs_conflict_set* cs, int64_t need, int64_t tail_need) {
    if (need <= cs->hist_cap && tail_need <= cs->tail_cap) return FDBCS_OK;
    int rc = sync_sizes(cs);
    if (rc) return rc;
    const int64_t tail_used = cs->tail_ub;
    if (need > cs->hist_cap) {
        int64_t cap = std::max<int64_t>(need, cs->hist_cap);
        cap = std::max<int64_t>(cap + cap / 4, 1 << 16);
        if ((rc = grow_sets(cs, cs->hkey, cs->hlt, cs->hver, cs->cur, cs->n_ub, cap))) return rc;
        if ((rc = alloc_levels(cs->lvl, cap, &cs->lvl3_n, &cs->lvl2_n))) return rc;
        if (cs->directory && (rc = cs->dir.ensure(4 * (size_t)kDirAlloc))) return rc;
        cs->hist_cap = cap;
        launch_rangemax(cs->stream, levels_of(cs, cs->cur), (Scalars*)cs->scal.p, &((Scalars*)cs->scal.p)->n,
                        cs->lvl3_n, cs->lvl2_n, std::max<int64_t>(cs->n_ub, 1));
        HIPOK(take_launch_error());
    }
    if (tail_need > cs->tail_cap) {
        int64_t tcap = std::max<int64_t>(tail_need, cs->tail_cap);
        tcap = std::max<int64_t>(tcap + tcap / 2, 1 << 16);
        DBuf nt, spare;
        if ((rc = nt.ensure(tcap + kTailSlack)) || (rc = spare.ensure(tcap + kTailSlack))) return rc;
        if (tail_used)
            HIPOK(hipMemcpyAsync(nt.p, cs->htail[cs->tcur].p, tail_used, hipMemcpyDeviceToDevice, cs->stream));
        HIPOK(hipStreamSynchronize(cs->stream));
        cs->htail[cs->tcur] = std::move(nt);
        cs->htail[cs->tcur ^ 1] = std::move(spare);
        cs->tail_cap = tcap;
    }
    HIPOK(hipStreamSynchronize(cs->stream));
    return ensure_scan_arena(cs);
}

// Layout of a batch in pin_in / dev (UploadLayout, engine_impl.h).
// add_packed normalizes keys, owners and tails in place; the tail region is last so a capacity
// sized for an upper bound of the tail bytes costs no upload.
UploadLayout upload_layout(size_t T, size_t R, size_t W, size_t tail_bytes) {
    UploadLayout L;
    size_t off = 0;
    L.keys = off;
    off = align_up(off + sizeof(DKey) * 2 * (R + W), 64);
    L.rown = off;
    off = align_up(off + 4 * R, 64);
    L.wown = off;
    off = align_up(off + 4 * W, 64);
    L.snap = off;
    off = align_up(off + 8 * T, 64);
    L.roff = off;
    off = align_up(off + 4 * (T + 1), 64);
    L.woff = off;
    off = align_up(off + 4 * (T + 1), 64);
    L.flags = off;
    off = align_up(off + T, 64);
    L.tail = off;
    off = align_up(off + tail_bytes + 48, 64);  // slack for dkey.h tail_word
    L.total = off;
    return L;
}

// History tail bytes a key of this length takes when inserted (8-byte aligned, search.h tail_units).
inline int64_t padded_tail(int32_t len) { return len > 16 ? ((int64_t)len - 16 + 7) / 8 * 8 : 0; }

// Prefix words of a key (dkey_prefix), two big-endian loads when the key has 16 bytes or more.
inline void fast_prefix(const uint8_t* p, uint32_t len, uint64_t* hi, uint64_t* lo) {
    if (len >= 16) {
        uint64_t h, l;
        memcpy(&h, p, 8);
        memcpy(&l, p + 8, 8);
        *hi = __builtin_bswap64(h);
        *lo = __builtin_bswap64(l);
    } else {
        dkey_prefix(p, len, hi, lo);
    }
}

// Result buffer of a batch (host-mapped, written by the kernels): verdicts | scalars | completion
// flag, then the report copies rconf | hist | first_conf and, for a routed reporting batch (whose
// transactions the host never saw), roff | flags.
struct ResultLayout {
    size_t sc, fl, rc, hc, fc, ro, fg, total;
};
ResultLayout result_layout(size_t T, size_t R) {
    ResultLayout L;
    L.sc = (size_t)verdict_scalars_offset((int64_t)T);
    L.fl = align_up(L.sc + sizeof(Scalars), 64);
    L.rc = L.fl + 64;
    L.hc = align_up(L.rc + R + 1, 64);
    L.fc = align_up(L.hc + T + 1, 64);
    L.ro = align_up(L.fc + 4 * (T + 1), 64);
    L.fg = align_up(L.ro + 4 * (T + 1), 64);
    L.total = L.fg + T + 1;
    return L;
}

// Every allocation a batch of this shape needs, made at add time so that detect (the timed,
// latency-critical call) never allocates: device copy, pinned result buffer, device verdicts.
int ensure_slot(BatchSlot* sl, size_t upload_bytes, size_t T, size_t R) {
    int rc;
    if ((rc = sl->dev.ensure(upload_bytes))) return rc;
    if ((rc = sl->pin_out.ensure(result_layout(T, R).total, true))) return rc;
    return sl->dverdict.ensure(T + 64);
}

int make_slot_events(BatchSlot* sl) {
    if (sl->events_made) return FDBCS_OK;
    for (Event& e : sl->ev)
        if (int rc = e.make()) return rc;
    if (int rc = sl->ev_up.make(hipEventDisableTiming)) return rc;
    sl->events_made = true;
    return FDBCS_OK;
}

// A direct-mode batch back into the pageable vectors (a second add call after add_packed).
void materialize(fdbcs_batch* b) {
    if (!b->direct) return;
    const char* h = (const char*)b->slot->pin_in.p;
    const size_t R = b->R(), W = b->W();
    const DKey* k = (const DKey*)(h + b->d_keys);
    b->rkeys.assign(k, k + 2 * R);
    b->wkeys.assign(k + 2 * R, k + 2 * (R + W));
    const int32_t* ro = (const int32_t*)(h + b->d_rown);
    const int32_t* wo = (const int32_t*)(h + b->d_wown);
    b->rowner.assign(ro, ro + R);
    b->wowner.assign(wo, wo + W);
    const uint8_t* t = (const uint8_t*)(h + b->d_tail);
    b->tail.assign(t, t + b->d_tail_bytes);
    b->direct = false;
}

// Has batch x's epilogue published its completion flag (null: destroyed, so done)?  The flag
// says the batch's results are final; workgroups of the epilogue other than the publishing one may
// still be writing the delta index and zeroing workspace scratch, so it never stands alone for
// "the launch is over" (stage_b_done).
inline bool batch_done(const fdbcs_batch* x) { return !x || (x->h_flag && *x->h_flag == x->seq && x->seq != 0); }

// May a dependency on workspace k's last stage B be skipped?  Only once that batch's flag was seen
// (so its stage B was issued: ev_b[k]'s last record is its own) AND ev_b[k] has completed, i.e. the
// whole epilogue launch is over.
inline bool stage_b_done(fdbcs_conflict_set* cs, int k) {
    return batch_done(cs->ws_user[k]) && hipEventQuery(cs->ev_b[k]) == hipSuccess;
}

// H2D of the packed batch by the DMA engine, issued now on `us` (the upload stream, or stage A's
// stream when the phases are timed one after another); ev_up marks its completion.
int do_upload(fdbcs_batch* b, hipStream_t us) {
    BatchSlot* sl = b->slot.get();
    const size_t T = b->T(), R = b->R(), W = b->W();
    const UploadLayout L = upload_layout(T, R, W, b->tail_size());
    int rc;
    if (!b->direct && (rc = sl->pin_in.ensure(L.total, true))) return rc;
    if ((rc = ensure_slot(sl, L.total, T, R))) return rc;
    char* h = (char*)sl->pin_in.p;
    if (!b->direct) {  // add_transaction path: normalized keys are in the pageable vectors
        if (R) memcpy(h + L.keys, b->rkeys.data(), sizeof(DKey) * 2 * R);
        if (W) memcpy(h + L.keys + sizeof(DKey) * 2 * R, b->wkeys.data(), sizeof(DKey) * 2 * W);
        if (R) memcpy(h + L.rown, b->rowner.data(), 4 * R);
        if (W) memcpy(h + L.wown, b->wowner.data(), 4 * W);
        if (!b->tail.empty()) memcpy(h + L.tail, b->tail.data(), b->tail.size());
    }
    memcpy(h + L.snap, b->snap.data(), 8 * T);
    memcpy(h + L.roff, b->roff.data(), 4 * (T + 1));
    memcpy(h + L.woff, b->woff.data(), 4 * (T + 1));
    if (T) memcpy(h + L.flags, b->flags.data(), T);
    // Both stages wait for ev_up (made with the slot).  A reused slot's device copy may still be read
    // by the epilogue of the batch that used it last.
    HIPOK(hipMemcpyAsync(sl->dev.p, h, L.total, hipMemcpyHostToDevice, us));
    HIPOK(hipEventRecord(sl->ev_up, us));
    char* d = (char*)sl->dev.p;
    b->bd.T = (int32_t)T;
    b->bd.R = (int32_t)R;
    b->bd.W = (int32_t)W;
    b->bd.snap = (int64_t*)(d + L.snap);
    b->bd.roff = (int32_t*)(d + L.roff);
    b->bd.woff = (int32_t*)(d + L.woff);
    b->bd.rowner = (int32_t*)(d + L.rown);
    b->bd.wowner = (int32_t*)(d + L.wown);
    b->bd.keys = (DKey*)(d + L.keys);
    b->bd.flags = (uint8_t*)(d + L.flags);
    b->bd.tail = (uint8_t*)(d + L.tail);
    b->tail_bytes = b->tail_size();
    b->bd.tail_n = (int64_t)b->tail_bytes;
    b->state = 1;
    return FDBCS_OK;
}

// ---- two submitting threads (FDBCS_SUBMIT_THREAD=1)
void worker_main(fdbcs_conflict_set* cs) {
    (void)hipSetDevice(cs->device);
    for (;;) {
        int j = 0;
        for (int spin = 0; spin < 20000 && (j = cs->wjob.load(std::memory_order_acquire)) == 0; spin++)
            std::this_thread::yield();
        if (j == 0) {
            std::unique_lock<std::mutex> lk(cs->wmu);
            cs->wcv.wait(lk, [&] { return (j = cs->wjob.load(std::memory_order_acquire)) != 0; });
        }
        if (j == 2) return;
        const int64_t ta = cs->htrace ? mono_ns() : 0;
        hipError_t e = cs->work_a.replay(cs->work_sa);
        if (cs->htrace) cs->htr[1].push_back({cs->work_a_seq, 'A', ta, mono_ns()});
        if (!cs->work_y.recs.empty()) {
            while (cs->x_issued.load(std::memory_order_acquire) < cs->work_need_x) std::this_thread::yield();
            const int64_t ty = cs->htrace ? mono_ns() : 0;
            const hipError_t e3 = cs->work_y.replay(cs->work_ys);
            if (cs->htrace) cs->htr[1].push_back({cs->work_y_seq, 'Y', ty, mono_ns()});
            if (e == hipSuccess) e = e3;
            cs->work_y.clear();
            cs->b_issued.fetch_add(1, std::memory_order_release);
        }
        if (!cs->work_c.recs.empty()) {
            while (cs->b_issued.load(std::memory_order_acquire) < cs->work_need_b) std::this_thread::yield();
            const hipError_t e2 = cs->work_c.replay(cs->cstream);
            if (e == hipSuccess) e = e2;
        }
        if (e != hipSuccess) {
            int expected = 0;
            cs->werr.compare_exchange_strong(expected, (int)e);
        }
        cs->wjob.store(0, std::memory_order_release);
    }
}

// Wait until the helper has issued its job; its first error, if any.
int worker_wait(fdbcs_conflict_set* cs) {
    if (!cs->worker.joinable()) return FDBCS_OK;
    while (cs->wjob.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    cs->work_y_batch = nullptr;  // any Y it held is issued
    return cs->werr.exchange(0) ? FDBCS_E_DEVICE : FDBCS_OK;
}

void worker_start_job(fdbcs_conflict_set* cs) {
    if (!cs->worker.joinable()) cs->worker = std::thread(worker_main, cs);
    {
        std::lock_guard<std::mutex> lk(cs->wmu);
        cs->wjob.store(1, std::memory_order_release);
    }
    cs->wcv.notify_one();
}

void worker_stop(fdbcs_conflict_set* cs) {
    if (!cs->worker.joinable()) return;
    (void)worker_wait(cs);
    {
        std::lock_guard<std::mutex> lk(cs->wmu);
        cs->wjob.store(2, std::memory_order_release);
    }
    cs->wcv.notify_one();
    cs->worker.join();
}

// What the host knows of batch b's candidate edges: the word its edge scan's finish wrote
// (Work::hedge: {the batch's sequence number, any candidate edge}; the count first, a system-scope
// fence, then the tag).  Only a word tagged with b's own sequence number speaks for b: until the
// scan has run, the word is still that of the workspace's previous user.
// -1: not known yet (or not tracked), 0: no candidate edge, 1: some.
int x_edges(const fdbcs_conflict_set* cs, const fdbcs_batch* b) {
    if (!b || !cs->skip_edges || !cs->hedge.p) return -1;
    const volatile uint32_t* h = (const volatile uint32_t*)((char*)cs->hedge.p + 64 * b->wp);
    if (h[0] != b->seq) return -1;
    std::atomic_thread_fence(std::memory_order_acquire);
    return h[1] == 0u ? 0 : 1;
}

// The skip groups of batch b's X half at its replay: the kGroupEdges launches are left out once
// b's edge scan told the host that b has no candidate edge; otherwise (scan not over, or not
// tracked) everything is issued.
uint8_t x_skip(const fdbcs_conflict_set* cs, const fdbcs_batch* b) { return x_edges(cs, b) == 0 ? kGroupEdges : 0; }

// Is there nothing to gain from holding h's X half back another call?  So when its edge word has
// arrived, when the word is not tracked, or when the list has no launch a count of 0 leaves out
// (timed kernels are always issued).
bool x_known(const fdbcs_conflict_set* cs, const fdbcs_conflict_set::Held& h) {
    if (!cs->skip_edges || !cs->hedge.p || x_edges(cs, h.batch) >= 0) return true;
    for (const LaunchList::Rec& r : h.x.recs)
        if (r.kind == LaunchList::kKernel && (r.group & kGroupEdges)) return false;
    return true;
}

// Batch b's recorded X half onto the batch-order stream, now.
hipError_t issue_x(fdbcs_conflict_set* cs, fdbcs_batch* b, LaunchList& x) {
    const uint8_t skip = x_skip(cs, b);
    const int64_t tx = cs->htrace ? mono_ns() : 0;
    const hipError_t e = x.replay(cs->stream, skip, &cs->stats.x_launches_skipped);
    if (cs->htrace) cs->htr[0].push_back({b->seq, 'X', tx, mono_ns()});
    // issued whole with launches a known count of 0 would have left out: too early if b is edge-free
    b->x_unskipped = false;
    if (!skip && cs->skip_edges && cs->hedge.p)
        for (const LaunchList::Rec& r : x.recs)
            if (r.kind == LaunchList::kKernel && (r.group & kGroupEdges)) b->x_unskipped = true;
    x.clear();
    return e;
}

// The held batches leave the front of the queue (n of them: their lists were issued or handed on).
void drop_held(fdbcs_conflict_set* cs, int n) {
    for (int k = n; k < cs->n_held; k++) std::swap(cs->held[k - n], cs->held[k]);
    cs->n_held -= n;
    for (int k = cs->n_held; k < kMaxHold; k++) cs->held[k].batch = nullptr;
}

// Issue the held stage-B lists, oldest first, up to and including batch `upto` (null: all of
// them).  A batch that is not held needs nothing issued.
int flush_pending(fdbcs_conflict_set* cs, const fdbcs_batch* upto) {
    if (int rc = worker_wait(cs)) return rc;  // stage A / check of the held batches issued
    int n = cs->n_held;
    if (upto) {
        n = 0;
        for (int k = 0; k < cs->n_held; k++)
            if (cs->held[k].batch == upto) n = k + 1;
    }
    int rc = FDBCS_OK;
    for (int k = 0; k < n; k++) {
        fdbcs_conflict_set::Held& h = cs->held[k];
        if (issue_x(cs, h.batch, h.x) != hipSuccess) rc = FDBCS_E_DEVICE;
        cs->x_issued.fetch_add(1, std::memory_order_release);
        const int64_t ty = cs->htrace ? mono_ns() : 0;
        if (h.y.replay(h.ys) != hipSuccess) rc = FDBCS_E_DEVICE;
        if (cs->htrace) cs->htr[0].push_back({h.batch->seq, 'Y', ty, mono_ns()});
        cs->b_issued.fetch_add(1, std::memory_order_release);
        h.y.clear();
        cs->stats.x_flushed += 1;
    }
    drop_held(cs, n);
    return rc;
}

}  // namespace fdbcs::impl

extern "C" {

const char* fdbcs_strerror(int s) {
    switch (s) {
        case FDBCS_OK: return "ok";
        case FDBCS_E_INVALID: return "invalid argument";
        case FDBCS_E_DEVICE: return "HIP device error";
        case FDBCS_E_NOMEM: return "out of memory";
        case FDBCS_E_VERSION: return "version below the history's newest version";
        case FDBCS_E_STATE: return "call out of order";
        case FDBCS_E_NODEVICE: return "no HIP device";
        case FDBCS_E_TIMEOUT: return "routed batch: the shares were never ready";
        default: return "unknown status";
    }
}

int fdbcs_new_conflict_set(int device, fdbcs_conflict_set** out) {
    if (!out) return FDBCS_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FDBCS_E_NODEVICE;
    if (device < 0 || device >= ndev) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(device));
    fdbcs_conflict_set* cs = new (std::nothrow) fdbcs_conflict_set();
    if (!cs) return FDBCS_E_NOMEM;
    cs->device = device;
    if (const char* v = getenv("FDBCS_VALIDATE")) cs->validate = v[0] == '1';
    if (const char* v = getenv("FDBCS_SORT_BUCKET")) cs->bucket_target = atoi(v);
    if (const char* v = getenv("FDBCS_SORT_COLD")) cs->sort_cold = v[0] == '1';
    if (const char* v = getenv("FDBCS_TRACE")) cs->trace = v[0] == '1';
    if (const char* v = getenv("FDBCS_SERIAL")) cs->serial = v[0] == '1';
    if (const char* v = getenv("FDBCS_RESOLVE_PREPASS")) cs->no_prepass = v[0] == '0';
    if (const char* v = getenv("FDBCS_SUBMIT_THREAD")) cs->submit_thread = v[0] != '0';
    if (const char* v = getenv("FDBCS_ADD_THREADS")) cs->add_threads = std::max(0, std::min(64, atoi(v)));
    if (const char* v = getenv("FDBCS_SKIP_EDGES")) cs->skip_edges = v[0] != '0';
    if (const char* v = getenv("FDBCS_WAIT_QUERY_MS")) cs->wait_query_ms = std::max(0, atoi(v));
    if (getenv("FDBCS_HOST_TRACE")) {
        cs->htrace = true;
        cs->htr[0].reserve(1 << 16);
        cs->htr[1].reserve(1 << 16);
    }
    if (const char* v = getenv("FDBCS_SPLIT_CHECK")) cs->split_check = atoi(v);
    if (const char* v = getenv("FDBCS_WRITE_GROUPS")) cs->write_groups = v[0] != '0';
    if (const char* v = getenv("FDBCS_DIRECTORY")) cs->directory = v[0] != '0';
    if (const char* v = getenv("FDBCS_DIR_BITS")) cs->dir_bits = std::max(0, std::min(kDirMaxBits, atoi(v)));
    if (const char* v = getenv("FDBCS_TAIL_RECLAIM")) cs->tail_reclaim = std::max<long long>(1, atoll(v));
    if (const char* v = getenv("FDBCS_ROUTE_TIMEOUT_MS")) cs->route_timeout_ms = std::max<long long>(1, atoll(v));
    static std::once_flag attr_once;
    std::call_once(attr_once, init_kernel_attributes);
    // Five streams at the default priority, every CU: stream priorities and CU partitions between
    // the chains measured slower (extra hardware queues; the chains slow each other
    // through the memory system, not by competing for CU slots).
    bool ok = true;
    for (Stream* st : {&cs->stream, &cs->ystream, &cs->astream, &cs->ustream, &cs->cstream}) ok = ok && !st->make();
    for (Event* e : {&cs->ev_cmp, &cs->ev_quant}) ok = ok && !e->make(hipEventDisableTiming);
    for (int k = 0; k < kNumWork; k++)
        for (Event* e : {&cs->ev_a[k], &cs->ev_c[k], &cs->ev_b[k], &cs->ev_res[k]})
            ok = ok && !e->make(hipEventDisableTiming);
    if (!ok) {
        fdbcs_destroy_conflict_set(cs);
        return FDBCS_E_DEVICE;
    }

    int rc = cs->scal.ensure(sizeof(Scalars));
    if (!rc) rc = cs->quant.ensure(2 * sizeof(SplitKey) * kQuant);
    if (!rc) rc = (hipMemsetAsync(cs->scal.p, 0, sizeof(Scalars), cs->stream) == hipSuccess) ? 0 : FDBCS_E_DEVICE;
    for (int k = 0; k < 2 && !rc && cs->directory; k++) {  // zeroed: epoch 0 entries are never trusted
        rc = cs->edir[k].ensure(8 * (size_t)kDirAlloc);
        if (!rc && hipMemsetAsync(cs->edir[k].p, 0, 8 * (size_t)kDirAlloc, cs->stream) != hipSuccess)
            rc = FDBCS_E_DEVICE;
    }
    if (!rc) rc = set_dir_map(cs, nullptr, 0);
    if (!rc) rc = ensure_history(cs, 1 << 16, 1 << 16);
    if (!rc) rc = ensure_delta(cs, 1 << 14);
    if (!rc) rc = ensure_workspace(cs, 1024, 4096, 4096);
    if (!rc) rc = ensure_btail(cs, 0);
    if (!rc && cs->trace) rc = cs->trace_buf.ensure(8 * kTrSlots);
    if (!rc && cs->skip_edges) rc = cs->hedge.ensure(64 * kNumWork, true);
    if (!rc && cs->skip_edges) {
        memset(cs->hedge.p, 0, 64 * kNumWork);
        for (int k = 0; k < kNumWork; k++) cs->work[k].hedge = (uint32_t*)((char*)cs->hedge.dp + 64 * k);
    }
    if (rc) {
        fdbcs_destroy_conflict_set(cs);
        return rc;
    }
    *out = cs;
    return FDBCS_OK;
}

void fdbcs_destroy_conflict_set(fdbcs_conflict_set* cs) {
    if (!cs) return;
    (void)hipSetDevice(cs->device);
    (void)flush_pending(cs);
    worker_stop(cs);
    if (cs->htrace) {
        char path[512];
        snprintf(path, sizeof(path), "%s.%d.csv", getenv("FDBCS_HOST_TRACE"), (int)getpid());
        if (FILE* f = fopen(path, "w")) {
            fprintf(f, "thread,seq,kind,t0,t1\n");
            for (int k = 0; k < 2; k++)
                for (const HSpan& h : cs->htr[k])
                    fprintf(f, "%d,%u,%c,%lld,%lld\n", k, h.seq, h.kind, (long long)h.t0, (long long)h.t1);
            fclose(f);
        }
    }
    if (getenv("FDBCS_ADD_PROFILE") && cs->add_prof_n)
        fprintf(stderr, "fdbcs add profile (%d threads, ms per batch over %lld): serial %.4f slot %.4f count %.4f fill %.4f\n",
                cs->add_threads, (long long)cs->add_prof_n, cs->add_prof[0] / cs->add_prof_n,
                cs->add_prof[1] / cs->add_prof_n, cs->add_prof[2] / cs->add_prof_n, cs->add_prof[3] / cs->add_prof_n);
    delete cs->add_pool;
    for (const Stream* st : {&cs->ustream, &cs->cstream, &cs->astream, &cs->stream, &cs->ystream})
        if (*st) (void)hipStreamSynchronize(*st);
    // batches that outlive their set (e.g. garbage-collection order in a binding) keep their own
    // slot and refuse every further call
    for (fdbcs_batch* b : cs->live) b->cs = nullptr;
    delete cs;  // every buffer and event, the pooled slots, and last the streams (engine_impl.h)
}

int fdbcs_clear_conflict_set(fdbcs_conflict_set* cs, int64_t version) {
    if (!cs) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    if (int rc = flush_pending(cs)) return rc;
    if (int rc = sync_all(cs)) return rc;
    cs->x_valid = false;
    HIPOK(hipMemsetAsync(cs->scal.p, 0, sizeof(Scalars), cs->stream));
    HIPOK(hipStreamSynchronize(cs->stream));
    cs->header_version = version;
    cs->max_written = version;
    cs->ddir_epoch[0] = cs->ddir_epoch[1] = 0;
    if (int rc = set_dir_map(cs, nullptr, 0)) return rc;
    cs->prev_segs = false;
    cs->n_ub = 0;
    cs->nd_ub = 0;
    cs->tail_ub = 0;
    return FDBCS_OK;
}

int fdbcs_set_oldest_version(fdbcs_conflict_set* cs, int64_t v) {
    if (!cs) return FDBCS_E_INVALID;
    if (v > cs->oldest) cs->oldest = v;
    return FDBCS_OK;
}

int fdbcs_get_oldest_version(const fdbcs_conflict_set* cs, int64_t* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    *out = cs->oldest;
    return FDBCS_OK;
}

int fdbcs_reserve(fdbcs_conflict_set* cs, int64_t boundaries, int64_t tail_bytes, int32_t max_txns,
                  int32_t max_reads, int32_t max_writes) {
    if (!cs || boundaries < 0 || tail_bytes < 0 || max_txns < 0 || max_reads < 0 || max_writes < 0)
        return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    int rc = ensure_workspace(cs, max_txns, max_reads, max_writes);
    if (rc) return rc;
    const int64_t dneed = delta_limit_for(cs, boundaries) + 2 * (int64_t)max_writes + 2;
    if ((rc = ensure_delta(cs, dneed))) return rc;
    return ensure_history(cs, std::max<int64_t>(boundaries + dneed, cs->hist_cap),
                          std::max<int64_t>(tail_bytes, cs->tail_cap));
}

int fdbcs_set_gc_interval(fdbcs_conflict_set* cs, int32_t every) {
    if (!cs || every < 0) return FDBCS_E_INVALID;
    cs->gc_interval = every;
    return FDBCS_OK;
}

int fdbcs_set_timing(fdbcs_conflict_set* cs, int32_t level) {
    if (!cs || level < 0 || level > 3) return FDBCS_E_INVALID;
    cs->timing = level;
    return FDBCS_OK;
}

int fdbcs_set_delta_limit(fdbcs_conflict_set* cs, int64_t boundaries) {
    if (!cs || boundaries < 0) return FDBCS_E_INVALID;
    cs->delta_limit = boundaries;
    return FDBCS_OK;
}

int fdbcs_history_size(fdbcs_conflict_set* cs, int64_t* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    int rc = sync_sizes(cs);
    if (rc) return rc;
    *out = cs->n_ub + cs->nd_ub;
    return FDBCS_OK;
}

int fdbcs_load_history(fdbcs_conflict_set* cs, int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                       const int64_t* versions, int64_t header_version) {
    if (!cs || n < 0 || (n > 0 && (!key_bytes || !key_offsets || !versions))) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    cs->x_valid = false;
    std::vector<ulonglong2> k(n);
    std::vector<uint2> lt(n);
    std::vector<uint8_t> tail;
    int64_t maxv = header_version;
    for (int64_t i = 0; i < n; i++) {
        const uint8_t* p = key_bytes + key_offsets[i];
        const int32_t len = (int32_t)(key_offsets[i + 1] - key_offsets[i]);
        if (len < 0) return FDBCS_E_INVALID;
        if (i > 0) {
            const uint8_t* q = key_bytes + key_offsets[i - 1];
            const int32_t ql = (int32_t)(key_offsets[i] - key_offsets[i - 1]);
            if (cmp_bytes(q, ql, p, len) >= 0) return FDBCS_E_INVALID;  // strictly ascending
        }
        uint64_t hi, lo;
        dkey_prefix(p, (uint32_t)len, &hi, &lo);
        k[i] = make_ulonglong2(hi, lo);
        uint32_t toff = 0;
        if (len > 16) {  // 8-byte aligned, offset in 8-byte units
            if ((int64_t)tail.size() + len >= kTailLimit) return FDBCS_E_NOMEM;
            toff = (uint32_t)(tail.size() / 8);
            tail.insert(tail.end(), p + 16, p + len);
            tail.resize((tail.size() + 7) / 8 * 8, 0);
        }
        lt[i] = make_uint2((uint32_t)len, toff);
        maxv = std::max(maxv, versions[i]);
    }
    int rc = ensure_history(cs, n + 1, (int64_t)tail.size() + 1);
    if (rc) return rc;
    if (n) {
        HIPOK(hipMemcpyAsync(cs->hkey[cs->cur].p, k.data(), 16 * n, hipMemcpyHostToDevice, cs->stream));
        HIPOK(hipMemcpyAsync(cs->hlt[cs->cur].p, lt.data(), 8 * n, hipMemcpyHostToDevice, cs->stream));
        HIPOK(hipMemcpyAsync(cs->hver[cs->cur].p, versions, 8 * n, hipMemcpyHostToDevice, cs->stream));
    }
    if (!tail.empty())
        HIPOK(hipMemcpyAsync(cs->htail[cs->tcur].p, tail.data(), tail.size(), hipMemcpyHostToDevice, cs->stream));
    Scalars s{};
    s.n = n;
    s.tail_used = (int64_t)tail.size();
    HIPOK(hipMemcpyAsync(cs->scal.p, &s, sizeof(s), hipMemcpyHostToDevice, cs->stream));
    // the directory code of the loaded keys (k_directory below builds on it)
    if (int rc = set_dir_map(cs, k.data(), n)) return rc;
    launch_rangemax(cs->stream, levels_of(cs, cs->cur), (Scalars*)cs->scal.p, &((Scalars*)cs->scal.p)->n, cs->lvl3_n,
                    cs->lvl2_n, std::max<int64_t>(n, 1));
    HIPOK(take_launch_error());
    HIPOK(hipStreamSynchronize(cs->stream));
    cs->header_version = header_version;
    cs->max_written = maxv;
    cs->ddir_epoch[0] = cs->ddir_epoch[1] = 0;  // no delta directory entry of the old slot mapping is trusted
    cs->prev_segs = false;
    cs->n_ub = n;
    cs->nd_ub = 0;
    cs->tail_ub = (int64_t)tail.size();
    return FDBCS_OK;
}

int fdbcs_get_stats(fdbcs_conflict_set* cs, fdbcs_stats* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    *out = cs->stats;
    out->x_held = cs->n_held;  // (a gauge: what is held now)
    return FDBCS_OK;
}

int fdbcs_reset_stats(fdbcs_conflict_set* cs) {
    if (!cs) return FDBCS_E_INVALID;
    memset(&cs->stats, 0, sizeof(cs->stats));
    cs->kprof.clear();
    return FDBCS_OK;
}

// Demangled kernel name without its namespace and argument list ("k_scan<3, fdbcs::PosScan>").
static std::string kernel_name(const void* func, hipStream_t s) {
    const char* m = hipKernelNameRefByPtr(func, s);
    if (!m) return "?";
    int st = 0;
    char* d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
    std::string n = (st == 0 && d) ? d : m;
    free(d);
    // drop the return type, namespace prefix and parameter list
    if (n.rfind("void ", 0) == 0) n = n.substr(5);
    int depth = 0;
    for (size_t i = 0; i < n.size(); i++) {
        if (n[i] == '<') depth++;
        if (n[i] == '>') depth--;
        if (n[i] == '(' && depth == 0) {
            n = n.substr(0, i);
            break;
        }
    }
    if (n.rfind("fdbcs::", 0) == 0) n = n.substr(7);
    return n;
}

int fdbcs_kernel_profile(fdbcs_conflict_set* cs, int32_t index, char* name, int32_t cap, int64_t* launches,
                         double* ms) {
    if (!cs || index < 0 || index >= (int32_t)cs->kprof.size()) return FDBCS_E_INVALID;
    const auto& k = cs->kprof[index];
    if (name && cap > 0) {
        const std::string n = kernel_name(k.func, cs->stream);
        snprintf(name, (size_t)cap, "%s", n.c_str());
    }
    if (launches) *launches = k.launches;
    if (ms) *ms = k.ms;
    return FDBCS_OK;
}

int fdbcs_debug_hold(fdbcs_conflict_set* cs, int32_t on) {
    if (!cs) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    if (int rc = cs->hold.ensure(64, true)) return rc;
    volatile uint32_t* word = (volatile uint32_t*)cs->hold.p;
    if (!on) {
        __atomic_store_n((uint32_t*)word, 1u, __ATOMIC_SEQ_CST);
        return FDBCS_OK;
    }
    if (int rc = sync_all(cs)) return rc;
    *word = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    for (const Stream* st : {&cs->ustream, &cs->astream, &cs->cstream, &cs->stream})
        launch_hold(*st, (const uint32_t*)cs->hold.dp);
    HIPOK(take_launch_error());
    return FDBCS_OK;
}

int fdbcs_set_timed_kernel(fdbcs_conflict_set* cs, const char* name) {
    if (!cs) return FDBCS_E_INVALID;
    cs->timed_func = nullptr;
    if (!name || !name[0]) return FDBCS_OK;
    for (const auto& k : cs->kprof)
        if (kernel_name(k.func, cs->stream) == name) {
            cs->timed_func = k.func;
            return FDBCS_OK;
        }
    return FDBCS_E_INVALID;  // only kernels seen by a profiled batch can be named
}

int fdbcs_batch_new(fdbcs_conflict_set* cs, int report_keys, fdbcs_batch** out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    fdbcs_batch* b = new (std::nothrow) fdbcs_batch();
    if (!b) return FDBCS_E_NOMEM;
    b->cs = cs;
    if (!cs->pool.empty()) {
        b->slot = std::move(cs->pool.back());
        cs->pool.pop_back();
    } else {
        b->slot.reset(new (std::nothrow) BatchSlot());
        const int rc = b->slot ? make_slot_events(b->slot.get()) : FDBCS_E_NOMEM;
        if (rc) {
            delete b;
            return rc;
        }
    }
    cs->live.insert(b);
    b->report_enabled = report_keys ? 1 : 0;
    *out = b;
    return FDBCS_OK;
}

void fdbcs_batch_destroy(fdbcs_batch* b) {
    if (!b) return;
    if (!b->cs) {  // its set was destroyed first (and synchronized its streams): the slot dies with it
        delete b;
        return;
    }
    if (b->state == 2) {  // still in flight: its set (which must outlive it) owns the stream
        (void)hipSetDevice(b->cs->device);
        (void)flush_pending(b->cs);
        for (const Stream* st : {&b->cs->ustream, &b->cs->cstream, &b->cs->astream, &b->cs->stream, &b->cs->ystream})
            (void)hipStreamSynchronize(*st);
        b->cs->inflight--;
    } else if (b->state == 1) {  // uploaded, never submitted: the copy may still be in flight
        (void)hipSetDevice(b->cs->device);
        (void)hipStreamSynchronize(b->cs->ustream);
        (void)hipStreamSynchronize(b->cs->astream);
    }
    if (b->sp_pending) {  // a share pack nobody waited for: it uses the slot's scan state
        (void)hipSetDevice(b->cs->device);
        (void)finish_share_pack(b);
    }
    // a sample runs behind the routing, off the detect pipeline: the slot's device copy and the
    // sample's own buffers are the next batch's only once it is over
    if (b->slot && b->slot->is_inflight) {
        (void)hipSetDevice(b->cs->device);
        (void)hipEventSynchronize(b->slot->is_span.e1);
        b->slot->is_inflight = false;
    }
    // done (waited or synchronized): dependencies on it need no wait any more
    for (int k = 0; k < kNumWork; k++) {
        if (b->cs->ws_user[k] == b) b->cs->ws_user[k] = nullptr;
        if (b->cs->xfree_user[k] == b) b->cs->xfree_user[k] = nullptr;
    }
    // the slot goes back to the set's pool (its buffers and events are reused by the next batch)
    if (b->slot) b->cs->pool.push_back(std::move(b->slot));
    b->cs->live.erase(b);
    delete b;
}

int fdbcs_batch_add_transaction(fdbcs_batch* b, int64_t read_snapshot, int report_conflicting_keys, int32_t n_reads,
                                const uint8_t* const* read_begin, const int32_t* read_begin_len,
                                const uint8_t* const* read_end, const int32_t* read_end_len, int32_t n_writes,
                                const uint8_t* const* write_begin, const int32_t* write_begin_len,
                                const uint8_t* const* write_end, const int32_t* write_end_len) {
    if (!b || n_reads < 0 || n_writes < 0) return FDBCS_E_INVALID;
    if (b->state != 0 || !b->cs || b->share_packed) return FDBCS_E_STATE;  // (a batch that packed a share takes routed adds only)
    if ((n_reads && (!read_begin || !read_end || !read_begin_len || !read_end_len)) ||
        (n_writes && (!write_begin || !write_end || !write_begin_len || !write_end_len)))
        return FDBCS_E_INVALID;
    // KeyRangeRef rejects begin > end (FDBTypes.h:288-291): validate before mutating anything.
    for (int32_t i = 0; i < n_reads; i++)
        if (read_begin_len[i] < 0 || read_end_len[i] < 0 ||
            cmp_bytes(read_begin[i], read_begin_len[i], read_end[i], read_end_len[i]) > 0)
            return FDBCS_E_INVALID;
    for (int32_t i = 0; i < n_writes; i++)
        if (write_begin_len[i] < 0 || write_end_len[i] < 0 ||
            cmp_bytes(write_begin[i], write_begin_len[i], write_end[i], write_end_len[i]) > 0)
            return FDBCS_E_INVALID;
    materialize(b);
    const int32_t t = b->T();
    uint8_t fl = (report_conflicting_keys && b->report_enabled) ? kFlagReport : 0;
    b->n_report += fl ? 1 : 0;
    const bool too_old = read_snapshot < b->cs->oldest && n_reads > 0;  // SkipList.cpp:770
    if (too_old) fl |= kFlagTooOld;
    b->snap.push_back(read_snapshot);
    b->flags.push_back(fl);
    if (!too_old) {
        for (int32_t i = 0; i < n_reads; i++) {
            add_key(b, b->rkeys, read_begin[i], read_begin_len[i]);
            add_key(b, b->rkeys, read_end[i], read_end_len[i]);
            b->rowner.push_back(t);
        }
        for (int32_t i = 0; i < n_writes; i++) {
            add_key(b, b->wkeys, write_begin[i], write_begin_len[i]);
            add_key(b, b->wkeys, write_end[i], write_end_len[i]);
            b->wtail += padded_tail(write_begin_len[i]) + padded_tail(write_end_len[i]);
            b->wowner.push_back(t);
        }
    }
    b->roff.push_back(b->roff.back() + (too_old ? 0 : n_reads));
    b->woff.push_back(b->woff.back() + (too_old ? 0 : n_writes));
    return FDBCS_OK;
}

// begin <= end of one range (KeyRangeRef, FDBTypes.h:288-291) from the normalized prefixes, the
// tails only when both prefixes tie and both keys run past 16 bytes (SkipList.cpp:53-60 order).
static inline bool range_inverted(const DKey& a, const DKey& b, const uint8_t* ka, const uint8_t* kb) {
    if (a.hi != b.hi) return a.hi > b.hi;
    if (a.lo != b.lo) return a.lo > b.lo;
    if (a.len <= 16 || b.len <= 16) return a.len > b.len;  // the shorter is a prefix of the longer
    return cmp_bytes(ka + 16, (int32_t)a.len - 16, kb + 16, (int32_t)b.len - 16) > 0;
}

static inline void normalize_key(const uint8_t* p, uint32_t len, DKey* out) {
    fast_prefix(p, len, &out->hi, &out->lo);
    out->len = len;
    out->tail = 0;
}

// addTransaction of a whole packed batch into an empty batch (offsets already checked monotone):
// the endpoint keys are validated and normalized straight into the batch's pinned staging, in
// chunks of transactions over the conflict set's add threads (AddPool), with no per-range
// vectors and no copy at upload.  All-or-nothing: an inverted range leaves the batch empty.
static int add_packed_direct(fdbcs_batch* b, const fdbcs_packed_batch* pb) {
    fdbcs_conflict_set* cs = b->cs;
    const int32_t T = pb->n_txn;
    const int64_t oldest = cs->oldest;
    using clk = std::chrono::steady_clock;
    const auto tp0 = clk::now();
    b->snap.assign(pb->read_snapshot, pb->read_snapshot + T);
    b->flags.resize(T);
    b->roff.resize(T + 1);
    b->woff.resize(T + 1);
    int32_t Ra = 0, Wa = 0, n_report = 0;
    for (int32_t t = 0; t < T; t++) {
        const int32_t nr = pb->read_offsets[t + 1] - pb->read_offsets[t];
        const int32_t nw = pb->write_offsets[t + 1] - pb->write_offsets[t];
        uint8_t fl = (pb->report_conflicting_keys && pb->report_conflicting_keys[t] && b->report_enabled)
                         ? kFlagReport
                         : 0;
        n_report += fl ? 1 : 0;
        const bool too_old = pb->read_snapshot[t] < oldest && nr > 0;  // SkipList.cpp:770
        if (too_old) fl |= kFlagTooOld;
        b->flags[t] = fl;
        b->roff[t] = Ra;
        b->woff[t] = Wa;
        if (!too_old) {
            Ra += nr;
            Wa += nw;
        }
    }
    b->roff[T] = Ra;
    b->woff[T] = Wa;
    const int32_t R = pb->read_offsets[T];
    const int64_t nk = 2 * ((int64_t)R + pb->write_offsets[T]);
    const size_t tail_bound = nk ? (size_t)(pb->key_offsets[nk] - pb->key_offsets[0]) : 0;
    const UploadLayout L = upload_layout(T, Ra, Wa, tail_bound);
    auto fail = [&](int rc) {
        b->snap.clear();
        b->flags.clear();
        b->roff.assign(1, 0);
        b->woff.assign(1, 0);
        return rc;
    };
    const auto tp1 = clk::now();
    if (int rc = b->slot->pin_in.ensure(L.total, true)) return fail(rc);
    if (int rc = ensure_slot(b->slot.get(), L.total, T, Ra)) return fail(rc);
    const auto tp2 = clk::now();
    char* h = (char*)b->slot->pin_in.p;
    DKey* keys = (DKey*)(h + L.keys);
    DKey* wk = keys + 2 * (size_t)Ra;
    int32_t* rown = (int32_t*)(h + L.rown);
    int32_t* wown = (int32_t*)(h + L.wown);
    uint8_t* tail = (uint8_t*)(h + L.tail);
    const uint8_t* kb = pb->key_bytes;
    const int64_t* ko = pb->key_offsets;
    // chunks of ~512 ranges; one chunk (no pool) for small batches
    const int64_t G = (int64_t)R + pb->write_offsets[T];
    const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(256, G / 512));
    struct Chunk {
        int32_t t0, t1;
        int64_t tails, wtail;
        int32_t max_len;
        bool bad;
    };
    std::vector<Chunk> ch(nchunk);
    for (int c = 0; c < nchunk; c++) {
        ch[c] = Chunk{(int32_t)((int64_t)T * c / nchunk), (int32_t)((int64_t)T * (c + 1) / nchunk), 0, 0, 0, false};
    }
    const bool pooled = nchunk > 1 && cs->add_threads > 0;
    if (pooled && !cs->add_pool) {
        try {
            cs->add_pool = new AddPool(cs->add_threads);
        } catch (...) {  // no memory or no threads left: this call and later ones run serially
            cs->add_pool = nullptr;
            cs->add_threads = 0;
        }
    }
    // pass 1 (tickets [0, nchunk)): tail bytes of each chunk's admitted keys (key offsets only), so
    // the tails pack exactly in transaction order; pass 2 (tickets [nchunk, 2 nchunk)) waits for
    // every count (tickets go out in order, so every count is held by a running thread)
    std::atomic<int> counted{0};
    const std::function<void(int)> count = [&](int c) {
        Chunk& k = ch[c];
        int64_t tb = 0;
        for (int32_t t = k.t0; t < k.t1; t++) {
            if (b->flags[t] & kFlagTooOld) continue;
            const int64_t r0 = 2 * (int64_t)pb->read_offsets[t], r1 = 2 * (int64_t)pb->read_offsets[t + 1];
            const int64_t w0 = 2 * ((int64_t)R + pb->write_offsets[t]), w1 = 2 * ((int64_t)R + pb->write_offsets[t + 1]);
            for (int64_t q = r0; q < r1; q++) tb += std::max<int64_t>(0, ko[q + 1] - ko[q] - 16);
            for (int64_t q = w0; q < w1; q++) tb += std::max<int64_t>(0, ko[q + 1] - ko[q] - 16);
        }
        k.tails = tb;
        counted.fetch_add(1, std::memory_order_release);
    };
    const auto tp3 = clk::now();
    // pass 2: every range validated (TooOld transactions' too: KeyRangeRef asserts begin <= end
    // whatever the batch does with it), admitted ones normalized with their owners and tails
    const std::function<void(int)> fill = [&](int c) {
        Chunk& k = ch[c];
        while (counted.load(std::memory_order_acquire) < nchunk) __builtin_ia32_pause();
        int64_t tb = 0, wt = 0;
        for (int q = 0; q < c; q++) tb += ch[q].tails;
        int32_t ml = 0;
        bool bad = false;
        auto put = [&](DKey* out, int64_t q) {
            const uint8_t* p = kb + ko[q];
            const uint32_t len = (uint32_t)(ko[q + 1] - ko[q]);
            normalize_key(p, len, out);
            if ((int32_t)len > ml) ml = (int32_t)len;
            if (len > 16) {
                out->tail = (uint32_t)tb;
                memcpy(tail + tb, p + 16, len - 16);
                tb += len - 16;
            }
        };
        for (int32_t t = k.t0; t < k.t1 && !bad; t++) {
            const int32_t r0 = pb->read_offsets[t], r1 = pb->read_offsets[t + 1];
            const int32_t w0 = pb->write_offsets[t], w1 = pb->write_offsets[t + 1];
            if (b->flags[t] & kFlagTooOld) {
                auto check = [&](int64_t q) {
                    DKey x, y;
                    normalize_key(kb + ko[q], (uint32_t)(ko[q + 1] - ko[q]), &x);
                    normalize_key(kb + ko[q + 1], (uint32_t)(ko[q + 2] - ko[q + 1]), &y);
                    bad |= range_inverted(x, y, kb + ko[q], kb + ko[q + 1]);
                };
                for (int32_t r = r0; r < r1; r++) check(2 * (int64_t)r);
                for (int32_t w = w0; w < w1; w++) check(2 * ((int64_t)R + w));
                continue;
            }
            const int32_t ra = b->roff[t], wa = b->woff[t];
            for (int32_t r = r0, i = 0; r < r1; r++, i++) {
                DKey* o = keys + 2 * (size_t)(ra + i);
                put(o, 2 * (int64_t)r);
                put(o + 1, 2 * (int64_t)r + 1);
                bad |= range_inverted(o[0], o[1], kb + ko[2 * (int64_t)r], kb + ko[2 * (int64_t)r + 1]);
                rown[ra + i] = t;
            }
            for (int32_t w = w0, i = 0; w < w1; w++, i++) {
                DKey* o = wk + 2 * (size_t)(wa + i);
                const int64_t q = 2 * ((int64_t)R + w);
                put(o, q);
                put(o + 1, q + 1);
                bad |= range_inverted(o[0], o[1], kb + ko[q], kb + ko[q + 1]);
                wt += padded_tail((int32_t)(ko[q + 1] - ko[q])) + padded_tail((int32_t)(ko[q + 2] - ko[q + 1]));
                wown[wa + i] = t;
            }
        }
        k.wtail = wt;
        k.max_len = ml;
        k.bad = bad;
    };
    const std::function<void(int)> both = [&](int q) { q < nchunk ? count(q) : fill(q - nchunk); };
    if (pooled && cs->add_pool)
        cs->add_pool->parallel_for(2 * nchunk, both);
    else
        for (int q = 0; q < 2 * nchunk; q++) both(q);
    int64_t tb_total = 0;
    for (int c = 0; c < nchunk; c++) tb_total += ch[c].tails;
    const auto tp4 = clk::now();
    {
        auto ms = [](clk::time_point a, clk::time_point b_) { return std::chrono::duration<double, std::milli>(b_ - a).count(); };
        cs->add_prof[0] += ms(tp0, tp1);
        cs->add_prof[1] += ms(tp1, tp2);
        cs->add_prof[2] += ms(tp2, tp3);  // (nothing: count and fill run as one job)
        cs->add_prof[3] += ms(tp3, tp4);
        cs->add_prof_n++;
    }
    int64_t wtail = 0;
    int32_t max_len = b->max_len;
    for (const Chunk& k : ch) {
        if (k.bad) return fail(FDBCS_E_INVALID);
        wtail += k.wtail;
        max_len = std::max(max_len, k.max_len);
    }
    b->wtail += wtail;
    b->max_len = max_len;
    b->n_report += n_report;
    b->direct = true;
    b->d_keys = L.keys;
    b->d_rown = L.rown;
    b->d_wown = L.wown;
    b->d_tail = L.tail;
    b->d_tail_bytes = (size_t)tb_total;
    return FDBCS_OK;
}

static inline double host_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int add_packed_impl(fdbcs_batch* b, const fdbcs_packed_batch* pb);

int fdbcs_batch_add_packed(fdbcs_batch* b, const fdbcs_packed_batch* pb) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = add_packed_impl(b, pb);
    if (rc == FDBCS_OK && b->cs) {
        b->cs->stats.host_ms_add += host_ms_since(t0);
        b->cs->stats.added_txns += pb->n_txn;
    }
    return rc;
}

static int add_packed_impl(fdbcs_batch* b, const fdbcs_packed_batch* pb) {
    if (!b || !pb || pb->n_txn < 0) return FDBCS_E_INVALID;
    if (b->state != 0 || !b->cs || b->share_packed) return FDBCS_E_STATE;  // (a batch that packed a share takes routed adds only)
    const int32_t T = pb->n_txn;
    if (T == 0) return FDBCS_OK;
    if (!pb->read_snapshot || !pb->read_offsets || !pb->write_offsets || !pb->key_offsets) return FDBCS_E_INVALID;
    const int32_t R = pb->read_offsets[T];
    const int64_t nk = 2 * ((int64_t)R + pb->write_offsets[T]);
    if (nk && !pb->key_bytes) return FDBCS_E_INVALID;
    // validate everything first (all-or-nothing): offsets here, ranges below (fused with the
    // normalization on the direct path)
    for (int32_t t = 0; t < T; t++)
        if (pb->read_offsets[t + 1] < pb->read_offsets[t] || pb->write_offsets[t + 1] < pb->write_offsets[t])
            return FDBCS_E_INVALID;
    for (int64_t k = 0; k < nk; k++)
        if (pb->key_offsets[k + 1] < pb->key_offsets[k]) return FDBCS_E_INVALID;
    if (b->T() == 0 && !b->direct) return add_packed_direct(b, pb);
    for (int64_t k = 0; k < nk; k += 2) {
        const int64_t a0 = pb->key_offsets[k], a1 = pb->key_offsets[k + 1], a2 = pb->key_offsets[k + 2];
        if (cmp_bytes(pb->key_bytes + a0, (int32_t)(a1 - a0), pb->key_bytes + a1, (int32_t)(a2 - a1)) > 0)
            return FDBCS_E_INVALID;
    }
    const int64_t oldest = b->cs->oldest;
    materialize(b);
    b->snap.reserve(b->snap.size() + T);
    for (int32_t t = 0; t < T; t++) {
        const int32_t tt = b->T();
        const int32_t r0 = pb->read_offsets[t], r1 = pb->read_offsets[t + 1];
        const int32_t w0 = pb->write_offsets[t], w1 = pb->write_offsets[t + 1];
        uint8_t fl = (pb->report_conflicting_keys && pb->report_conflicting_keys[t] && b->report_enabled)
                         ? kFlagReport
                         : 0;
        b->n_report += fl ? 1 : 0;
        const bool too_old = pb->read_snapshot[t] < oldest && r1 > r0;
        if (too_old) fl |= kFlagTooOld;
        b->snap.push_back(pb->read_snapshot[t]);
        b->flags.push_back(fl);
        if (!too_old) {
            for (int32_t r = r0; r < r1; r++) {
                for (int e = 0; e < 2; e++) {
                    const int64_t k = 2 * (int64_t)r + e;
                    add_key(b, b->rkeys, pb->key_bytes + pb->key_offsets[k],
                            (int32_t)(pb->key_offsets[k + 1] - pb->key_offsets[k]));
                }
                b->rowner.push_back(tt);
            }
            for (int32_t w = w0; w < w1; w++) {
                for (int e = 0; e < 2; e++) {
                    const int64_t k = 2 * ((int64_t)R + w) + e;
                    b->wtail += padded_tail((int32_t)(pb->key_offsets[k + 1] - pb->key_offsets[k]));
                    add_key(b, b->wkeys, pb->key_bytes + pb->key_offsets[k],
                            (int32_t)(pb->key_offsets[k + 1] - pb->key_offsets[k]));
                }
                b->wowner.push_back(tt);
            }
        }
        b->roff.push_back(b->roff.back() + (too_old ? 0 : r1 - r0));
        b->woff.push_back(b->woff.back() + (too_old ? 0 : w1 - w0));
    }
    return FDBCS_OK;
}

// ---- multi-resolver routing: proxy shares (engine.h ShareHeader) and the device split

// (C++ linkage inside the C-ABI block, as finish_route below: ingest.cpp's share pack calls it,
// declared in engine_impl.h)
extern "C++" size_t fdbcs::impl::share_layout(int32_t T, int64_t R, int64_t W, int64_t tail, ShareHeader* h) {
    size_t off = sizeof(ShareHeader);
    h->T = T;
    h->R = (int32_t)R;
    h->W = (int32_t)W;
    h->off_keys = (int64_t)off;
    off = align_up(off + sizeof(DKey) * 2 * (size_t)(R + W), 64);
    h->off_snap = (int64_t)off;
    off = align_up(off + 8 * (size_t)T, 64);
    h->off_roff = (int64_t)off;
    off = align_up(off + 4 * ((size_t)T + 1), 64);
    h->off_woff = (int64_t)off;
    off = align_up(off + 4 * ((size_t)T + 1), 64);
    h->off_report = (int64_t)off;
    off = align_up(off + (size_t)T, 64);
    h->off_owner = (int64_t)off;
    off = align_up(off + 4 * (size_t)(R + W), 64);
    h->off_tail = (int64_t)off;
    h->tail_bytes = tail;
    off = align_up(off + (size_t)tail + 64, 64);  // slack for dkey.h tail_word
    h->bytes = (int64_t)off;
    return off;
}

static int64_t packed_tail_bytes(const fdbcs_packed_batch* pb) {
    const int32_t T = pb->n_txn;
    const int64_t nk = T > 0 ? 2 * ((int64_t)pb->read_offsets[T] + pb->write_offsets[T]) : 0;
    int64_t tail = 0;
    for (int64_t k = 0; k < nk; k++) {
        const int64_t len = pb->key_offsets[k + 1] - pb->key_offsets[k];
        if (len > 16) tail += len - 16;
    }
    return tail;
}

int fdbcs_share_bytes(const fdbcs_packed_batch* pb, int64_t* out) {
    if (!pb || !out || pb->n_txn < 0) return FDBCS_E_INVALID;
    if (pb->n_txn > 0 && (!pb->read_offsets || !pb->write_offsets || !pb->key_offsets)) return FDBCS_E_INVALID;
    const int32_t T = pb->n_txn;
    ShareHeader h{};
    *out = (int64_t)share_layout(T, T ? pb->read_offsets[T] : 0, T ? pb->write_offsets[T] : 0, packed_tail_bytes(pb), &h);
    return FDBCS_OK;
}

int fdbcs_share_pack(const fdbcs_packed_batch* pb, void* out, int64_t cap, int64_t* used) {
    if (!pb || !out || pb->n_txn < 0) return FDBCS_E_INVALID;
    const int32_t T = pb->n_txn;
    if (T > 0 && (!pb->read_snapshot || !pb->read_offsets || !pb->write_offsets || !pb->key_offsets))
        return FDBCS_E_INVALID;
    const int64_t R = T ? pb->read_offsets[T] : 0, W = T ? pb->write_offsets[T] : 0;
    const int64_t nk = 2 * (R + W);
    if (nk && !pb->key_bytes) return FDBCS_E_INVALID;
    for (int32_t t = 0; t < T; t++)
        if (pb->read_offsets[t + 1] < pb->read_offsets[t] || pb->write_offsets[t + 1] < pb->write_offsets[t])
            return FDBCS_E_INVALID;
    for (int64_t k = 0; k < nk; k += 2) {  // KeyRangeRef: begin <= end (FDBTypes.h:288-291)
        const int64_t a0 = pb->key_offsets[k], a1 = pb->key_offsets[k + 1], a2 = pb->key_offsets[k + 2];
        if (a1 < a0 || a2 < a1) return FDBCS_E_INVALID;
        if (cmp_bytes(pb->key_bytes + a0, (int32_t)(a1 - a0), pb->key_bytes + a1, (int32_t)(a2 - a1)) > 0)
            return FDBCS_E_INVALID;
    }
    ShareHeader h{};
    const size_t bytes = share_layout(T, R, W, packed_tail_bytes(pb), &h);
    if ((int64_t)bytes > cap) return FDBCS_E_NOMEM;
    char* o = (char*)out;
    memcpy(o, &h, sizeof(h));
    DKey* keys = (DKey*)(o + h.off_keys);
    uint8_t* tail = (uint8_t*)(o + h.off_tail);
    uint32_t tb = 0;
    for (int64_t k = 0; k < nk; k++) {
        const uint8_t* p = pb->key_bytes + pb->key_offsets[k];
        const uint32_t len = (uint32_t)(pb->key_offsets[k + 1] - pb->key_offsets[k]);
        DKey d;
        fast_prefix(p, len, &d.hi, &d.lo);
        d.len = len;
        d.tail = 0;
        if (len > 16) {
            d.tail = tb;
            memcpy(tail + tb, p + 16, len - 16);
            tb += len - 16;
        }
        keys[k] = d;
    }
    memset(tail + tb, 0, 64);
    if (T) {
        memcpy(o + h.off_snap, pb->read_snapshot, 8 * (size_t)T);
        memcpy(o + h.off_roff, pb->read_offsets, 4 * ((size_t)T + 1));
        memcpy(o + h.off_woff, pb->write_offsets, 4 * ((size_t)T + 1));
        if (pb->report_conflicting_keys)
            memcpy(o + h.off_report, pb->report_conflicting_keys, (size_t)T);
        else
            memset(o + h.off_report, 0, (size_t)T);
        int32_t* owner = (int32_t*)(o + h.off_owner);
        for (int32_t t = 0; t < T; t++) {
            for (int32_t r = pb->read_offsets[t]; r < pb->read_offsets[t + 1]; r++) owner[r] = t;
            for (int32_t w = pb->write_offsets[t]; w < pb->write_offsets[t + 1]; w++) owner[R + w] = t;
        }
    }
    if (used) *used = (int64_t)bytes;
    return FDBCS_OK;
}

// ---- keyResolvers maps (fdbcs_route_map_pack, fdbcs_batch_add_routed_map)

// The map's own validity (the header's list) and the resolver id.
static int route_map_check(const fdbcs_key_resolvers* m, int32_t resolver) {
    if (!m || resolver < 0 || m->n_ranges < 1 || m->n_ranges > kRouteMapMaxRanges || !m->bound_offsets ||
        !m->hist_offsets || !m->hist_versions || !m->hist_resolvers)
        return FDBCS_E_INVALID;
    const int32_t M = m->n_ranges;
    const int64_t *bo = m->bound_offsets, *ho = m->hist_offsets;
    if (bo[0] < 0 || bo[1] != bo[0] || ho[0] < 0) return FDBCS_E_INVALID;  // the first bound is the empty key
    for (int32_t i = 0; i < M; i++) {
        if (bo[i + 1] < bo[i] || bo[i + 1] - bo[i] > INT32_MAX) return FDBCS_E_INVALID;
        if (ho[i + 1] <= ho[i]) return FDBCS_E_INVALID;  // a range without an owner
    }
    if (bo[M] > bo[0] && !m->bound_bytes) return FDBCS_E_INVALID;
    for (int32_t i = 1; i < M; i++)
        if (cmp_bytes(m->bound_bytes + bo[i - 1], (int32_t)(bo[i] - bo[i - 1]), m->bound_bytes + bo[i],
                      (int32_t)(bo[i + 1] - bo[i])) >= 0)
            return FDBCS_E_INVALID;
    for (int32_t i = 0; i < M; i++)
        for (int64_t k = ho[i]; k < ho[i + 1]; k++) {
            if (m->hist_resolvers[k] < 0) return FDBCS_E_INVALID;
            if (k > ho[i] && m->hist_versions[k] < m->hist_versions[k - 1]) return FDBCS_E_INVALID;
        }
    return FDBCS_OK;
}

// own[] and until[] of a checked map for one resolver (engine.h RouteArgs::map).
static void route_map_derive(const fdbcs_key_resolvers* m, int32_t resolver, uint8_t* own, int64_t* until) {
    for (int32_t i = 0; i < m->n_ranges; i++) {
        const int64_t h0 = m->hist_offsets[i], h1 = m->hist_offsets[i + 1];
        uint8_t o = m->hist_resolvers[h1 - 1] == resolver ? 1 : 0;
        int64_t u = INT64_MIN;
        for (int64_t k = h0; k + 1 < h1; k++)
            if (m->hist_resolvers[k] == resolver) {
                o |= 2;
                u = std::max(u, m->hist_versions[k + 1]);
            }
        own[i] = o;
        until[i] = u;
    }
}

int fdbcs_route_map_pack(const fdbcs_key_resolvers* map, int32_t resolver, uint8_t* own_out, int64_t* until_out) {
    if (!own_out || !until_out) return FDBCS_E_INVALID;
    if (int rc = route_map_check(map, resolver)) return rc;
    route_map_derive(map, resolver, own_out, until_out);
    return FDBCS_OK;
}

// Bytes of a checked map's device block (route_map_layout, its bounds' tails each padded to 8, and
// the slack tail_cmp's aligned loads need).
static size_t route_map_bytes(const fdbcs_key_resolvers* m) {
    int64_t tails = 0;
    for (int32_t i = 0; i < m->n_ranges; i++) tails += padded_tail((int32_t)(m->bound_offsets[i + 1] - m->bound_offsets[i]));
    return (size_t)(route_map_layout(m->n_ranges).tail + tails + 64);
}

// The block itself, into `out` (pinned staging of route_map_bytes bytes).
static void route_map_fill(const fdbcs_key_resolvers* m, int32_t resolver, uint8_t* out, size_t bytes) {
    const int32_t M = m->n_ranges;
    const RouteMapLayout L = route_map_layout(M);
    memset(out + L.own, 0, bytes - (size_t)L.own);  // padding, summaries' padding, tail slack
    DKey* bounds = (DKey*)(out + L.bounds);
    int64_t* until = (int64_t*)(out + L.until);
    int64_t* sum_until = (int64_t*)(out + L.sum_until);
    uint8_t *own = out + L.own, *sum_own = out + L.sum_own, *tail = out + L.tail;
    route_map_derive(m, resolver, own, until);
    uint32_t tb = 0;
    for (int32_t i = 0; i < M; i++) {
        const uint8_t* k = m->bound_bytes + m->bound_offsets[i];
        const int32_t len = (int32_t)(m->bound_offsets[i + 1] - m->bound_offsets[i]);
        DKey d;
        fast_prefix(k, (uint32_t)len, &d.hi, &d.lo);
        d.len = (uint32_t)len;
        d.tail = 0;
        if (len > 16) {
            d.tail = tb;
            memcpy(tail + tb, k + 16, (size_t)len - 16);
            tb += (uint32_t)padded_tail(len);
        }
        bounds[i] = d;
        if (i % kRouteMapSum == 0) sum_until[i / kRouteMapSum] = INT64_MIN;
        sum_own[i / kRouteMapSum] |= own[i];
        sum_until[i / kRouteMapSum] = std::max(sum_until[i / kRouteMapSum], until[i]);
    }
}

// fdbcs_batch_add_routed (map null: the static range [lo, hi)) and fdbcs_batch_add_routed_map (map
// checked by the caller; lo / hi unused).
static int add_routed_impl(fdbcs_batch* b, const void* shares, int64_t stride, int32_t n_shares, int32_t max_share_txns,
                           const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key, int32_t hi_len,
                           const fdbcs_key_resolvers* map, int32_t resolver, int32_t cap_txns, int32_t cap_reads,
                           int32_t cap_writes, int64_t cap_tail, uint8_t* conflict_out, int64_t n_global,
                           const uint32_t* ready_flag, uint32_t ready_value) {
    if (!b || !shares || stride <= (int64_t)sizeof(ShareHeader) || n_shares <= 0 || max_share_txns < 0 || cap_txns < 0 ||
        cap_reads < 0 || cap_writes < 0 || cap_tail < 0 || (lo_len > 0 && !lo_key) || (hi_len > 0 && !hi_key) ||
        n_global < 0 || (conflict_out && n_global > (int64_t)n_shares * max_share_txns))
        return FDBCS_E_INVALID;
    if (!b->cs || b->state != 0 || b->T() != 0 || b->direct) return FDBCS_E_STATE;
    if ((int64_t)cap_txns > kMaxTxnLds) return FDBCS_E_INVALID;
    // the batch's own share may still be packing (fdbcs_batch_share_pack_device): its error comes first
    if (b->sp_pending) {
        HIPOK(hipSetDevice(b->cs->device));
        if (int rc = finish_share_pack(b)) return rc;
    }
    if (lo_len >= 0 && hi_len >= 0 && cmp_bytes(lo_key, lo_len, hi_key, hi_len) >= 0) return FDBCS_E_INVALID;
    fdbcs_conflict_set* cs = b->cs;
    HIPOK(hipSetDevice(cs->device));
    BatchSlot* sl = b->slot.get();
    int rc;
    RouteArgs a{};
    size_t map_bytes = 0;
    if (map) {
        // the map travels with the batch: a block of its slot, filled and copied below
        map_bytes = route_map_bytes(map);
        if ((rc = sl->rt_map.ensure(map_bytes))) return rc;
        if ((rc = sl->rt_map_pin.ensure(map_bytes))) return rc;
        a.map = (const uint8_t*)sl->rt_map.p;
        a.map_n = map->n_ranges;
    } else {
        // bounds of this resolver's key range: prefixes by value, tails in a small device arena
        std::vector<uint8_t> want;
        auto put_len = [&](int32_t n) {
            for (int i = 0; i < 4; i++) want.push_back((uint8_t)((uint32_t)n >> (8 * i)));
        };
        put_len(lo_len);
        if (lo_len > 0) want.insert(want.end(), lo_key, lo_key + lo_len);
        put_len(hi_len);
        if (hi_len > 0) want.insert(want.end(), hi_key, hi_key + hi_len);
        std::vector<uint8_t> btail;
        auto bound = [&](const uint8_t* k, int32_t len, DKey* d) {
            fast_prefix(k, (uint32_t)len, &d->hi, &d->lo);
            d->len = (uint32_t)len;
            d->tail = 0;
            if (len > 16) {
                d->tail = (uint32_t)btail.size();
                btail.insert(btail.end(), k + 16, k + len);
                while (btail.size() % 8) btail.push_back(0);
            }
        };
        a.has_lo = lo_len >= 0;
        a.has_hi = hi_len >= 0;
        if (a.has_lo) bound(lo_key, lo_len, &a.lo);
        if (a.has_hi) bound(hi_key, hi_len, &a.hi);
        btail.resize(btail.size() + 64, 0);
        if (want != cs->route_bounds) {
            if ((rc = sync_all(cs))) return rc;
            if ((rc = cs->route_btail.ensure(btail.size()))) return rc;
            HIPOK(hipMemcpy(cs->route_btail.p, btail.data(), btail.size(), hipMemcpyHostToDevice));
            cs->route_bounds = want;
        }
        a.btail = (const uint8_t*)cs->route_btail.p;
    }
    // the routed batch's layout at capacity offsets (upload layout)
    const UploadLayout L = upload_layout((size_t)cap_txns, (size_t)cap_reads, (size_t)cap_writes, (size_t)cap_tail);
    if ((rc = ensure_slot(sl, L.total, (size_t)cap_txns, (size_t)cap_reads))) return rc;
    const int64_t n_elems = (int64_t)n_shares * max_share_txns;
    // ranges of one share: each takes 48 bytes of endpoint records, so the stride bounds them
    const int64_t rstride = std::max<int64_t>(1, (stride - (int64_t)sizeof(ShareHeader)) / (2 * (int64_t)sizeof(DKey)));
    // a batch created with report_keys routes the shares' report flags too: a seventh scan counter
    // and the global read index of each kept read (int32: bounded by the ranges the shares can hold)
    const bool reports = b->report_enabled != 0;
    if (reports && (int64_t)n_shares * rstride > INT32_MAX) return FDBCS_E_INVALID;
    const size_t scan_bytes = 8 * (size_t)route_scan_words(n_elems, reports);
    if ((rc = sl->rt_scan.ensure(scan_bytes))) return rc;
    if (reports && (rc = sl->rt_gids.ensure(4 * ((size_t)cap_reads + 1)))) return rc;
    if ((rc = sl->rt_info.ensure(4 * (size_t)(n_shares * rstride)))) return rc;
    if ((rc = sl->rt_txpre.ensure(16 * (size_t)std::max<int64_t>(n_elems, 1)))) return rc;
    if ((rc = sl->rt_inv.ensure(4 * (size_t)std::max<int64_t>(n_elems, 1)))) return rc;
    if ((rc = sl->rt_rids.ensure(4 * ((size_t)cap_reads + 1)))) return rc;
    if ((rc = sl->rt_dres.ensure(sizeof(RouteResult)))) return rc;
    if ((rc = sl->rt_res.ensure(sizeof(RouteResult), true))) return rc;
    if ((rc = make_slot_events(sl))) return rc;
    const auto t_host = std::chrono::steady_clock::now();
    char* d = (char*)sl->dev.p;
    a.shares = (const uint8_t*)shares;
    a.stride = stride;
    a.n_shares = n_shares;
    a.tcap = std::max(1, max_share_txns);
    a.report_enabled = reports ? 1 : 0;
    a.cap_T = cap_txns;
    a.cap_R = cap_reads;
    a.cap_W = cap_writes;
    a.cap_tail = cap_tail;
    a.keys = (DKey*)(d + L.keys);
    a.info = (uint32_t*)sl->rt_info.p;
    a.rstride = rstride;
    a.txpre = (int4*)sl->rt_txpre.p;
    a.rown = (int32_t*)(d + L.rown);
    a.wown = (int32_t*)(d + L.wown);
    a.snap = (int64_t*)(d + L.snap);
    a.roff = (int32_t*)(d + L.roff);
    a.woff = (int32_t*)(d + L.woff);
    a.flags = (uint8_t*)(d + L.flags);
    a.tail = (uint8_t*)(d + L.tail);
    a.inv = (int32_t*)sl->rt_inv.p;
    a.inv_n = std::max<int64_t>(n_elems, 1);
    a.read_ids = (int32_t*)sl->rt_rids.p;
    a.read_gids = reports ? (int32_t*)sl->rt_gids.p : nullptr;
    a.out_zero = conflict_out;
    a.out_n = n_global;
    a.res = (RouteResult*)sl->rt_res.dp;
    a.dres = (RouteResult*)sl->rt_dres.p;
    ((RouteResult*)sl->rt_res.p)->error = -1;  // not written yet
    hipStream_t us = cs->ustream;
    // the shares are complete once *ready_flag == ready_value (k_route_wait); the slot's previous
    // batch may still read its device buffer
    a.ready = ready_flag;
    a.ready_value = ready_value;
    a.wait_ticks = (uint64_t)cs->route_timeout_ms * 100000ull;  // 100 MHz wall clock
    a.wait_err = (uint32_t*)((uint64_t*)sl->rt_scan.p + 2);
    HIPOK(hipMemsetAsync(sl->rt_scan.p, 0, scan_bytes, us));
    // global indices past the shares' transactions stay "not routed here"
    HIPOK(hipMemsetAsync(sl->rt_inv.p, 0xFF, 4 * (size_t)a.inv_n, us));
    if (map) {
        // derived for this resolver into the slot's pinned staging (its last copy is over: the
        // slot's previous routing was waited for), then onto the device ahead of the kernels; no
        // drain, and the batches in flight keep the blocks of their own slots
        route_map_fill(map, resolver, (uint8_t*)sl->rt_map_pin.p, map_bytes);
        HIPOK(hipMemcpyAsync(sl->rt_map.p, sl->rt_map_pin.p, map_bytes, hipMemcpyHostToDevice, us));
    }
    uint64_t* sw = (uint64_t*)sl->rt_scan.p;
    ScanState st{sw + 8, (int*)sw, (int*)(sw + 1)};
    t_record = nullptr;
    if ((rc = sl->rt_span.begin(us))) return rc;
    launch_route(us, a, st);
    HIPOK(take_launch_error());
    if ((rc = sl->rt_span.end(us))) return rc;
    sl->rt_timed = true;
    HIPOK(hipEventRecord(sl->ev_up, us));
    cs->stats.host_ms_route += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    b->bd.keys = a.keys;
    b->bd.rowner = a.rown;
    b->bd.wowner = a.wown;
    b->bd.snap = a.snap;
    b->bd.roff = a.roff;
    b->bd.woff = a.woff;
    b->bd.flags = a.flags;
    b->bd.tail = a.tail;
    b->routed = true;
    b->route_pending = true;
    b->rT = b->rR = b->rW = 0;
    b->r_cap_ranges = (int64_t)cap_reads + cap_writes;
    b->r_cap_tail = cap_tail;
    b->is_req = b->is_done = false;
    b->out_dev = conflict_out;
    b->out_n = n_global;
    b->out_ids.clear();
    b->rep_dev = nullptr;
    b->rep_n = 0;
    b->state = 1;
    return FDBCS_OK;
}

int fdbcs_batch_add_routed(fdbcs_batch* b, const void* shares, int64_t stride, int32_t n_shares, int32_t max_share_txns,
                           const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key, int32_t hi_len, int32_t cap_txns,
                           int32_t cap_reads, int32_t cap_writes, int64_t cap_tail, uint8_t* conflict_out,
                           int64_t n_global, const uint32_t* ready_flag, uint32_t ready_value) {
    return add_routed_impl(b, shares, stride, n_shares, max_share_txns, lo_key, lo_len, hi_key, hi_len, nullptr, 0,
                           cap_txns, cap_reads, cap_writes, cap_tail, conflict_out, n_global, ready_flag, ready_value);
}

int fdbcs_batch_add_routed_map(fdbcs_batch* b, const void* shares, int64_t stride, int32_t n_shares,
                               int32_t max_share_txns, const fdbcs_key_resolvers* map, int32_t resolver,
                               int32_t cap_txns, int32_t cap_reads, int32_t cap_writes, int64_t cap_tail,
                               uint8_t* conflict_out, int64_t n_global, const uint32_t* ready_flag,
                               uint32_t ready_value) {
    if (int rc = route_map_check(map, resolver)) return rc;  // before the batch is touched
    return add_routed_impl(b, shares, stride, n_shares, max_share_txns, nullptr, -1, nullptr, -1, map, resolver,
                           cap_txns, cap_reads, cap_writes, cap_tail, conflict_out, n_global, ready_flag, ready_value);
}

// Sizes of a routed batch, once its route kernels are done (blocks until then).
extern "C++" int fdbcs::impl::finish_route(fdbcs_batch* b) {
    if (!b->route_pending) return FDBCS_OK;
    if (b->dev_added) return finish_device_add(b);
    BatchSlot* sl = b->slot.get();
    HIPOK(hipEventSynchronize(sl->ev_up));
    std::atomic_thread_fence(std::memory_order_acquire);
    RouteResult r;
    memcpy(&r, (const void*)sl->rt_res.p, sizeof(r));
    if (r.error != 0) {
        // 2: the shares never arrived; 1: the routed part exceeds the capacities given; 3: n_global
        // differs from the shares' transaction count.  Whatever the routing kernels placed is
        // unusable either way: the batch goes back to the empty state, so it can be routed again
        // (with corrected arguments) or destroyed, never detected half-routed.
        if (r.error == 2) fprintf(stderr, "fdbcs: routed batch: the shares' ready flag was never set\n");
        b->routed = b->route_pending = false;
        b->out_dev = nullptr;
        b->out_n = 0;
        b->rep_dev = nullptr;
        b->rep_n = 0;
        b->is_req = b->is_done = false;  // (its kernel found the error too and wrote an empty sample)
        b->state = 0;
        return r.error == 2 ? FDBCS_E_TIMEOUT
                            : r.error == 1 ? FDBCS_E_NOMEM : r.error == 3 ? FDBCS_E_INVALID : FDBCS_E_DEVICE;
    }
    b->rT = r.T;
    b->rR = r.R;
    b->rW = r.W;
    b->r_tail = (size_t)r.tail_bytes;
    b->tail_bytes = b->r_tail;
    b->bd.tail_n = r.tail_bytes;
    b->bd.T = r.T;
    b->bd.R = r.R;
    b->bd.W = r.W;
    // history tail bytes the batch's write endpoints can add, each tail padded to 8 (a bound: the
    // kept tails plus 7 bytes of padding per write endpoint)
    b->wtail = r.tail_bytes + 14 * (int64_t)r.W;
    b->max_len = r.n_gt24 ? 25 : (r.n_gt19 ? 20 : 16);
    b->any_report = r.reports > 0;
    b->r_global_R = r.global_R;
    b->route_pending = false;
    return FDBCS_OK;
}

int fdbcs_batch_routed_info(fdbcs_batch* b, int32_t* T, int32_t* R, int32_t* W, void** inv_dev, void** read_ids_dev) {
    if (!b) return FDBCS_E_INVALID;
    if (!b->routed || b->dev_added) return FDBCS_E_STATE;
    if (int rc = finish_route(b)) return rc;
    if (T) *T = b->rT;
    if (R) *R = b->rR;
    if (W) *W = b->rW;
    if (inv_dev) *inv_dev = b->slot->rt_inv.p;
    if (read_ids_dev) *read_ids_dev = b->slot->rt_rids.p;
    return FDBCS_OK;
}

int fdbcs_sync(fdbcs_conflict_set* cs) {
    if (!cs) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    return sync_all(cs);
}

int fdbcs_batch_upload(fdbcs_batch* b) {
    if (!b) return FDBCS_E_INVALID;
    if (!b->cs) return FDBCS_E_STATE;
    if (b->state != 0) return b->state == 1 ? FDBCS_OK : FDBCS_E_STATE;
    HIPOK(hipSetDevice(b->cs->device));
    return do_upload(b, b->cs->ustream);
}

// ---- the detect call, step by step ("The detect call's steps")

// What one detect call decides before it records anything and that more than one of its steps
// reads.  Every step below takes the set, the batch and this plan, and reads no other step's
// locals.  Fields are set by plan_layout unless another step is named.
struct DetectPlan {
    fdbcs_conflict_set* const cs;
    fdbcs_batch* const b;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    const int64_t now, oldest_arg;  // the call's `now` and new_oldest_version
    // sizes and layout (detect_admit, detect_bind_results)
    int64_t T = 0, R = 0, W = 0, tail_add = 0;
    ResultLayout RL{};
    // the batch's resources
    BatchSlot* const sl;
    const int wp;  // the workspace (cs->wpar as the call found it) and its Work
    Work& w;
    // streams: batch order (X), stage A, half Y, the upload
    hipStream_t s = nullptr, sa = nullptr, ys = nullptr, us = nullptr;
    // layout flags
    int timing = 0;
    bool sampled = false, kprof = false, split = false, threaded = false, pipe = false, use_prev = false;
    bool own_upload = false, was_uploaded = false, long_keys = false;
    bool ws_busy = false;  // (record_stage_a: its event query stays where the waits are recorded)
    // tier views (plan_views): what the merge reads (delta) and what the check reads (cdelta, ps)
    Tier base, delta, cdelta;
    PrevSegs ps{};
    uint8_t* htail = nullptr;
    Scalars* sc = nullptr;
    int bsrc = 0, dsrc = 0, dchk = 0;
    // what the sort leaves for the epilogue to re-zero of its scratch (record_stage_a)
    int sort_nb = 0, sort_samples = 0;
    // the Y decisions (decide_y).  The launch arguments that read the state it rolls forward are
    // taken before it moves: the GC's (gc_oldest before gc_applied, gc_htail before tcur) and the
    // merge's view of the delta buffer it writes (merge_dlv, before that buffer's directory epoch)
    int dnew = 0, final_base = 0;
    int64_t nd_after = 0, new_oldest = 0, base_hint = 0, gc_oldest = 0;
    bool compact = false, gc = false;
    uint8_t* gc_htail = nullptr;
    MaxLevels merge_dlv;

    DetectPlan(fdbcs_conflict_set* cs_, fdbcs_batch* b_, int64_t now_, int64_t oldest_)
        : cs(cs_), b(b_), now(now_), oldest_arg(oldest_), sl(b_->slot.get()), wp(cs_->wpar), w(cs_->work[cs_->wpar]) {}

    // phase events: level 2 records every phase, level 1 only the hot kernels (roofline)
    // level 3 (per-kernel profile) records only the events around every kernel
    // level 1 with a timed kernel (fdbcs_set_timed_kernel) records only that kernel's events
    hipEvent_t rec(int ph, int level) const {
        if (timing == 3 || timing < level || (level == 1 && (!sampled || cs->timed_func))) return nullptr;
        b->recorded |= 1u << ph;
        return sl->ev[ph];
    }
    void mark(int ph) const {
        if (hipEvent_t e = rec(ph, 2)) fdb_event(LaunchList::kTimingRecord, e, s);
    }
};

// Redirects this thread's fdb_launch / fdb_event into `l` for as long as it lives, so that no
// return of a recording step, early or late, leaves t_record set (every later direct launch on the
// thread would be appended to a dead list instead of being issued).
struct RecordInto {
    explicit RecordInto(LaunchList& l) { t_record = &l; }
    ~RecordInto() { t_record = nullptr; }
    RecordInto(const RecordInto&) = delete;
    RecordInto& operator=(const RecordInto&) = delete;
};

// Step 1: may this batch be detected now, and is there room for it?
static int detect_admit(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    HIPOK(hipSetDevice(cs->device));
    if (p.now < cs->max_written) return FDBCS_E_VERSION;
    if (int rc0 = finish_route(b)) return rc0;  // a routed batch's sizes (its route ran ahead)
    if (b->routed && b->rep_dev && b->rep_n != b->r_global_R) {
        // report bytes for every read of the shares, no more and no fewer (like the conflict
        // output's size, error 3 of the routing): the batch is empty again, to be routed anew
        b->routed = false;
        b->out_dev = b->rep_dev = nullptr;
        b->out_n = b->rep_n = 0;
        b->state = 0;
        return FDBCS_E_INVALID;
    }
    if (b->T() > kMaxTxnLds) return FDBCS_E_INVALID;
    // tail offsets are 32-bit: refuse a batch that could overflow the arena (GC repacks it long before)
    // history tail bytes this batch can append (each inserted tail padded to 8 bytes)
    // only write endpoints ever enter the history (merge inserts segment begins and ends)
    p.tail_add = b->wtail;
    if (cs->tail_ub + p.tail_add + 1 >= kTailLimit) return FDBCS_E_NOMEM;
    p.T = b->T(), p.R = b->R(), p.W = b->W();
    int rc;
    if ((rc = ensure_workspace(cs, p.T, p.R, p.W))) return rc;
    if ((rc = ensure_btail(cs, (int64_t)b->tail_size()))) return rc;
    if ((rc = ensure_delta(cs, cs->nd_ub + 2 * p.W + 1))) return rc;
    if ((rc = ensure_history(cs, cs->n_ub + cs->nd_ub + 2 * p.W + 1, cs->tail_ub + p.tail_add + 1)))
        return rc;
    if ((rc = make_slot_events(b->slot.get()))) return rc;
    if (cs->ddir_counter == UINT32_MAX && cs->edir[0].p) {
        // the delta directory's 32-bit epoch tag is about to wrap: clear every entry (once per 2^32
        // batches) so that no entry left by an old fill can carry the reused epoch value
        if ((rc = sync_all(cs))) return rc;
        for (int k = 0; k < 2; k++) HIPOK(hipMemsetAsync(cs->edir[k].p, 0, 8 * (size_t)kDirAlloc, cs->stream));
        HIPOK(hipStreamSynchronize(cs->stream));
        cs->ddir_counter = 0;
    }
    return FDBCS_OK;
}

// Step 2: where the batch's results go, and its sequence number.
// results (host-mapped; verdicts written by k_resolve, scalars and flag by the epilogue):
// verdicts | scalars | completion flag, then the
// report copies rconf | hist | first_conf
static int detect_bind_results(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    const int64_t T = p.T;
    const ResultLayout& RL = p.RL = result_layout(T, p.R);
    BatchSlot* sl = p.sl;
    int rc;
    if ((rc = sl->pin_out.ensure(RL.total, true))) return rc;
    char* ho = (char*)sl->pin_out.p;
    b->h_verdict = (uint8_t*)ho;
    b->h_scal = (Scalars*)(ho + RL.sc);
    b->h_flag = (volatile uint32_t*)(ho + RL.fl);
    b->h_rconf = (uint8_t*)(ho + RL.rc);
    b->h_hist = (uint8_t*)(ho + RL.hc);
    b->h_first = (int32_t*)(ho + RL.fc);
    b->h_roff = b->routed ? (const int32_t*)(ho + RL.ro) : b->roff.data();
    b->h_flags = b->routed ? (const uint8_t*)(ho + RL.fg) : b->flags.data();
    if ((rc = sl->dverdict.ensure(T + 64))) return rc;
    if (b->out_dev && b->out_n > 0 && (!b->routed || b->dev_added)) {  // (a device-added batch: host txn_ids)
        // global -> batch transaction map, read by k_conflict_output straight from host-mapped
        // memory (n_global * 4 bytes; the slot's previous batch finished with it: its flag was seen)
        if ((int64_t)b->out_ids.size() != T) return FDBCS_E_STATE;  // transactions added after the call
        if ((rc = sl->pin_inv.ensure(4 * (size_t)b->out_n + 64, true))) return rc;
        int32_t* inv = (int32_t*)sl->pin_inv.p;
        std::fill(inv, inv + b->out_n, -1);
        for (int32_t t = 0; t < (int32_t)T; t++) inv[b->out_ids[t]] = t;
    }
    if (!b->routed) {  // (a routed batch's count came with its sizes)
        b->any_report = b->n_report > 0;  // (counted as the transactions were added)
    }
    b->seq = ++cs->seq;
    if (b->seq == 0) b->seq = ++cs->seq;  // 0 means "not done"
    *b->h_flag = 0;
    b->recorded = 0;
    return FDBCS_OK;
}

// Step 3: the stream layout and its flags, the batch's workspace, the empty stage lists and the
// tier views.  Nothing here can fail, and nothing is issued or recorded.
static void plan_layout(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    hipStream_t s = p.s = cs->stream;
    const int timing = p.timing = cs->timing;
    // Stage A (sort, positions, candidate edges) depends only on this batch: it runs on its own
    // stream and overlaps stage B of the previous batch.  Phase timing (level 2) runs both stages on
    // one stream so the phases are measured one after another.
    p.sa = (timing == 2 || cs->serial) ? s : cs->astream;  // level 3 keeps the timed layout
    cs->wpar = (p.wp + 1) % kNumWork;
    b->wp = p.wp;
    Work& w = p.w;
    // write groups need the group minima in the resolver's LDS beside the status bytes
    w.groups = cs->write_groups && p.W > 0 && p.W <= kMaxGroupWrites && p.T <= kMaxTxnLds ? 1 : 0;
    // level-1 (roofline) events on one batch in timing_every: each event record is a runtime call
    // on the submitting thread, and the per-launch averages need only a sample of the batches
    p.sampled = timing >= 2 || b->seq % (uint32_t)kTimingEvery == 0;
    p.was_uploaded = b->state == 1;
    // per-kernel events: every kernel at level 3, the kernel fdbcs_set_timed_kernel named at level 1
    // (sampled batches)
    p.sl->prof_next = 0;
    p.sl->prof_spans.clear();
    p.kprof = timing == 3 || (timing == 1 && p.sampled && cs->timed_func);
    for (LaunchList* L : {&cs->rec_a, &cs->rec_b, &cs->rec_c, &cs->rec_y}) {
        L->clear();
        L->prof = p.kprof ? &p.sl->prof : nullptr;
        L->timed_func = timing == 3 ? nullptr : cs->timed_func;
    }
    // Split read check: the base tier changes only at compactions, so unless one is still pending
    // on the stream its half of D.CheckRead runs beside stage A on its own stream; stage B keeps the
    // delta half.
    p.split = (cs->split_check == 1 || (cs->split_check == 2 && cs->n_ub >= kSplitCheckMinBase)) && !cs->serial &&
              timing != 2;
    // two submitting threads: this batch's stage A and check go out from the helper, stage B on the
    // next call.  The previous batch's stage B is recorded but maybe not issued yet, so an event it
    // records cannot be queried here: waits on its events are kept unconditionally.
    p.threaded = cs->submit_thread && timing < 2 && !cs->trace && p.sa != s;
    // The upload runs on its own stream unless the phases are timed one after another (then on
    // stage A's stream, bracketed by the upload phase's events).
    p.own_upload = timing != 2 && !cs->serial;
    p.us = p.own_upload ? cs->ustream : p.sa;
    // long-key probes pay off once tails run past a word (a 17-byte end key k\0 of a 16-byte key
    // ties on the prefix with k only, and the length decides)
    p.long_keys = b->max_len > 24;
    p.sc = (Scalars*)cs->scal.p;
    p.bsrc = cs->cur, p.dsrc = cs->dcur;
    // Stage B in two halves (fdbcs_conflict_set::ystream): X = check, resolution, D.Combine on
    // `stream`; Y = merge, compaction / GC, epilogue on `ystream`.  Unless the previous batch
    // compacted, this batch's check reads the delta before the previous batch's merge (buffer
    // dsrc ^ 1, complete once the batch before it finished Y) plus the previous batch's union
    // segments at its `now` (PrevSegs): the same history, so the check need not wait for that merge.
    p.pipe = !(timing == 2 || cs->serial);
    p.ys = p.pipe ? cs->ystream : s;
    p.use_prev = p.pipe && cs->prev_segs;
    p.dchk = p.use_prev ? p.dsrc ^ 1 : p.dsrc;
    w.trace = cs->trace ? (unsigned long long*)cs->trace_buf.p : nullptr;
    w.no_prepass = cs->no_prepass ? 1 : 0;
}

// Step 3, second part: the tier views.  Apart from plan_layout only because the views are built
// under the record span of the host-time stats (host_ms_record), as they always were.
static void plan_views(fdbcs_conflict_set* cs, DetectPlan& p) {
    Scalars* sc = p.sc;
    const int bsrc = p.bsrc, dsrc = p.dsrc, dchk = p.dchk;
    p.base = Tier{hist_of(cs, bsrc), levels_of(cs, bsrc), &sc->n, cs->header_version};
    p.delta = Tier{delta_of(cs, dsrc), dlevels_of(cs, dsrc), &sc->ndb[dsrc], kHole};
    p.cdelta = Tier{delta_of(cs, dchk), dlevels_of(cs, dchk), &sc->ndb[dchk], kHole};  // what the check reads
    if (p.use_prev) {
        const Work& pw = cs->work[cs->prev_wp];
        p.ps = PrevSegs{pw.segk, pw.btail, &pw.bsc->n_segments, cs->prev_now};
    }
    p.htail = (uint8_t*)cs->htail[cs->tcur].p;
}

// FDBCS_TRACE: the device timestamps start over with every batch (the pipeline is drained first).
static int reset_trace(fdbcs_conflict_set* cs, const Work& w) {
    HIPOK(hipStreamSynchronize(cs->astream));
    HIPOK(hipStreamSynchronize(cs->stream));
    unsigned long long init[kTrSlots];
    for (int i = 0; i < kTrSlots; i++)
        init[i] = (i == kTrSampleBegin || i == kTrCheckBegin || i == kTrEpiBegin || i == kTrResBegin || i == kTrResW0min ||
                   i == kTrPartBegin || i == kTrBktBegin)
                      ? ~0ull
                      : 0ull;
    HIPOK(hipMemcpy(w.trace, init, sizeof(init), hipMemcpyHostToDevice));
    return FDBCS_OK;
}

// Step 4: the upload (issued now) and the record of stage A: D.Sort and the candidate edges of
// D.CheckIntraBatch.
static int record_stage_a(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    hipStream_t s = p.s, sa = p.sa;
    const int wp = p.wp;
    Work& w = p.w;
    BatchSlot* sl = p.sl;
    int rc;
    if (hipEvent_t e = p.rec(kPhStart, 2)) HIPOK(hipEventRecord(e, sa));
    if (b->state == 0 && (rc = do_upload(b, p.us))) return rc;
    if (hipEvent_t e = p.rec(kPhUpload, 2)) HIPOK(hipEventRecord(e, sa));
    RecordInto recording(cs->rec_a);
    // workspace wp was last used kNumWork batches ago: that batch's epilogue re-zeroed it.
    // ev_b[wp] is recorded by every batch's stage B, whatever its stream layout, so the query is
    // never answered by a stale or never-recorded event (a timing-level change with batches in
    // flight included).
    p.ws_busy = cs->wused[wp] && (p.threaded || !stage_b_done(cs, wp));
    if (p.ws_busy && (sa != s || cs->y_async[wp])) fdb_event(LaunchList::kSyncWait, cs->ev_b[wp], sa);
    // and the check after that batch may still read its union segments and their tails
    if (cs->xfree_rec[wp] && sa != s && (p.threaded || !batch_done(cs->xfree_user[wp])))
        fdb_event(LaunchList::kSyncWait, cs->xfree_ev[wp], sa);
    cs->xfree_rec[wp] = false;
    cs->wused[wp] = true;
    cs->ws_user[wp] = b;
    // stage A reads the batch: wait for the upload stream
    if (p.own_upload || (p.was_uploaded && hipEventQuery(sl->ev_up) != hipSuccess))
        fdb_event(LaunchList::kSyncWait, sl->ev_up, sa);
    const BatchDev& bd = b->bd;
    // a routed batch's TooOld test (SkipList.cpp:770) against the oldest version every earlier
    // detect left (its routing may have run before the previous batch's detect): stage A, ahead
    // of every kernel that reads the flags (stage B)
    if (b->routed) launch_route_too_old(sa, bd, cs->oldest);
    if (w.trace && (rc = reset_trace(cs, w))) return rc;
    // D.Sort and the sorted positions.  Splitters: the quantiles the last batch of >= kQuantMinE
    // endpoints left (stage A runs in batch order on one stream), or this batch's ranked samples
    // when there are none yet (cold start)
    {
        const int64_t E = 2 * (p.R + p.W);
        const int nbk = sort_bucket_count(E, cs->bucket_target, w.slab_buckets);
        const bool cold = nbk > 1 && (cs->sort_cold || !cs->quant_valid);
        p.sort_nb = E > 0 ? nbk : 0;
        p.sort_samples = E > 0 && cold ? sort_cold_samples(E, nbk) : 0;
        const bool write_quant = E >= kQuantMinE;
        SplitKey* qt = (SplitKey*)cs->quant.p;
        if (cs->quant_sa && cs->quant_sa != sa) {
            // the splitter tables were last read and written by a sort on another stream: order
            // this sort after it (every stage A before this one has been issued: flush the helper)
            if ((rc = flush_pending(cs))) return rc;
            HIPOK(hipEventRecord(cs->ev_quant, cs->quant_sa));
            fdb_event(LaunchList::kSyncWait, cs->ev_quant, sa);
        }
        cs->quant_sa = sa;
        launch_sort(sa, bd, w, qt + cs->qcur * kQuant, write_quant ? qt + (cs->qcur ^ 1) * kQuant : nullptr, cold,
                    cs->bucket_target, b->max_len > (int32_t)kSortNxLen, cs->validate, p.rec(kPhSortBegin, 1),
                    p.rec(kPhSortEnd, 1));
        if (write_quant) {
            cs->qcur ^= 1;
            cs->quant_valid = true;
        }
    }
    p.mark(kPhSort);
    if (cs->validate) launch_validate_sort(sa, bd, w);
    w.hseq = b->seq;  // (Work is passed by value: the edge scan's finish tags its host word)
    launch_edges(sa, bd, w);
    if (sa != s) fdb_event(LaunchList::kSyncRecord, cs->ev_a[wp], sa);
    p.mark(kPhEdges);
    return FDBCS_OK;
}

// Step 5 (split check only): the record of the base-tier check, on its own stream.
static void record_base_check(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    RecordInto recording(cs->rec_c);
    const int wp = p.wp;
    hipStream_t sc_ = cs->cstream;
    fdb_event(LaunchList::kSyncWait, p.sl->ev_up, sc_);
    if (p.ws_busy) fdb_event(LaunchList::kSyncWait, cs->ev_b[wp], sc_);
    if (cs->cmp_recorded && (p.threaded || hipEventQuery(cs->ev_cmp) != hipSuccess))
        fdb_event(LaunchList::kSyncWait, cs->ev_cmp, sc_);
    fdb_event(LaunchList::kTimingRecord, p.rec(kPhCheckBegin, 1), sc_);
    launch_check_tier(sc_, b->bd, p.w, p.base, true, p.htail, p.long_keys, PrevSegs{});
    fdb_event(LaunchList::kTimingRecord, p.rec(kPhCheckEnd, 1), sc_);
    fdb_event(LaunchList::kSyncRecord, cs->ev_c[wp], sc_);
}

// Step 6: the record of stage B, half X: D.CheckRead, then batch order (resolution, D.Combine, the
// conflict output and the report copies), ended by ev_res.
static void record_half_x(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    RecordInto recording(cs->rec_b);
    hipStream_t s = p.s, sa = p.sa;
    const int wp = p.wp;
    const int64_t T = p.T, R = p.R;
    Work& w = p.w;
    BatchSlot* sl = p.sl;
    const BatchDev& bd = b->bd;
    const ResultLayout& RL = p.RL;
    if (sa == s || !p.was_uploaded || hipEventQuery(sl->ev_up) != hipSuccess) fdb_event(LaunchList::kSyncWait, sl->ev_up, s);
    {
        // the delta the check reads is complete: Y of the batch before the previous one (with the
        // previous batch's segments), or of the previous batch (it compacted, or nothing pending).
        // Only a Y on ystream needs the event (a timing-level change may switch layouts mid-flight).
        const int wy = p.use_prev ? cs->prev2_wp : cs->last_wp;
        if (wy >= 0 && cs->y_async[wy] && (p.threaded || !stage_b_done(cs, wy)))
            fdb_event(LaunchList::kSyncWait, cs->ev_b[wy], s);
    }
    if (p.split) {
        b->check_hist = cs->n_ub;  // the timed (base-tier) check
        launch_check_tier(s, bd, w, p.cdelta, false, p.htail, p.long_keys, p.ps);
    } else {
        b->check_hist = cs->n_ub + cs->nd_ub;
        fdb_event(LaunchList::kTimingRecord, p.rec(kPhCheckBegin, 1), s);
        launch_check(s, bd, w, p.base, p.cdelta, p.htail, p.long_keys, p.ps);
        fdb_event(LaunchList::kTimingRecord, p.rec(kPhCheckEnd, 1), s);
    }
    if (p.use_prev) {  // the previous batch's workspace may be reused once this check is done with it
        cs->xfree_ev[cs->prev_wp] = cs->ev_res[wp];  // recorded at the end of this half X
        cs->xfree_user[cs->prev_wp] = b;
        cs->xfree_rec[cs->prev_wp] = true;
    }
    p.mark(kPhCheck);
    if (sa != s) fdb_event(LaunchList::kSyncWait, cs->ev_a[wp], s);
    if (p.split) fdb_event(LaunchList::kSyncWait, cs->ev_c[wp], s);
    w.vdev = (uint8_t*)sl->dverdict.p;  // (Work by value: the resolution's launches carry it)
    launch_resolve(s, bd, w, b->any_report, (uint8_t*)sl->pin_out.dp, p.sc);
    w.vdev = nullptr;
    if (b->out_dev && b->out_n > 0)  // multi-resolver combine input, final before the completion flag
        launch_conflict_output(s, bd, w,
                               b->routed && !b->dev_added ? (const int32_t*)sl->rt_inv.p : (const int32_t*)sl->pin_inv.dp,
                               b->out_n, b->out_dev);
    if (b->any_report) {  // before the epilogue re-zeroes hist_conf (into the host-mapped results)
        char* hdv = (char*)sl->pin_out.dp;
        if (R) launch_copy_bytes(s, hdv + RL.rc, w.rconf, R);
        launch_copy_bytes(s, hdv + RL.hc, w.hist_conf, T);
        launch_copy_bytes(s, hdv + RL.fc, w.first_conf, 4 * T);
        if (b->routed) {  // the report loop's roff and flags (TooOld included: stage A is done)
            launch_copy_bytes(s, hdv + RL.ro, bd.roff, 4 * (T + 1));
            launch_copy_bytes(s, hdv + RL.fg, bd.flags, T);
        }
    }
    // the multi-resolver report input (zeros when no sub-transaction reports); history conflicts
    // are reported without candidate edges too, so outside the resolution's skip group
    if (b->routed && b->rep_dev && b->rep_n > 0)
        launch_report_bytes(s, bd, w, (const int32_t*)sl->rt_gids.p, b->rep_n, b->rep_dev);
    p.mark(kPhIntra);
    p.mark(kPhCombine);
    fdb_event(LaunchList::kSyncRecord, cs->ev_res[wp], s);
}

// Step 7: what half Y will do: compaction, the GC turn, the delta directory's epoch.  Host state
// only: nothing is recorded and nothing can fail, so the policy reads (and changes) in one place.
static void decide_y(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    const int dnew = p.dnew = p.dsrc ^ 1;
    p.nd_after = cs->nd_ub + 2 * p.W;
    p.new_oldest = std::max(cs->oldest, p.oldest_arg);
    // Compaction when the delta may outgrow its bound (or on the forced cadence); removeBefore
    // (SkipList.cpp:880-889) runs with it whenever the oldest version moved.
    bool compact = p.nd_after > delta_limit_for(cs, cs->n_ub);
    if (cs->gc_interval > 0 && ++cs->batches_since_compact >= cs->gc_interval) compact = true;
    if (cs->tail_ub > cs->tail_reclaim) compact = true;
    bool gc = false;
    p.final_base = p.bsrc;
    p.base_hint = cs->n_ub + p.nd_after + 1;
    if (compact) {
        p.final_base = p.bsrc ^ 1;
        cs->batches_since_compact = 0;
        // Size-triggered compactions (gc_interval 0) run removeBefore on every kGcEveryCompactions-th
        // one: a full pass over the base costs ~10x the compaction copy at C2 while one
        // window-step of oldest-version movement makes few boundaries removable (a boundary goes
        // only when it and its predecessor are both older, SkipList.cpp:555-561). Verdict-neutral
        // either way; a forced cadence (gc_interval > 0) keeps GC at every compaction.  Past the
        // tail-reclaim threshold the GC also repacks the tail arena.
        const bool gc_turn = cs->gc_interval > 0 || ++cs->compactions_since_gc >= kGcEveryCompactions;
        gc = (p.new_oldest > cs->gc_applied && gc_turn) || cs->tail_ub > cs->tail_reclaim;
        if (gc) cs->compactions_since_gc = 0;
    }
    if (gc) {  // from the compaction's output into the other base buffer and the other tail arena
        p.gc_htail = (uint8_t*)cs->htail[cs->tcur ^ 1].p;
        p.gc_oldest = std::max(p.new_oldest, cs->gc_applied);
        cs->tcur ^= 1;
        p.final_base ^= 1;
        cs->gc_applied = p.new_oldest;
    }
    p.compact = b->compacted = compact;
    p.gc = b->gc_ran = gc;
    // the epilogue that rebuilds the delta tier's index also fills its directory under a new epoch
    // (a compaction leaves none).  The epoch tag is 32 bits: before it wraps, every entry is
    // cleared (detect_admit), so a slot an old fill left behind is never trusted.
    p.merge_dlv = dlevels_of(cs, dnew);  // (the merge's launches carry the epoch the buffer had)
    if (compact || !cs->edir[dnew].p) {
        cs->ddir_epoch[dnew] = 0;
    } else {
        cs->ddir_epoch[dnew] = ++cs->ddir_counter;
    }
}

// Step 8: the record of stage B, half Y, after X (ev_res): D.MergeWrite, compaction / GC and the
// epilogue, ended by ev_b (and ev_cmp when the base was rewritten).
static void record_half_y(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    RecordInto recording(cs->rec_y);
    hipStream_t s = p.s, ys = p.ys;
    const int wp = p.wp, bsrc = p.bsrc, dsrc = p.dsrc, dnew = p.dnew;
    const int64_t nd_after = p.nd_after;
    const bool compact = p.compact, gc = p.gc, long_keys = p.long_keys;
    Work& w = p.w;
    const BatchDev& bd = b->bd;
    Scalars* sc = p.sc;
    uint8_t* htail = p.htail;
    if (ys != s) fdb_event(LaunchList::kSyncWait, cs->ev_res[wp], ys);
    // D.MergeWrite into the delta tier
    char* hd = (char*)p.sl->pin_out.dp;
    launch_merge(ys, bd, w, p.delta.h, p.delta.m, delta_of(cs, dnew), p.merge_dlv, &sc->ndb[dsrc], htail, sc,
                 p.now, cs->dlvl3_n, cs->dlvl2_n, cs->nd_ub + 1, p.rec(kPhCopyBegin, 1), p.rec(kPhCopyEnd, 1), long_keys);
    p.mark(kPhMerge);
    if (compact)
        launch_compact(ys, w, p.base.h, p.base.m, delta_of(cs, dnew), hist_of(cs, bsrc ^ 1), htail, sc,
                       cs->header_version, cs->lvl3_n, cs->lvl2_n, nd_after + 1, cs->n_ub + 1, p.rec(kPhCompBegin, 1),
                       p.rec(kPhCompEnd, 1), long_keys ? 2 : 1, cs->n_ub <= (16 << 20) ? 1024 : 4096,
                       cs->n_ub > (16 << 20));
    p.mark(kPhCompact);
    if (gc)  // (final_base already names the buffer the GC writes)
        launch_gc(ys, w, hist_of(cs, p.final_base ^ 1), hist_of(cs, p.final_base), htail, p.gc_htail, sc, p.gc_oldest,
                  cs->header_version, p.base_hint);
    p.mark(kPhGc);
    launch_epilogue(ys, bd, w, compact ? levels_of(cs, p.final_base) : dlevels_of(cs, dnew), sc, compact ? 1 : 0,
                    gc ? 1 : 0, (uint8_t*)hd, (uint32_t*)(hd + p.RL.fl), b->seq,
                    compact ? p.base_hint : nd_after + 1, &sc->ndb[dnew], p.sort_nb, p.sort_samples);
    fdb_event(LaunchList::kSyncRecord, cs->ev_b[wp], ys);
    // (no event marks the slot free: a slot returns to the pool only from fdbcs_batch_destroy,
    // after the batch's completion flag was seen or its streams were synchronized; every kernel
    // of the batch that reads or writes the slot precedes the epilogue, which touches none of it)
    if (compact || gc) {  // later base-tier checks wait for this rewrite of the base
        fdb_event(LaunchList::kSyncRecord, cs->ev_cmp, ys);
        cs->cmp_recorded = true;
    }
    p.mark(kPhEpilogue);
    p.mark(kPhEnd);
}

// Step 9: hand the lists to the helper thread, or issue them now.
static int submit_lists(fdbcs_conflict_set* cs, fdbcs_batch* b, DetectPlan& p) {
    LaunchList &la = cs->rec_a, &lb = cs->rec_b, &lc = cs->rec_c, &ly = cs->rec_y;
    hipStream_t s = p.s, sa = p.sa, ys = p.ys;
    int rc;
    if (p.threaded) {
        // the helper issues this batch's stage A and check while this thread issues the stage B
        // of earlier batches; this batch's stage B is held for a later call (or a flush)
        if ((rc = worker_wait(cs))) return rc;
        std::swap(cs->work_a, la);
        std::swap(cs->work_c, lc);  // empty unless split
        cs->work_sa = sa;
        cs->work_a_seq = b->seq;
        // Which held X halves go out now, oldest first: the batch of two calls ago whatever the
        // host knows, the previous batch's once its edge word is there (x_known).  A split check
        // goes out behind every Y recorded so far (it may wait on the ev_cmp one of them records),
        // so under that layout nothing is held a second call.
        int go = cs->n_held == kMaxHold ? 1 : 0;
        cs->stats.x_forced += go;
        while (go < cs->n_held && (p.split || x_known(cs, cs->held[go]))) go++;
        // Two at one call: the older one's X and Y both from this thread, before the hand-over.  The
        // newer one's X may wait on the older one's ev_b (its check reads the delta that Y leaves,
        // when that batch compacted or no segments stand in for it), and a wait takes the event's
        // last record: that Y must be issued before this X, not beside it by the helper.
        while (go > 1) {
            if (flush_pending(cs, cs->held[0].batch)) return FDBCS_E_DEVICE;
            go--;
        }
        fdbcs_batch* xb = nullptr;
        if (go) {  // its Y half to the helper, after the X this thread issues below
            fdbcs_conflict_set::Held& h = cs->held[0];
            cs->work_y_seq = h.batch->seq;
            std::swap(cs->work_y, h.y);
            cs->work_ys = h.ys;
            cs->work_y_batch = xb = h.batch;
            std::swap(cs->go_x, h.x);  // (go_x: empty, kept in the set for its capacity)
            cs->work_need_x = cs->x_issued.load(std::memory_order_relaxed) + 1;
            drop_held(cs, 1);
        }
        // the check goes out once every stage B that is issued at this call is
        cs->work_need_b = cs->b_recorded - (uint32_t)cs->n_held;
        worker_start_job(cs);
        if (xb) {
            const hipError_t e = issue_x(cs, xb, cs->go_x);
            cs->x_issued.fetch_add(1, std::memory_order_release);  // (the helper issues its Y)
            if (e != hipSuccess) return FDBCS_E_DEVICE;
        }
        fdbcs_conflict_set::Held& h = cs->held[cs->n_held++];
        std::swap(h.x, lb);
        std::swap(h.y, ly);
        h.ys = ys;
        h.batch = b;
        cs->b_recorded++;
    } else if (flush_pending(cs)) {
        return FDBCS_E_DEVICE;
    } else {
        HIPOK(la.replay(sa));
        if (p.split) HIPOK(lc.replay(cs->cstream));
        HIPOK(lb.replay(s));
        HIPOK(ly.replay(ys));
    }
    HIPOK(take_launch_error());
    return FDBCS_OK;
}

// Step 10: the batch is on its way: roll the set's cross-batch state forward.
static void commit_batch(fdbcs_conflict_set* cs, fdbcs_batch* b, const DetectPlan& p) {
    const int wp = p.wp;
    cs->cur = p.final_base;
    cs->dcur = p.dnew;
    // the next batch's check: this batch's segments stand in for its merge unless it compacted
    cs->prev_segs = p.pipe && !p.compact;
    cs->prev2_wp = cs->last_wp;
    cs->last_wp = wp;
    cs->y_async[wp] = p.ys != p.s;
    cs->prev_wp = wp;
    cs->prev_now = p.now;
    cs->oldest = p.new_oldest;  // SkipList.cpp:880-882
    if (p.W) cs->max_written = std::max(cs->max_written, p.now);
    if (p.compact) {
        cs->n_ub += p.nd_after;
        cs->nd_ub = 0;
    } else {
        cs->nd_ub = p.nd_after;
    }
    cs->tail_ub += p.tail_add;
    cs->inflight++;
    cs->x_valid = false;
    b->state = 2;
    if (cs->htrace) cs->htr[0].push_back({b->seq, 'D', mono_ns(p.t_begin), mono_ns()});
}

int fdbcs_batch_detect_async(fdbcs_batch* b, int64_t now, int64_t new_oldest_version) {
    if (!b) return FDBCS_E_INVALID;
    if (!b->cs) return FDBCS_E_STATE;
    if (b->state > 1) return FDBCS_E_STATE;
    fdbcs_conflict_set* cs = b->cs;
    DetectPlan p(cs, b, now, new_oldest_version);
    int rc;
    if ((rc = detect_admit(cs, b, p))) return rc;
    if ((rc = detect_bind_results(cs, b, p))) return rc;
    plan_layout(cs, b, p);
    // a layout that issues from this thread alone holds nothing back: whatever an earlier layout
    // left held goes out first, so that every event this batch's steps query has been recorded
    if (!p.threaded && cs->n_held && (rc = flush_pending(cs))) return rc;
    cs->stats.host_ms_prepare += host_ms_since(p.t_begin);
    const auto t_rec = std::chrono::steady_clock::now();
    plan_views(cs, p);
    if ((rc = record_stage_a(cs, b, p))) return rc;
    if (p.split) record_base_check(cs, b, p);
    record_half_x(cs, b, p);
    decide_y(cs, b, p);
    record_half_y(cs, b, p);
    cs->stats.host_ms_record += host_ms_since(t_rec);
    const auto t_sub = std::chrono::steady_clock::now();
    if ((rc = submit_lists(cs, b, p))) return rc;
    cs->stats.host_ms_submit += host_ms_since(t_sub);
    commit_batch(cs, b, p);
    return FDBCS_OK;
}

// ---- the wait for a detected batch, step by step

// Until the batch's completion flag is seen: its stage B issued if it still waits for the next
// detect or for the helper, then the spin.
static int wait_flag(fdbcs_conflict_set* cs, fdbcs_batch* b) {
    const int64_t tw0 = cs->htrace ? mono_ns() : 0;
    HIPOK(hipSetDevice(cs->device));
    for (int k = 0; k < cs->n_held; k++)
        if (cs->held[k].batch == b) {  // its stage B is still held: issue it now, behind every batch before it
            if (int rc = flush_pending(cs, b)) return rc;
            break;
        }
    if (cs->work_y_batch == b)  // its Y is with the helper: issued (events and all) before reading them
        if (int rc = worker_wait(cs)) return rc;
    // the epilogue publishes b->seq; poll it, checking the streams for errors only every ~2 ms:
    // hipStreamQuery takes runtime locks the helper thread's launches need, so querying at
    // the spin rate slows the submission of the batches behind this one
    auto t_q = std::chrono::steady_clock::now();
    for (uint64_t spin = 0; *b->h_flag != b->seq; spin++) {
        __builtin_ia32_pause();
        if ((spin & 4095) != 4095) continue;
        if (std::chrono::steady_clock::now() - t_q < std::chrono::milliseconds(cs->wait_query_ms)) continue;
        t_q = std::chrono::steady_clock::now();
        // the flag comes from the epilogue (stage B's Y half): done or failing once both
        // halves are idle
        hipError_t e = hipStreamQuery(cs->astream);
        if (e == hipSuccess || e == hipErrorNotReady) e = hipStreamQuery(cs->stream);
        if (e == hipSuccess) e = hipStreamQuery(cs->ystream);
        if (e != hipSuccess && e != hipErrorNotReady) {
            fprintf(stderr, "fdbcs: stream error while waiting: %s\n", hipGetErrorString(e));
            return FDBCS_E_DEVICE;
        }
        if (e == hipSuccess && *b->h_flag != b->seq) {
            fprintf(stderr, "fdbcs: stream idle but batch %u not completed\n", b->seq);
            return FDBCS_E_DEVICE;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (cs->htrace) cs->htr[0].push_back({b->seq, 'W', tw0, mono_ns()});
    return FDBCS_OK;
}

// FDBCS_TRACE=1: the device timestamps of the batch's kernel sections, printed.
static int print_trace(fdbcs_conflict_set* cs, const fdbcs_batch* b) {
    if (int rc = sync_all(cs)) return rc;
    unsigned long long tr[kTrSlots];
    HIPOK(hipMemcpy(tr, cs->trace_buf.p, sizeof(tr), hipMemcpyDeviceToHost));
    auto us = [&](int a, int z) { return (double)((long long)(tr[z] - tr[a])) / 100.0; };  // 100 MHz
    fprintf(stderr,
            "fdbcs trace: sample %.2f us, check %.2f us (check starts %+.2f us after sample); epilogue "
            "levels %.2f, zero %.2f, host %.2f, fence %.2f us\n",
            us(kTrSampleBegin, kTrSampleEnd), us(kTrCheckBegin, kTrCheckEnd), us(kTrSampleBegin, kTrCheckBegin),
            us(kTrEpiBegin, kTrEpiLevels), us(kTrEpiLevels, kTrEpiZero), us(kTrEpiZero, kTrEpiHost),
            us(kTrEpiHost, kTrEpiFence));
    fprintf(stderr,
            "fdbcs trace: sort partition fill %.2f, search %.2f, end %.2f us; bucket prologue %.2f, "
            "sorted %.2f, ties %.2f, end %.2f us (partition start to bucket start %.2f us)\n",
            us(kTrPartBegin, kTrPartFill), us(kTrPartBegin, kTrPartSearch), us(kTrPartBegin, kTrPartEnd),
            us(kTrBktBegin, kTrBktPrologue), us(kTrBktBegin, kTrBktSorted), us(kTrBktBegin, kTrBktTies),
            us(kTrBktBegin, kTrBktEnd), us(kTrPartBegin, kTrBktBegin));
    const double nw = tr[kTrBktWaves] ? (double)tr[kTrBktWaves] : 1.0;
    fprintf(stderr,
            "fdbcs trace: bucket tie runs: %llu lanes in runs, %llu ranked in registers, %llu serially, "
            "longest run %llu\n",
            tr[kTrBktRuns], tr[kTrBktSimple], tr[kTrBktSlow], tr[kTrBktMaxRun]);
    fprintf(stderr, "fdbcs trace: bucket per wave (%llu waves): load %.2f, sort %.2f, ties %.2f, put %.2f us\n",
            tr[kTrBktWaves], tr[kTrBktSumLoad] / nw / 100.0, tr[kTrBktSumSort] / nw / 100.0,
            tr[kTrBktSumTies] / nw / 100.0, tr[kTrBktSumPut] / nw / 100.0);
    const double np = tr[kTrPartWaves] ? (double)tr[kTrPartWaves] : 1.0;
    fprintf(stderr,
            "fdbcs trace: partition per wave (%llu waves): fill %.2f, tail copy %.2f, search %.2f, "
            "place %.2f us\n",
            tr[kTrPartWaves], tr[kTrPartSumFill] / np / 100.0, tr[kTrPartSumCopy] / np / 100.0,
            tr[kTrPartSumSearch] / np / 100.0, tr[kTrPartSumPlace] / np / 100.0);
    fprintf(stderr,
            "fdbcs trace: resolve pre-pass %.2f us, wait %.2f us, rounds %.2f us (setup %.2f, first round "
            "%.2f of which minima %.2f, %d rounds), finish %.2f us; waves start %.2f..%.2f us before the first kernarg use\n",
            us(kTrResBegin, kTrResPre), us(kTrResPre, kTrResWait), us(kTrResWait, kTrResRounds),
            us(kTrResWait, kTrResSetup), us(kTrResSetup, kTrResRound1), us(kTrResSetup, kTrResMin1),
            (int)b->h_scal->intra_rounds, us(kTrResRounds, kTrResEnd), us(kTrResW0min, kTrResWait),
            us(kTrResW0max, kTrResWait));
    fprintf(stderr, "fdbcs trace: combine chunk 0: loads %.2f, scan1 %.2f, scan2 %.2f, stores %.2f us\n",
            us(kTrResRounds, kTrCmbLoad), us(kTrCmbLoad, kTrCmbScan1), us(kTrCmbScan1, kTrCmbScan2),
            us(kTrCmbScan2, kTrCmbStore));
    return FDBCS_OK;
}

// conflictingKeyRangeMap: every conflicting read for history conflicts (SkipList.cpp:641-645),
// the first for intra-batch conflicts (SkipList.cpp:821-828).
static void rebuild_conflicting_reads(fdbcs_batch* b) {
    const int32_t T = b->T();
    b->conf_off.assign(T + 1, 0);
    b->conf_idx.clear();
    if (!b->any_report) return;
    // (a routed batch: the sub-transaction's own indexInTx, as the resolver's map holds it)
    const int32_t* roff = b->h_roff;
    const uint8_t* flags = b->h_flags;
    for (int32_t t = 0; t < T; t++) {
        if ((flags[t] & kFlagReport) && b->h_verdict[t] == FDBCS_TRANSACTION_CONFLICT) {
            if (b->h_hist[t]) {
                for (int32_t r = roff[t]; r < roff[t + 1]; r++)
                    if (b->h_rconf[r]) b->conf_idx.push_back(r - roff[t]);
            } else if (b->h_first[t] != INT_MAX) {
                b->conf_idx.push_back(b->h_first[t]);
            }
        }
        b->conf_off[t + 1] = (int32_t)b->conf_idx.size();
    }
}

// The finished batch's share of the set's stats: counts, the phase and roofline times of the
// events it recorded (synchronized first) and the per-kernel profile.
static int account_stats(fdbcs_conflict_set* cs, fdbcs_batch* b) {
    fdbcs_stats& st = cs->stats;
    st.batches++;
    st.transactions += b->T();
    st.read_ranges += b->R();
    st.write_ranges += b->W();
    // timing events may trail the completion flag: wait for the last one recorded
    for (int e : {(int)kPhEnd, (int)kPhCompEnd, (int)kPhCopyEnd, (int)kPhCheckEnd})
        if ((b->recorded >> e) & 1u) {
            HIPOK(hipEventSynchronize(b->slot->ev[e]));
            break;
        }
    for (const auto& sp : b->slot->prof_spans) {  // per-kernel events (levels 3 and 1)
        HIPOK(hipEventSynchronize(sp.second.second));
        const double ms = Span::between(sp.second.first, sp.second.second);
        auto it = std::find_if(cs->kprof.begin(), cs->kprof.end(), [&](const auto& k) { return k.func == sp.first; });
        if (it == cs->kprof.end()) {
            cs->kprof.push_back({sp.first, 0, 0.0});
            it = cs->kprof.end() - 1;
        }
        it->launches += 1;
        it->ms += ms;
    }
    if (!b->slot->prof_spans.empty()) b->slot->prof_pool.count();
    b->slot->prof_spans.clear();
    auto ph = [&](int a, int z) {
        return ((b->recorded >> a) & (b->recorded >> z) & 1u) ? Span::between(b->slot->ev[a], b->slot->ev[z]) : 0.0;
    };
    st.ms_upload += ph(kPhStart, kPhUpload);
    st.ms_sort += ph(kPhUpload, kPhSort);
    st.ms_intra += ph(kPhSort, kPhEdges) + ph(kPhCheck, kPhIntra);
    st.ms_check_read += ph(kPhEdges, kPhCheck);
    st.ms_combine += ph(kPhIntra, kPhCombine);
    st.ms_merge += ph(kPhCombine, kPhMerge);
    st.ms_compact += ph(kPhMerge, kPhCompact);
    st.ms_gc += ph(kPhCompact, kPhGc);
    st.ms_epilogue += ph(kPhGc, kPhEpilogue);
    st.ms_total += ph(kPhUpload, kPhEnd);
    // roofline inputs: a kernel's launches, bytes and device time are counted together, on the
    // batches whose events were recorded (timing level 1 samples 1 batch in timing_every)
    if (b->h_scal->intra_edges < 0) {
        st.intra_fallbacks += 1;
    } else {
        st.intra_edges += b->h_scal->intra_edges;
        st.intra_rounds += b->h_scal->intra_rounds;
    }
    // an edge-free batch whose X half went out whole: the host issued it before the edge word came
    if (b->x_unskipped && b->h_scal->intra_edges == 0) st.x_edge_free_unskipped += 1;
    b->x_unskipped = false;
    // algorithmic bytes of the copy kernels (roofline.py): read every kept old boundary and
    // every inserted one (its key from the batch), write every boundary of the result, 32 B
    // each (16 B key, 8 B length/tail, 8 B version); kept + inserted = the result's size
    {
        const int64_t kept = b->h_scal->d_before - b->h_scal->d_rem, out = b->h_scal->nd_next;
        const int64_t bytes = 32 * (kept + (out - kept) + out);
        st.merge_bytes_all += bytes;
        st.delta_sum += b->h_scal->d_before;
        st.base_sum += b->h_scal->n;
        st.segments_sum += b->h_scal->n_segments;
        if ((b->recorded >> kPhCopyEnd) & 1u) {
            st.ms_merge_kernel += ph(kPhCopyBegin, kPhCopyEnd);
            st.merge_launches += 1;
            st.merge_bytes += bytes;
        }
    }
    if ((b->recorded >> kPhCheckEnd) & 1u) {
        st.ms_check_kernel += ph(kPhCheckBegin, kPhCheckEnd);
        st.check_launches += b->R() > 0;
        st.check_reads += b->R();
        st.check_history += b->R() > 0 ? b->check_hist : 0;
    }
    if ((b->recorded >> kPhSortEnd) & 1u) {
        st.ms_sort_kernel += ph(kPhSortBegin, kPhSortEnd);
        st.sort_launches += 1;
        st.sort_items += 2 * (int64_t)(b->R() + b->W());
    }
    st.gc_runs += b->gc_ran ? 1 : 0;
    st.sort_big_buckets += b->h_scal->sort_big;
    if (b->routed && !b->dev_added && b->slot->rt_timed) {
        st.ms_route_kernels += b->slot->rt_span.ms();
        st.routed_batches += 1;
        b->slot->rt_timed = false;
    }
    if (b->compacted) {
        st.compactions += 1;
        // kept base boundaries read, delta boundaries inserted read, result written
        const int64_t kept = b->h_scal->c_before - b->h_scal->c_rem;
        const int64_t bytes = 32 * (kept + (b->h_scal->n_next - kept) + b->h_scal->n_next);
        st.compact_bytes_all += bytes;
        if ((b->recorded >> kPhCompEnd) & 1u) {
            st.ms_compact_kernel += ph(kPhCompBegin, kPhCompEnd);
            st.compact_launches += 1;
            st.compact_bytes += bytes;
        }
    }
    return FDBCS_OK;
}

int fdbcs_batch_wait(fdbcs_batch* b, uint8_t* verdicts, int32_t* n_committed, int32_t* n_too_old) {
    if (!b) return FDBCS_E_INVALID;
    if (b->state == 2 && !b->cs) return FDBCS_E_STATE;
    fdbcs_conflict_set* cs = b->cs;
    if (b->state == 2) {
        int rc;
        if ((rc = wait_flag(cs, b))) return rc;
        if (cs->trace && cs->inflight == 1 && (rc = print_trace(cs, b))) return rc;
        if (b->h_scal->debug_error) {
            fprintf(stderr, "fdbcs: device invariant check failed (debug_error=%d)\n", b->h_scal->debug_error);
            cs->inflight--;
            b->state = 3;
            return FDBCS_E_DEVICE;
        }
        const int32_t T = b->T();
        int32_t nc = 0, nt = 0;
        for (int32_t t = 0; t < T; t++) {
            nc += b->h_verdict[t] == FDBCS_TRANSACTION_COMMITTED;
            nt += b->h_verdict[t] == FDBCS_TRANSACTION_TOO_OLD;
        }
        b->n_committed = nc;
        b->n_too_old = nt;
        rebuild_conflicting_reads(b);
        if ((rc = account_stats(cs, b))) return rc;
        cs->inflight--;
        if (cs->inflight == 0) {
            cs->n_ub = b->h_scal->n;
            cs->nd_ub = b->h_scal->nd;
            cs->tail_ub = b->h_scal->tail_used;
        }
        b->state = 3;
    }
    if (b->state != 3) return FDBCS_E_STATE;
    if (verdicts && b->T()) memcpy(verdicts, b->h_verdict, b->T());
    if (n_committed) *n_committed = b->n_committed;
    if (n_too_old) *n_too_old = b->n_too_old;
    return FDBCS_OK;
}

int fdbcs_batch_detect_conflicts(fdbcs_batch* b, int64_t now, int64_t new_oldest_version, uint8_t* verdicts,
                                 int32_t* n_committed, int32_t* n_too_old) {
    int rc = fdbcs_batch_detect_async(b, now, new_oldest_version);
    if (rc) return rc;
    return fdbcs_batch_wait(b, verdicts, n_committed, n_too_old);
}

int fdbcs_batch_conflicting_reads(fdbcs_batch* b, int32_t txn, int32_t* idx_out, int32_t cap, int32_t* n_out) {
    if (!b || !n_out) return FDBCS_E_INVALID;
    if (b->state != 3) return FDBCS_E_STATE;
    if (txn < 0 || txn >= b->T()) return FDBCS_E_INVALID;
    const int32_t a = b->conf_off[txn], e = b->conf_off[txn + 1];
    *n_out = e - a;
    if (idx_out)
        for (int32_t i = a; i < e && i - a < cap; i++) idx_out[i - a] = b->conf_idx[i];
    return FDBCS_OK;
}

int fdbcs_batch_too_old(fdbcs_batch* b, int32_t* idx_out, int32_t cap, int32_t* n_out) {
    if (!b || !n_out || cap < 0) return FDBCS_E_INVALID;
    if (b->routed) return FDBCS_E_STATE;  // decided at detect (k_route_too_old)
    int32_t n = 0;
    for (int32_t t = 0; t < (int32_t)b->flags.size(); t++) {
        if (!(b->flags[t] & kFlagTooOld)) continue;
        if (idx_out && n < cap) idx_out[n] = t;
        n++;
    }
    *n_out = n;
    return FDBCS_OK;
}

int fdbcs_batch_device_verdicts(fdbcs_batch* b, void** dptr) {
    if (!b || !dptr) return FDBCS_E_INVALID;
    if (b->state < 2) return FDBCS_E_STATE;
    *dptr = b->slot->dverdict.p;
    return FDBCS_OK;
}

int fdbcs_batch_set_conflict_output(fdbcs_batch* b, const int32_t* txn_ids, int32_t n_global, uint8_t* dev_out) {
    if (!b || n_global < 0 || (n_global > 0 && !dev_out)) return FDBCS_E_INVALID;
    if (!b->cs || b->state >= 2) return FDBCS_E_STATE;
    const int32_t T = b->T();
    if (T > 0 && !txn_ids) return FDBCS_E_INVALID;
    std::vector<uint8_t> seen((size_t)n_global, 0);
    for (int32_t t = 0; t < T; t++) {
        if (txn_ids[t] < 0 || txn_ids[t] >= n_global) return FDBCS_E_INVALID;
        if (seen[txn_ids[t]]++) return FDBCS_E_INVALID;  // one batch transaction per global index
    }
    b->out_ids.assign(txn_ids, txn_ids + T);
    b->out_n = n_global;
    b->out_dev = dev_out;
    return FDBCS_OK;
}

int fdbcs_batch_set_report_output(fdbcs_batch* b, uint8_t* dev_out, int64_t n_global_reads) {
    if (!b || !dev_out || n_global_reads < 0) return FDBCS_E_INVALID;
    if (!b->cs || !b->routed || b->dev_added || !b->report_enabled || b->state >= 2) return FDBCS_E_STATE;
    // the size is compared with the shares' reads at detect, once the routing kernels have run
    b->rep_dev = dev_out;
    b->rep_n = n_global_reads;
    return FDBCS_OK;
}

int fdbcs_batch_report_entries(fdbcs_batch* b, uint8_t* entry_out, int32_t cap) {
    if (!b || cap < 0 || (cap > 0 && !entry_out)) return FDBCS_E_INVALID;
    if (b->state != 3) return FDBCS_E_STATE;
    // conflictingKeyRangeMap[t] exists iff addTransaction registered a read range of a reporting,
    // admitted (not TooOld) transaction (SkipList.cpp:770-784)
    const int32_t n = std::min(cap, b->T());
    for (int32_t t = 0; t < n; t++)
        entry_out[t] = b->any_report && (b->h_flags[t] & kFlagReport) && b->h_roff[t + 1] > b->h_roff[t] &&
                       b->h_verdict[t] != FDBCS_TRANSACTION_TOO_OLD;
    return FDBCS_OK;
}

int fdbcs_debug_kernel_time(fdbcs_batch* b, int which, int reps, double* us_per_launch) {
    if (!b || !us_per_launch || reps <= 0 || which < 0 || which > 4) return FDBCS_E_INVALID;
    if (!b->cs) return FDBCS_E_STATE;
    fdbcs_conflict_set* cs = b->cs;
    HIPOK(hipSetDevice(cs->device));
    if (b->state == 0)
        if (int rc = fdbcs_batch_upload(b)) return rc;
    if (b->state != 1) return FDBCS_E_STATE;
    if (cs->inflight) return FDBCS_E_STATE;
    const int64_t T = b->T(), R = b->R(), W = b->W();
    if (int rc = ensure_workspace(cs, T, R, W)) return rc;
    if (int rc = sync_all(cs)) return rc;
    Work& w = cs->work[cs->wpar];
    Scalars* sc = (Scalars*)cs->scal.p;
    const Tier base{hist_of(cs, cs->cur), levels_of(cs, cs->cur), &sc->n, cs->header_version};
    const Tier delta{delta_of(cs, cs->dcur), dlevels_of(cs, cs->dcur), &sc->ndb[cs->dcur], kHole};
    if (which == 1 || which == 2) {  // the sort kernels
        if (!cs->quant_valid) return FDBCS_E_STATE;  // warm splitters only: detect a batch first
        HIPOK(debug_time_sort(cs->stream, b->bd, w, (SplitKey*)cs->quant.p + cs->qcur * kQuant, cs->bucket_target,
                              b->max_len > (int32_t)kSortNxLen, which, reps, us_per_launch));
        return FDBCS_OK;
    }
    Span span;
    const bool dlong = b->max_len > 24;
    // 0: the whole check; 3 / 4: the split check's base / delta tier launch alone
    auto one = [&]() {
        uint8_t* ht = (uint8_t*)cs->htail[cs->tcur].p;
        if (which == 0)
            launch_check(cs->stream, b->bd, w, base, delta, ht, dlong);
        else
            launch_check_tier(cs->stream, b->bd, w, which == 3 ? base : delta, which == 3, ht, dlong, PrevSegs{});
    };
    one();
    if (int rc = span.begin(cs->stream)) return rc;
    for (int i = 0; i < reps; i++) one();
    if (int rc = span.end(cs->stream)) return rc;
    HIPOK(hipEventSynchronize(span.e1));
    *us_per_launch = span.ms() * 1000.0 / reps;
    // the check leaves per-transaction conflict flags the next batch on this workspace expects zeroed
    HIPOK(hipMemsetAsync(w.hist_conf, 0, w.cap_T, cs->stream));
    HIPOK(hipMemsetAsync(w.rconf, 0, w.cap_R, cs->stream));
    HIPOK(hipStreamSynchronize(cs->stream));
    return FDBCS_OK;
}

int fdbcs_debug_live_resources(int64_t* device_buffers, int64_t* host_buffers, int64_t* events, int64_t* streams) {
    if (!device_buffers || !host_buffers || !events || !streams) return FDBCS_E_INVALID;
    *device_buffers = live_device_buffers.load();
    *host_buffers = live_host_buffers.load();
    *events = live_events.load();
    *streams = live_streams.load();
    return FDBCS_OK;
}

}  // extern "C"
