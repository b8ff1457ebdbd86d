// transfer.cpp — the maintenance entry points of the C-ABI (include/fdb_conflict_set.h): history
// export, the history digests, split keys, the two history imports, the resolver's iops sample and
// the read versions of a batch.
// They work on an idle set (or, for the sample, off the detect stream) through the state and
// helpers of engine_impl.h and launch the kernels of transfer.hip; the detect pipeline's host side
// is engine.cpp.
#include "engine_impl.h"
#include "transfer.h"

// The bounds of a key range as the entry points take them (a length below 0: no bound).
static int import_bounds_ok(const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key, int32_t hi_len) {
    if ((lo_len > 0 && !lo_key) || (hi_len > 0 && !hi_key)) return FDBCS_E_INVALID;
    if (lo_len >= 0 && hi_len >= 0 && cmp_bytes(lo_key, lo_len, hi_key, hi_len) > 0) return FDBCS_E_INVALID;
    return FDBCS_OK;
}

// A keyed result back to the host: n items of item_bytes each, n + 1 key offsets and the key bytes.
static int copy_keyed_result(int64_t n, int64_t nbytes, void* items, const void* d_items, size_t item_bytes,
                             int64_t* key_offsets, const void* d_offsets, uint8_t* key_bytes, const void* d_bytes) {
    if (n) HIPOK(hipMemcpy(items, d_items, item_bytes * (size_t)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(key_offsets, d_offsets, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost));
    if (nbytes) HIPOK(hipMemcpy(key_bytes, d_bytes, (size_t)nbytes, hipMemcpyDeviceToHost));
    return FDBCS_OK;
}

// What the export and the digest of an idle set read alike: the tiers as they stand, the floor and the
// bounds (lo / hi as RouteArgs::lo / hi: DKey + tail bytes, bt, for a small device buffer).
static int export_inputs(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t floor_version, ExportArgs& a, Scalars& sc, std::vector<uint8_t>& bt) {
    HIPOK(hipMemcpy(&sc, cs->scal.p, sizeof(sc), hipMemcpyDeviceToHost));
    a = ExportArgs{};
    a.nb = sc.n;
    a.nd = sc.ndb[cs->dcur];
    a.base = hist_of(cs, cs->cur);
    a.delta = delta_of(cs, cs->dcur);
    a.htail = (const uint8_t*)cs->htail[cs->tcur].p;
    a.hdr = cs->header_version;
    a.floor = floor_version;
    auto norm = [&](const uint8_t* p, int32_t len, DKey& k) {
        dkey_prefix(p, (uint32_t)len, &k.hi, &k.lo);
        k.len = (uint32_t)len;
        k.tail = (uint32_t)bt.size();
        if (len > 16) bt.insert(bt.end(), p + 16, p + len);
    };
    a.has_lo = lo_len >= 0;
    a.has_hi = hi_len >= 0;
    if (a.has_lo) norm(lo_key, lo_len, a.lo);
    if (a.has_hi) norm(hi_key, hi_len, a.hi);
    return FDBCS_OK;
}

// Their scratch: the bounds' tails and one position and one value per delta boundary.  Neither keeps
// anything there past its own call.
static int export_scratch(fdbcs_conflict_set* cs, ExportArgs& a, const std::vector<uint8_t>& bt) {
    int rc;
    if ((rc = cs->x_btail.ensure(bt.size() + kTailSlack))) return rc;
    if ((rc = cs->x_pos.ensure(8 * (size_t)(a.nd + 1)))) return rc;
    if ((rc = cs->x_val.ensure(8 * (size_t)(a.nd + 1)))) return rc;
    a.btail = (const uint8_t*)cs->x_btail.p;
    a.d_pos = (int64_t*)cs->x_pos.p;
    a.d_val = (int64_t*)cs->x_val.p;
    return FDBCS_OK;
}

// The words and chains of the digest (include/fdb_conflict_set.h), restated for host arrays.
static inline uint64_t digest_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// e_c(k, v) of the definition for both lanes.
static inline void digest_entry(const uint8_t* p, uint64_t len, int64_t version, uint64_t (&e)[2]) {
    constexpr uint64_t G = 0x9E3779B97F4A7C15ull, S[2] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull};
    uint64_t h[2] = {digest_mix(S[0] + len), digest_mix(S[1] + len)};
    for (uint64_t o = 0; o < len; o += 8) {
        uint64_t w = 0;  // bytes [o, o + 8) big-endian, zero past the key
        for (uint64_t b = 0; b < 8; b++) w = (w << 8) | (o + b < len ? p[o + b] : 0);
        for (uint64_t& x : h) x = digest_mix((x ^ w) + G);
    }
    for (int c = 0; c < 2; c++) e[c] = digest_mix((h[c] ^ (uint64_t)version) + G);
}

// The arrays of a digest on the host (fdbcs_history_digest_arrays and its partitioned form).
static int digest_arrays_ok(int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets, const int64_t* versions) {
    if (n < 0 || (n > 0 && (!key_offsets || !versions))) return FDBCS_E_INVALID;
    if (n > 0 && key_offsets[0] != 0) return FDBCS_E_INVALID;
    for (int64_t i = 0; i < n; i++)
        if (key_offsets[i + 1] < key_offsets[i]) return FDBCS_E_INVALID;
    if (n > 0 && key_offsets[n] > 0 && !key_bytes) return FDBCS_E_INVALID;
    return FDBCS_OK;
}

constexpr int64_t kMaxDigestRanges = 65536;  // as the routing map's ranges

// The bounds of a partition (fdbcs_history_digest_ranges and its host form): ascending keys in the
// export's layout; *K_out: the ranges they and the open ends define.
static int ranges_bounds_ok(int32_t n_bounds, const uint8_t* bound_bytes, const int64_t* bound_offsets, int open_lo,
                            int open_hi, int64_t* K_out) {
    if (n_bounds < 0 || (n_bounds > 0 && !bound_offsets)) return FDBCS_E_INVALID;
    const int64_t K = (int64_t)n_bounds - 1 + (open_lo ? 1 : 0) + (open_hi ? 1 : 0);
    if (K < 1) return FDBCS_E_INVALID;
    if (n_bounds > 0 && bound_offsets[0] != 0) return FDBCS_E_INVALID;
    for (int32_t i = 0; i < n_bounds; i++) {
        const int64_t len = bound_offsets[i + 1] - bound_offsets[i];
        if (len < 0 || len > (int64_t)INT32_MAX) return FDBCS_E_INVALID;
    }
    if (n_bounds > 0 && bound_offsets[n_bounds] > 0 && !bound_bytes) return FDBCS_E_INVALID;
    if (K > kMaxDigestRanges) return FDBCS_E_NOMEM;
    for (int32_t i = 1; i < n_bounds; i++) {
        const int64_t* o = bound_offsets + i - 1;
        if (cmp_bytes(bound_bytes + o[0], (int32_t)(o[1] - o[0]), bound_bytes + o[1], (int32_t)(o[2] - o[1])) > 0)
            return FDBCS_E_INVALID;
    }
    *K_out = K;
    return FDBCS_OK;
}

extern "C" {

int fdbcs_history_export(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t floor_version, int64_t* n_out, int64_t* key_bytes_out,
                         int64_t* header_version_out) {
    if (!cs || !n_out || !key_bytes_out || !header_version_out) return FDBCS_E_INVALID;
    if (int rc = import_bounds_ok(lo_key, lo_len, hi_key, hi_len)) return rc;
    if (cs->inflight) return FDBCS_E_STATE;
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    cs->x_valid = false;
    Scalars sc;
    ExportArgs a;
    std::vector<uint8_t> bt;
    int rc;
    if ((rc = export_inputs(cs, lo_key, lo_len, hi_key, hi_len, floor_version, a, sc, bt))) return rc;
    const int64_t total = a.nb + a.nd;
    // the byte scan's exact range (transfer.hip, history export): refuse rather than wrap
    if (total >= ((int64_t)1 << 29) || 16 * total + sc.tail_used >= ((int64_t)1 << 35)) return FDBCS_E_NOMEM;
    const int64_t tiles = export_tiles(total);
    if ((rc = export_scratch(cs, a, bt))) return rc;
    if ((rc = cs->x_state.ensure(8 * (size_t)(kXwWords + 4 * tiles)))) return rc;
    if ((rc = cs->x_ver.ensure(8 * (size_t)(total + 1)))) return rc;
    if ((rc = cs->x_off.ensure(8 * (size_t)(total + 1)))) return rc;
    if ((rc = cs->x_bytes.ensure((size_t)(16 * total + sc.tail_used + 64)))) return rc;
    a.words = (int64_t*)cs->x_state.p;
    a.tile_tb = a.words + kXwWords + 3 * tiles;  // after the scan's granules
    a.versions = (int64_t*)cs->x_ver.p;
    a.offsets = (int64_t*)cs->x_off.p;
    a.bytes = (uint8_t*)cs->x_bytes.p;
    a.bytes_cap = (int64_t)cs->x_bytes.cap;
    hipStream_t s = cs->stream;
    if (!bt.empty()) HIPOK(hipMemcpyAsync(cs->x_btail.p, bt.data(), bt.size(), hipMemcpyHostToDevice, s));
    HIPOK(hipMemsetAsync(cs->x_state.p, 0, 8 * (size_t)(kXwWords + 3 * tiles), s));
    if (int rc = cs->x_span.begin(s)) return rc;
    launch_export(s, a, levels_of(cs, cs->cur), (uint64_t*)cs->x_state.p + kXwWords, sc.tail_used > 0 ? 2 : 1);
    HIPOK(take_launch_error());
    if (int rc = cs->x_span.end(s)) return rc;
    int64_t words[kXwWords];
    HIPOK(hipMemcpyAsync(words, cs->x_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->x_ms_kernels = cs->x_span.ms();
    cs->x_ms_d2h = 0;
    if (((const int32_t*)&words[kXwScan])[1]) return FDBCS_E_DEVICE;  // look-back bound, positions out of order, key buffer
    cs->x_n = words[kXwN];
    cs->x_nbytes = words[kXwBytes];
    cs->x_hdr = words[kXwHeader];
    cs->x_valid = true;
    *n_out = cs->x_n;
    *key_bytes_out = cs->x_nbytes;
    *header_version_out = words[kXwHeader];
    return FDBCS_OK;
}

int fdbcs_history_export_read(fdbcs_conflict_set* cs, uint8_t* key_bytes, int64_t key_bytes_cap, int64_t* key_offsets,
                              int64_t* versions, int64_t cap) {
    if (!cs || key_bytes_cap < 0 || cap < 0 || !key_offsets) return FDBCS_E_INVALID;
    if (!cs->x_valid) return FDBCS_E_STATE;
    if (cap < cs->x_n || key_bytes_cap < cs->x_nbytes) return FDBCS_E_NOMEM;
    if ((cs->x_n && !versions) || (cs->x_nbytes && !key_bytes)) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = copy_keyed_result(cs->x_n, cs->x_nbytes, versions, cs->x_ver.p, 8, key_offsets, cs->x_off.p, key_bytes,
                                   cs->x_bytes.p))
        return rc;
    cs->x_ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    cs->x_valid = false;
    return FDBCS_OK;
}

int fdbcs_history_export_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_d2h) {
    if (!cs || !ms_kernels || !ms_d2h) return FDBCS_E_INVALID;
    *ms_kernels = cs->x_ms_kernels;
    *ms_d2h = cs->x_ms_d2h;
    return FDBCS_OK;
}

int fdbcs_history_digest(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t floor_version, fdbcs_digest* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    if (int rc = import_bounds_ok(lo_key, lo_len, hi_key, hi_len)) return rc;
    if (cs->inflight) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    Scalars sc;
    ExportArgs a;
    std::vector<uint8_t> bt;
    int rc;
    if ((rc = export_inputs(cs, lo_key, lo_len, hi_key, hi_len, floor_version, a, sc, bt))) return rc;
    // no result arrays and no scan: words, then one start per tile.  A pending export's words
    // (x_state) and result arrays are not touched.
    const int64_t tiles = export_tiles(a.nb + a.nd);
    if ((rc = export_scratch(cs, a, bt))) return rc;
    if ((rc = cs->g_state.ensure(8 * (size_t)(kXwWords + tiles)))) return rc;
    a.words = (int64_t*)cs->g_state.p;
    a.tile_tb = a.words + kXwWords;
    hipStream_t s = cs->stream;
    if (!bt.empty()) HIPOK(hipMemcpyAsync(cs->x_btail.p, bt.data(), bt.size(), hipMemcpyHostToDevice, s));
    HIPOK(hipMemsetAsync(cs->g_state.p, 0, 8 * (size_t)kXwWords, s));
    if (int rc = cs->g_span.begin(s)) return rc;
    launch_export_digest(s, a, levels_of(cs, cs->cur), sc.tail_used > 0 ? 2 : 1);
    HIPOK(take_launch_error());
    if (int rc = cs->g_span.end(s)) return rc;
    int64_t words[kXwWords];
    HIPOK(hipMemcpyAsync(words, cs->g_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->g_ms_kernels = cs->g_span.ms();
    cs->g_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (((const int32_t*)&words[kXwScan])[1]) return FDBCS_E_DEVICE;  // positions out of order
    out->n = words[kXwN];
    out->key_bytes = words[kXwBytes];
    out->header_version = words[kXwHeader];
    out->sum[0] = (uint64_t)words[kDwSum0];
    out->sum[1] = (uint64_t)words[kDwSum1];
    return FDBCS_OK;
}

int fdbcs_history_digest_arrays(int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                                const int64_t* versions, int64_t header_version, fdbcs_digest* out) {
    if (!out) return FDBCS_E_INVALID;
    if (int rc = digest_arrays_ok(n, key_bytes, key_offsets, versions)) return rc;
    uint64_t sum[2] = {0, 0};
    for (int64_t i = 0; i < n; i++) {
        uint64_t e[2];
        digest_entry(key_bytes + key_offsets[i], (uint64_t)(key_offsets[i + 1] - key_offsets[i]), versions[i], e);
        sum[0] += e[0];
        sum[1] += e[1];
    }
    out->n = n;
    out->key_bytes = n > 0 ? key_offsets[n] : 0;
    out->header_version = header_version;
    out->sum[0] = sum[0];
    out->sum[1] = sum[1];
    return FDBCS_OK;
}

int fdbcs_history_digest_ranges(fdbcs_conflict_set* cs, int32_t n_bounds, const uint8_t* bound_bytes,
                                const int64_t* bound_offsets, int open_lo, int open_hi, int64_t floor_version,
                                fdbcs_digest* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    int64_t K = 0;
    if (int rc = ranges_bounds_ok(n_bounds, bound_bytes, bound_offsets, open_lo, open_hi, &K)) return rc;
    const int64_t nbytes = n_bounds > 0 ? bound_offsets[n_bounds] : 0;
    if (nbytes + 16 >= ((int64_t)1 << 32)) return FDBCS_E_NOMEM;  // a bound's tail offset is 32-bit
    if (cs->inflight) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    // the span's bounds for the launches the digest shares: the first and the last bound
    const uint8_t* lo_key = nullptr;
    const uint8_t* hi_key = nullptr;
    int32_t lo_len = -1, hi_len = -1;
    if (!open_lo) lo_key = bound_bytes, lo_len = (int32_t)bound_offsets[1];
    if (!open_hi) {
        hi_key = bound_bytes + bound_offsets[n_bounds - 1];
        hi_len = (int32_t)(nbytes - bound_offsets[n_bounds - 1]);
    }
    Scalars sc;
    ExportArgs a;
    std::vector<uint8_t> bt;
    int rc;
    if ((rc = export_inputs(cs, lo_key, lo_len, hi_key, hi_len, floor_version, a, sc, bt))) return rc;
    const int64_t tiles = export_tiles(a.nb + a.nd);
    if ((rc = export_scratch(cs, a, bt))) return rc;
    if ((rc = cs->g_state.ensure(8 * (size_t)(kXwWords + tiles)))) return rc;
    if ((rc = cs->r_bytes.ensure((size_t)nbytes + kTailSlack))) return rc;
    if ((rc = cs->r_off.ensure(8 * (size_t)(n_bounds + 1)))) return rc;
    if ((rc = cs->r_pos.ensure(16 * (size_t)(K + 1)))) return rc;
    if ((rc = cs->r_out.ensure(8 * (size_t)(kDrWords * K)))) return rc;
    a.words = (int64_t*)cs->g_state.p;
    a.tile_tb = a.words + kXwWords;
    DigestRangesArgs r{};
    r.n_bounds = n_bounds;
    r.open_lo = open_lo ? 1 : 0;
    r.open_hi = open_hi ? 1 : 0;
    r.K = K;
    r.bytes = (const uint8_t*)cs->r_bytes.p;
    r.offsets = (const int64_t*)cs->r_off.p;
    r.lt = (int64_t*)cs->r_pos.p;
    r.le = r.lt + (K + 1);
    r.out = (int64_t*)cs->r_out.p;
    hipStream_t s = cs->stream;
    if (!bt.empty()) HIPOK(hipMemcpyAsync(cs->x_btail.p, bt.data(), bt.size(), hipMemcpyHostToDevice, s));
    if (nbytes) HIPOK(hipMemcpyAsync(cs->r_bytes.p, bound_bytes, (size_t)nbytes, hipMemcpyHostToDevice, s));
    if (n_bounds)
        HIPOK(hipMemcpyAsync(cs->r_off.p, bound_offsets, 8 * (size_t)(n_bounds + 1), hipMemcpyHostToDevice, s));
    HIPOK(hipMemsetAsync(cs->g_state.p, 0, 8 * (size_t)kXwWords, s));
    HIPOK(hipMemsetAsync(cs->r_out.p, 0, 8 * (size_t)(kDrWords * K), s));
    if (int rc = cs->g_span.begin(s)) return rc;
    launch_export_digest_ranges(s, a, r, levels_of(cs, cs->cur), sc.tail_used > 0 ? 2 : 1);
    HIPOK(take_launch_error());
    if (int rc = cs->g_span.end(s)) return rc;
    int64_t words[kXwWords];
    std::vector<int64_t> res((size_t)(kDrWords * K));
    HIPOK(hipMemcpyAsync(words, cs->g_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    HIPOK(hipMemcpyAsync(res.data(), cs->r_out.p, 8 * res.size(), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->g_ms_kernels = cs->g_span.ms();
    cs->g_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (((const int32_t*)&words[kXwScan])[1]) return FDBCS_E_DEVICE;  // positions out of order
    for (int64_t i = 0; i < K; i++) {
        const int64_t* w = res.data() + kDrWords * i;
        out[i].n = w[kDrN];
        out[i].key_bytes = w[kDrBytes];
        out[i].header_version = w[kDrHeader];
        out[i].sum[0] = (uint64_t)w[kDrSum0];
        out[i].sum[1] = (uint64_t)w[kDrSum1];
    }
    return FDBCS_OK;
}

int fdbcs_history_digest_arrays_ranges(int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                                       const int64_t* versions, int64_t header_version, int32_t n_bounds,
                                       const uint8_t* bound_bytes, const int64_t* bound_offsets, int open_lo,
                                       int open_hi, fdbcs_digest* out) {
    if (!out) return FDBCS_E_INVALID;
    if (int rc = digest_arrays_ok(n, key_bytes, key_offsets, versions)) return rc;
    int64_t K = 0;
    if (int rc = ranges_bounds_ok(n_bounds, bound_bytes, bound_offsets, open_lo, open_hi, &K)) return rc;
    for (int64_t i = 0; i < n; i++)
        if (key_offsets[i + 1] - key_offsets[i] > (int64_t)INT32_MAX) return FDBCS_E_INVALID;
    for (int64_t i = 0; i < K; i++) out[i] = fdbcs_digest{0, 0, header_version, {0, 0}};
    const int shift = open_lo ? 1 : 0;  // bound b is edge b + shift
    auto header = [&](int64_t b, int64_t v) {
        if (b + shift < K) out[b + shift].header_version = v;
    };
    auto cmp = [&](int64_t b, int64_t i) {  // bound b against boundary i
        return cmp_bytes(bound_bytes + bound_offsets[b], (int32_t)(bound_offsets[b + 1] - bound_offsets[b]),
                         key_bytes + key_offsets[i], (int32_t)(key_offsets[i + 1] - key_offsets[i]));
    };
    // one walk over the boundaries and the bounds, both ascending: b = bounds at or below boundary i
    int64_t cur = header_version, b = 0;
    for (int64_t i = 0; i < n; i++) {
        while (b < n_bounds && cmp(b, i) < 0) header(b++, cur);  // the bound lies below this boundary
        cur = versions[i];
        bool on_bound = false;
        while (b < n_bounds && cmp(b, i) == 0) header(b++, cur), on_bound = true;
        const int64_t range = b - 1 + shift;  // after its last bound at or below
        if (on_bound || range < 0 || range >= K) continue;
        uint64_t e[2];
        const uint64_t len = (uint64_t)(key_offsets[i + 1] - key_offsets[i]);
        digest_entry(key_bytes + key_offsets[i], len, versions[i], e);
        out[range].n += 1;
        out[range].key_bytes += (int64_t)len;
        out[range].sum[0] += e[0];
        out[range].sum[1] += e[1];
    }
    while (b < n_bounds) header(b++, cur);
    return FDBCS_OK;
}

int fdbcs_history_split_keys(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                             int32_t hi_len, int32_t want, int64_t* n_out, int64_t* key_bytes_out) {
    if (!cs || !n_out || !key_bytes_out || want < 0) return FDBCS_E_INVALID;
    if (int rc = import_bounds_ok(lo_key, lo_len, hi_key, hi_len)) return rc;
    if (want > kMaxDigestRanges) return FDBCS_E_NOMEM;
    if (cs->inflight) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    cs->k_valid = false;
    Scalars sc;
    ExportArgs x;  // the tiers and the bounds as the export reads them
    std::vector<uint8_t> bt;
    int rc;
    if ((rc = export_inputs(cs, lo_key, lo_len, hi_key, hi_len, kHole, x, sc, bt))) return rc;
    if ((rc = cs->x_btail.ensure(bt.size() + kTailSlack))) return rc;
    if ((rc = cs->k_state.ensure(8 * (size_t)kSwWords))) return rc;
    if ((rc = cs->k_off.ensure(8 * (size_t)(want + 1)))) return rc;
    SplitArgs a{};
    a.base = x.base;
    a.delta = x.delta;
    a.htail = x.htail;
    a.nb = x.nb;
    a.nd = x.nd;
    a.has_lo = x.has_lo;
    a.has_hi = x.has_hi;
    a.lo = x.lo;
    a.hi = x.hi;
    a.btail = (const uint8_t*)cs->x_btail.p;
    a.want = want;
    a.words = (int64_t*)cs->k_state.p;
    a.offsets = (int64_t*)cs->k_off.p;
    hipStream_t s = cs->stream;
    if (!bt.empty()) HIPOK(hipMemcpyAsync(cs->x_btail.p, bt.data(), bt.size(), hipMemcpyHostToDevice, s));
    HIPOK(hipMemsetAsync(cs->k_state.p, 0, 8 * (size_t)kSwWords, s));
    if (int rc = cs->k_span.begin(s)) return rc;
    launch_split_plan(s, a);
    HIPOK(take_launch_error());
    if (int rc = cs->k_span.end(s)) return rc;
    int64_t words[kSwWords];
    HIPOK(hipMemcpyAsync(words, cs->k_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    double ms = cs->k_span.ms();
    const int64_t n = words[kSwN], nbytes = words[kSwBytes];
    if (n < 0 || n > want || nbytes < 0 || nbytes > 16 * n + sc.tail_used) return FDBCS_E_DEVICE;
    if (n > 0) {
        if ((rc = cs->k_bytes.ensure((size_t)nbytes + 64))) return rc;
        a.bytes = (uint8_t*)cs->k_bytes.p;
        a.bytes_cap = (int64_t)cs->k_bytes.cap;
        if (int rc = cs->k_span.begin(s)) return rc;
        launch_split_gather(s, a, n);
        HIPOK(take_launch_error());
        if (int rc = cs->k_span.end(s)) return rc;
        HIPOK(hipMemcpyAsync(words, cs->k_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
        HIPOK(hipStreamSynchronize(s));
        ms += cs->k_span.ms();
        if ((int32_t)words[kSwError]) return FDBCS_E_DEVICE;  // an offset past the key buffer
    }
    cs->k_ms_kernels = ms;
    cs->k_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    cs->k_n = n;
    cs->k_nbytes = nbytes;
    cs->k_valid = true;
    *n_out = n;
    *key_bytes_out = nbytes;
    return FDBCS_OK;
}

int fdbcs_history_split_keys_read(fdbcs_conflict_set* cs, uint8_t* key_bytes, int64_t key_bytes_cap,
                                  int64_t* key_offsets, int64_t cap) {
    if (!cs || key_bytes_cap < 0 || cap < 0 || !key_offsets) return FDBCS_E_INVALID;
    if (!cs->k_valid) return FDBCS_E_STATE;
    if (cap < cs->k_n || key_bytes_cap < cs->k_nbytes) return FDBCS_E_NOMEM;
    if (cs->k_nbytes && !key_bytes) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(cs->device));
    HIPOK(hipMemcpy(key_offsets, cs->k_off.p, 8 * (size_t)(cs->k_n + 1), hipMemcpyDeviceToHost));
    if (cs->k_nbytes) HIPOK(hipMemcpy(key_bytes, cs->k_bytes.p, (size_t)cs->k_nbytes, hipMemcpyDeviceToHost));
    cs->k_valid = false;
    return FDBCS_OK;
}

int fdbcs_history_split_keys_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host) {
    if (!cs || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    *ms_kernels = cs->k_ms_kernels;
    *ms_host = cs->k_ms_host;
    return FDBCS_OK;
}

int fdbcs_history_digest_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host) {
    if (!cs || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    *ms_kernels = cs->g_ms_kernels;
    *ms_host = cs->g_ms_host;
    return FDBCS_OK;
}

// What the last successful import did (fdbcs_history_import_info).
static void import_note(fdbcs_conflict_set* cs, int32_t path, int64_t base, int64_t delta_before, int64_t delta_after) {
    cs->i_path = path;
    cs->i_info_base = base;
    cs->i_info_before = delta_before;
    cs->i_info_after = delta_after;
}

// What phase 1 of an import leaves for its continuation.
struct ImportPlan {
    Scalars sc;            // the set's scalars before the import
    int64_t m;             // overlay boundaries
    int64_t u_end;         // 8-byte units of the overlay's tail arena
    ImportDeltaArgs d;     // d.a: the arguments both imports share; the rest is the delta import's
    int64_t dw[kIdWords];  // what k_impd_bounds found (to_delta only)
};

// The tier pointers of an import's arguments (again after a capacity change: the buffers may have
// moved).  The fold writes the non-current base buffer and arena, the delta import the non-current
// delta buffer and the current arena.
static void import_tiers(fdbcs_conflict_set* cs, ImportArgs& a, bool to_delta) {
    a.base = hist_of(cs, cs->cur);
    a.delta = delta_of(cs, cs->dcur);
    a.htail = (const uint8_t*)cs->htail[cs->tcur].p;
    a.dst = to_delta ? delta_of(cs, cs->dcur ^ 1) : hist_of(cs, cs->cur ^ 1);
    a.tdst = (uint8_t*)cs->htail[to_delta ? cs->tcur : cs->tcur ^ 1].p;
    a.dst_cap = to_delta ? cs->delta_cap : cs->hist_cap;
    a.tdst_units = cs->tail_cap / 8;
}

// The merged arrays of phase 2, for `total` positions.
static int import_merged(fdbcs_conflict_set* cs, ImportArgs& a, int64_t total) {
    int rc;
    if ((rc = cs->i_mval.ensure(8 * (size_t)total))) return rc;
    if ((rc = cs->i_mkey.ensure(16 * (size_t)total))) return rc;
    if ((rc = cs->i_mlt.ensure(8 * (size_t)total))) return rc;
    if ((rc = cs->i_dblt.ensure(8 * (size_t)(a.nd + 1)))) return rc;
    a.m_val = (int64_t*)cs->i_mval.p;
    a.m_key = (ulonglong2*)cs->i_mkey.p;
    a.m_lt = (uint2*)cs->i_mlt.p;
    a.d_blt = (int64_t*)cs->i_dblt.p;
    return FDBCS_OK;
}

// Phase 1 of both imports, on device arrays.  The set is idle, its streams drained; d_bytes is
// 8-byte aligned with >= 16 readable bytes past nbytes.  The host does no per-boundary work: it
// sizes the overlay from n and nbytes, launches the validation and the overlay's build (to_delta:
// and the search that places lo and hi in both tiers) and reads the words back once.  *done: the
// import is over (an empty range: validated, nothing to do).
static int import_phase1(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t n, const uint8_t* d_bytes, int64_t nbytes, const int64_t* d_off,
                         const int64_t* d_ver, int64_t ihdr, int64_t* boundaries_out, bool to_delta, ImportPlan& pl,
                         bool* done) {
    *done = false;
    Scalars& sc = pl.sc;
    HIPOK(hipMemcpy(&sc, cs->scal.p, sizeof(sc), hipMemcpyDeviceToHost));
    const int64_t nb = sc.n, nd = sc.ndb[cs->dcur];
    if (nb + nd + n + 2 >= ((int64_t)1 << 31)) return FDBCS_E_NOMEM;  // the fold's 32-bit scan components
    const bool has_lo = lo_len >= 0, has_hi = hi_len >= 0;
    const int64_t ll = has_lo ? lo_len : 0, hl = has_hi ? hi_len : 0;
    // overlay tails, in 8-byte units: imported boundary j at (offset_j >> 3) + j, then lo's and hi's
    const int64_t u_lo = ((nbytes + 7) >> 3) + n + 1, u_hi = u_lo + ((ll + 7) >> 3) + 1, u_end = u_hi + ((hl + 7) >> 3) + 1;
    // the fold packs at most that many units behind the arena's bytes, the delta import appends
    // them from the next whole unit on
    const int64_t tail_base = (sc.tail_used + 7) >> 3;
    const int64_t tail_need = to_delta ? 8 * (tail_base + u_end) : sc.tail_used + 8 * u_end;
    if (tail_need + 1 >= kTailLimit) return FDBCS_E_NOMEM;
    int rc;
    const int64_t bnd_hi = (ll + 7) / 8 * 8 + 16;
    if ((rc = cs->i_bnd.ensure((size_t)(bnd_hi + hl + 64)))) return rc;
    if ((rc = cs->i_okey.ensure(16 * (size_t)(n + 2)))) return rc;
    if ((rc = cs->i_olt.ensure(8 * (size_t)(n + 2)))) return rc;
    if ((rc = cs->i_over.ensure(8 * (size_t)(n + 2)))) return rc;
    if ((rc = cs->i_otail.ensure(8 * (size_t)u_end + kTailSlack))) return rc;
    if ((rc = cs->i_vblt.ensure(8 * (size_t)(n + 2)))) return rc;
    if ((rc = cs->i_state.ensure(8 * (size_t)kIwWords))) return rc;
    if (to_delta && (rc = cs->i_dstate.ensure(8 * (size_t)kIdWords))) return rc;
    pl.u_end = u_end;
    pl.d = ImportDeltaArgs{};
    ImportArgs& a = pl.d.a;
    import_tiers(cs, a, to_delta);
    a.nb = nb;
    a.nd = nd;
    a.hdr = cs->header_version;
    a.n = n;
    a.bytes = d_bytes;
    a.nbytes = nbytes;
    a.offsets = d_off;
    a.versions = d_ver;
    a.ihdr = ihdr;
    a.has_lo = has_lo;
    a.has_hi = has_hi;
    a.lo_len = (int32_t)ll;
    a.hi_len = (int32_t)hl;
    a.bnd = (const uint8_t*)cs->i_bnd.p;
    a.bnd_hi = bnd_hi;
    a.ov.key = (ulonglong2*)cs->i_okey.p;
    a.ov.lt = (uint2*)cs->i_olt.p;
    a.ov.ver = (int64_t*)cs->i_over.p;
    a.otail = (uint8_t*)cs->i_otail.p;
    a.otail_lo = u_lo;
    a.otail_hi = u_hi;
    a.ovhdr = has_lo ? kHole : ihdr;
    a.words = (int64_t*)cs->i_state.p;
    a.v_blt = (int64_t*)cs->i_vblt.p;
    a.new_hdr = has_lo ? cs->header_version : std::max(cs->header_version, ihdr);
    pl.d.dwords = (int64_t*)cs->i_dstate.p;
    pl.d.tail_base = tail_base;
    hipStream_t s = cs->stream;
    if (ll) HIPOK(hipMemcpyAsync(cs->i_bnd.p, lo_key, (size_t)ll, hipMemcpyHostToDevice, s));
    if (hl) HIPOK(hipMemcpyAsync((uint8_t*)cs->i_bnd.p + bnd_hi, hi_key, (size_t)hl, hipMemcpyHostToDevice, s));
    HIPOK(hipMemsetAsync(cs->i_state.p, 0, 8 * (size_t)kIwWords, s));
    if (to_delta) HIPOK(hipMemsetAsync(cs->i_dstate.p, 0, 8 * (size_t)kIdWords, s));
    const int64_t none = kHole;
    HIPOK(hipMemcpyAsync(&a.words[kIwMaxVer], &none, 8, hipMemcpyHostToDevice, s));
    int64_t words[kIwWords];
    if (int rc = cs->i_span[0].begin(s)) return rc;
    launch_import_overlay(s, a);
    if (to_delta) launch_import_delta_bounds(s, pl.d);
    HIPOK(take_launch_error());
    if (int rc = cs->i_span[0].end(s)) return rc;
    HIPOK(hipMemcpyAsync(words, cs->i_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    if (to_delta) HIPOK(hipMemcpyAsync(pl.dw, cs->i_dstate.p, sizeof(pl.dw), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->i_ms_kernels = cs->i_span[0].ms();
    if ((int32_t)words[kIwError] & 1) return FDBCS_E_INVALID;
    if (words[kIwError]) return FDBCS_E_DEVICE;
    if (has_lo && has_hi && cmp_bytes(lo_key, lo_len, hi_key, hi_len) == 0) {
        *boundaries_out = nb + nd;
        import_note(cs, to_delta ? 1 : 0, nb, nd, nd);
        *done = true;
        return FDBCS_OK;
    }
    pl.m = words[kIwM];
    if (pl.m < (has_lo ? 1 : 0) + (has_hi ? 1 : 0) || pl.m > n + 2) return FDBCS_E_DEVICE;
    return FDBCS_OK;
}

// The end both imports share, once the device scalars hold the new sizes: rebuild the range-max
// levels of the tier that changed (n_new boundaries), read its greatest version off their top and
// raise the set's header and greatest written version.
static int import_finish(fdbcs_conflict_set* cs, const ImportArgs& a, bool delta_tier, int64_t n_new) {
    hipStream_t s = cs->stream;
    Scalars* dsc = (Scalars*)cs->scal.p;
    const MaxLevels lv = delta_tier ? dlevels_of(cs, cs->dcur) : levels_of(cs, cs->cur);
    const int64_t lvl3_n = delta_tier ? cs->dlvl3_n : cs->lvl3_n, lvl2_n = delta_tier ? cs->dlvl2_n : cs->lvl2_n;
    if (int rc = cs->i_span[2].begin(s)) return rc;
    launch_rangemax(s, lv, dsc, delta_tier ? &dsc->ndb[cs->dcur] : &dsc->n, lvl3_n, lvl2_n,
                    std::max<int64_t>(n_new, 1));
    // the top of the rebuilt levels (holes are INT64_MIN), never a pass over the elements
    launch_import_max(s, lv, lvl3_n, &a.words[kIwMaxVer]);
    HIPOK(take_launch_error());
    if (int rc = cs->i_span[2].end(s)) return rc;
    int64_t max_ver;
    HIPOK(hipMemcpyAsync(&max_ver, &a.words[kIwMaxVer], 8, hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->i_ms_kernels += cs->i_span[2].ms();
    cs->header_version = a.new_hdr;
    cs->max_written = std::max({cs->max_written, a.new_hdr, max_ver});
    cs->ddir_epoch[0] = cs->ddir_epoch[1] = 0;  // the delta's directory: not trusted until an epilogue refills it
    cs->prev_segs = false;
    return FDBCS_OK;
}

// Phase 2 of the fold, from a finished phase 1 of either import: merges the three streams into the
// non-current base buffer and tail arena and, on success, switches to them with an empty delta.
static int import_fold(fdbcs_conflict_set* cs, ImportPlan& pl, int64_t* boundaries_out) {
    ImportArgs& a = pl.d.a;
    const int64_t nb = a.nb, nd = a.nd, m = pl.m;
    const int64_t total_ub = nb + nd + a.n + 2;
    const int64_t tail_need = pl.sc.tail_used + 8 * pl.u_end;
    int rc;
    if ((rc = ensure_history(cs, total_ub + 1, tail_need + 1))) return rc;
    if ((rc = import_merged(cs, a, total_ub))) return rc;
    // the scan's granules have a buffer of their own: the words of phase 1 stay where they are
    const size_t gran = 8 * (size_t)scan_granules(total_ub, 2);
    if ((rc = cs->i_gran.ensure(gran))) return rc;
    import_tiers(cs, a, false);
    hipStream_t s = cs->stream;
    HIPOK(hipMemsetAsync(cs->i_gran.p, 0, gran, s));
    if (int rc = cs->i_span[1].begin(s)) return rc;
    HIPOK(hipMemsetAsync(cs->i_mlt.p, 0, 8 * (size_t)(nb + nd + m), s));
    launch_import_fold(s, a, m, (uint64_t*)cs->i_gran.p);
    HIPOK(take_launch_error());
    if (int rc = cs->i_span[1].end(s)) return rc;
    int64_t words[kIwWords];
    HIPOK(hipMemcpyAsync(words, cs->i_state.p, sizeof(words), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->i_ms_kernels += cs->i_span[1].ms();
    if ((int32_t)words[kIwError] & 8) return FDBCS_E_NOMEM;
    if (words[kIwError] || ((const int32_t*)&words[kIwScan])[1]) return FDBCS_E_DEVICE;
    // success: the buffers the fold filled become current, the delta is empty
    const int64_t kept = words[kIwKept], tail_used = 8 * words[kIwTailUnits];
    cs->cur ^= 1;
    cs->tcur ^= 1;
    Scalars ns{};
    ns.n = kept;
    ns.tail_used = tail_used;
    HIPOK(hipMemcpyAsync(cs->scal.p, &ns, sizeof(ns), hipMemcpyHostToDevice, s));
    if ((rc = import_finish(cs, a, false, kept))) return rc;
    cs->n_ub = kept;
    cs->nd_ub = 0;
    cs->tail_ub = tail_used;
    *boundaries_out = kept;
    import_note(cs, 0, kept, nd, 0);
    return FDBCS_OK;
}

// The import that folds into a new base (both of its entry points end here).
static int import_device(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t n, const uint8_t* d_bytes, int64_t nbytes, const int64_t* d_off,
                         const int64_t* d_ver, int64_t ihdr, int64_t* boundaries_out) {
    ImportPlan pl;
    bool done;
    const int rc = import_phase1(cs, lo_key, lo_len, hi_key, hi_len, n, d_bytes, nbytes, d_off, d_ver, ihdr,
                                 boundaries_out, false, pl, &done);
    return rc || done ? rc : import_fold(cs, pl, boundaries_out);
}

// The import into the delta tier (same contract).  After phase 1 the host knows an upper bound of
// the delta afterwards and either goes on (phase 2 writes the non-current delta buffer and arena
// bytes past tail_used, and the host switches to them after reading the result words) or goes on
// with the fold's phase 2 on the overlay it has, which leaves an empty delta.
static int import_delta_device(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                               int32_t hi_len, int64_t n, const uint8_t* d_bytes, int64_t nbytes, const int64_t* d_off,
                               const int64_t* d_ver, int64_t ihdr, int64_t* boundaries_out) {
    ImportPlan pl;
    bool done;
    int rc = import_phase1(cs, lo_key, lo_len, hi_key, hi_len, n, d_bytes, nbytes, d_off, d_ver, ihdr, boundaries_out,
                           true, pl, &done);
    if (rc || done) return rc;
    ImportDeltaArgs& d = pl.d;
    ImportArgs& a = d.a;
    ImportWindow& w = d.w;
    Scalars& sc = pl.sc;
    const int64_t nb = a.nb, nd = a.nd, m = pl.m;
    const int64_t* dw = pl.dw;
    w.p_lo = dw[kIdPlo];
    w.p_hi = dw[kIdPhi];
    w.q_lo = dw[kIdQlo];
    w.q_hi = dw[kIdQhi];
    w.e_ver = dw[kIdEver];
    d.e_skip = dw[kIdEskip] ? 1 : 0;
    if (w.p_lo < 0 || w.p_lo > w.p_hi || w.p_hi > nd || w.q_lo < 0 || w.q_lo > w.q_hi || w.q_hi > nb) return FDBCS_E_DEVICE;
    const int64_t nbr = w.q_hi - w.q_lo;
    w.closing = a.has_hi ? 1 : 0;
    w.mr = m - w.closing;
    w.R = (w.p_hi - w.p_lo) + nbr + w.mr;
    // the delta afterwards holds at most its boundaries outside the range, the range's and the closing one
    const int64_t nd_bound = nd + nbr + m + 2;
    bool fold = nd_bound > delta_limit_for(cs, cs->n_ub);
    if (!fold) {
        rc = ensure_delta(cs, nd_bound);
        if (rc == FDBCS_E_NOMEM)
            fold = true;
        else if (rc)
            return rc;
    }
    // the fold takes every range the delta cannot hold: exact, with an empty delta
    if (fold) return import_fold(cs, pl, boundaries_out);
    if ((rc = ensure_history(cs, cs->hist_cap, 8 * (d.tail_base + pl.u_end) + 1))) return rc;
    const int64_t total = w.R + w.closing;
    const int64_t gran = scan_granules(total, 2);
    if ((rc = import_merged(cs, a, total + 1))) return rc;
    if ((rc = cs->i_dstate.ensure(8 * (size_t)(kIdWords + gran)))) return rc;
    import_tiers(cs, a, true);
    d.dwords = (int64_t*)cs->i_dstate.p;
    hipStream_t s = cs->stream;
    HIPOK(hipMemsetAsync(cs->i_dstate.p, 0, 8 * (size_t)(kIdWords + gran), s));
    if (int rc = cs->i_span[1].begin(s)) return rc;
    HIPOK(hipMemsetAsync(cs->i_mlt.p, 0, 8 * (size_t)(total + 1), s));
    launch_import_delta_merge(s, d, (uint64_t*)cs->i_dstate.p + kIdWords);
    HIPOK(take_launch_error());
    if (int rc = cs->i_span[1].end(s)) return rc;
    HIPOK(hipMemcpyAsync(pl.dw, cs->i_dstate.p, sizeof(pl.dw), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->i_ms_kernels += cs->i_span[1].ms();
    if ((int32_t)dw[kIdError] & 8) return FDBCS_E_NOMEM;
    if (dw[kIdError] || ((const int32_t*)&dw[kIdScan])[1]) return FDBCS_E_DEVICE;
    const int64_t kept = dw[kIdKept], units = dw[kIdTailUnits];
    const int64_t nd_new = w.p_lo + kept + (nd - w.p_hi);
    if (kept < 0 || kept > total || nd_new > cs->delta_cap || units < 0 || units > pl.u_end) return FDBCS_E_DEVICE;
    // success: the delta buffer the kernels filled becomes current, the appended tails count
    const int64_t tail_used = units ? 8 * (d.tail_base + units) : sc.tail_used;
    cs->dcur ^= 1;
    sc.nd = nd_new;
    sc.ndb[cs->dcur] = nd_new;
    sc.tail_used = tail_used;
    HIPOK(hipMemcpyAsync(cs->scal.p, &sc, sizeof(sc), hipMemcpyHostToDevice, s));
    if ((rc = import_finish(cs, a, true, nd_new))) return rc;
    cs->nd_ub = nd_new;  // exact: the next batch's compaction trigger counts the import
    cs->tail_ub = tail_used;
    *boundaries_out = nb + nd_new;
    import_note(cs, 1, nb, nd, nd_new);
    return FDBCS_OK;
}

static int import_arrays(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                         const int64_t* versions, int64_t header_version, int64_t* boundaries_out, bool to_delta) {
    if (!cs || !boundaries_out || n < 0 || (n > 0 && (!key_offsets || !versions))) return FDBCS_E_INVALID;
    if (int rc = import_bounds_ok(lo_key, lo_len, hi_key, hi_len)) return rc;
    const int64_t nbytes = n ? key_offsets[n] : 0;
    if (nbytes < 0 || (nbytes > 0 && !key_bytes)) return FDBCS_E_INVALID;
    if (cs->inflight) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    cs->x_valid = false;
    // the three arrays go up as they are
    int rc;
    if ((rc = cs->i_bytes.ensure((size_t)nbytes + 64))) return rc;
    if ((rc = cs->i_off.ensure(8 * (size_t)(n + 1)))) return rc;
    if ((rc = cs->i_ver.ensure(8 * (size_t)(n + 1)))) return rc;
    hipStream_t s = cs->stream;
    if (nbytes) HIPOK(hipMemcpyAsync(cs->i_bytes.p, key_bytes, (size_t)nbytes, hipMemcpyHostToDevice, s));
    if (n) {
        HIPOK(hipMemcpyAsync(cs->i_off.p, key_offsets, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        HIPOK(hipMemcpyAsync(cs->i_ver.p, versions, 8 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    rc = (to_delta ? import_delta_device : import_device)(
        cs, lo_key, lo_len, hi_key, hi_len, n, (const uint8_t*)cs->i_bytes.p, nbytes, (const int64_t*)cs->i_off.p,
        (const int64_t*)cs->i_ver.p, header_version, boundaries_out);
    cs->i_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

static int import_pending(fdbcs_conflict_set* dst, fdbcs_conflict_set* src, const uint8_t* lo_key, int32_t lo_len,
                          const uint8_t* hi_key, int32_t hi_len, int64_t* boundaries_out, bool to_delta) {
    if (!dst || !src || src == dst || !boundaries_out || src->device != dst->device) return FDBCS_E_INVALID;
    if (int rc = import_bounds_ok(lo_key, lo_len, hi_key, hi_len)) return rc;
    if (dst->inflight || src->inflight || !src->x_valid) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(dst->device));
    if (int rc = sync_all(dst)) return rc;
    dst->x_valid = false;
    // src's export finished on its own stream before fdbcs_history_export returned: its result
    // arrays are read in place, and stay pending
    const int rc = (to_delta ? import_delta_device : import_device)(
        dst, lo_key, lo_len, hi_key, hi_len, src->x_n, (const uint8_t*)src->x_bytes.p, src->x_nbytes,
        (const int64_t*)src->x_off.p, (const int64_t*)src->x_ver.p, src->x_hdr, boundaries_out);
    dst->i_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int fdbcs_history_import(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                         int32_t hi_len, int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                         const int64_t* versions, int64_t header_version, int64_t* boundaries_out) {
    return import_arrays(cs, lo_key, lo_len, hi_key, hi_len, n, key_bytes, key_offsets, versions, header_version,
                         boundaries_out, false);
}

int fdbcs_history_import_pending(fdbcs_conflict_set* dst, fdbcs_conflict_set* src, const uint8_t* lo_key, int32_t lo_len,
                                 const uint8_t* hi_key, int32_t hi_len, int64_t* boundaries_out) {
    return import_pending(dst, src, lo_key, lo_len, hi_key, hi_len, boundaries_out, false);
}

int fdbcs_history_import_delta(fdbcs_conflict_set* cs, const uint8_t* lo_key, int32_t lo_len, const uint8_t* hi_key,
                               int32_t hi_len, int64_t n, const uint8_t* key_bytes, const int64_t* key_offsets,
                               const int64_t* versions, int64_t header_version, int64_t* boundaries_out) {
    return import_arrays(cs, lo_key, lo_len, hi_key, hi_len, n, key_bytes, key_offsets, versions, header_version,
                         boundaries_out, true);
}

int fdbcs_history_import_delta_pending(fdbcs_conflict_set* dst, fdbcs_conflict_set* src, const uint8_t* lo_key,
                                       int32_t lo_len, const uint8_t* hi_key, int32_t hi_len, int64_t* boundaries_out) {
    return import_pending(dst, src, lo_key, lo_len, hi_key, hi_len, boundaries_out, true);
}

int fdbcs_history_import_info(fdbcs_conflict_set* cs, int32_t* path, int64_t* base_boundaries, int64_t* delta_before,
                              int64_t* delta_after) {
    if (!cs || !path || !base_boundaries || !delta_before || !delta_after) return FDBCS_E_INVALID;
    *path = cs->i_path;
    *base_boundaries = cs->i_info_base;
    *delta_before = cs->i_info_before;
    *delta_after = cs->i_info_after;
    return FDBCS_OK;
}

int fdbcs_history_import_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host) {
    if (!cs || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    *ms_kernels = cs->i_ms_kernels;
    *ms_host = cs->i_ms_host;
    return FDBCS_OK;
}

// ---- the resolver's iops sample of a routed batch (Resolver.actor.cpp:178-192)

int fdbcs_batch_set_iops_sample(fdbcs_batch* b, int32_t units, uint64_t seed) {
    if (!b || units < 1) return FDBCS_E_INVALID;
    if (!b->cs || !b->routed || b->dev_added || b->state >= 2) return FDBCS_E_STATE;
    // the scan counts key bytes in 32 bits: every begin key's 16 prefix bytes and the whole tail arena bound them
    const int64_t cap = b->r_cap_ranges, bytes_cap = 16 * cap + b->r_cap_tail;
    if (bytes_cap >= ((int64_t)1 << 32)) return FDBCS_E_NOMEM;
    fdbcs_conflict_set* cs = b->cs;
    HIPOK(hipSetDevice(cs->device));
    BatchSlot* sl = b->slot.get();
    if (sl->is_inflight) {  // a request replaced: its kernel is over before its buffers are touched
        HIPOK(hipEventSynchronize(sl->is_span.e1));
        sl->is_inflight = false;
    }
    b->is_req = b->is_done = false;
    int rc;
    const size_t state_bytes = 8 * (size_t)iops_scan_words(cap);
    if ((rc = sl->is_state.ensure(state_bytes))) return rc;
    if ((rc = sl->is_met.ensure(4 * (size_t)(cap + 1)))) return rc;
    if ((rc = sl->is_idx.ensure(4 * (size_t)(cap + 1)))) return rc;
    if ((rc = sl->is_off.ensure(8 * (size_t)(cap + 1)))) return rc;
    if ((rc = sl->is_bytes.ensure((size_t)bytes_cap + 64))) return rc;
    if ((rc = sl->is_tot.ensure(sizeof(IopsTotals), true))) return rc;
    IopsArgs a{};
    a.keys = b->bd.keys;
    a.tail = b->bd.tail;
    a.dres = (const RouteResult*)sl->rt_dres.p;
    a.units = (uint32_t)units;
    a.seed = seed;
    a.cap = cap;
    a.bytes_cap = bytes_cap;
    a.metrics = (int32_t*)sl->is_met.p;
    a.index = (int32_t*)sl->is_idx.p;
    a.key_offsets = (int64_t*)sl->is_off.p;
    a.bytes = (uint8_t*)sl->is_bytes.p;
    a.totals = (IopsTotals*)sl->is_tot.dp;
    ((IopsTotals*)sl->is_tot.p)->n = -1;  // not written yet
    // behind the routing kernels and the ev_up record on their stream: the detect pipeline waits
    // for ev_up only, so it never waits for the sample
    hipStream_t us = cs->ustream;
    HIPOK(hipMemsetAsync(sl->is_state.p, 0, state_bytes, us));
    uint64_t* sw = (uint64_t*)sl->is_state.p;
    ScanState st{sw + 8, (int*)sw, (int*)(sw + 1)};
    t_record = nullptr;
    if (int rc = sl->is_span.begin(us)) return rc;
    launch_iops_sample(us, a, st);
    HIPOK(take_launch_error());
    if (int rc = sl->is_span.end(us)) return rc;
    sl->is_inflight = true;
    b->is_req = true;
    return FDBCS_OK;
}

int fdbcs_batch_iops_sample(fdbcs_batch* b, int64_t* n_out, int64_t* key_bytes_out) {
    if (!b || !n_out || !key_bytes_out) return FDBCS_E_INVALID;
    if (!b->cs) return FDBCS_E_STATE;
    HIPOK(hipSetDevice(b->cs->device));
    if (int rc = finish_route(b)) return rc;  // the routing's error first (the request went with the batch)
    if (!b->is_req) return FDBCS_E_STATE;
    BatchSlot* sl = b->slot.get();
    if (!b->is_done) {
        HIPOK(hipEventSynchronize(sl->is_span.e1));
        sl->is_inflight = false;
        std::atomic_thread_fence(std::memory_order_acquire);
        IopsTotals t;
        memcpy(&t, (const void*)sl->is_tot.p, sizeof(t));
        int32_t words[4];  // the scan's counter and error words
        HIPOK(hipMemcpy(words, sl->is_state.p, sizeof(words), hipMemcpyDeviceToHost));
        if (words[2] || t.n < 0) return FDBCS_E_DEVICE;  // look-back bound, key buffer
        b->is_n = t.n;
        b->is_nbytes = t.key_bytes;
        b->is_ms = sl->is_span.ms();
        b->is_done = true;
    }
    *n_out = b->is_n;
    *key_bytes_out = b->is_nbytes;
    return FDBCS_OK;
}

int fdbcs_batch_iops_sample_read(fdbcs_batch* b, uint8_t* key_bytes, int64_t key_bytes_cap, int64_t* key_offsets,
                                 int32_t* metrics, int32_t* index, int64_t cap) {
    if (!b || key_bytes_cap < 0 || cap < 0 || !key_offsets) return FDBCS_E_INVALID;
    if (!b->cs || !b->is_req || !b->is_done) return FDBCS_E_STATE;
    if (cap < b->is_n || key_bytes_cap < b->is_nbytes) return FDBCS_E_NOMEM;
    if ((b->is_n && !metrics) || (b->is_nbytes && !key_bytes)) return FDBCS_E_INVALID;
    HIPOK(hipSetDevice(b->cs->device));
    const BatchSlot* sl = b->slot.get();
    if (b->is_n && index) HIPOK(hipMemcpy(index, sl->is_idx.p, 4 * (size_t)b->is_n, hipMemcpyDeviceToHost));
    return copy_keyed_result(b->is_n, b->is_nbytes, metrics, sl->is_met.p, 4, key_offsets, sl->is_off.p, key_bytes,
                             sl->is_bytes.p);
}

int fdbcs_batch_iops_sample_timing(fdbcs_batch* b, double* ms_kernels) {
    if (!b || !ms_kernels) return FDBCS_E_INVALID;
    if (!b->is_req || !b->is_done) return FDBCS_E_STATE;
    *ms_kernels = b->is_ms;
    return FDBCS_OK;
}

// ---- the version each read of a batch is checked against

// Either form of the query: the host form writes the set's own buffer and copies it out, the device
// form writes the caller's memory.  The batch ends as an uploaded, undetected batch; neither the
// set, its batch workspaces nor a pending export is touched.
static int read_versions(fdbcs_batch* b, int64_t floor_version, int64_t* out, int64_t cap, bool device_form) {
    if (!b) return FDBCS_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    fdbcs_conflict_set* cs = b->cs;
    if (!cs) return FDBCS_E_STATE;
    if (b->share_packed || (b->routed && !b->dev_added) || b->state > 1) return FDBCS_E_STATE;
    if (cs->inflight) return FDBCS_E_STATE;
    HIPOK(hipSetDevice(cs->device));
    // a device-added batch: its add kernels first (a malformed one is FDBCS_E_INVALID and empty again)
    if (int rc = finish_route(b)) return rc;
    const int64_t R = b->R();
    if (R == 0) return FDBCS_OK;
    if (!out) return FDBCS_E_INVALID;
    if (cap < R) return FDBCS_E_NOMEM;
    if (b->state == 0)
        if (int rc = fdbcs_batch_upload(b)) return rc;
    if (int rc = sync_all(cs)) return rc;  // the upload too
    if (cs->rv_err.ensure(sizeof(int))) return FDBCS_E_NOMEM;
    if (!device_form && cs->rv_out.ensure(8 * (size_t)R)) return FDBCS_E_NOMEM;
    Scalars* sc = (Scalars*)cs->scal.p;
    ReadVersionsArgs a{};
    a.b = b->bd;
    a.base = Tier{hist_of(cs, cs->cur), levels_of(cs, cs->cur), &sc->n, cs->header_version};
    a.delta = Tier{delta_of(cs, cs->dcur), dlevels_of(cs, cs->dcur), &sc->ndb[cs->dcur], kHole};
    a.htail = (const uint8_t*)cs->htail[cs->tcur].p;
    a.floor = floor_version;
    a.out = device_form ? out : (int64_t*)cs->rv_out.p;
    a.error = (int*)cs->rv_err.p;
    hipStream_t s = cs->stream;
    t_record = nullptr;
    HIPOK(hipMemsetAsync(cs->rv_err.p, 0, sizeof(int), s));
    if (int rc = cs->rv_span.begin(s)) return rc;
    // the long-key form by the read check's rule (engine.cpp plan_layout)
    const void* func = launch_read_versions(s, a, b->max_len > 24);
    HIPOK(take_launch_error());
    if (int rc = cs->rv_span.end(s)) return rc;
    int err = 0;
    HIPOK(hipMemcpyAsync(&err, cs->rv_err.p, sizeof(err), hipMemcpyDeviceToHost, s));
    if (!device_form) HIPOK(hipMemcpyAsync(out, cs->rv_out.p, 8 * (size_t)R, hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->rv_ms_kernels = cs->rv_span.ms();
    // which instantiation ran, as fdbcs_kernel_profile reports the pipeline's kernels
    auto it = std::find_if(cs->kprof.begin(), cs->kprof.end(), [&](const auto& k) { return k.func == func; });
    if (it == cs->kprof.end()) it = cs->kprof.insert(cs->kprof.end(), {func, 0, 0.0});
    it->launches += 1;
    it->ms += cs->rv_ms_kernels;
    cs->rv_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return err ? FDBCS_E_DEVICE : FDBCS_OK;  // a lookup left its tier: the tiers are inconsistent
}

int fdbcs_batch_read_versions(fdbcs_batch* b, int64_t floor_version, int64_t* versions_out, int64_t cap) {
    return read_versions(b, floor_version, versions_out, cap, false);
}

int fdbcs_batch_read_versions_device(fdbcs_batch* b, int64_t floor_version, int64_t* dev_out, int64_t cap) {
    return read_versions(b, floor_version, dev_out, cap, true);
}

int fdbcs_batch_read_versions_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host) {
    if (!b || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    if (!b->cs) return FDBCS_E_STATE;
    *ms_kernels = b->cs->rv_ms_kernels;
    *ms_host = b->cs->rv_ms_host;
    return FDBCS_OK;
}

}  // extern "C"
