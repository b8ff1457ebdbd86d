// verify.cpp — fdbcs_history_verify of the C-ABI (include/fdb_conflict_set.h has the definition):
// the host side of the stored-state check.  It works on an idle set through the state and helpers
// of engine_impl.h, reads the sizes, clamps them to what the set allocated, validates the override
// against them and launches the kernels of verify.hip; nothing of the set is written.
#include "engine_impl.h"
#include "verify.h"

static_assert(FDBCS_VERIFY_CLASSES == kVcCount, "the public class count is the kernels'");
static_assert(FDBCS_VERIFY_EDIR == 1 << kVcEdir && FDBCS_VERIFY_DOMINANCE == 1 << kVcDominance, "class bits");
static_assert(FDBCS_VERIFY_OV_TAIL_WORD == kVwTailWord && FDBCS_VERIFY_OV_LVL1 == kVwLvl1, "override names");
static_assert(sizeof(fdbcs_verify_report) == 600 && sizeof(fdbcs_verify_override) == 40, "public layouts");

// Elements of the array an override names, in the set as it stands (0: the array does not exist).
static int64_t override_elements(const VerifyArgs& a, const fdbcs_verify_override& o) {
    if (o.what == kVwTailWord) return a.tail_used / 8;
    if (o.tier < 0 || o.tier > 1) return 0;
    const VerifyTier& t = a.t[o.tier];
    const int64_t n = t.n;
    auto per = [&](int64_t span) { return (n + span - 1) / span; };
    switch (o.what) {
        case kVwKey:
        case kVwLenTail:
        case kVwVersion: return n;
        case kVwLvl1: return per(kFan);
        case kVwLvl2: return per((int64_t)kFan * kFan);
        case kVwLvl3: return per((int64_t)kFan * kFan * kFan) * kL3Rep;
        case kVwSkey8: return per(8);
        case kVwSkey: {
            if (o.level < 0 || o.level >= kIdxLevels) return 0;
            int64_t span = kFan;  // at most 64 * 8^11: a level above the tier's size has entry 0 alone
            for (int L = 0; L < o.level; L++) span *= kArity;
            return per(span);
        }
        case kVwDir: return o.tier == 0 && t.has_dir ? (int64_t)t.m.dir_top + 2 : 0;
        case kVwEdir: return o.tier == 1 && t.has_edir ? (int64_t)t.m.dir_top + 2 : 0;
    }
    return 0;
}

extern "C" {

int fdbcs_history_verify(fdbcs_conflict_set* cs, uint32_t checks, const fdbcs_verify_override* ov,
                         fdbcs_verify_report* out) {
    if (!cs || !out) return FDBCS_E_INVALID;
    if (checks >> kVcCount) return FDBCS_E_INVALID;
    if (ov && (ov->what < kVwKey || ov->what >= kVwCount)) return FDBCS_E_INVALID;
    if (cs->inflight) return FDBCS_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    HIPOK(hipSetDevice(cs->device));
    if (int rc = sync_all(cs)) return rc;
    Scalars sc;
    HIPOK(hipMemcpy(&sc, cs->scal.p, sizeof(sc), hipMemcpyDeviceToHost));
    auto clamp = [](int64_t x, int64_t cap) { return std::min(std::max<int64_t>(x, 0), std::max<int64_t>(cap, 0)); };
    VerifyArgs a{};
    a.t[0].h = hist_of(cs, cs->cur);
    a.t[0].m = levels_of(cs, cs->cur);
    a.t[0].n = clamp(sc.n, cs->hist_cap);
    a.t[0].has_dir = a.t[0].m.dir != nullptr;
    a.t[1].h = delta_of(cs, cs->dcur);
    a.t[1].m = dlevels_of(cs, cs->dcur);
    a.t[1].n = clamp(sc.ndb[cs->dcur], cs->delta_cap);
    a.t[1].has_edir = a.t[1].m.edir != nullptr;
    for (VerifyTier& t : a.t)  // the slots a directory holds: never past what was allocated
        if ((int64_t)t.m.dir_top + 2 > kDirAlloc) t.has_dir = t.has_edir = 0;
    a.tail = (const uint64_t*)cs->htail[cs->tcur].p;
    a.tail_used = a.tail ? clamp(sc.tail_used, cs->tail_cap) : 0;
    a.hdr = cs->header_version;
    a.checks = checks ? checks : (1u << kVcCount) - 1u;
    if (ov) {
        a.ov = VerifyOv{ov->what, ov->tier, ov->level, 0, ov->index, ov->xor_lo, ov->xor_hi};
        if (ov->index < 0 || ov->index >= override_elements(a, *ov)) return FDBCS_E_INVALID;
    }
    // the words, then one true maximum per level-3 entry of each tier
    const int64_t span3 = (int64_t)kFan * kFan * kFan;
    const int64_t n3 = (a.t[0].n + span3 - 1) / span3 + (a.t[1].n + span3 - 1) / span3;
    if (int rc = cs->v_state.ensure(8 * (size_t)(kVfWords + n3))) return rc;
    a.words = (unsigned long long*)cs->v_state.p;
    hipStream_t s = cs->stream;
    HIPOK(hipMemsetAsync(a.words, 0, 8 * (size_t)kVfCounts, s));
    HIPOK(hipMemsetAsync(a.words + kVfCounts, 0xff, 8 * (size_t)kVfFirsts, s));
    if (n3) HIPOK(hipMemsetAsync(a.words + kVfWords, 0, 8 * (size_t)n3, s));
    if (int rc = cs->v_span.begin(s)) return rc;
    launch_verify(s, a);
    HIPOK(take_launch_error());
    if (int rc = cs->v_span.end(s)) return rc;
    unsigned long long w[kVfWords];
    HIPOK(hipMemcpyAsync(w, a.words, sizeof(w), hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    cs->v_ms_kernels = cs->v_span.ms();
    *out = fdbcs_verify_report{};
    out->tier[0].n = sc.n;
    out->tier[1].n = sc.ndb[cs->dcur];
    for (int t = 0; t < 2; t++)
        for (int c = 0; c < kVcCount; c++) {
            fdbcs_verify_class& r = out->tier[t].cls[c];
            r.examined = (int64_t)w[vf_count(t, c, 0)];
            r.violations = (int64_t)w[vf_count(t, c, 1)];
            r.first = r.violations ? (int64_t)w[vf_first(t, c)] : -1;
        }
    out->edir_trusted = (int64_t)w[kVfTrusted];
    cs->v_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FDBCS_OK;
}

int fdbcs_history_verify_timing(fdbcs_conflict_set* cs, double* ms_kernels, double* ms_host) {
    if (!cs || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    *ms_kernels = cs->v_ms_kernels;
    *ms_host = cs->v_ms_host;
    return FDBCS_OK;
}

int fdbcs_history_verify_sizes(int64_t* report_bytes, int64_t* override_bytes) {
    if (!report_bytes || !override_bytes) return FDBCS_E_INVALID;
    *report_bytes = (int64_t)sizeof(fdbcs_verify_report);
    *override_bytes = (int64_t)sizeof(fdbcs_verify_override);
    return FDBCS_OK;
}

}  // extern "C"
