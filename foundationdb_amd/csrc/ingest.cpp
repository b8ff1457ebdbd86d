// ingest.cpp — the device-add entry points of the C-ABI (include/fdb_conflict_set.h): a whole batch
// in the plain fdbcs_packed_batch form, already in device memory, added without the host reading any
// of it.  The call sizes the batch's slot from the sizes it is given, enqueues the kernels of
// ingest.hip on the stream the routing kernels use (off the detect pipeline's chains) and returns;
// the batch then is what a routed batch is to the detect steps (engine.cpp), told apart by
// fdbcs_batch::dev_added.  fdbcs_batch_share_pack_device takes the same arrays through the same
// checks and writes them as the proxy share fdbcs_share_pack would (engine.h ShareHeader) into the
// caller's device buffer; the batch stays empty.
#include "engine_impl.h"
#include "ingest.h"

// Wait for the add kernels and take their totals (finish_route's sibling).  On an error the batch
// is empty again: whatever the kernels placed is in the slot's own buffers, and the set was never
// touched.
int fdbcs::impl::finish_device_add(fdbcs_batch* b) {
    if (!b->route_pending) return FDBCS_OK;
    BatchSlot* sl = b->slot.get();
    HIPOK(hipEventSynchronize(sl->ev_up));
    std::atomic_thread_fence(std::memory_order_acquire);
    IngestResult r;
    memcpy(&r, (const void*)sl->da_res.p, sizeof(r));
    b->da_ms_kernels = sl->da_span.ms();
    if (r.error != 0) {
        // 1: the arrays break the layout or hold an inverted range; 2: the ready flag was never set;
        // 4: the scan's look-back gave up
        if (r.error == 2) fprintf(stderr, "fdbcs: device-added batch: the arrays' ready flag was never set\n");
        b->routed = b->dev_added = b->route_pending = false;
        b->rT = b->rR = b->rW = 0;
        b->r_tail = 0;
        b->out_dev = nullptr;
        b->out_n = 0;
        b->out_ids.clear();
        b->state = 0;
        return r.error == 1 ? FDBCS_E_INVALID : r.error == 2 ? FDBCS_E_TIMEOUT : FDBCS_E_DEVICE;
    }
    b->r_tail = (size_t)r.tail_bytes;
    b->tail_bytes = b->r_tail;
    b->bd.tail_n = r.tail_bytes;
    // history tail bytes the batch's write endpoints can add: every tail is already padded to 8
    b->wtail = r.tail_bytes;
    b->max_len = r.n_gt24 ? 25 : (r.n_gt19 ? 20 : 16);
    b->any_report = r.reports > 0;
    b->route_pending = false;
    return FDBCS_OK;
}

// Wait for the pack kernels and take their outcome.  The batch was empty and stays so; on an error
// the kernels left the empty share in the caller's buffer.
int fdbcs::impl::finish_share_pack(fdbcs_batch* b) {
    if (!b->sp_pending) return b->sp_rc;
    BatchSlot* sl = b->slot.get();
    b->sp_pending = false;
    b->sp_rc = FDBCS_E_DEVICE;
    HIPOK(hipEventSynchronize(sl->da_span.e1));
    std::atomic_thread_fence(std::memory_order_acquire);
    ShareResult r;
    memcpy(&r, (const void*)sl->da_res.p, sizeof(r));
    b->sp_ms_kernels = sl->da_span.ms();
    b->sp_bytes = r.bytes;
    b->sp_tail = r.tail_bytes;
    if (r.error != 0) {
        // 1: the arrays break the layout or hold an inverted range; 2: the ready flag was never set;
        // 3: the share with its tails passes cap; 4 (or a block never written): the scan gave up
        if (r.error == 2) fprintf(stderr, "fdbcs: share pack: the arrays' ready flag was never set\n");
        b->sp_T = b->sp_R = b->sp_W = 0;
        b->sp_rc = r.error == 1 ? FDBCS_E_INVALID : r.error == 2 ? FDBCS_E_TIMEOUT : r.error == 3 ? FDBCS_E_NOMEM : FDBCS_E_DEVICE;
        return b->sp_rc;
    }
    b->sp_rc = FDBCS_OK;
    return FDBCS_OK;
}

extern "C" {

int fdbcs_share_bytes_bound(int32_t n_txn, int32_t n_reads, int32_t n_writes, int64_t key_bytes_len, int64_t* bytes) {
    if (!bytes || n_txn < 0 || n_reads < 0 || n_writes < 0 || key_bytes_len < 0) return FDBCS_E_INVALID;
    ShareHeader h{};
    *bytes = (int64_t)share_layout(n_txn, n_reads, n_writes, key_bytes_len, &h);
    return FDBCS_OK;
}

int fdbcs_batch_share_pack_device(fdbcs_batch* b, const fdbcs_packed_batch_dev* pb, void* out_dev, int64_t cap,
                                  const uint32_t* ready_flag, uint32_t ready_value) {
    const auto t_host = std::chrono::steady_clock::now();
    if (!b || !pb || pb->n_txn < 0 || pb->n_reads < 0 || pb->n_writes < 0 || pb->key_bytes_len < 0 || cap < 0)
        return FDBCS_E_INVALID;
    if (!b->cs || b->state != 0 || b->T() != 0 || b->direct || b->routed || b->sp_pending) return FDBCS_E_STATE;
    // the empty share reads no array: its sizes are all zero
    const int32_t T = pb->n_txn, R = T ? pb->n_reads : 0, W = T ? pb->n_writes : 0;
    const int64_t nbytes = T ? pb->key_bytes_len : 0;
    const int64_t nk = 2 * ((int64_t)R + W);
    if (T && (!pb->read_snapshot || !pb->read_offsets || !pb->write_offsets || (nk && !pb->key_offsets) ||
              (nk && nbytes && !pb->key_bytes)))
        return FDBCS_E_INVALID;
    if ((int64_t)T > kMaxTxnLds) return FDBCS_E_INVALID;
    if (!out_dev || ((uintptr_t)out_dev & 63)) return FDBCS_E_INVALID;
    // tail offsets and the scan's sums are 32-bit; a range id takes 29 bits of a sort item
    if (nbytes >= ((int64_t)1 << 32) || (int64_t)R + W >= ((int64_t)1 << 28)) return FDBCS_E_NOMEM;
    ShareHeader hdr{}, empty{};
    // every region but the tail's end is placed by T, R and W alone
    if (cap < (int64_t)share_layout(T, R, W, 0, &hdr)) return FDBCS_E_NOMEM;
    // the empty share's header, for an error (its 320 bytes, kShareEmptyBytes, are a constant of the
    // layout that tests/test_share_pack_device_abi.py pins)
    share_layout(0, 0, 0, 0, &empty);
    fdbcs_conflict_set* cs = b->cs;
    HIPOK(hipSetDevice(cs->device));
    BatchSlot* sl = b->slot.get();
    int rc;
    const int64_t n_elems = ingest_elems(T, nk);
    const size_t scan_bytes = align_up(8 * (size_t)share_scan_words(n_elems), 16);
    if ((rc = sl->da_scan.ensure(scan_bytes))) return rc;
    if ((rc = sl->da_dres.ensure(sizeof(ShareResult)))) return rc;
    if ((rc = sl->da_res.ensure(sizeof(ShareResult), true))) return rc;
    if ((rc = sl->sp_toff.ensure(4 * (size_t)std::max<int64_t>(nk, 1)))) return rc;
    ShareArgs a{};
    a.in.T = T;
    a.in.R = R;
    a.in.W = W;
    a.in.nk = nk;
    a.in.nbytes = nbytes;
    a.in.snap = pb->read_snapshot;
    a.in.report = pb->report_conflicting_keys;
    a.in.roff = pb->read_offsets;
    a.in.woff = pb->write_offsets;
    a.in.kbytes = pb->key_bytes;
    a.in.koff = pb->key_offsets;
    a.in.ready = ready_flag;
    a.in.ready_value = ready_value;
    a.in.wait_ticks = (uint64_t)cs->route_timeout_ms * 100000ull;  // 100 MHz wall clock
    uint64_t* sw = (uint64_t*)sl->da_scan.p;
    a.in.wait_err = (uint32_t*)(sw + 2);
    a.out = (uint8_t*)out_dev;
    a.cap = cap;
    static_assert(sizeof(a.hdr) == sizeof(ShareHeader) && sizeof(a.empty) == sizeof(ShareHeader), "header words");
    memcpy(a.hdr, &hdr, sizeof(hdr));
    memcpy(a.empty, &empty, sizeof(empty));
    a.toff = (uint32_t*)sl->sp_toff.p;
    a.res = (ShareResult*)sl->da_res.dp;
    a.dres = (ShareResult*)sl->da_dres.p;
    ((ShareResult*)sl->da_res.p)->error = -1;  // not written yet
    // the stream of the routing kernels: a routed add of the same handle runs behind the pack
    hipStream_t us = cs->ustream;
    HIPOK(hipMemsetAsync(sl->da_scan.p, 0, scan_bytes, us));
    ScanState st{sw + 8, (int*)sw, (int*)(sw + 1)};
    t_record = nullptr;
    if (int rc = sl->da_span.begin(us)) return rc;
    launch_share_pack(us, a, st);
    HIPOK(take_launch_error());
    if (int rc = sl->da_span.end(us)) return rc;
    b->share_packed = b->sp_pending = true;
    b->sp_rc = FDBCS_OK;
    b->sp_T = T;
    b->sp_R = R;
    b->sp_W = W;
    b->sp_bytes = b->sp_tail = 0;
    b->sp_ms_kernels = 0;
    b->sp_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    return FDBCS_OK;
}

int fdbcs_batch_share_pack_info(fdbcs_batch* b, int64_t* bytes, int32_t* n_txn, int32_t* n_reads, int32_t* n_writes,
                                int64_t* tail_bytes) {
    if (!b) return FDBCS_E_INVALID;
    if (!b->cs || !b->share_packed) return FDBCS_E_STATE;
    HIPOK(hipSetDevice(b->cs->device));
    if (int rc = finish_share_pack(b)) return rc;
    if (bytes) *bytes = b->sp_bytes;
    if (n_txn) *n_txn = b->sp_T;
    if (n_reads) *n_reads = b->sp_R;
    if (n_writes) *n_writes = b->sp_W;
    if (tail_bytes) *tail_bytes = b->sp_tail;
    return FDBCS_OK;
}

int fdbcs_batch_share_pack_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host) {
    if (!b || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    if (!b->share_packed || b->sp_pending) return FDBCS_E_STATE;
    *ms_kernels = b->sp_ms_kernels;
    *ms_host = b->sp_ms_host;
    return FDBCS_OK;
}

int fdbcs_batch_add_packed_device(fdbcs_batch* b, const fdbcs_packed_batch_dev* pb, const uint32_t* ready_flag,
                                  uint32_t ready_value) {
    const auto t_host = std::chrono::steady_clock::now();
    if (!b || !pb || pb->n_txn < 0 || pb->n_reads < 0 || pb->n_writes < 0 || pb->key_bytes_len < 0)
        return FDBCS_E_INVALID;
    if (!b->cs || b->state != 0 || b->T() != 0 || b->direct || b->routed || b->share_packed) return FDBCS_E_STATE;
    const int32_t T = pb->n_txn, R = pb->n_reads, W = pb->n_writes;
    if (T == 0) return FDBCS_OK;
    const int64_t nk = 2 * ((int64_t)R + W);
    if (!pb->read_snapshot || !pb->read_offsets || !pb->write_offsets || (nk && !pb->key_offsets) ||
        (nk && pb->key_bytes_len && !pb->key_bytes))
        return FDBCS_E_INVALID;
    if ((int64_t)T > kMaxTxnLds) return FDBCS_E_INVALID;
    // tail offsets and the scan's sums are 32-bit; a range id takes 29 bits of a sort item
    if (pb->key_bytes_len >= ((int64_t)1 << 32) || (int64_t)R + W >= ((int64_t)1 << 28)) return FDBCS_E_NOMEM;
    fdbcs_conflict_set* cs = b->cs;
    HIPOK(hipSetDevice(cs->device));
    BatchSlot* sl = b->slot.get();
    int rc;
    // a key's tail, padded to 8, is shorter than the key: the arena's size bounds the tail region
    const UploadLayout L = upload_layout((size_t)T, (size_t)R, (size_t)W, (size_t)pb->key_bytes_len);
    if ((rc = ensure_slot(sl, L.total, (size_t)T, (size_t)R))) return rc;
    const int64_t n_elems = ingest_elems(T, nk);
    const size_t scan_bytes = align_up(8 * (size_t)ingest_scan_words(n_elems), 16);  // (a fill of whole 16-byte units)
    if ((rc = sl->da_scan.ensure(scan_bytes))) return rc;
    if ((rc = sl->da_dres.ensure(sizeof(IngestResult)))) return rc;
    if ((rc = sl->da_res.ensure(sizeof(IngestResult), true))) return rc;
    if ((rc = make_slot_events(sl))) return rc;
    char* d = (char*)sl->dev.p;
    IngestArgs a{};
    a.T = T;
    a.R = R;
    a.W = W;
    a.report_enabled = b->report_enabled ? 1 : 0;
    a.nk = nk;
    a.nbytes = pb->key_bytes_len;
    a.snap = pb->read_snapshot;
    a.report = pb->report_conflicting_keys;
    a.roff = pb->read_offsets;
    a.woff = pb->write_offsets;
    a.kbytes = pb->key_bytes;
    a.koff = pb->key_offsets;
    a.keys = (DKey*)(d + L.keys);
    a.rown = (int32_t*)(d + L.rown);
    a.wown = (int32_t*)(d + L.wown);
    a.osnap = (int64_t*)(d + L.snap);
    a.oroff = (int32_t*)(d + L.roff);
    a.owoff = (int32_t*)(d + L.woff);
    a.flags = (uint8_t*)(d + L.flags);
    a.tail = (uint8_t*)(d + L.tail);
    a.res = (IngestResult*)sl->da_res.dp;
    a.dres = (IngestResult*)sl->da_dres.p;
    ((IngestResult*)sl->da_res.p)->error = -1;  // not written yet
    a.ready = ready_flag;
    a.ready_value = ready_value;
    a.wait_ticks = (uint64_t)cs->route_timeout_ms * 100000ull;  // 100 MHz wall clock
    uint64_t* sw = (uint64_t*)sl->da_scan.p;
    a.wait_err = (uint32_t*)(sw + 2);
    // the stream of the routing kernels and the uploads: the detect pipeline waits for ev_up only
    hipStream_t us = cs->ustream;
    HIPOK(hipMemsetAsync(sl->da_scan.p, 0, scan_bytes, us));
    ScanState st{sw + 8, (int*)sw, (int*)(sw + 1)};
    t_record = nullptr;
    if (int rc = sl->da_span.begin(us)) return rc;
    launch_ingest(us, a, st);
    HIPOK(take_launch_error());
    if (int rc = sl->da_span.end(us)) return rc;
    HIPOK(hipEventRecord(sl->ev_up, us));
    b->bd.T = T;
    b->bd.R = R;
    b->bd.W = W;
    b->bd.keys = a.keys;
    b->bd.rowner = a.rown;
    b->bd.wowner = a.wown;
    b->bd.snap = a.osnap;
    b->bd.roff = a.oroff;
    b->bd.woff = a.owoff;
    b->bd.flags = a.flags;
    b->bd.tail = a.tail;
    b->bd.tail_n = 0;
    b->routed = b->dev_added = true;
    b->route_pending = true;
    b->rT = T;
    b->rR = R;
    b->rW = W;
    b->r_tail = 0;
    b->r_global_R = 0;
    b->r_cap_ranges = b->r_cap_tail = 0;
    b->is_req = b->is_done = false;
    b->rep_dev = nullptr;
    b->rep_n = 0;
    b->state = 1;
    b->da_ms_kernels = 0;
    b->da_ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    return FDBCS_OK;
}

int fdbcs_batch_device_add_info(fdbcs_batch* b, int32_t* n_txn, int32_t* n_reads, int32_t* n_writes,
                                int64_t* tail_bytes) {
    if (!b) return FDBCS_E_INVALID;
    if (!b->cs || !b->dev_added) return FDBCS_E_STATE;
    HIPOK(hipSetDevice(b->cs->device));
    if (int rc = finish_device_add(b)) return rc;
    if (n_txn) *n_txn = b->rT;
    if (n_reads) *n_reads = b->rR;
    if (n_writes) *n_writes = b->rW;
    if (tail_bytes) *tail_bytes = (int64_t)b->r_tail;
    return FDBCS_OK;
}

int fdbcs_batch_device_add_timing(fdbcs_batch* b, double* ms_kernels, double* ms_host) {
    if (!b || !ms_kernels || !ms_host) return FDBCS_E_INVALID;
    if (!b->dev_added || b->route_pending) return FDBCS_E_STATE;
    *ms_kernels = b->da_ms_kernels;
    *ms_host = b->da_ms_host;
    return FDBCS_OK;
}

}  // extern "C"
