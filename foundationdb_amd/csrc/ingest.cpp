// ingest.cpp — the device-add entry points of the C-ABI (include/fdb_conflict_set.h): a whole batch
// in the plain fdbcs_packed_batch form, already in device memory, added without the host reading any
// of it.  The call sizes the batch's slot from the sizes it is given, enqueues the kernels of
// ingest.hip on the stream the routing kernels use (off the detect pipeline's chains) and returns;
// the batch then is what a routed batch is to the detect steps (engine.cpp), told apart by
// fdbcs_batch::dev_added.
#include "engine_impl.h"
#include "ingest.h"

// Wait for the add kernels and take their totals (finish_route's sibling).  On an error the batch
// is empty again: whatever the kernels placed is in the slot's own buffers, and the set was never
// touched.
int fdbcs::impl::finish_device_add(fdbcs_batch* b) {
    if (!b->route_pending) return FDBCS_OK;
    BatchSlot* sl = b->slot;
    HIPOK(hipEventSynchronize(sl->ev_up));
    std::atomic_thread_fence(std::memory_order_acquire);
    IngestResult r;
    memcpy(&r, (const void*)sl->da_res.p, sizeof(r));
    b->da_ms_kernels = ev_ms(sl->ev_da0, sl->ev_da1);
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

extern "C" {

int fdbcs_batch_add_packed_device(fdbcs_batch* b, const fdbcs_packed_batch_dev* pb, const uint32_t* ready_flag,
                                  uint32_t ready_value) {
    const auto t_host = std::chrono::steady_clock::now();
    if (!b || !pb || pb->n_txn < 0 || pb->n_reads < 0 || pb->n_writes < 0 || pb->key_bytes_len < 0)
        return FDBCS_E_INVALID;
    if (!b->cs || b->state != 0 || b->T() != 0 || b->direct || b->routed) return FDBCS_E_STATE;
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
    BatchSlot* sl = b->slot;
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
    if (!sl->ev_da0) HIPOK(hipEventCreate(&sl->ev_da0));
    if (!sl->ev_da1) HIPOK(hipEventCreate(&sl->ev_da1));
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
    HIPOK(hipEventRecord(sl->ev_da0, us));
    launch_ingest(us, a, st);
    HIPOK(take_launch_error());
    HIPOK(hipEventRecord(sl->ev_da1, us));
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
