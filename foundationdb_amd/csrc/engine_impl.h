// engine_impl.h — the host engine's state, shared by engine.cpp (the detect pipeline and the C-ABI's
// lifecycle calls), transfer.cpp (history export and import, the iops sample) and ingest.cpp (whole
// batches added from device memory): the owner types of its buffers, events and streams and their
// live counts, the definitions of the conflict set, the batch and its staging slot, and the helpers of
// engine.cpp that the maintenance entry points call.  Internal: nothing outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <cxxabi.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/fdb_conflict_set.h"
#include "engine.h"

using namespace fdbcs;

#define HIPOK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            fprintf(stderr, "fdbcs: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, \
                    __LINE__);                                                                        \
            return FDBCS_E_DEVICE;                                                                    \
        }                                                                                             \
    } while (0)

namespace fdbcs::impl {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr int64_t kTailSlack = 64;  // bytes past a tail arena's capacity (dkey.h tail_word reads aligned words)
// History tails are 8-byte aligned and addressed in 8-byte units by the uint32 Hist::lt.y: the
// arena holds up to 32 GiB of tail bytes per conflict set (detect refuses a batch past that).
constexpr int64_t kTailLimit = (int64_t)8 << 32;
constexpr int64_t kTailReclaimDefault = kTailLimit / 2;  // force the GC repack past half of that

// Owners of the engine's device resources.  Each frees what it holds when it dies and can be moved
// but not copied, so a buffer, event or stream that is a member of the set or of a slot needs no
// line anywhere else.  The live_* counts (fdbcs_debug_live_resources) go up where the runtime
// handed a resource out and down where it took one back, nowhere else.
inline std::atomic<int64_t> live_device_buffers{0}, live_host_buffers{0}, live_events{0}, live_streams{0};

// Grow-only device allocation.
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DBuf& operator=(DBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return FDBCS_OK;
        size_t want = std::max(bytes, cap + cap / 2);
        want = align_up(want < 256 ? 256 : want, 256);
        if (p) {
            HIPOK(hipFree(p));
            live_device_buffers--;
        }
        p = nullptr;
        cap = 0;
        HIPOK(hipMalloc(&p, want));
        live_device_buffers++;
        cap = want;
        return FDBCS_OK;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            live_device_buffers--;
        }
        p = nullptr;
        cap = 0;
    }
};

// Grow-only pinned host allocation; `mapped` buffers are fine-grained and written by kernels directly.
struct HBuf {
    void* p = nullptr;
    void* dp = nullptr;  // device view (mapped buffers)
    size_t cap = 0;
    HBuf() = default;
    HBuf(const HBuf&) = delete;
    HBuf& operator=(const HBuf&) = delete;
    HBuf(HBuf&& o) noexcept
        : p(std::exchange(o.p, nullptr)), dp(std::exchange(o.dp, nullptr)), cap(std::exchange(o.cap, 0)) {}
    HBuf& operator=(HBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            dp = std::exchange(o.dp, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~HBuf() { release(); }
    int ensure(size_t bytes, bool mapped = false, bool noncoherent = false) {
        if (bytes <= cap) return FDBCS_OK;
        size_t want = align_up(std::max(bytes, cap + cap / 2), 4096);
        if (p) {
            HIPOK(hipHostFree(p));
            live_host_buffers--;
        }
        p = dp = nullptr;
        cap = 0;
        const unsigned fl = !mapped ? hipHostMallocDefault
                                    : (hipHostMallocMapped | (noncoherent ? hipHostMallocNonCoherent : hipHostMallocCoherent));
        HIPOK(hipHostMalloc(&p, want, fl));
        live_host_buffers++;
        if (mapped) HIPOK(hipHostGetDevicePointer(&dp, p, 0));
        cap = want;
        return FDBCS_OK;
    }
    void release() {
        if (p) {
            (void)hipHostFree(p);
            live_host_buffers--;
        }
        p = dp = nullptr;
        cap = 0;
    }
};

// A move-only holder of one runtime handle, destroyed with it.
template <typename H, hipError_t (*Destroy)(H), std::atomic<int64_t>& Live>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        reset(std::exchange(o.h, nullptr));
        return *this;
    }
    ~Handle() { reset(); }
    void reset(H next = nullptr) {
        if (h) {
            (void)Destroy(h);
            Live--;
        }
        h = next;
    }
    operator H() const { return h; }
};

// One event, created by the first make().
struct Event : Handle<hipEvent_t, hipEventDestroy, live_events> {
    int make(unsigned flags = hipEventDefault) {
        if (h) return FDBCS_OK;
        HIPOK(hipEventCreateWithFlags(&h, flags));
        live_events++;
        return FDBCS_OK;
    }
};

// One non-blocking stream, created by the first make().
struct Stream : Handle<hipStream_t, hipStreamDestroy, live_streams> {
    int make() {
        if (h) return FDBCS_OK;
        HIPOK(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        live_streams++;
        return FDBCS_OK;
    }
};

// Two timing events around a group of launches: begin(s), the launches, end(s), and once the
// second event has completed, ms().
struct Span {
    Event e0, e1;
    int begin(hipStream_t s) {
        if (int rc = e0.make()) return rc;
        if (int rc = e1.make()) return rc;
        HIPOK(hipEventRecord(e0, s));
        return FDBCS_OK;
    }
    int end(hipStream_t s) {
        HIPOK(hipEventRecord(e1, s));
        return FDBCS_OK;
    }
    // Milliseconds between two completed events (0 when either was never recorded).
    static double between(hipEvent_t a, hipEvent_t b) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.0;
        return (double)ms;
    }
    double ms() const { return between(e0, e1); }
};

// The per-kernel events of a slot.  LaunchList::Profile (launch.h) points into `v` and creates the
// events it hands out, so they are counted here, by count() once a profiled batch is done.
struct EventPool {
    std::vector<hipEvent_t> v;
    size_t counted = 0;
    EventPool() = default;
    EventPool(EventPool&& o) noexcept : v(std::move(o.v)), counted(std::exchange(o.counted, 0)) {}
    void count() {
        live_events += (int64_t)(v.size() - counted);
        counted = v.size();
    }
    ~EventPool() {
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
        live_events -= (int64_t)counted;
    }
};

template <typename... T>
constexpr bool move_only_v = ((!std::is_copy_constructible_v<T> && std::is_nothrow_move_constructible_v<T>) && ...);
static_assert(move_only_v<DBuf, HBuf, Event, Stream, Span, EventPool>);

enum Phase {
    kPhStart, kPhUpload, kPhSort, kPhEdges, kPhCheck, kPhIntra, kPhCombine, kPhCopyBegin, kPhCopyEnd, kPhMerge,
    kPhCompBegin, kPhCompEnd, kPhCompact, kPhGc, kPhEpilogue, kPhEnd,
    kPhCheckBegin, kPhCheckEnd, kPhSortBegin, kPhSortEnd, kPhCount
};

}  // namespace fdbcs::impl
using namespace fdbcs::impl;

struct fdbcs_batch;
struct BatchSlot;

// ws[k] slots: ensure_workspace TAKEs [0, kWsTileSlot); then the copy-tile index and the scan arena.
constexpr int kWsTileSlot = 54, kWsArenaSlot = 55;
// Batch workspaces in rotation: stage A of batch i starts once Y of batch i - kNumWork and X of
// batch i - kNumWork + 1 are over, so it can run up to kNumWork - 1 batches ahead of stage B.
// Eight: in a loop that keeps eight batches in flight the host issues A(i) when batch i - 8 is
// done, so the ring never holds stage A back and its edge word reaches the host before X(i) has
// to be issued (the depth's measurement: DESIGN.md §5, builds of 4, 6, 8 and 12 through
// FDBCS_NUM_WORK, `profiles/x_tail_skip_ab.jsonl`).
#ifndef FDBCS_NUM_WORK
#define FDBCS_NUM_WORK 8
#endif
constexpr int kNumWork = FDBCS_NUM_WORK;
// A held X half (kMaxHold below) is issued while the helper issues stage A of the batch two calls
// later: that stage A waits on the events of the X half kNumWork - 1 batches back, which must
// have been issued by an earlier call.
static_assert(kNumWork >= 4, "the workspace ring must outlast the two-call hold of an X half");
// Stage-B lists (X and the Y behind it) recorded and not yet issued: at most the last two batches'.
constexpr int kMaxHold = 2;
constexpr int kGcEveryCompactions = 4;  // removeBefore cadence of size-triggered compactions

// FDBCS_HOST_TRACE=<path>: host-side spans of the pipeline (steady_clock ns, the clock rocprofv3
// timestamps use), written as CSV when the set is destroyed: per batch sequence number the detect
// call (D), the helper's issue of stage A (A) and of a Y half (Y), the calling thread's issue of an
// X half (X) and the wait for the completion flag (W).  scripts/host_trace.py joins them with a
// rocprofv3 kernel trace: when each chain's launches were issued against when they ran.
struct HSpan {
    uint32_t seq;
    char kind;
    int64_t t0, t1;
};
inline int64_t mono_ns(std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now()) {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(t.time_since_epoch()).count();
}

// Host threads for addTransaction of whole batches (fdbcs_batch_add_packed): the endpoint keys'
// validation and normalization into pinned staging split over chunks of transactions.  The
// calling thread works too.  A ticket carries the job's generation, so a worker that wakes late
// never takes a ticket of a later job with the earlier job's function.  Between jobs a worker
// sleeps on the condition variable (spinning ~300 us for the next job measured no better:
// DESIGN.md §5).
struct AddPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<uint64_t> ticket{0};  // generation << 32 | next ticket
    std::atomic<int> done{0};         // tickets finished in the current generation
    std::atomic<uint32_t> gen{0};
    std::atomic<int> sleepers{0};
    int n = 0;
    const std::function<void(int)>* job = nullptr;
    bool stop = false;

    // std::thread's constructor throws (std::system_error) at the process's thread limit: the
    // workers already started are stopped and joined before the exception leaves, so the caller
    // can fall back to the serial loop
    explicit AddPool(int workers) {
        try {
            for (int i = 0; i < workers; i++) th.emplace_back([this] { worker(); });
        } catch (...) {
            shutdown();
            throw;
        }
    }
    ~AddPool() { shutdown(); }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
            gen.fetch_add(1);
        }
        cv.notify_all();
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
    void run(uint32_t g, int nn, const std::function<void(int)>* fn) {
        uint64_t cur = ticket.load(std::memory_order_acquire);
        for (;;) {
            if ((uint32_t)(cur >> 32) != g || (int)(cur & 0xffffffffu) >= nn) return;
            if (ticket.compare_exchange_weak(cur, cur + 1, std::memory_order_acq_rel)) {
                (*fn)((int)(cur & 0xffffffffu));
                done.fetch_add(1, std::memory_order_acq_rel);
                cur = ticket.load(std::memory_order_acquire);
            }
        }
    }
    void worker() {
        uint32_t seen = 0;
        for (;;) {
            uint32_t g;
            int nn;
            const std::function<void(int)>* fn;
            {
                std::unique_lock<std::mutex> lk(m);
                if (gen.load(std::memory_order_relaxed) == seen && !stop) {
                    sleepers.fetch_add(1);
                    cv.wait(lk, [&] { return stop || gen.load(std::memory_order_relaxed) != seen; });
                    sleepers.fetch_sub(1);
                }
                if (stop) return;
                seen = g = gen.load(std::memory_order_relaxed);
                nn = n;
                fn = job;
            }
            run(g, nn, fn);
        }
    }
    // fn(c) for c in [0, tickets), in ticket order across the workers and the calling thread;
    // returns when all are done.
    void parallel_for(int tickets, const std::function<void(int)>& fn) {
        uint32_t g;
        {
            std::lock_guard<std::mutex> lk(m);
            g = gen.load(std::memory_order_relaxed) + 1;
            n = tickets;
            job = &fn;
            done.store(0, std::memory_order_relaxed);
            ticket.store((uint64_t)g << 32, std::memory_order_release);
            gen.store(g, std::memory_order_release);
        }
        if (sleepers.load(std::memory_order_acquire) > 0) cv.notify_all();
        run(g, tickets, &fn);
        while (done.load(std::memory_order_acquire) < tickets) __builtin_ia32_pause();
    }
};

// Ownership: every buffer, event and stream below is an owner type (DBuf, HBuf, Event, Span, Stream),
// so `delete cs` releases them all and a new one needs its member and nothing else.  Members die in
// reverse declaration order: the five streams are declared before every buffer and event, so they
// go last (no event outlives the stream it was recorded on for the runtime to chase), in the order
// ustream, cstream, astream, stream, ystream.  fdbcs_destroy_conflict_set has synchronized them.
struct fdbcs_conflict_set {
    int device = 0;
    // Stage B in two halves on two streams: X (`stream`: read check, resolution, D.Combine) and Y
    // (`ystream`: merge into the delta, compaction / GC, epilogue).  The check of batch i + 1 runs
    // against the delta before batch i's merge plus batch i's union segments (PrevSegs), so it does
    // not wait for that merge: Y(i) overlaps X(i + 1).
    Stream ystream;
    Stream stream;   // stage B: everything that reads or writes the history, in batch order
    Stream astream;  // stage A (and every upload): history-independent sort and edges
    Stream cstream;  // split read check: the base-tier half (history-independent between
                     // compactions) beside stage A
    Stream ustream;  // batch uploads (k_upload over PCIe), so batch i+1's upload overlaps
                     // batch i's stage A; stage A waits for the upload's event
    Event ev_c[kNumWork];  // base-tier check of the batch using workspace k is done
    Event ev_cmp;          // stage B of the last batch that rewrote the base (compaction / GC)
    bool cmp_recorded = false;
    // FDBCS_SPLIT_CHECK: 0 = one read check over both tiers in stage B, 1 = the base-tier half on
    // its own stream beside stage A, 2 (default) = split only over a large base tier (>= 16M
    // boundaries): there the base check is long (C4: ~150 us) and must leave the batch-order
    // chain; over a 5M base (C2) the single launch measured faster (device-resident 34.0M vs
    // 32.1M txns/s: one launch and two cross-stream events fewer, no third stream competing)
    int split_check = 2;
    Event ev_a[kNumWork];    // stage A of the batch using workspace k is done
    Event ev_b[kNumWork];    // stage B (epilogue) of the batch using workspace k is done
    Event ev_res[kNumWork];  // X of the batch using workspace k is done (Y waits for it)
    // the next batch's check is done with workspace k's segments: that batch's ev_res (the end of
    // its half X, recorded anyway, and not re-recorded before workspace k's next user records);
    // an alias of ev_res[], which owns the event
    hipEvent_t xfree_ev[kNumWork] = {};
    bool prev_segs = false;             // the last batch's segments are not merged when the next check runs
    int prev_wp = 0;
    int64_t prev_now = 0;
    int last_wp = -1, prev2_wp = -1;    // workspaces of the last two batches submitted (their Y events)
    bool xfree_rec[kNumWork] = {};      // xfree_ev[k] set since workspace k's last use
    // The batches behind ws ev_b[k] (workspace k's last user) and xfree_ev[k] (the batch whose check
    // reads workspace k's segments), or null once destroyed: while a batch lives its completion
    // flag tells whether its stages are done, one load from host-mapped memory instead of an event
    // query (a runtime call) per dependency per batch.
    fdbcs_batch* ws_user[kNumWork] = {};
    fdbcs_batch* xfree_user[kNumWork] = {};
    bool y_async[kNumWork] = {};        // Y of workspace k's last batch ran on ystream (not in `stream` order)
    bool wused[kNumWork] = {};
    int wpar = 0;                   // workspace of the next batch
    int timing = 0;       // 0: no events; 1: the copy kernels; 2: every phase (fdbcs_set_timing)
    uint32_t seq = 0;     // batches submitted (completion flag values)
    int64_t oldest = 0;          // ConflictSet::oldestVersion (SkipList.cpp:736)
    int64_t header_version = 0;  // SkipList(Version) header (SkipList.cpp:398-404)
    int64_t max_written = 0;     // highest version present in the history
    int gc_interval = 0;          // compaction (and GC) at least every this many batches; 0: by size only
    int batches_since_compact = 0;
    int compactions_since_gc = 0;
    int64_t gc_applied = 0;
    int64_t delta_limit = 0;      // compaction once the delta may exceed this; 0: automatic

    // base tier: two buffer sets (ping-pong) + range-max levels
    DBuf hkey[2], hlt[2], hver[2];
    DBuf lvl[kMaxLevels];  // lvl[0]: sampled key index (the level-0 versions are hver[cur])
    DBuf dir;              // radix directory over the base tier's level-0 samples (k_directory)
    DBuf edir[2];          // each delta buffer's directory (epoch-tagged entries, filled by k_epilogue)
    uint32_t ddir_epoch[2] = {0, 0};  // epoch of each delta buffer's directory (0: none)
    uint32_t ddir_counter = 0;  // last epoch handed out
    int cur = 0;
    int64_t hist_cap = 0;  // elements per buffer set
    int64_t n_ub = 0;      // upper bound of live base boundaries (exact after a wait)
    int64_t lvl3_n = 0;
    int64_t lvl2_n = 0;
    // delta tier: the same layout, small
    DBuf dkey[2], dlt[2], dver[2];
    DBuf dlvl[2][kMaxLevels];  // per delta buffer: the next batch's check reads one while the epilogue builds the other
    int dcur = 0;
    int64_t delta_cap = 0;
    int64_t nd_ub = 0;
    int64_t dlvl3_n = 0;
    int64_t dlvl2_n = 0;
    DBuf cws[6];  // compaction arrays (per delta boundary)
    DBuf htail[2];  // tail arenas (bytes [16, len) of long keys): append-only between GCs; each GC
    int tcur = 0;   // repacks the live tails into the other one, reclaiming the rest
    int64_t tail_ub = 0;
    int64_t tail_cap = 0;
    DBuf scal;  // Scalars
    int64_t route_timeout_ms = 60000;  // FDBCS_ROUTE_TIMEOUT_MS: bound of a routed batch's wait for its shares
    DBuf route_btail;                  // device routing: tails of this resolver's key-range bounds
    std::vector<uint8_t> route_bounds; // the bounds route_btail holds (lo | hi bytes), to skip re-uploads
    // batch workspaces (rotating)
    DBuf ws[kNumWork][56];  // [0, kWsTileSlot): TAKE slots of ensure_workspace
    DBuf wbtail[kNumWork];  // Work::btail of each workspace (ensure_btail)
    int64_t ws_T = -1, ws_R = -1, ws_W = -1;
    Work work[kNumWork]{};
    int64_t edge_cap = 0;

    int inflight = 0;
    bool validate = false;  // FDBCS_VALIDATE=1: device-side invariant checks (tests)
    int bucket_target = 0;  // FDBCS_SORT_BUCKET: endpoints per sort bucket on average (0 = kSortTarget)
    bool sort_cold = false; // FDBCS_SORT_COLD=1: splitters from every batch's own samples (tests)
    DBuf quant;             // the sort's splitter source, two tables: quantiles of the last batch of
    int qcur = 0;           // >= kQuantMinE endpoints in table qcur; the next such batch writes the other
    bool quant_valid = false;
    // the stream of the last stage A (its sort read one splitter table and wrote the other): a batch
    // whose stage A runs on another stream (a timing-level change) waits for ev_quant recorded there
    hipStream_t quant_sa = nullptr;
    Event ev_quant;
    int64_t sort_big_buckets = 0;  // buckets past kSlab so far (host view, from the published scalars)
    bool trace = false;     // FDBCS_TRACE=1: device timestamps of kernel sections printed per batch
    bool serial = false;    // FDBCS_SERIAL=1: both stages on one stream (no cross-batch overlap)
    bool no_prepass = false;  // FDBCS_RESOLVE_PREPASS=0: k_resolve without its pre-pass (tests)
    int64_t tail_reclaim = kTailReclaimDefault;  // FDBCS_TAIL_RECLAIM: tail bytes that force the GC repack
    bool write_groups = true;  // FDBCS_WRITE_GROUPS=0: one candidate edge per (read, writer) pair (A/B)
    bool directory = true;  // FDBCS_DIRECTORY=0: base-tier lookups descend the whole sample tree (A/B)
    // Directory code (MaxLevels::dir_p .. dir_w; set_dir_map): the loaded keys' common prefix
    // (capped at 15) and the value range of each byte position after it, as many positions as fit
    // the slot budget (dir_bits).  Keys written later outside the loaded values take neighbouring
    // codes, so the mapping stays monotone.  (Round 4's directory on the first two key bytes, and
    // its prefix-only variant, are the special cases this code replaced: DESIGN.md §5.)
    uint32_t dir_p = 0;
    uint64_t dir_phi = 0, dir_plo = 0;
    uint32_t dir_e = 0, dir_top = 0;
    uint32_t dir_pos[kDirPos] = {}, dir_w[kDirPos] = {};
    // FDBCS_DIR_BITS: slot budget 2^bits.  0 (default): 2^16, doubled while the base has over
    // eight level-0 samples per slot (C4: 2^17; a slot of up to 16 samples is counted directly).
    // A directory is read cold by every batch's check, so a larger one costs cache misses: C2's
    // isolated check 11.0 us at 2^16, 16.4 at 2^18; C4's 57.3 at 2^17, 62 at 2^19 and 2^20, 64 on
    // the first two bytes.
    int dir_bits = 0;
    DBuf trace_buf;
    // Per-kernel device time (fdbcs_kernel_profile): launches and milliseconds by kernel, from the
    // events of timing level 3 (every kernel) or of the timed kernel at level 1.
    struct KProf {
        const void* func;
        int64_t launches;
        double ms;
    };
    std::vector<KProf> kprof;
    const void* timed_func = nullptr;  // fdbcs_set_timed_kernel
    HBuf hold;                         // fdbcs_debug_hold: host-mapped release word of the hold kernels
    HBuf hedge;                        // per workspace {batch seq, any candidate edge} (Work::hedge)
    bool skip_edges = true;            // FDBCS_SKIP_EDGES=0: always issue the kGroupEdges launches
    fdbcs_stats stats{};
    std::vector<std::unique_ptr<BatchSlot>> pool;  // staging slots of destroyed batches, reused by new ones
    // Two submitting threads (the default since round 4: C2 +3-10 % over five same-box A/Bs, C3 and
    // C4 unchanged; FDBCS_SUBMIT_THREAD=0 keeps one).  A helper thread issues stage A of batch i
    // (and its base-tier check) while the calling thread issues the held X halves that are due
    // (batch i-2's, and batch i-1's once its edge word is known: `held`); the helper then issues
    // each of those batches' Y half once its X is out:
    // kernel launches on two streams from two threads take about half the wall time of one
    // thread's (tools/threadbench.hip: 3.4 -> 1.85 us per launch).  The
    // check of batch i waits (host side) until stage B of batch i-1 is issued, because it may wait
    // on that stage's compaction event; stage B of batch i waits for the helper to go idle.
    bool submit_thread = true;
    // addTransaction threads (FDBCS_ADD_THREADS, workers besides the calling thread; 0 = serial)
    int add_threads = 5;
    AddPool* add_pool = nullptr;
    int wait_query_ms = 2;  // FDBCS_WAIT_QUERY_MS: stream error checks while a wait spins (0: every 4096 spins)
    // FDBCS_HOST_TRACE: spans of the calling thread [0] and of the helper [1]
    bool htrace = false;
    std::vector<HSpan> htr[2];
    uint32_t work_a_seq = 0;
    double add_prof[4] = {0, 0, 0, 0};  // FDBCS_ADD_PROFILE: ms in add's serial pass, slot, count, fill
    int64_t add_prof_n = 0;
    std::thread worker;
    std::mutex wmu;
    std::condition_variable wcv;
    std::atomic<int> wjob{0};           // 0 idle, 1 job queued or running, 2 exit
    std::atomic<uint32_t> b_issued{0};  // stage-B lists issued (their Y halves: helper or flush)
    uint32_t b_recorded = 0;            // stage-B lists recorded
    std::atomic<int> werr{0};           // first HIP error of the helper
    LaunchList work_a, work_c;          // the helper's lists
    hipStream_t work_sa = nullptr;
    uint32_t work_need_b = 0;           // the check goes out once b_issued >= this
    // Stage B's Y half of the batch whose X half the calling thread issues at this call, issued
    // by the helper once that X half is out.  The calling thread issues record + X, the helper
    // stage A + Y + base check: their runtime calls split about evenly instead of ~2:1.
    LaunchList work_y;
    hipStream_t work_ys = nullptr;
    uint32_t work_y_seq = 0;
    uint32_t work_need_x = 0;            // Y goes out once x_issued >= this
    std::atomic<uint32_t> x_issued{0};   // stage-B X lists issued (calling thread)
    fdbcs_batch* work_y_batch = nullptr; // whose Y the helper holds (calling thread's view)
    LaunchList rec_a, rec_b, rec_c, rec_y;
    // Recorded stage-B lists not yet issued, oldest first.  X(i) is held until the host has seen
    // batch i's edge word (x_known), at most two calls: it goes out at call i + 1 when the word is
    // there, at call i + 2 whatever the word says, and before that whenever somebody waits for
    // batch i or a later one (flush_pending).  Always in batch order.
    struct Held {
        fdbcs_batch* batch = nullptr;
        LaunchList x, y;
        hipStream_t ys = nullptr;  // the stream of y
    };
    Held held[kMaxHold];
    int n_held = 0;
    LaunchList go_x;  // the X list being issued at this call (taken out of `held`)
    std::unordered_set<fdbcs_batch*> live;  // batches not yet destroyed (detached if the set goes first)
    // fdbcs_history_export: scratch (per delta boundary), the bounds' tails, scan granules + export
    // words, and the result arrays; all allocated by the first export.  x_valid: a result is pending
    // and the set has not changed since (detect, load, clear and another export end it).
    DBuf x_pos, x_val, x_btail, x_state, x_ver, x_off, x_bytes;
    bool x_valid = false;
    int64_t x_n = 0, x_nbytes = 0;
    Span x_span;                                  // around the export's kernels
    double x_ms_kernels = 0, x_ms_d2h = 0;        // of the last export / read (fdbcs_history_export_timing)
    int64_t x_hdr = 0;                            // the pending result's header version
    // fdbcs_history_digest: its own words and per-tile starts (a pending export's words stay as they
    // are); x_pos, x_val and x_btail are shared with the export, which keeps no result in them
    DBuf g_state;
    Span g_span;                                  // around the digest's kernels
    double g_ms_kernels = 0, g_ms_host = 0;       // of the last digest (fdbcs_history_digest_timing)
    // fdbcs_history_digest_ranges: the bounds as uploaded (bytes, offsets), two stream positions per
    // edge and the result blocks; they grow with the number of ranges only.  Words, tile starts and
    // timing are the digest's (g_state, g_span, g_ms_*).
    DBuf r_bytes, r_off, r_pos, r_out;
    // fdbcs_history_split_keys: its words, and the result (offsets, key bytes) until it is read.  The
    // result is a copy, so it outlives changes of the set; another call replaces it.
    DBuf k_state, k_off, k_bytes;
    bool k_valid = false;
    int64_t k_n = 0, k_nbytes = 0;
    Span k_span;
    double k_ms_kernels = 0, k_ms_host = 0;       // of the last call (fdbcs_history_split_keys_timing)
    // fdbcs_batch_read_versions: the host form's result (grow-only; the device form writes to the
    // caller's memory) and the error word, allocated by the first query; nothing of the export's
    DBuf rv_out, rv_err;
    Span rv_span;                                 // around the query's kernel
    double rv_ms_kernels = 0, rv_ms_host = 0;     // of the last query (fdbcs_batch_read_versions_timing)
    // fdbcs_history_import: device copies of the imported arrays (host-array form), the bounds' bytes,
    // the overlay stream (keys, lt, versions, tails), the merged stream (value, key, lt) and the import
    // words; all allocated by the first import and freed with the set.
    DBuf i_bytes, i_off, i_ver, i_bnd, i_okey, i_olt, i_over, i_otail, i_mval, i_mkey, i_mlt, i_dblt, i_vblt, i_state;
    DBuf i_gran;                                  // the fold's scan granules
    Span i_span[3];                               // around the import's three groups of kernels
    double i_ms_kernels = 0, i_ms_host = 0;       // of the last import (fdbcs_history_import_timing)
    // fdbcs_history_import_delta: its words + scan granules (allocated by the first delta import), and
    // what the last successful import of either kind did (fdbcs_history_import_info)
    DBuf i_dstate;
    int32_t i_path = 0;                           // 0: folded into a new base, 1: merged into the delta
    int64_t i_info_base = 0, i_info_before = 0, i_info_after = 0;  // base size; delta size around it
    // fdbcs_history_verify: its counts, first indices and one true maximum per level-3 entry (allocated
    // by the first verify; a set that never verifies holds nothing of it)
    DBuf v_state;
    Span v_span;                                  // around the verify's kernels
    double v_ms_kernels = 0, v_ms_host = 0;       // of the last verify (fdbcs_history_verify_timing)
};

// Host/device staging of one batch.  Batches are short-lived (one per commit batch, as the
// reference's ConflictBatch), so their pinned and device buffers come from a per-set pool instead
// of fresh allocations.  A slot goes back to the pool only when its batch is
// destroyed, after its completion flag was seen (the epilogue's last store) or, for a batch still
// in flight, after its streams were synchronized: the next user's upload needs no event.
struct BatchSlot {
    DBuf dev;
    HBuf pin_in;
    HBuf pin_out;
    DBuf dverdict;
    Event ev[kPhCount];
    bool events_made = false;  // ev[] and ev_up exist (make_slot_events)
    Event ev_up;               // upload done (recorded on stage A's stream)
    HBuf pin_inv;  // fdbcs_batch_set_conflict_output: global -> batch transaction map (host-mapped)
    // device routing (fdbcs_batch_add_routed): scan state, global -> batch map, read ids, totals
    DBuf rt_scan, rt_inv, rt_rids, rt_dres, rt_info, rt_txpre;
    DBuf rt_gids;  // global read index of each kept read (reporting routed batches only)
    // fdbcs_batch_add_routed_map: the keyResolvers map the batch is routed under (route_map_layout)
    // and the pinned staging it is copied from
    DBuf rt_map;
    HBuf rt_map_pin;
    HBuf rt_res;
    Span rt_span;  // around the routing kernels
    bool rt_timed = false;
    // fdbcs_batch_set_iops_sample: scan state, result arrays, host-mapped totals and the events
    // around the kernel, all allocated by the slot's first sampled batch.  is_inflight: a sample
    // was enqueued and nobody has waited for its end since (it reads the slot's device copy)
    DBuf is_state, is_met, is_idx, is_off, is_bytes;
    HBuf is_tot;
    Span is_span;
    bool is_inflight = false;
    // fdbcs_batch_add_packed_device: scan state, the device and host-mapped totals and the events
    // around the add kernels, all allocated by the slot's first device-added batch
    DBuf da_scan, da_dres;
    HBuf da_res;
    Span da_span;
    // fdbcs_batch_share_pack_device shares them (a batch does one or the other) and adds each key's
    // place in the share's tail region, the scan's store
    DBuf sp_toff;
    // per-kernel events of the batch (timing level 3, or the timed kernel at level 1)
    EventPool prof_pool;
    size_t prof_next = 0;
    std::vector<std::pair<const void*, std::pair<hipEvent_t, hipEvent_t>>> prof_spans;
    LaunchList::Profile prof{&prof_pool.v, &prof_next, &prof_spans};
};

struct fdbcs_batch {
    fdbcs_conflict_set* cs = nullptr;
    std::unique_ptr<BatchSlot> slot;  // back to the set's pool when the batch dies, or freed with it once the set is gone
    int report_enabled = 0;
    int state = 0;  // 0 adding, 1 uploaded, 2 submitted, 3 done
    // host staging (pageable); in `direct` mode (one fdbcs_batch_add_packed) the endpoint keys,
    // owners and tails were normalized straight into slot->pin_in at add time
    std::vector<int64_t> snap;
    std::vector<uint8_t> flags;
    std::vector<int32_t> roff{0}, woff{0};
    std::vector<int32_t> rowner, wowner;
    std::vector<DKey> rkeys, wkeys;
    std::vector<uint8_t> tail;
    bool direct = false;
    size_t d_keys = 0, d_rown = 0, d_wown = 0, d_tail = 0, d_small = 0;  // pin_in offsets (direct mode)
    size_t d_tail_bytes = 0;
    // device copy
    BatchDev bd{};
    size_t tail_bytes = 0;
    // results
    uint8_t* h_verdict = nullptr;
    Scalars* h_scal = nullptr;
    uint8_t* h_rconf = nullptr;
    uint8_t* h_hist = nullptr;
    int32_t* h_first = nullptr;
    bool gc_ran = false;
    bool compacted = false;
    uint32_t seq = 0;
    volatile uint32_t* h_flag = nullptr;
    int64_t n_report = 0;  // transactions added with report_conflicting_keys (and reports enabled)
    uint32_t recorded = 0;  // phases whose events were recorded (bit per Phase)
    bool any_report = false;
    int64_t check_hist = 0;  // boundaries (both tiers, upper bound) the read check searched
    std::vector<int32_t> out_ids;  // fdbcs_batch_set_conflict_output: global index per transaction
    int64_t out_n = 0;
    uint8_t* out_dev = nullptr;
    int wp = 0;           // the workspace this batch's detect used
    // its X half was issued whole although it had launches a known edge count of 0 leaves out
    // (account_stats: counted as too early when the batch turns out edge-free)
    bool x_unskipped = false;
    int32_t max_len = 0;  // longest key added (the sort stages tail windows only past kSortNxLen)
    int64_t wtail = 0;       // history tail bytes the batch's write endpoints could add (8-byte padded)
    std::vector<int32_t> conf_off, conf_idx;
    int32_t n_committed = 0, n_too_old = 0;

    // device-routed batch (fdbcs_batch_add_routed): sizes known once the route kernels finished
    bool routed = false, route_pending = false;
    int32_t rT = 0, rR = 0, rW = 0;
    size_t r_tail = 0;
    int64_t r_global_R = 0;  // reads of all shares
    int64_t r_cap_ranges = 0, r_cap_tail = 0;  // read + write and tail capacities it was routed with
    // fdbcs_batch_set_iops_sample: requested; its totals read (fdbcs_batch_iops_sample)
    bool is_req = false, is_done = false;
    int64_t is_n = 0, is_nbytes = 0;
    double is_ms = 0;
    // fdbcs_batch_set_report_output: device bytes per global read, written at detect
    uint8_t* rep_dev = nullptr;
    int64_t rep_n = 0;
    // a routed reporting batch's roff [T+1] and flags [T], copied into the result buffer at detect
    // (the wait-time report loop reads them; other batches read the host vectors above)
    const int32_t* h_roff = nullptr;
    const uint8_t* h_flags = nullptr;
    // device-added batch (fdbcs_batch_add_packed_device): built on the device like a routed one, so
    // it is `routed` too (sizes in rT / rR / rW, known at the call; TooOld judged at detect; roff |
    // flags copied into the result buffer) and this flag tells it apart: no global map, no read
    // ids, no sample, and its conflict output takes the host txn_ids
    bool dev_added = false;
    double da_ms_host = 0, da_ms_kernels = 0;  // of its add call / add kernels (fdbcs_batch_device_add_timing)

    // fdbcs_batch_share_pack_device: the batch packed a share (it stays empty, and takes no add but a
    // routed one from then on); the pack's kernels are not waited for yet; its outcome and times
    bool share_packed = false, sp_pending = false;
    int sp_rc = 0;
    int32_t sp_T = 0, sp_R = 0, sp_W = 0;
    int64_t sp_bytes = 0, sp_tail = 0;
    double sp_ms_host = 0, sp_ms_kernels = 0;

    int32_t T() const { return routed ? rT : (int32_t)snap.size(); }
    int32_t R() const { return routed ? rR : roff.back(); }
    int32_t W() const { return routed ? rW : woff.back(); }
    size_t tail_size() const { return routed ? r_tail : direct ? d_tail_bytes : tail.size(); }
};

// Helpers defined in engine.cpp.
namespace fdbcs::impl {
int cmp_bytes(const uint8_t* a, int32_t al, const uint8_t* b, int32_t bl);  // memcmp, then length
int sync_all(fdbcs_conflict_set* cs);  // drain the set's streams and its helper thread
// Views of base / delta buffer set k and its range-max levels and key index.
Hist hist_of(fdbcs_conflict_set* cs, int k);
MaxLevels levels_of(fdbcs_conflict_set* cs, int k);
Hist delta_of(fdbcs_conflict_set* cs, int k);
MaxLevels dlevels_of(fdbcs_conflict_set* cs, int k);
// Grow the tiers (and the tail arenas) to hold `need` boundaries; the live contents move along.
int ensure_delta(fdbcs_conflict_set* cs, int64_t need);
int ensure_history(fdbcs_conflict_set* cs, int64_t need, int64_t tail_need);
int64_t delta_limit_for(const fdbcs_conflict_set* cs, int64_t n_base);  // delta size that triggers a compaction
int finish_route(fdbcs_batch* b);  // wait for a routed batch's routing and take its sizes and error
// Its sibling for a device-added batch (ingest.cpp; finish_route hands such a batch over): wait for
// the add kernels and take the totals; on an error the batch is empty again.
int finish_device_add(fdbcs_batch* b);
// And for a batch that packed a share (ingest.cpp): wait for the pack kernels and take their outcome;
// the pack's status, which fdbcs_batch_share_pack_info repeats.
int finish_share_pack(fdbcs_batch* b);
// The wire layout of a share (engine.h ShareHeader) into *h; its size.
size_t share_layout(int32_t T, int64_t R, int64_t W, int64_t tail, ShareHeader* h);
// Layout of a batch in pin_in / dev: [keys | rowner | wowner | snap | roff | woff | flags | tail].
struct UploadLayout {
    size_t keys, rown, wown, snap, roff, woff, flags, tail, total;
};
UploadLayout upload_layout(size_t T, size_t R, size_t W, size_t tail_bytes);
// Every allocation a batch of this shape needs (device copy, pinned results, device verdicts), and
// the slot's phase and upload events.
int ensure_slot(BatchSlot* sl, size_t upload_bytes, size_t T, size_t R);
int make_slot_events(BatchSlot* sl);
}  // namespace fdbcs::impl
