/*
 * host_internal.h — what the C-ABI translation units share: the owners of GPU
 * resources (device and pinned arrays, events, streams), the rule that orders a
 * shared buffer across streams, the pass state of the components that queue
 * work for a second pass (PassState: tget, cut, kids, cols, ents, rows), the
 * context, descriptor, plan and per-stream scratch records, the entry guard,
 * the argument records of one batch, the host batch of the thrift/generic and
 * t2j entries (HostBatch) and the error helpers (j2t_host.hip defines the
 * functions; t2j_host, tget_host, cut_host, editm_host, kids_host, cols_host,
 * ents_host, rows_host, vals_host, evals_host and j2t_pipe use them). What only
 * cols, ents and rows share is in plan_internal.h.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/dgj2t.h"
#include "../../include/dgj2t_desc.h"
#include "host_layout.h"

__attribute__((visibility("hidden"))) int set_err(int code, const char *fmt, ...);
#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) return set_err(DG_E_HIP, "%s: %s", #x, hipGetErrorString(e_));  \
    } while (0)

/* ---- owners: move-only, freed by their destructors and nowhere else. hipFree
 * and hipHostFree wait for the whole device, so an owner frees only when it
 * dies or when grow() finds it too small: a buffer that fits is reused. ---- */

/* what DevArr and PinArr share: pointer + capacity (in elements) */
template <class T, hipError_t (*FREE)(void *)>
struct ArrBase {
    T *p = nullptr;
    uint64_t cap = 0;
    ArrBase() = default;
    ArrBase(ArrBase &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    ArrBase &operator=(ArrBase &&o) noexcept
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~ArrBase() { reset(); }
    void reset()
    {
        if (p) (void)FREE(p);
        p = nullptr, cap = 0;
    }
    operator T *() const { return p; }
};

/* device memory. grow: free first, then max(want, 2 cap) elements */
template <class T>
struct DevArr : ArrBase<T, hipFree> {
    int alloc(uint64_t n) /* exactly n elements, once */
    {
        HIPCHK(hipMalloc(&this->p, n * sizeof(T)));
        this->cap = n;
        return DG_OK;
    }
    int grow(uint64_t want)
    {
        if (this->cap >= want) return DG_OK;
        const uint64_t nc = std::max<uint64_t>(want, this->cap * 2);
        this->reset();
        return alloc(nc);
    }
};

/* pinned host memory, grown on demand (hipHostMalloc is slow: keep it) */
template <class T>
struct PinArr : ArrBase<T, hipHostFree> {
    int alloc(uint64_t n, unsigned flags = hipHostMallocDefault)
    {
        HIPCHK(hipHostMalloc((void **)&this->p, n * sizeof(T), flags));
        this->cap = n;
        return DG_OK;
    }
    int grow(uint64_t want) /* like DevArr::grow, and at least 64 KiB */
    {
        if (this->cap >= want) return DG_OK;
        const uint64_t nc = std::max<uint64_t>(std::max<uint64_t>(want, this->cap * 2), (1 << 16) / sizeof(T));
        this->reset();
        /* DG_HOST_NUMA=1: on the allocating thread's NUMA node (its policy)
         * instead of the driver's default placement */
        static const unsigned fl = getenv("DG_HOST_NUMA") ? hipHostMallocNumaUser : hipHostMallocDefault;
        return alloc(nc, fl);
    }
};

/* what Event and Stream share: a HIP handle destroyed with its owner */
template <class H, hipError_t (*DESTROY)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
    Handle &operator=(Handle &&o) noexcept
    {
        std::swap(h, o.h);
        return *this;
    }
    ~Handle()
    {
        if (h) (void)DESTROY(h);
    }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create() { return hipEventCreate(&h); } /* a timing event */
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&h, flags); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&h, flags); }
};

/* The ordering rule of everything several streams share (a scratch, a
 * per-context workspace): `done` is recorded on the stream that used it
 * last, and a launch on another stream waits for it first. The event orders
 * execution only -- no host reads data through it, and a kernel's own
 * dispatch fences already publish its writes to the kernels after it -- so
 * it carries no system-scope fence: that fence cost every batch a 5-6 us gap
 * before the stream's next kernel (r8g trace; r8h/r8i: C2 in flight 336 ->
 * 353 GB/s; a device-scope release instead gained nothing). */
struct StreamOrder {
    Event done;                 /* created by the first acquire */
    hipStream_t last = nullptr; /* stream of the last launch that used it (null: none pending) */
    hipError_t acquire(hipStream_t s)
    {
        if (!done) {
            hipError_t e = done.create(hipEventDisableTiming | hipEventDisableSystemFence);
            if (e != hipSuccess) return e;
        }
        return last && last != s ? hipStreamWaitEvent(s, done, 0) : hipSuccess;
    }
    hipError_t publish(hipStream_t s)
    {
        hipError_t e = hipEventRecord(done, s);
        if (e == hipSuccess) last = s;
        return e;
    }
    /* the host waits for the last launch (before a buffer it may read goes) */
    hipError_t wait_host() const { return last ? hipEventSynchronize(done) : hipSuccess; }
    /* grow a buffer it guards: the old one may still be used by the last
     * launch, so wait for it before freeing */
    template <class T>
    int grow(DevArr<T> &a, uint64_t want)
    {
        if (a.cap >= want) return DG_OK;
        HIPCHK(wait_host());
        return a.grow(want);
    }
    /* streams s[0..n) are about to be destroyed and the device is idle */
    void forget(const hipStream_t *s, int n)
    {
        if (std::find(s, s + n, last) != s + n) last = nullptr;
    }
};

/* one workspace per context, shared across streams (t2j's deep frames and
 * token regions); ws is freed before done is destroyed */
struct SharedWs : StreamOrder {
    DevArr<uint8_t> ws;
};

/* Two counter sets used by alternate launches: each launch counts in mine()
 * and its deep pass zeroes other(), the set the previous launch used (no
 * memset per launch). finish: flip after a good launch; after a failed one
 * the deep pass may not have run, so both sets are cleared on the stream. */
struct AltCounters {
    uint32_t *set[2] = {nullptr, nullptr};
    uint32_t bytes = 0, cur = 0;
    uint32_t *mine() const { return set[cur]; }
    uint32_t *other() const { return set[cur ^ 1u]; }
    /* first use: the two sets, `words` counters each, in buf, zeroed */
    int init(DevArr<uint32_t> &buf, uint32_t words)
    {
        if (!buf)
            if (int rc = buf.alloc(4)) return rc;
        HIPCHK(hipMemset(buf, 0, 16));
        HIPCHK(hipDeviceSynchronize()); /* before a non-blocking stream counts on it */
        set[0] = buf, set[1] = buf + words, bytes = 4 * words;
        return DG_OK;
    }
    void finish(bool ok, hipStream_t s)
    {
        if (ok) cur ^= 1u;
        else
            for (uint32_t *p : set) (void)hipMemsetAsync(p, 0, bytes, s);
    }
};

/* What a component whose lane pass queues work for a second pass keeps per
 * context (tget, cut, kids, cols, ents, rows): the deep frames (cut has none),
 * the queue, the two alternating counter sets and the scan's tile sums (where
 * it scans). One per context and shared by every stream, so it is ordered
 * like a workspace: a launch on another stream than the previous one waits
 * for it. The buffers are freed before `done` is destroyed. */
struct PassState : StreamOrder {
    DevArr<uint8_t> ws;
    DevArr<uint32_t> list, cnt_buf;
    AltCounters cnt;
    DevArr<uint64_t> sums;
    /* first use: ws_bytes of frames (0: none) and the counters, `words` a set */
    int first_use(uint64_t ws_bytes, uint32_t words)
    {
        if (cnt.set[0]) return DG_OK; /* set by a complete init: a first use that failed half way is taken up again */
        if (ws_bytes && !ws)
            if (int rc = ws.alloc(ws_bytes)) return rc;
        return cnt.init(cnt_buf, words);
    }
    /* room for `queue` entries and `tiles` tile sums (grow waits for the previous launch) */
    int room(uint64_t queue, uint64_t tiles = 0)
    {
        if (int rc = grow(list, queue)) return rc;
        return grow(sums, tiles);
    }
    /* One enqueue on stream s: acquire, the caller's launches (they answer the
     * first launch error), publish -- also after a failed enqueue, and before
     * its error is returned -- and the error as "<what> launch: ...". */
    template <class F>
    int enqueue(hipStream_t s, const char *what, F launches)
    {
        HIPCHK(acquire(s));
        const hipError_t e = launches();
        HIPCHK(publish(s));
        if (e != hipSuccess) return set_err(DG_E_HIP, "%s launch: %s", what, hipGetErrorString(e));
        return DG_OK;
    }
    /* inside enqueue: one lane pass with its second pass, launch(mine, other), on the counter set whose turn it
     * is; a launch of two steps leaves the second out when hipPeekAtLastError shows the first failed */
    template <class F>
    hipError_t pass(hipStream_t s, F launch)
    {
        launch(cnt.mine(), cnt.other());
        const hipError_t e = hipGetLastError();
        cnt.finish(e == hipSuccess, s);
        return e;
    }
};

/* Scratch::counts: DG_NCOUNTS u32 counters, each owned by ONE path.
 * j2t: [CNT_BAIL .. CNT_DEEP_DONE] are reset by the launch's last kernel
 *      (list mode), or by a stream memset of DG_J2T_COUNTS_BYTES when an
 *      enqueue fails half way;
 * pack: CNT_PACK is dg_pack_device_scan's arrivals, the next its departures,
 *      [12] its slot-overflow count (MsgFrame::ovf_out) -- self-reset;
 * t2j: launches alternate between the sets at CNT_T2J_A and CNT_T2J_B
 *      (Scratch::t2j_cnt); within a set, the T2J_* offsets. */
enum : uint32_t {
    CNT_BAIL = 0,      /* bails */
    CNT_BIG = 1,       /* large messages */
    CNT_WAVEQ = 2,     /* wave queue */
    CNT_HUGE = 3,      /* huge messages */
    CNT_DEEP = 4,      /* deep count */
    CNT_DEEP_DONE = 5, /* blocks done (deep pass) */
    CNT_PACK = 6,
    CNT_T2J_A = 8,
    CNT_T2J_B = 16,
    T2J_DEEPQ = 0, /* deep-pass queue length */
    T2J_BIG = 1,   /* long messages */
    T2J_WAVEQ = 2, /* the wave kernel's queue */
    T2J_BAIL = 3,  /* its bails */
};
constexpr uint32_t DG_NCOUNTS = 24;
constexpr uint32_t DG_J2T_COUNTS_BYTES = 6 * 4;
constexpr uint32_t FRAME_CAP = 4096;

/* Device scratch of one launch pipeline: the bail/big lists, their
 * self-resetting counters, the wave queue and the workspaces. Launches on the
 * SAME stream reuse it in stream order. Each stream a caller passes gets its
 * own scratch (up to DG_MAX_SCRATCH per context), so concurrent streams never
 * share lists or counters; past that cap a scratch is shared and the next
 * launch on another stream waits for its previous launch (StreamOrder), which
 * keeps the ordering rule true in every case.
 * Destruction: the host waits for the last launch and for the side stream,
 * then the members go in reverse order: buffers, side events, side stream,
 * `done`. */
constexpr int DG_MAX_SCRATCH = 40; /* an aggregator ring (<= AGG_RING_MAX = 24 streams) + the context's stream
                                    * + the in-flight side streams (<= 7) + the host pipeline's 3 */
struct Scratch : StreamOrder {
    hipStream_t owner = nullptr; /* the stream it was created for */
    /* a second stream of this scratch's launches (created on first use): the
     * t2j wave kernel runs on it beside the lane pass (Knobs::t2j_overlap) */
    Stream side;
    Event side_done, side_go;
    DevArr<uint8_t> ws_fast; /* ws_fast_lanes lanes; deep_list grows with it */
    uint64_t ws_fast_lanes = 0;
    DevArr<uint64_t> deep_list;
    DevArr<uint32_t> counts;
    DevArr<uint32_t> bail_list, big_list;
    DevArr<uint8_t> ws_wave, ws_deep;
    DevArr<uint64_t> sums;      /* dg_pack_device_scan: per-block byte totals (n_cu) */
    DevArr<uint8_t> d_frame;    /* dg_pack_device_framed: header + footer bytes */
    std::vector<uint8_t> frame; /* what d_frame holds */
    DevArr<uint32_t> t2j_list;  /* t2j: messages queued for the deep pass */
    DevArr<uint32_t> t2j_big;   /* t2j: long messages for the wave kernel */
    DevArr<uint32_t> t2j_bail;  /* t2j: the wave kernel's bails */
    AltCounters t2j_cnt;
    ~Scratch()
    {
        (void)wait_host();
        if (side) (void)hipStreamSynchronize(side);
    }
};

/* routing knobs: env at dg_ctx_create, then dg_ctx_set_knob (include/dgj2t.h) */
struct Knobs {
    int64_t flat = -1;
    int64_t wave_min = 512;
    int64_t wave_occ = 0;
    int64_t small_mpw = 64;
    int64_t list_blocks = 16;
    int64_t t2j_spread = 0;
    int64_t t2j_overlap = 0;    /* t2j: 1 = the wave kernel on a second stream beside the lane pass; r4n t2j-c3: 65.1 GB/s with, 66.6 without (the lane pass is ~15 us of 1.21 ms, the route kernel adds 14) */
    int64_t t2j_wave_min = 256; /* t2j messages longer than this take the wave kernel (0: never); r4k t2j-c3: 128 / 192 / 256 / 384 / 512 / 1024 -> 66.1 / 66.5 / 66.3 / 59.4 / 53.7 / 23.3 GB/s */
    int64_t flat_wrap = -1;     /* the flat kernel's wrapped mode for roots that wrap a flat struct (0: off) */
    int64_t tget_spread = 0;    /* tget: lanes per (message, path) pair, 0 = from the longest message (tget_host.hip) */
    int64_t cut_wave_min = 4096; /* cut: messages at least this long take the wave route (0: all of them); ~1.1 KB x 65 536: 256 / 1024 / 4096 / 16384 -> 29.5 / 44.0 / 227.2 / 227.6 GB/s; ~83 KB x 4 096: lane 23.5, wave 26.5 */
    int64_t edit_reuse_rec = 0;   /* edit and editm, timing only: 1 = a launch of as many messages and items as the context's previous edit launch skips the lookup and splices from its records (the same batch and paths, or the result is undefined) */
    int64_t edit_lanes = 4;       /* edit: lanes per message on the splice's lane route, 1, 4 or 16 (anything else: 1); splice alone at 1 / 4 / 16, ~227 B x 65 536: 259 / 291 / 264 GB/s, ~1.1 KB x 65 536: 593 / 876 / 978, ~83 KB x 4 096: 54 / 250 / 814 */
    int64_t edit_wave_min = 4096; /* edit: outputs at least this long take the splice's wave route (0: all of them); ~1.1 KB x 65 536 at 4 lanes, 256 / 1024 / 4096 / 16384 -> 588 / 546 / 877 / 875 GB/s; ~83 KB x 4 096: lane route 250, wave route 1 550 */
    int64_t kids_wide_min = 256;  /* kids: a list, set or map node of fixed-size entries with at least this many children is emitted by the record-parallel kernel (0: never); emit pass, 16 384 x list<i64> of 64 / 128 / 256 / 1024, lane route 0.107 / 0.159 / 0.261 / 1.314 ms, wide route 0.264 / 0.270 / 0.278 / 0.350 */
    int64_t kids_no_scan = 0;     /* kids, timing only: 1 = a call leaves the scan out (rec_off is not written) */
    int64_t cols_full_search = 0; /* cols, timing only: 1 = every lane of the list emit searches all n offsets (0: between the answers of its block's first and last lane) */
    int64_t ents_stage = 16;      /* ents: entries a lane of the variable-stride emit stages in LDS a round before the wave writes them out in runs, 4, 8 or 16 (anything else: 0 = every lane stores its entries itself); emit call (scan + emit) at 0 / 4 / 8 / 16, 16 384 x list<string> of 64 strings of 8 bytes: 0.127 / 0.126 / 0.116 / 0.114 ms, x map<string, i64> of 64 with keys of 64 bytes: 0.167 / 0.154 / 0.152 / 0.151; of 4 and 16 entries all four within 3 % */
    int64_t vals_lane_emit = 0;   /* vals: 1 = one lane per cell writes all of it, payload and elements included (0: the head pass and the wave-parallel body pass); call at 0 / 1, 16 384 x one string of 64 / 1 024 / 16 384 bytes: 0.128 / 0.139 / 0.440 against 0.095 / 0.141 / 0.882 ms, x list<double> of 64 / 256 / 1 024: 0.138 / 0.163 / 0.240 against 0.125 / 0.229 / 0.660 */
};

/* one chunk in flight of dg_j2t_pipeline_host (j2t_pipe.hip) */
struct PipeBuf;
struct PipeBufDelete {
    void operator()(PipeBuf *p) const;
};

/* Destruction order is part of the behaviour. ~dg_ctx selects the device and
 * synchronises the context's stream; then the members go in reverse order of
 * declaration, which is why they are declared in this order: the pipeline's
 * chunks (each synchronises its own stream, then frees) and its staging, the
 * scratches (before any stream they were last used on: an event last recorded
 * on a destroyed stream is not safe to wait on), the staging buffers, the
 * shared workspaces and the components' pass states (each frees its buffers
 * before its own event), the in-flight side streams and their events, and
 * the context's own stream last. */
struct dg_ctx {
    int device = 0;
    Stream stream;
    int n_cu = 0;
    Knobs knobs;
    uint32_t rr = 0; /* round-robin pick once DG_MAX_SCRATCH scratches exist */
    std::mutex mu;
    /* dg_j2t_batch_device_ktime: while set, enqueue() records kt[0] before the
     * batch's first kernel, kt[1] after it, kt[2] after the wave kernel and
     * kt[3] after the list pass (timing events, on the launch stream) */
    const Event *kt = nullptr;
    /* dg_j2t_batch_device_inflight: the context's extra streams and their
     * fork/join events (created on first use) */
    Event fork_ev;
    std::vector<Event> side_ev;
    std::vector<Stream> side;
    /* The components' pass states (PassState: deep frames of 32 MB allocated by
     * the first call, queue, two alternating counter sets, tile sums), one
     * each, so that a call of one component on any stream shares nothing with
     * a call of another. tget (tget_host.hip): no sums. */
    PassState tget;
    /* cut (cut_host.hip): the wave route's queue; no frames and no sums */
    PassState cut;
    /* edit and editm (editm_host.hip): the lookup's (K + 1) n records of one
     * batch, ordered across streams like a pass state */
    StreamOrder edit;
    DevArr<dg_tget_rec> edit_rec;
    uint64_t edit_rec_n = 0, edit_rec_k = 0; /* messages and items of the launch that filled edit_rec */
    /* kids (kids_host.hip): the queue holds the deep and the wide queue (n
     * entries each), a counter set is {deep, wide} */
    PassState kids;
    /* cols (cols_host.hip) */
    PassState cols;
    /* vals (vals_host.hip): the size pass's lengths (n * K) and the scan's tile
     * sums: its own, ordered across streams */
    StreamOrder vals;
    DevArr<uint32_t> vals_len;
    DevArr<uint64_t> vals_sums;
    /* ents (ents_host.hip) */
    PassState ents;
    /* rows (rows_host.hip): its three lane passes share the state; beside it
     * the heads' counts (n) and the row index of a call that gives none,
     * ordered by it */
    PassState rows;
    DevArr<uint32_t> rows_counts;
    DevArr<dg_row_ent> rows_index;
    /* the t2j wave kernel's token regions (t2j_wave_ws_bytes, ~200 MB) */
    SharedWs t2j_tok;
    /* t2j deep pass: T2J_DEEP_DEPTH frames per lane (about 100 MB, allocated
     * by the first t2j launch) */
    SharedWs t2j_deep;
    /* staging for the host API */
    PinArr<uint8_t> h_down;     /* pinned: ret + out_len (+ packed bytes) */
    PinArr<uint8_t> h_up;       /* pinned: offsets + JSON, one H2D */
    DevArr<uint64_t> d_pack_off;
    DevArr<uint8_t> d_pack;     /* packed Thrift (dg_pack_device_scan) */
    DevArr<uint8_t> d_cb;       /* t2j: callback answers (entries + bytes) */
    DevArr<uint64_t> d_aux;     /* t2j: per-message response-base spans */
    DevArr<uint64_t> d_ret;
    DevArr<uint32_t> d_out_len;
    DevArr<uint64_t> d_out_off;
    DevArr<uint8_t> d_out;
    DevArr<uint64_t> d_in_off;
    DevArr<uint8_t> d_json;
    DevArr<unsigned long long> d_stats; /* {bails, deeps} since the last dg_ctx_stats reset */
    DevArr<uint64_t> d_zero;            /* 8 zero bytes (device) */
    DevArr<uint32_t> d_pending;
    std::vector<std::unique_ptr<Scratch>> scratch;
    /* dg_j2t_pipeline_host: its per-chunk buffers, kept across calls; pipe_mu
     * serialises pipeline calls */
    std::mutex pipe_mu;
    PinArr<uint8_t> h_pipe_aux, h_pipe_out; /* pinned staging when the caller's buffers are pageable */
    PinArr<uint8_t> h_pipe_ovf;             /* slot overflows per chunk (pinned) */
    DevArr<uint64_t> d_pipe_cur;            /* chunk k's start in out (device) */
    std::vector<std::unique_ptr<PipeBuf, PipeBufDelete>> pipe;
    ~dg_ctx()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

/* What every entry point does first: the null checks (`ok` carries the
 * entry's own), the context lock, the device, the stream's default.
 *   Entry g(c, c && d, stream); if (g.rc) return g.rc; */
struct Entry {
    std::unique_lock<std::mutex> lk;
    hipStream_t s = nullptr;
    int rc = DG_OK;
    Entry(dg_ctx *c, bool ok, void *stream = nullptr, const char *what = "bad args")
    {
        if (!ok) {
            rc = set_err(DG_E_INVALID, "%s", what);
            return;
        }
        lk = std::unique_lock<std::mutex>(c->mu);
        const hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) rc = set_err(DG_E_HIP, "hipSetDevice(c->device): %s", hipGetErrorString(e));
        s = stream ? (hipStream_t)stream : (hipStream_t)c->stream;
    }
};

struct dg_desc {
    dg_ctx *ctx = nullptr;
    DevArr<uint8_t> d_blob;
    DevArr<uint8_t> d_flat;     /* the flat kernel's image (flat_image.h); none when the blob cannot take that kernel */
    size_t len = 0;
    dg_desc_hdr hdr;
    DevArr<uint8_t> d_side;     /* t2j side table (dg_desc_attach_t2j) */
    std::vector<uint8_t> hblob; /* host copy of the blob (launch decisions) */
    size_t side_len = 0;
};

/* a path set on its context's device (tget_host.hip; an edit owns one) */
struct dg_path {
    dg_ctx *ctx;
    DevArr<uint8_t> d_blob;
    dg_path_hdr hdr;
};

/* a plan of typed columns on its context's device: a path set and one kind
 * per path. The column plan (cols_host.hip, DG_COL_* kinds) and the
 * entry-column plan (ents_host.hip, DG_ENT_* kinds) are this record; the
 * opaque types of the C header stay distinct. */
struct PlanRec {
    dg_ctx *ctx;
    DevArr<uint8_t> d_blob;
    dg_path_hdr hdr;
    uint8_t kinds[DG_TGET_MAX_PATHS];
};
struct dg_cols : PlanRec {};
struct dg_ents : PlanRec {};

/* a row-column plan (rows_host.hip): the parent's path set of one path
 * (d_blob, hdr), the sub-paths' set and one DG_COL_* kind per sub-path */
static_assert(DG_ROWS_MAX_COLS == DG_TGET_MAX_PATHS, "a kind per sub-path");
struct dg_rows : PlanRec {
    DevArr<uint8_t> d_sub;
    dg_path_hdr sub_hdr;
    uint32_t key_kind = 0; /* 0: a list plan; DG_ROWS_KEY_*: a map plan (dg_rows_create_map) */
};

/* one batch of messages (device pointers) and where the lookup's records go */
struct TGetBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    dg_tget_rec *rec;
    uint64_t *val_off; /* optional, with val_len */
    uint32_t *val_len;
    uint64_t max_len;
};

/* dg_path_create's checks of a path-set blob (DG_E_ARG with its texts); h =
 * the blob's header */
__attribute__((visibility("hidden"))) int dg_i_path_validate(const void *blob, size_t len, dg_path_hdr &h);

/* the lookup of one batch on stream s (ctx mutex held): tget_host.hip */
__attribute__((visibility("hidden"))) int tget_launch(dg_ctx *c, const dg_path *ps, uint8_t root_type,
                                                      const TGetBatch &b, hipStream_t s);

/* the callback answers of a batch (dg_cb_tables, dgj2t_defs.h): HTTP-mapping
 * entries (DG_F_HM_SPLIT) and value-mapping entries; all null when absent */
struct HMIn {
    const dg_hm_entry *tab = nullptr;
    uint32_t n_hm = 0;
    const uint8_t *bytes = nullptr;
    const dg_cb_entry *vm = nullptr; /* t2j: the answer entries */
};

/* one batch, either direction: device pointers at the launches, host
 * pointers at the host entry points (there `ret` and `aux` are the caller's) */
struct BatchArgs {
    const uint8_t *src = nullptr; /* JSON (j2t), Thrift (t2j) */
    const uint64_t *in_off = nullptr;
    uint64_t n = 0, flags = 0;    /* flags: DG_F_* (j2t), DG_T2J_* options (t2j) */
    uint8_t *out = nullptr;
    const uint64_t *out_off = nullptr;
    uint32_t *out_len = nullptr;
    uint64_t *ret = nullptr;
    uint32_t *pending = nullptr;
    uint64_t max_len = 0;         /* the longest message, 0: unknown */
    HMIn hm;
    uint64_t *aux = nullptr;      /* t2j: per-message response-base spans */
};

/* where a host entry point leaves its results (the caller's pageable memory) */
struct HostOut {
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *out_off, *out_need;
};

/* the optional chaining of a packing (dg_i_convert_pack): positions start at
 * *base_in, bytes past dst_cap are not written (0: no limit); base_mod16 =
 * 1 | phase << 1: positions start at (*base_in + phase) & 15 instead.
 * ret_dst (optional): the status words copied there. cur_out (device,
 * optional): the end position (the next chunk's base). ovf_out (optional,
 * e.g. pinned): the count of DG_ST_OUT_OVERFLOW messages. The packing waits
 * for pack_after (another stream's event) when it is set. */
struct PackChain {
    const uint64_t *base_in = nullptr;
    uint64_t dst_cap = 0;
    int base_mod16 = 0;
    uint64_t *ret_dst = nullptr, *cur_out = nullptr, *ovf_out = nullptr;
    hipEvent_t pack_after = nullptr;
};

/* before streams s[0..n) are destroyed: the device is synchronized, the
 * scratches they own are freed, and nothing shared keeps one of them as the
 * stream of its last launch (takes the ctx mutex) */
__attribute__((visibility("hidden"))) void dg_i_scratch_release(dg_ctx *c, const hipStream_t *s, int n);

/* the scratch for a launch on stream s (ctx mutex held) */
__attribute__((visibility("hidden"))) int scratch_for(dg_ctx *c, hipStream_t s, Scratch **out);

/* one batch converted and packed on stream s (takes the ctx mutex): message
 * i's Thrift at packed + pack_off[i], pack_off[n] = total; failed and
 * overflowed messages pack as nothing (their ret says why). packed /
 * pack_off may be pinned host memory. */
__attribute__((visibility("hidden"))) int dg_i_convert_pack(dg_ctx *c, const dg_desc *d, uint32_t root,
                                                            const BatchArgs &b, uint8_t *packed, uint64_t *pack_off,
                                                            hipStream_t s, const PackChain &ch);

/* dg_pack_device_scan on stream s with the ctx mutex held: b's out / out_off /
 * out_len / n, and with b.ret set the messages whose status is not 0 pack as
 * nothing */
__attribute__((visibility("hidden"))) int dg_i_pack_scan(dg_ctx *c, hipStream_t s, const BatchArgs &b, uint8_t *d_dst,
                                                         uint64_t *d_dst_off);

/* a host array's copy on the device (exact size, at least one element; `spare` zeroed elements behind it) */
template <class T>
inline int to_device(DevArr<T> &d, const T *h, uint64_t count, uint64_t spare = 0)
{
    if (int rc = d.alloc(count + spare + 1)) return rc;
    if (count) HIPCHK(hipMemcpy(d.p, h, count * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d.p + count, 0, (spare + 1) * sizeof(T)));
    return DG_OK;
}

/* the answer of a host entry to n = 0 */
inline int empty_batch(uint64_t *off, uint64_t *need)
{
    if (off) off[0] = 0;
    if (need) *need = 0;
    return DG_OK;
}

/* One batch of a host entry (tget, cut, edit, editm, kids, cols, t2j; j2t's overflow
 * rerun takes copy / sync and the destructor only), made
 * after Entry: the layout (host_layout.h) in vectors it owns, their upload into
 * the context's staging buffers, the packing and the download. Every copy is
 * asynchronous on s and several read io / so / vo, so the destructor
 * synchronises s when a copy was issued and no synchronise has followed it: an
 * entry may return wherever it likes. What a download writes must be declared
 * before the HostBatch (or be the caller's) for the same reason. */
struct HostBatch {
    dg_ctx *const c;
    const hipStream_t s;
    std::vector<uint64_t> io, so, vo, src; /* message, slot and value offsets; a gathering layout's sources */
    uint64_t n = 0, max_len = 0;
    bool busy = false; /* a copy may be in flight */
    HostBatch(dg_ctx *c_, hipStream_t s_) : c(c_), s(s_) {}
    HostBatch(const HostBatch &) = delete;
    ~HostBatch()
    {
        if (busy) (void)hipStreamSynchronize(s);
    }
    int sync()
    {
        busy = false;
        HIPCHK(hipStreamSynchronize(s));
        return DG_OK;
    }
    int copy(void *dst, const void *from, uint64_t bytes, hipMemcpyKind kind)
    {
        busy = true;
        if (bytes) HIPCHK(hipMemcpyAsync(dst, from, bytes, kind, s));
        return DG_OK;
    }
    /* The layout of the messages idx[0..m) of the caller's in_off (idx null: of
     * all m, which also sets max_len), each with a slot of cap_of(i, len)
     * bytes when with_slots. A gather (idx) is of an in_off an earlier layout
     * has checked. */
    template <class F>
    int layout(const uint64_t *in_off, const uint64_t *idx, uint64_t m, F cap_of, bool with_slots = true,
               bool longest = true)
    {
        n = m, io.resize(m + 1), src.resize(idx ? m : 0);
        if (with_slots) so.resize(m + 1);
        uint64_t bad = 0, cap = 0;
        const int rc = dg::hl_layout(in_off, idx, m, cap_of, io.data(), with_slots ? so.data() : nullptr,
                                     idx ? src.data() : nullptr, longest && !idx ? &max_len : nullptr, &bad, &cap);
        if (rc == dg::HL_DESCENDING) return set_err(DG_E_INVALID, "in_off not ascending");
        if (rc) return set_err(DG_E_INVALID, "message %llu: an output of %llu bytes", (unsigned long long)bad,
                               (unsigned long long)cap);
        return DG_OK;
    }
    /* no slots: tget and kids write records; kids has no use for max_len either */
    int messages(const uint64_t *in_off, uint64_t m, bool longest = true)
    {
        return layout(in_off, nullptr, m, [](uint64_t, uint64_t) { return uint64_t(0); }, false, longest);
    }
    /* vo[m K + 1] and max_val[K] from the val_off of m messages, message-major */
    int values(const uint64_t *val_off, uint64_t m, uint64_t K, uint64_t *max_val)
    {
        vo.resize(m * K + 1);
        return dg::hl_rebase(val_off, m * K, K, vo.data(), max_val) ? set_err(DG_E_INVALID, "val_off not ascending") : DG_OK;
    }
    /* d_json: the messages and 64 zero bytes, d_in_off: io. The arena in one
     * copy from in_off[0], or after a gathering layout message by message. */
    int upload_messages(const uint8_t *thrift, const uint64_t *in_off)
    {
        int rc;
        if ((rc = c->d_json.grow(io[n] + 64)) || (rc = c->d_in_off.grow(n + 1))) return rc;
        if (src.empty()) rc = copy(c->d_json, thrift + in_off[0], io[n], hipMemcpyHostToDevice);
        for (uint64_t k = 0; k < src.size() && !rc; k++)
            rc = copy(c->d_json + io[k], thrift + src[k], io[k + 1] - io[k], hipMemcpyHostToDevice);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(c->d_json + io[n], 0, 64, s));
        return copy(c->d_in_off, io.data(), (n + 1) * 8, hipMemcpyHostToDevice);
    }
    /* the output side: the slots, their lengths and status words, and for an
     * entry that packs on the device (all but t2j) the packing */
    int upload_slots(bool packs = true)
    {
        int rc;
        if ((rc = c->d_out.grow(so[n] + 64)) || (rc = c->d_out_off.grow(n + 1)) || (rc = c->d_out_len.grow(n + 1)) ||
            (rc = c->d_ret.grow(n + 1)) ||
            (packs && ((rc = c->d_pack.grow(so[n] + 64)) || (rc = c->d_pack_off.grow(n + 1)))))
            return rc;
        return copy(c->d_out_off, so.data(), (n + 1) * 8, hipMemcpyHostToDevice);
    }
    /* d_cb: the values and 64 zero bytes. With val_off (after values()) those
     * it spans and d_aux: vo; without, val[0, shared) for every message */
    int upload_values(const uint8_t *val, const uint64_t *val_off, uint64_t shared)
    {
        const uint64_t vtotal = val_off ? vo.back() : shared;
        int rc;
        if ((rc = c->d_cb.grow(vtotal + 64)) || (rc = c->d_aux.grow(vo.size())) ||
            (rc = copy(c->d_cb, val_off ? val + val_off[0] : val, vtotal, hipMemcpyHostToDevice)))
            return rc;
        HIPCHK(hipMemsetAsync(c->d_cb + vtotal, 0, 64, s));
        return copy(c->d_aux, vo.data(), vo.size() * 8, hipMemcpyHostToDevice);
    }
    /* the slots packed into d_pack / d_pack_off: by the lengths, or with by_ret
     * only the messages of status 0; then the status words, the packed
     * offsets and (optional) the lengths on the host */
    int pack(bool by_ret, uint64_t *ret, uint64_t *pack_off, uint32_t *len = nullptr)
    {
        BatchArgs pb;
        pb.out = c->d_out, pb.out_off = c->d_out_off, pb.out_len = c->d_out_len, pb.n = n;
        if (by_ret) pb.ret = c->d_ret;
        int rc;
        if ((rc = dg_i_pack_scan(c, s, pb, c->d_pack, c->d_pack_off)) ||
            (rc = copy(ret, c->d_ret, n * 8, hipMemcpyDeviceToHost)) ||
            (len && (rc = copy(len, c->d_out_len, n * 4, hipMemcpyDeviceToHost))) ||
            (rc = copy(pack_off, c->d_pack_off, (n + 1) * 8, hipMemcpyDeviceToHost)))
            return rc;
        return sync();
    }
    int download(void *dst, const void *d_from, uint64_t bytes)
    {
        if (int rc = copy(dst, d_from, bytes, hipMemcpyDeviceToHost)) return rc;
        return bytes ? sync() : DG_OK;
    }
    /* the packing goes by the lengths: 0 for every failed message (no slot can overflow) */
    int pack_and_download(const HostOut &o, uint64_t *ret)
    {
        if (int rc = pack(false, ret, o.out_off)) return rc;
        const uint64_t total = o.out_off[n];
        if (o.out_need) *o.out_need = total;
        if (total > o.out_cap || (!o.out && total))
            return set_err(DG_E_NOMEM, "output needs %llu bytes", (unsigned long long)total);
        return download(o.out, c->d_pack, total);
    }
};

/* a plan's blob on the device with 16 zero bytes after it (keys and literals
 * are read 16 bytes at a time) */
inline int upload_blob(DevArr<uint8_t> &d, const void *blob, size_t len, const char *what)
{
    if (int rc = d.alloc(len + 16)) return rc;
    hipError_t e = hipMemcpy(d, blob, len, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d + len, 0, 16);
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* before launches on non-blocking streams read it */
    if (e != hipSuccess) return set_err(DG_E_HIP, "%s upload: %s", what, hipGetErrorString(e));
    return DG_OK;
}

/* the end of a plan (dg_path, dg_cut, dg_cols, dg_ents, dg_rows): its blobs go
 * under the context lock, on its device */
inline void reset_blobs(dg_rows &p) { p.d_blob.reset(), p.d_sub.reset(); }
template <class P>
void reset_blobs(P &p) { p.d_blob.reset(); }
template <class P>
void destroy_with_blob(P *p)
{
    if (!p) return;
    {
        Entry g(p->ctx, true);
        reset_blobs(*p);
    }
    delete p;
}

/* what a SET can add to a message besides the value, by the last step's kind */
inline uint32_t edit_step_extra(uint32_t kind, uint32_t key_len)
{
    return kind == DG_PS_FIELD ? 3u : kind == DG_PS_INDEX ? 0u : kind == DG_PS_STRKEY ? 4u + key_len
           : kind == DG_PS_BINKEY ? key_len : 8u;
}

/* The splice of edit and editm: lane(lanes per message), then wave(blocks of
 * `waves` waves, a message each). A route no message can take is not launched:
 * the lane route when edit_wave_min is 0, the wave route when the caller's
 * hints bound every output below edit_wave_min (no_wave). */
template <class Lane, class Wave>
hipError_t launch_splice_routes(const dg_ctx *c, uint64_t n, uint32_t waves, bool no_wave, Lane lane, Wave wave)
{
    hipError_t err = hipSuccess;
    if (c->knobs.edit_wave_min > 0) {
        const int64_t g = c->knobs.edit_lanes;
        lane(g == 4 || g == 16 ? (uint32_t)g : 1u);
        err = hipGetLastError();
    }
    if (err == hipSuccess && !no_wave) {
        const uint64_t want = (n + waves - 1) / waves;
        wave((uint32_t)std::min<uint64_t>(want, (uint64_t)c->n_cu * 8));
        err = hipGetLastError();
    }
    return err;
}
