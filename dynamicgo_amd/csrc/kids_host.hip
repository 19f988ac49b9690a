/*
 * kids_host.hip — the C ABI of batched Children (include/dgj2t.h dg_kids_*; the
 * reference's thrift/generic Node.Children behind GetByPath). Kernels:
 * kids_device.h, kids_kern.hip.
 */
#include <string.h>

#include "host_internal.h"
#include "kids_device.h"

using namespace dg;

static const uint64_t KIDS_WS = (uint64_t)2 * KD_DEEP_DEPTH * KD_DEEP_LANES * 8;

/* one batch (device pointers) */
struct KidsBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    dg_kids_head *head;
    uint64_t *rec_off;
    dg_kid_rec *recs;
    uint64_t rec_cap;
};

/* one batch on stream s (ctx mutex held): count pass -> scan -> emit pass,
 * each pass followed by its deep pass, the emit pass by the wide kernel, on the
 * component's pass state (the counter sets alternate per pass). */
static int kids_launch(dg_ctx *c, const dg_path *ps, uint8_t root_type, uint32_t flags, const KidsBatch &b, hipStream_t s)
{
    const uint64_t n = b.n;
    if (n == 0) return DG_OK;
    if (!b.src || !b.in_off || !b.head || !b.rec_off) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)b.head & 15) || ((uintptr_t)b.recs & 15) || ((uintptr_t)b.rec_off & 7))
        return set_err(DG_E_INVALID, "heads or records not 16-byte aligned"); /* 16-byte stores */
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    if (flags & ~(DG_KIDS_F_RECURSE | DG_KIDS_F_COUNTED)) return set_err(DG_E_INVALID, "unknown flags %x", flags);
    PassState &st = c->kids;
    int rc;
    /* the queue: the deep and the wide one; a counter set: {deep, wide} */
    if ((rc = st.first_use(KIDS_WS, 2)) || (rc = st.room(2 * n, (n + SCAN_TILE - 1) / SCAN_TILE))) return rc;
    KDParams A;
    memset(&A, 0, sizeof A);
    A.tg.src = b.src, A.tg.in_off = b.in_off, A.tg.root_type = root_type;
    A.tg.blob = ps->d_blob, A.tg.off_steps = ps->hdr.off_steps, A.tg.off_pool = ps->hdr.off_pool;
    A.n = n;
    A.n_steps = ps->hdr.n_steps; /* one path: all the steps are its own */
    A.recurse = flags & DG_KIDS_F_RECURSE ? 1u : 0u;
    A.head = b.head, A.rec_off = b.rec_off, A.recs = b.recs, A.rec_cap = b.rec_cap;
    A.wide_min = c->knobs.kids_wide_min < 0 ? 0 : (uint64_t)c->knobs.kids_wide_min;
    A.deep_list = st.list, A.wide_list = st.list + n;
    A.ws = (uint64_t *)(void *)st.ws;
    A.stats = c->d_stats;
    return st.enqueue(s, "kids", [&] {
        hipError_t e = hipSuccess;
        if (!(flags & DG_KIDS_F_COUNTED)) {
            e = st.pass(s, [&](uint32_t *mine, uint32_t *other) {
                A.cnt = mine, A.reset = other;
                launch_kids_count(s, A);
            });
            if (e == hipSuccess && c->knobs.kids_no_scan != 1) { /* the knob: time the count pass alone */
                launch_kids_scan(s, A, st.sums);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess && b.recs)
            e = st.pass(s, [&](uint32_t *mine, uint32_t *other) {
                A.cnt = mine, A.reset = other;
                launch_kids_emit(s, A, (uint32_t)std::max(c->n_cu, 1) * 4u);
            });
        return e;
    });
}

static int kids_args(const dg_ctx *c, const dg_path *ps)
{
    if (!c || !ps || ps->ctx != c) return set_err(DG_E_INVALID, "null ctx/path, or a path of another context");
    if (ps->hdr.n_paths != 1) return set_err(DG_E_ARG, "children: %u paths (exactly 1)", ps->hdr.n_paths);
    return DG_OK;
}

extern "C" {

int dg_kids_batch_device(dg_ctx *c, const dg_path *ps, uint8_t root_type, uint32_t flags, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, dg_kids_head *d_head, uint64_t *d_rec_off,
                         dg_kid_rec *d_recs, uint64_t rec_cap, void *stream, uint64_t max_len)
{
    if (int rc = kids_args(c, ps)) return rc;
    (void)max_len; /* one lane route at every length today */
    Entry g(c, true, stream);
    if (g.rc) return g.rc;
    return kids_launch(c, ps, root_type, flags, KidsBatch{d_thrift, d_in_off, n, d_head, d_rec_off, d_recs, rec_cap}, g.s);
}

int dg_kids_batch_host(dg_ctx *c, const dg_path *ps, uint8_t root_type, uint32_t flags, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, dg_kids_head *head, uint64_t *rec_off, dg_kid_rec *recs,
                       uint64_t rec_cap, uint64_t *need)
{
    if (int rc = kids_args(c, ps)) return rc;
    if (flags & DG_KIDS_F_COUNTED) return set_err(DG_E_INVALID, "DG_KIDS_F_COUNTED is the device entry's");
    if (n == 0) return empty_batch(rec_off, need);
    if (!thrift || !in_off || !head || !rec_off) return set_err(DG_E_INVALID, "null buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    const hipStream_t s = g.s;
    HostBatch hb(c, s);
    int rc;
    if ((rc = hb.messages(in_off, n, false)) || (rc = c->d_aux.grow(2 * n + 2)) || (rc = c->d_ret.grow(n + 1)) ||
        (rc = hb.upload_messages(thrift, in_off)))
        return rc;
    dg_kids_head *d_head = (dg_kids_head *)(void *)c->d_aux.p;
    KidsBatch b{c->d_json, c->d_in_off, n, d_head, c->d_ret, nullptr, 0};
    if ((rc = kids_launch(c, ps, root_type, flags, b, s)) || /* count and scan */
        (rc = hb.copy(rec_off, c->d_ret, (n + 1) * 8, hipMemcpyDeviceToHost)) ||
        (rc = hb.download(head, d_head, n * sizeof(dg_kids_head))))
        return rc;
    const uint64_t want = rec_off[n];
    if (need) *need = want;
    if (!recs && !rec_cap) return DG_OK; /* sizing */
    if (want > rec_cap || (!recs && want)) return set_err(DG_E_NOMEM, "children need %llu records", (unsigned long long)want);
    if (!want) return DG_OK;
    if ((rc = c->d_out.grow(want * sizeof(dg_kid_rec) + 64))) return rc;
    b.recs = (dg_kid_rec *)(void *)c->d_out.p, b.rec_cap = want;
    if ((rc = kids_launch(c, ps, root_type, flags | DG_KIDS_F_COUNTED, b, s))) return rc;
    return hb.download(recs, c->d_out, want * sizeof(dg_kid_rec));
}

}  // extern "C"
