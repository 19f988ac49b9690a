/*
 * cut_host.hip — the C ABI of batched MarshalTo (include/dgj2t.h dg_cut_*; the
 * reference's thrift/generic Value.MarshalTo). Kernels: cut_device.h.
 */
#include <string.h>

#include "cut_device.h"
#include "host_internal.h"

using namespace dg;

struct dg_cut {
    dg_ctx *ctx;
    DevArr<uint8_t> d_blob;
    dg_cut_hdr hdr;
};

/* the blob's tables, checked entry by entry: the kernels read them unchecked */
static int cut_validate(const uint8_t *b, size_t len, dg_cut_hdr &h)
{
    if (len < sizeof(dg_cut_hdr)) return set_err(DG_E_ARG, "cut plan of %zu bytes: no header", len);
    memcpy(&h, b, sizeof h);
    if (h.magic != DG_CUT_MAGIC || h.version != DG_CUT_VERSION)
        return set_err(DG_E_ARG, "cut plan: bad magic or version (%08x, %u)", h.magic, h.version);
    const uint64_t e_nodes = (uint64_t)h.off_nodes + (uint64_t)h.n_nodes * sizeof(dg_cut_node),
                   e_fields = (uint64_t)h.off_fields + (uint64_t)h.n_fields * sizeof(dg_cut_field),
                   e_lits = (uint64_t)h.off_lits + (uint64_t)h.n_lits * sizeof(dg_cut_lit);
    if (h.total_len > len || ((h.off_nodes | h.off_fields | h.off_lits | h.off_pool) & 7) ||
        h.off_nodes < sizeof(dg_cut_hdr) || e_nodes > h.off_fields || e_fields > h.off_lits || e_lits > h.off_pool ||
        (uint64_t)h.off_pool + h.pool_len != h.total_len || h.n_nodes < 1 || h.root >= h.n_nodes)
        return set_err(DG_E_ARG, "cut plan: tables outside the blob");
    uint64_t max_unset = 0;
    for (uint32_t k = 0; k < h.n_nodes; k++) {
        dg_cut_node N;
        memcpy(&N, b + h.off_nodes + (uint64_t)k * sizeof N, sizeof N);
        bool ok = true;
        if (N.kind == DG_CUT_COPY) ok = N.a < 256;
        else if (N.kind == DG_CUT_MISMATCH) ok = true;
        else if (N.kind == DG_CUT_LIST) ok = N.a < h.n_nodes;
        else if (N.kind == DG_CUT_MAP) ok = N.a < h.n_nodes && N.b < h.n_nodes;
        else if (N.kind == DG_CUT_STRUCT) {
            ok = (uint64_t)N.a + N.n_fields <= h.n_fields && (uint64_t)N.lit0 + N.n_lits <= h.n_lits && N.n_lits <= 64 &&
                 N.tracked == (N.n_lits == 64 ? ~0ull : (1ull << N.n_lits) - 1) && !(N.required & ~N.tracked);
            uint64_t unset = 0;
            for (uint32_t j = 0; ok && j < N.n_lits; j++) {
                dg_cut_lit L;
                memcpy(&L, b + h.off_lits + (uint64_t)(N.lit0 + j) * sizeof L, sizeof L);
                ok = (uint64_t)L.off + L.len <= h.pool_len && !((N.required >> j & 1) && L.len);
                unset += L.len;
            }
            max_unset = std::max(max_unset, unset);
            for (uint32_t j = 0; ok && j < N.n_fields; j++) {
                dg_cut_field F, G;
                memcpy(&F, b + h.off_fields + (uint64_t)(N.a + j) * sizeof F, sizeof F);
                if (j) {
                    memcpy(&G, b + h.off_fields + (uint64_t)(N.a + j - 1) * sizeof G, sizeof G);
                    ok = G.id < F.id;
                }
                ok = ok && (F.child == DG_CUT_DROP || F.child < h.n_nodes) &&
                     (F.bit == DG_CUT_NO_BIT || F.bit < N.n_lits);
            }
        } else
            ok = false;
        if (!ok) return set_err(DG_E_ARG, "cut plan: node %u breaks the layout", k);
    }
    if (max_unset != h.max_unset) return set_err(DG_E_ARG, "cut plan: max_unset %u, the tables give %llu", h.max_unset,
                                                 (unsigned long long)max_unset);
    return DG_OK;
}

/* one batch of messages (device pointers) and its slots */
struct CutBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint64_t *ret;
    uint64_t max_len;
};

/* one batch on stream s (ctx mutex held): the lane route over the whole batch,
 * then the wave route over what it queued, back to back, on the component's
 * pass state (a queue and its counters, no frames). */
static int cut_launch(dg_ctx *c, const dg_cut *pl, uint64_t opts, const CutBatch &b, hipStream_t s)
{
    const uint64_t n = b.n;
    if (n == 0) return DG_OK;
    if (!b.src || !b.in_off || !b.out || !b.out_off || !b.out_len || !b.ret) return set_err(DG_E_INVALID, "null buffer");
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    if (opts & ~(DG_CUT_WRITE_DEFAULT | DG_CUT_DISALLOW_UNKNOWN | DG_CUT_NOT_CHECK_REQ))
        return set_err(DG_E_INVALID, "unknown cut option bits %llx", (unsigned long long)opts);
    PassState &st = c->cut;
    int rc;
    if ((rc = st.first_use(0, 1)) || (rc = st.room(n))) return rc;
    CutParams A;
    memset(&A, 0, sizeof A);
    const uint8_t *blob = pl->d_blob;
    A.plan.nodes = (const dg_cut_node *)(const void *)(blob + pl->hdr.off_nodes);
    A.plan.fields = (const dg_cut_field *)(const void *)(blob + pl->hdr.off_fields);
    A.plan.lits = (const dg_cut_lit *)(const void *)(blob + pl->hdr.off_lits);
    A.plan.pool = blob + pl->hdr.off_pool;
    A.plan.root = pl->hdr.root;
    A.blob = blob, A.tab_len = pl->hdr.off_pool;
    A.off_nodes = pl->hdr.off_nodes, A.off_fields = pl->hdr.off_fields, A.off_lits = pl->hdr.off_lits;
    A.opts = opts;
    A.src = b.src, A.in_off = b.in_off, A.n = n;
    A.out = b.out, A.out_off = b.out_off, A.out_len = b.out_len, A.ret = b.ret;
    A.wave_min = c->knobs.cut_wave_min < 0 ? 0 : (uint64_t)c->knobs.cut_wave_min;
    A.wave_list = st.list;
    (void)b.max_len; /* a hint no route reads today: both kernels always run */
    return st.enqueue(s, "cut", [&] {
        return st.pass(s, [&](uint32_t *mine, uint32_t *other) {
            A.wave_count = mine, A.reset_count = other;
            launch_cut_lane(s, A);
            if (hipPeekAtLastError() != hipSuccess) return;
            /* a fixed grid striding over the queue, a wave per message: enough
             * waves to fill the device, no more blocks than the batch could queue */
            const uint64_t want = (n + CUT_WAVES - 1) / CUT_WAVES;
            launch_cut_wave(s, A, (uint32_t)std::min<uint64_t>(want, (uint64_t)c->n_cu * 4));
        });
    });
}

extern "C" {

int dg_cut_create(dg_ctx *c, const void *blob, size_t len, dg_cut **out)
{
    if (!c || !blob || !out) return set_err(DG_E_INVALID, "null ctx/blob/out");
    dg_cut_hdr h;
    if (int rc = cut_validate((const uint8_t *)blob, len, h)) return rc;
    Entry g(c, true);
    if (g.rc) return g.rc;
    std::unique_ptr<dg_cut> pl(new dg_cut());
    pl->ctx = c;
    pl->hdr = h;
    if (int rc = upload_blob(pl->d_blob, blob, h.total_len, "cut plan")) return rc;
    *out = pl.release();
    return DG_OK;
}

void dg_cut_destroy(dg_cut *p) { destroy_with_blob(p); }

uint64_t dg_cut_slot_bound(const dg_cut *p, uint64_t len, uint64_t opts)
{
    if (!p) return 0;
    const bool lits = (opts & DG_CUT_WRITE_DEFAULT) && !(opts & DG_CUT_NOT_CHECK_REQ) && p->hdr.max_unset;
    return lits ? len * (1 + (uint64_t)p->hdr.max_unset) : len;
}

int dg_cut_batch_device(dg_ctx *c, const dg_cut *pl, uint64_t opts, const uint8_t *d_thrift, const uint64_t *d_in_off,
                        uint64_t n, uint8_t *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                        void *stream, uint64_t max_len)
{
    Entry g(c, c && pl && pl->ctx == c, stream, "null ctx/plan, or a plan of another context");
    if (g.rc) return g.rc;
    return cut_launch(c, pl, opts, CutBatch{d_thrift, d_in_off, n, d_out, d_out_off, d_out_len, d_ret, max_len}, g.s);
}

/* pass 0: every message in a slot of min(dg_cut_slot_bound, its length + 256)
 * bytes (the bound is a worst case: a struct per byte, each with every literal);
 * pass 1: the overflowed ones again, each in a slot of the size it reported.
 * Each pass packs its results on the device and downloads exactly those. */
int dg_cut_batch_host(dg_ctx *c, const dg_cut *pl, uint64_t opts, const uint8_t *thrift, const uint64_t *in_off,
                      uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need)
{
    if (!c || !pl || pl->ctx != c) return set_err(DG_E_INVALID, "null ctx/plan, or a plan of another context");
    if (n == 0) return empty_batch(out_off, out_need);
    if (!thrift || !in_off || !out_off || !ret) return set_err(DG_E_INVALID, "null buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    /* what a pass downloads into is declared before the batch, whose destructor waits for the copies */
    std::vector<uint64_t> todo, where(n, 0), po, r;
    std::vector<uint32_t> olen(n, 0), l;
    std::vector<uint8_t> stage;
    HostBatch hb(c, g.s);
    int rc;
    for (int pass = 0; pass < 2 && (pass == 0 || !todo.empty()); pass++) {
        const uint64_t m = pass ? todo.size() : n;
        po.resize(m + 1), r.resize(m), l.resize(m);
        if ((rc = hb.layout(in_off, pass ? todo.data() : nullptr, m, [&](uint64_t i, uint64_t len) -> uint64_t {
                return pass == 0 ? std::min(dg_cut_slot_bound(pl, len, opts), len + 256) : olen[i];
            })) ||
            (rc = hb.upload_messages(thrift, in_off)) || (rc = hb.upload_slots()))
            return rc;
        const CutBatch b{c->d_json, c->d_in_off, m, c->d_out, c->d_out_off, c->d_out_len, c->d_ret, hb.max_len};
        /* the packing goes by ret: only status 0 packs */
        if ((rc = cut_launch(c, pl, opts, b, g.s)) || (rc = hb.pack(true, r.data(), po.data(), l.data()))) return rc;
        const uint64_t off0 = stage.size();
        stage.resize(off0 + po[m]);
        if ((rc = hb.download(stage.data() + off0, c->d_pack, po[m]))) return rc;
        std::vector<uint64_t> next;
        for (uint64_t k = 0; k < m; k++) {
            const uint64_t i = pass ? todo[k] : k;
            ret[i] = r[k];
            olen[i] = l[k];
            where[i] = off0 + po[k];
            if ((uint8_t)r[k] == DG_CUT_E_OVERFLOW) {
                if (pass == 1)
                    return set_err(DG_E_NOMEM, "message %llu overflowed its exact-size slot", (unsigned long long)i);
                next.push_back(i);
            }
        }
        todo.swap(next);
    }
    uint64_t total = 0;
    out_off[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (ret[i] != 0) olen[i] = 0; /* the reference returns no bytes on error */
        total += olen[i];
        out_off[i + 1] = total;
    }
    if (out_need) *out_need = total;
    if (total > out_cap || (!out && total)) return set_err(DG_E_NOMEM, "output needs %llu bytes", (unsigned long long)total);
    for (uint64_t i = 0; i < n; i++)
        if (olen[i]) memcpy(out + out_off[i], stage.data() + where[i], olen[i]);
    return DG_OK;
}

}  // extern "C"
