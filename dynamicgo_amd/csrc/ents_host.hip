/*
 * ents_host.hip — the C ABI of entry columns (include/dgj2t.h dg_ents_*; the
 * reference's Node.List of strings, Node.StrMap and Node.IntMap behind
 * GetByPath, cast.go:198-286). Kernels: ents_device.h, ents_kern.hip.
 */
#include <string.h>

#include "ents_device.h"
#include "plan_internal.h"

using namespace dg;

static const uint64_t ENTS_WS = (uint64_t)TG_DEEP_DEPTH * TG_DEEP_LANES * 8;

static bool ent_kind_ok(uint32_t kind)
{
    if (kind == DG_ENT_LISTSTR) return true;
    const uint32_t c = kind & ~15u, v = kind & 15u;
    return (c == DG_ENT_STRMAP || c == DG_ENT_INTMAP) &&
           (v == DG_ENT_BOOL || v == DG_ENT_INT || v == DG_ENT_F64 || v == DG_ENT_STR);
}
static bool kind_str_key(uint32_t kind) { return (kind & DG_ENT_STRMAP) != 0; }
static bool kind_str_val(uint32_t kind) { return kind == DG_ENT_LISTSTR || (kind & 15u) == DG_ENT_STR; }

static const PlanKinds ENTS_KINDS{ent_kind_ok, "ents", "paths", "entry kind"};

/* one batch (device pointers) */
struct EntsBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    uint64_t *val;
    dg_col_cell *cell;
    uint32_t *len, *span;
};

/* column k's parts of a cell pass's outputs and where its entries go */
struct EntsEmit {
    const uint64_t *val;
    const dg_col_cell *cell;
    const uint32_t *len, *span;
    uint64_t *off, *key;
    uint32_t *klen;
    uint64_t *v;
    uint32_t *vlen;
    uint64_t cap;
};

/* the cell pass of one batch on stream s (ctx mutex held), on the component's
 * pass state */
static int ents_launch(dg_ctx *c, const dg_ents *ep, uint8_t root_type, const EntsBatch &b, hipStream_t s)
{
    const uint64_t n = b.n, P = ep->hdr.n_paths;
    if (n == 0) return DG_OK;
    if (!b.src || !b.in_off || !b.val || !b.cell || !b.len || !b.span) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)b.val & 7) || ((uintptr_t)b.cell & 7) || ((uintptr_t)b.len & 3) || ((uintptr_t)b.span & 3))
        return set_err(DG_E_INVALID, "values or cells not 8-byte aligned"); /* one store each */
    const uint64_t pairs = n * P;
    if (n > 0xFFFFFFFFull || pairs > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %llu columns", (unsigned long long)n, (unsigned long long)P);
    PassState &st = c->ents;
    int rc;
    if ((rc = st.first_use(ENTS_WS, 1)) || (rc = st.room(pairs))) return rc;
    ENParams A;
    memset(&A, 0, sizeof A);
    A.tg.src = b.src, A.tg.in_off = b.in_off, A.tg.pairs = pairs, A.tg.P = (uint32_t)P, A.tg.root_type = root_type;
    A.tg.blob = ep->d_blob, A.tg.off_steps = ep->hdr.off_steps, A.tg.off_pool = ep->hdr.off_pool;
    A.tg.deep_list = st.list;
    A.tg.ws = (uint64_t *)(void *)st.ws;
    A.n = n, A.kinds = pack_kinds(ep->kinds, P);
    A.val = b.val, A.cell = (uint64_t *)(void *)b.cell, A.len = b.len, A.span = b.span;
    return st.enqueue(s, "ents", [&] {
        return st.pass(s, [&](uint32_t *mine, uint32_t *other) {
            A.tg.deep_count = mine, A.tg.reset_count = other;
            launch_ents_pass(s, A);
        });
    });
}

/* column k's scan and (with an output array and a capacity) emit on stream s
 * (ctx mutex held); the tile sums are the pass state's */
static int ents_emit_launch(dg_ctx *c, const dg_ents *ep, uint32_t k, const uint8_t *src, uint64_t n, const EntsEmit &o,
                            hipStream_t s)
{
    if (k >= ep->hdr.n_paths) return set_err(DG_E_ARG, "column %u of a plan of %u", k, ep->hdr.n_paths);
    if (!o.off) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)o.off & 7) || ((uintptr_t)o.key & 7) || ((uintptr_t)o.v & 7) || ((uintptr_t)o.klen & 3) ||
        ((uintptr_t)o.vlen & 3))
        return set_err(DG_E_INVALID, "offsets or entries not aligned");
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    if (n == 0) { /* the total, so that a reader of d_ent_off[n] finds 0 */
        HIPCHK(hipMemsetAsync(o.off, 0, 8, s));
        return DG_OK;
    }
    if (!src || !o.val || !o.cell || !o.len || !o.span) return set_err(DG_E_INVALID, "null buffer");
    PassState &st = c->ents;
    if (int rc = st.grow(st.sums, (n + SCAN_TILE - 1) / SCAN_TILE)) return rc;
    return st.enqueue(s, "ents emit", [&] {
        launch_cols_scan(s, o.len, n, st.sums, o.off);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && (o.key || o.klen || o.v || o.vlen) && o.cap) {
            /* an array the kind has nothing for is not touched */
            const uint32_t kind = ep->kinds[k];
            const ENEmit E{src, n, o.val, (const uint64_t *)(const void *)o.cell, o.len, o.span, o.off,
                           kind == DG_ENT_LISTSTR ? nullptr : o.key, kind_str_key(kind) ? o.klen : nullptr, o.v,
                           kind_str_val(kind) ? o.vlen : nullptr, o.cap, kind};
            const int64_t stage = c->knobs.ents_stage;
            launch_ents_emit(s, E, (uint32_t)std::max(c->n_cu, 1) * 8u,
                             stage == 4 || stage == 8 || stage == 16 ? (uint32_t)stage : 0u);
            e = hipGetLastError();
        }
        return e;
    });
}

extern "C" {

int dg_ents_create(dg_ctx *c, const void *blob, size_t len, const uint8_t *kinds, uint32_t n_kinds, dg_ents **out)
{
    return plan_create(c, blob, len, kinds, n_kinds, ENTS_KINDS, out);
}

void dg_ents_destroy(dg_ents *p) { destroy_with_blob(p); }

uint32_t dg_ents_count(const dg_ents *p) { return p ? p->hdr.n_paths : 0; }

int dg_ents_batch_device(dg_ctx *c, const dg_ents *ep, uint8_t root_type, const uint8_t *d_thrift, const uint64_t *d_in_off,
                         uint64_t n, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len, uint32_t *d_span, void *stream,
                         uint64_t max_len)
{
    (void)max_len; /* dense lanes at every length, as the lookup measured */
    Entry g(c, c && ep && ep->ctx == c, stream, "null ctx/entry columns, or entry columns of another context");
    if (g.rc) return g.rc;
    return ents_launch(c, ep, root_type, EntsBatch{d_thrift, d_in_off, n, d_val, d_cell, d_len, d_span}, g.s);
}

int dg_ents_emit_device(dg_ctx *c, const dg_ents *ep, uint32_t k, const uint8_t *d_thrift, uint64_t n,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k,
                        const uint32_t *d_span_k, uint64_t *d_ent_off, uint64_t *d_key, uint32_t *d_key_len, uint64_t *d_val,
                        uint32_t *d_val_len, uint64_t ent_cap, void *stream)
{
    Entry g(c, c && ep && ep->ctx == c, stream, "null ctx/entry columns, or entry columns of another context");
    if (g.rc) return g.rc;
    return ents_emit_launch(c, ep, k, d_thrift, n,
                            EntsEmit{d_val_k, d_cell_k, d_len_k, d_span_k, d_ent_off, d_key, d_key_len, d_val, d_val_len, ent_cap},
                            g.s);
}

int dg_ents_batch_host(dg_ctx *c, const dg_ents *ep, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, uint64_t *val, dg_col_cell *cell, uint32_t *len, uint64_t *ent_off, uint64_t *key,
                       uint32_t *key_len, uint64_t *ent_val, uint32_t *ent_val_len, uint64_t ent_cap, uint64_t *need)
{
    if (!c || !ep || ep->ctx != c) return set_err(DG_E_INVALID, "null ctx/entry columns, or entry columns of another context");
    const uint64_t P = ep->hdr.n_paths;
    if (!ent_off) return set_err(DG_E_INVALID, "null buffer");
    if (n == 0) {
        for (uint64_t k = 0; k < P; k++) ent_off[k] = 0;
        if (need) *need = 0;
        return DG_OK;
    }
    if (!thrift || !in_off || !val || !cell || !len) return set_err(DG_E_INVALID, "null buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    const hipStream_t s = g.s;
    HostBatch hb(c, s);
    const uint64_t cells = n * P;
    int rc;
    /* d_out: values, cells, lengths, spans; d_ret: the columns' offsets; d_pack: the entries */
    if ((rc = hb.messages(in_off, n, false)) || (rc = c->d_out.grow(cells * 24 + 64)) ||
        (rc = c->d_ret.grow(P * (n + 1) + 1)) || (rc = hb.upload_messages(thrift, in_off)))
        return rc;
    uint64_t *d_val = (uint64_t *)(void *)c->d_out.p;
    dg_col_cell *d_cell = (dg_col_cell *)(void *)(d_val + cells);
    uint32_t *d_len = (uint32_t *)(void *)(d_cell + cells), *d_span = d_len + cells;
    if ((rc = ents_launch(c, ep, root_type, EntsBatch{c->d_json, c->d_in_off, n, d_val, d_cell, d_len, d_span}, s))) return rc;
    const auto emit_of = [&](uint64_t k) {
        const uint64_t at = k * n;
        return EntsEmit{d_val + at, d_cell + at, d_len + at, d_span + at, c->d_ret + k * (n + 1), nullptr, nullptr, nullptr,
                        nullptr,    0};
    };
    for (uint64_t k = 0; k < P && !rc; k++) rc = ents_emit_launch(c, ep, (uint32_t)k, c->d_json, n, emit_of(k), s); /* sizing */
    if (rc || (rc = hb.copy(val, d_val, cells * 8, hipMemcpyDeviceToHost)) ||
        (rc = hb.copy(cell, d_cell, cells * 8, hipMemcpyDeviceToHost)) ||
        (rc = hb.copy(ent_off, c->d_ret, P * (n + 1) * 8, hipMemcpyDeviceToHost)) || (rc = hb.download(len, d_len, cells * 4)))
        return rc;
    /* offsets relative to the caller's arena: the upload began at in_off[0] */
    for (uint64_t i = 0; i < cells; i++)
        if (cell[i].status == DG_TGET_OK) val[i] += in_off[0];
    const std::vector<uint64_t> base = chain_columns(ent_off, P, n); /* the columns' entries one after the other */
    const uint64_t want = base[P];
    if (need) *need = want;
    const bool any = key || key_len || ent_val || ent_val_len;
    if (!any && !ent_cap) return DG_OK; /* sizing */
    if (want > ent_cap || (!any && want)) return set_err(DG_E_NOMEM, "entry columns need %llu entries", (unsigned long long)want);
    if (!want) return DG_OK;
    /* d_pack: keys, values (8 bytes a slot), then their lengths (4 a slot); zero where a kind writes nothing */
    if ((rc = c->d_pack.grow(want * 24 + 64))) return rc;
    HIPCHK(hipMemsetAsync(c->d_pack, 0, want * 24, s));
    uint64_t *d_key = (uint64_t *)(void *)c->d_pack.p, *d_ev = d_key + want;
    uint32_t *d_klen = (uint32_t *)(void *)(d_ev + want), *d_vlen = d_klen + want;
    for (uint64_t k = 0; k < P; k++) {
        const uint64_t cnt = base[k + 1] - base[k];
        if (!cnt) continue;
        EntsEmit o = emit_of(k);
        o.key = d_key + base[k], o.klen = d_klen + base[k], o.v = d_ev + base[k], o.vlen = d_vlen + base[k], o.cap = cnt;
        if ((rc = ents_emit_launch(c, ep, (uint32_t)k, c->d_json, n, o, s))) return rc;
    }
    if ((key && (rc = hb.copy(key, d_key, want * 8, hipMemcpyDeviceToHost))) ||
        (ent_val && (rc = hb.copy(ent_val, d_ev, want * 8, hipMemcpyDeviceToHost))) ||
        (key_len && (rc = hb.copy(key_len, d_klen, want * 4, hipMemcpyDeviceToHost))) ||
        (ent_val_len && (rc = hb.copy(ent_val_len, d_vlen, want * 4, hipMemcpyDeviceToHost))) || (rc = hb.sync()))
        return rc;
    for (uint64_t k = 0; k < P; k++) { /* payload offsets relative to the caller's arena */
        for (uint64_t j = base[k]; j < base[k + 1]; j++) {
            if (key && kind_str_key(ep->kinds[k])) key[j] += in_off[0];
            if (ent_val && kind_str_val(ep->kinds[k])) ent_val[j] += in_off[0];
        }
    }
    return DG_OK;
}

}  // extern "C"
