/*
 * tget_host.hip — the C ABI of the batched path lookup (include/dgj2t.h
 * dg_path_* / dg_tget_*; the reference's thrift/generic GetByPath). Kernels:
 * tget_device.h.
 */
#include <string.h>

#include "host_internal.h"
#include "tget_device.h"

using namespace dg;

static const uint64_t TGET_WS = (uint64_t)TG_DEEP_DEPTH * TG_DEEP_LANES * 8;

/* every how-manieth lane takes a (message, path) pair. The t2j lane pass
 * spreads ~1 KB messages over sparse waves (t2j_host.hip t2j_spread); the
 * lookup, which formats nothing, measured fastest with dense waves at both
 * batch sizes (ms per launch at spread 1 / 2 / 4: t2j-c3, ~1.2 KB, 4 paths
 * 0.150 / 0.226 / 0.356, 1 path 0.101 / 0.100 / 0.106; t2j-c2, ~100 B, 4 paths
 * 0.061 / 0.066 / 0.076), so max_len picks 1 at every length today and stays
 * the handle for a length where that stops holding. The tget_spread knob
 * (1|2|4) forces. */
static uint32_t tget_spread(const dg_ctx *c, uint64_t max_len)
{
    const int64_t v = c->knobs.tget_spread;
    if (v) return v == 1 || v == 4 ? (uint32_t)v : 2u;
    (void)max_len;
    return 1;
}

/* one batch on stream s (ctx mutex held), on the component's pass state */
int tget_launch(dg_ctx *c, const dg_path *ps, uint8_t root_type, const TGetBatch &b, hipStream_t s)
{
    const uint64_t n = b.n;
    if (n == 0) return DG_OK;
    if (!b.src || !b.in_off || !b.rec) return set_err(DG_E_INVALID, "null buffer");
    if ((uintptr_t)b.rec & 15) return set_err(DG_E_INVALID, "records not 16-byte aligned"); /* one store each */
    const uint64_t pairs = n * ps->hdr.n_paths;
    if (n > 0xFFFFFFFFull || pairs > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %u paths", (unsigned long long)n, ps->hdr.n_paths);
    PassState &st = c->tget;
    int rc;
    if ((rc = st.first_use(TGET_WS, 1)) || (rc = st.room(pairs))) return rc;
    TGParams A;
    memset(&A, 0, sizeof A);
    A.src = b.src;
    A.in_off = b.in_off;
    A.pairs = pairs;
    A.P = ps->hdr.n_paths;
    A.root_type = root_type;
    A.blob = ps->d_blob;
    A.off_steps = ps->hdr.off_steps;
    A.off_pool = ps->hdr.off_pool;
    A.rec = b.rec;
    A.val_off = b.val_off;
    A.val_len = b.val_len;
    A.deep_list = st.list;
    A.ws = (uint64_t *)(void *)st.ws;
    return st.enqueue(s, "tget", [&] {
        return st.pass(s, [&](uint32_t *mine, uint32_t *other) {
            A.deep_count = mine, A.reset_count = other;
            launch_tget_pass(s, A, tget_spread(c, b.max_len));
            if (hipPeekAtLastError() == hipSuccess) launch_tget_deep(s, A);
        });
    });
}

int dg_i_path_validate(const void *blob, size_t len, dg_path_hdr &h)
{
    if (len < sizeof(dg_path_hdr)) return set_err(DG_E_ARG, "path blob of %zu bytes: no header", len);
    memcpy(&h, blob, sizeof h);
    if (h.magic != DG_PATH_MAGIC || h.version != DG_PATH_VERSION)
        return set_err(DG_E_ARG, "path blob: bad magic or version (%08x, %u)", h.magic, h.version);
    if (h.n_paths < 1 || h.n_paths > DG_TGET_MAX_PATHS)
        return set_err(DG_E_ARG, "path blob: %u paths (1 to %u)", h.n_paths, DG_TGET_MAX_PATHS);
    if (h.total_len > len || (h.off_steps & 7) || (h.off_pool & 7) ||
        h.off_steps < sizeof(dg_path_hdr) + (uint64_t)h.n_paths * sizeof(dg_path_ent) ||
        (uint64_t)h.off_steps + (uint64_t)h.n_steps * sizeof(dg_path_step) > h.off_pool ||
        (uint64_t)h.off_pool + h.pool_len != h.total_len)
        return set_err(DG_E_ARG, "path blob: tables outside the blob");
    const uint8_t *b = (const uint8_t *)blob;
    for (uint32_t k = 0; k < h.n_paths; k++) {
        dg_path_ent pe;
        memcpy(&pe, b + sizeof(dg_path_hdr) + k * sizeof(dg_path_ent), sizeof pe);
        if (pe.count > DG_TGET_MAX_STEPS)
            return set_err(DG_E_ARG, "path %u: %u steps (at most %u)", k, pe.count, DG_TGET_MAX_STEPS);
        if ((uint64_t)pe.first + pe.count > h.n_steps) return set_err(DG_E_ARG, "path %u: steps outside the table", k);
        for (uint32_t s = 0; s < pe.count; s++) {
            dg_path_step st;
            memcpy(&st, b + h.off_steps + (uint64_t)(pe.first + s) * sizeof(dg_path_step), sizeof st);
            const bool key = st.kind == DG_PS_STRKEY || st.kind == DG_PS_BINKEY;
            if (st.kind < DG_PS_FIELD || st.kind > DG_PS_BINKEY)
                return set_err(DG_E_ARG, "path %u step %u: unknown kind %u", k, s, st.kind);
            if (st.kind == DG_PS_FIELD && (st.val < -32768 || st.val > 32767))
                return set_err(DG_E_ARG, "path %u step %u: field id %lld outside int16", k, s, (long long)st.val);
            if (st.kind == DG_PS_INDEX && st.val < 0)
                return set_err(DG_E_ARG, "path %u step %u: negative index %lld", k, s, (long long)st.val);
            if (key && (st.val < 0 || (uint64_t)st.val + st.key_len > h.pool_len))
                return set_err(DG_E_ARG, "path %u step %u: key outside the pool", k, s);
            if (!key && st.key_len) return set_err(DG_E_ARG, "path %u step %u: key_len on a keyless step", k, s);
        }
    }
    return DG_OK;
}

extern "C" {

int dg_path_create(dg_ctx *c, const void *blob, size_t len, dg_path **out)
{
    if (!c || !blob || !out) return set_err(DG_E_INVALID, "null ctx/blob/out");
    dg_path_hdr h;
    if (int rc = dg_i_path_validate(blob, len, h)) return rc;
    Entry g(c, true);
    if (g.rc) return g.rc;
    std::unique_ptr<dg_path> ps(new dg_path());
    ps->ctx = c;
    ps->hdr = h;
    if (int rc = upload_blob(ps->d_blob, blob, h.total_len, "path")) return rc;
    *out = ps.release();
    return DG_OK;
}

void dg_path_destroy(dg_path *p) { destroy_with_blob(p); }

uint32_t dg_path_count(const dg_path *p) { return p ? p->hdr.n_paths : 0; }

int dg_tget_batch_device(dg_ctx *c, const dg_path *ps, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, dg_tget_rec *d_rec, uint64_t *d_val_off,
                         uint32_t *d_val_len, void *stream, uint64_t max_len)
{
    Entry g(c, c && ps && ps->ctx == c, stream, "null ctx/paths, or paths of another context");
    if (g.rc) return g.rc;
    return tget_launch(c, ps, root_type, TGetBatch{d_thrift, d_in_off, n, d_rec, d_val_off, d_val_len, max_len}, g.s);
}

int dg_tget_batch_host(dg_ctx *c, const dg_path *ps, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, dg_tget_rec *rec)
{
    if (!c || !ps || ps->ctx != c) return set_err(DG_E_INVALID, "null ctx/paths, or paths of another context");
    if (n == 0) return DG_OK;
    if (!thrift || !in_off || !rec) return set_err(DG_E_INVALID, "null buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    const uint64_t rec_bytes = n * ps->hdr.n_paths * sizeof(dg_tget_rec);
    HostBatch hb(c, g.s);
    int rc;
    if ((rc = hb.messages(in_off, n)) || (rc = c->d_out.grow(rec_bytes + 64)) || (rc = hb.upload_messages(thrift, in_off)))
        return rc;
    const TGetBatch b{c->d_json, c->d_in_off, n, (dg_tget_rec *)(void *)c->d_out, nullptr, nullptr, hb.max_len};
    if ((rc = tget_launch(c, ps, root_type, b, g.s))) return rc;
    return hb.download(rec, c->d_out, rec_bytes);
}

}  // extern "C"
