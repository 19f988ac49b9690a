/*
 * evals_host.hip — the C ABI of entry column writes (include/dgj2t.h
 * dg_evals_*; the reference's NewNodeList / NewNodeSet / NewNodeMap,
 * thrift/generic/node.go:154-187). Kernels: evals_device.h, evals_kern.hip; the
 * scans are cols' (cols_kern.hip), the rebase vals' (vals_kern.hip).
 */
#include <string.h>

#include <hip/hip_runtime.h>

/* the size and kind helpers of evals_device.h serve the host here too */
#define TGI __host__ __device__ __forceinline__
#include "evals_device.h"
#include "write_internal.h"

using namespace dg;

/* where the parts of d_work lie, in bytes from its start (8-byte aligned each) */
struct EVWork {
    uint64_t len, cnt, cnt_off, sums, elen[DG_VALS_MAX_COLS], pos[DG_VALS_MAX_COLS], bytes;
};

static uint64_t scan_tiles(uint64_t n) { return (n + CL_SCAN_TILE - 1) / CL_SCAN_TILE; }

/* The launches are serial on one stream, so one set of tile sums serves every scan. */
static EVWork ev_work(const dg_evals *ep, uint64_t n, const uint64_t *n_ent)
{
    EVWork w;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t a = at;
        at += (bytes + 7) & ~7ull;
        return a;
    };
    const uint64_t pairs = n * ep->K;
    w.len = take(pairs * 4), w.cnt = take(pairs * 4), w.cnt_off = take((pairs + 1) * 8);
    uint64_t tiles = scan_tiles(pairs);
    for (uint32_t k = 0; k < ep->K; k++) {
        w.elen[k] = w.pos[k] = ~0ull;
        if (ev_stride(ep->kinds[k]) || !n_ent[k]) continue;
        w.elen[k] = take(n_ent[k] * 4), w.pos[k] = take((n_ent[k] + 1) * 8);
        tiles = std::max(tiles, scan_tiles(n_ent[k]));
    }
    w.sums = take(tiles * 8);
    w.bytes = at;
    return w;
}

/* a buffer the column's kind reads is null; the arenas may be: a column whose strings are all empty reads neither */
static bool ev_col_null(const dg_eval_col &v, uint32_t kt, uint32_t vt)
{
    return !v.d_ent_off || (v.n_ent && (!v.d_val || (kt && !v.d_key) || (kt == TT_STRING && !v.d_key_len) ||
                                        (vt == TT_STRING && !v.d_val_len)));
}

/* One batch on stream s (ctx mutex held). Everything proportional to the
 * cells or the entries lies in the caller's d_work. */
static int evals_launch(dg_ctx *c, const dg_evals *ep, const dg_eval_col *cols, const WriteCall &call, void *d_work,
                        uint64_t work_bytes, hipStream_t s)
{
    const uint32_t K = ep->K;
    const uint64_t n = call.n;
    if (int rc = write_prologue(ep, cols, call); rc || !n) return rc;
    uint64_t n_ent[DG_VALS_MAX_COLS], ents = 0;
    for (uint32_t k = 0; k < K; k++) {
        const dg_eval_col &v = cols[k];
        const uint32_t kt = ev_kt(ep->kinds[k]), vt = ev_vt(ep->kinds[k]);
        n_ent[k] = v.n_ent, ents += v.n_ent;
        if (ev_col_null(v, kt, vt)) return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (((uintptr_t)v.d_ent_off & 7) || ((uintptr_t)v.d_key & 7) || ((uintptr_t)v.d_val & 7) || ((uintptr_t)v.d_key_len & 3) ||
            ((uintptr_t)v.d_val_len & 3))
            return set_err(DG_E_INVALID, "column %u: offsets, keys, values or lengths not aligned", k);
    }
    const EVWork w = ev_work(ep, n, n_ent);
    if (!d_work || ((uintptr_t)d_work & 7)) return set_err(DG_E_INVALID, "d_work null or not 8-byte aligned");
    if (work_bytes < w.bytes)
        return set_err(DG_E_NOMEM, "d_work of %llu bytes, %llu needed", (unsigned long long)work_bytes, (unsigned long long)w.bytes);
    uint8_t *const wk = (uint8_t *)d_work;
    uint64_t *const sums = (uint64_t *)(wk + w.sums);
    EVParams A;
    write_params(A, ep, cols, call);
    const uint64_t pairs = A.pairs;
    A.len = (uint32_t *)(wk + w.len), A.cnt = (uint32_t *)(wk + w.cnt), A.cnt_off = (uint64_t *)(wk + w.cnt_off);
    hipError_t e = hipSuccess;
    for (uint32_t k = 0; k < K && e == hipSuccess; k++) {
        if (w.pos[k] == ~0ull) continue;
        uint32_t *elen = (uint32_t *)(wk + w.elen[k]);
        uint64_t *pos = (uint64_t *)(wk + w.pos[k]);
        A.pos[k] = pos;
        launch_evals_entry_size(s, cols[k], ev_kt(ep->kinds[k]), ev_vt(ep->kinds[k]), elen);
        if ((e = hipGetLastError()) != hipSuccess) break;
        launch_cols_scan(s, elen, n_ent[k], sums, pos);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_evals_cells(s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_cols_scan(s, A.len, pairs, sums, call.d_out_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess && call.out_base) {
        launch_vals_rebase(s, call.d_out_off, pairs + 1, call.out_base);
        e = hipGetLastError();
    }
    if (e == hipSuccess && call.d_out && call.cap > call.out_base) {
        launch_cols_scan(s, A.cnt, pairs, sums, A.cnt_off);
        e = hipGetLastError();
        if (e == hipSuccess) {
            /* the emitted entries are not known here: as many blocks as the columns' entries could fill */
            const uint64_t chunks = (ents + EV_CHUNK - 1) / EV_CHUNK, max_blocks = (uint64_t)std::max(c->n_cu, 1) * 8u;
            launch_evals_emit(s, A, (uint32_t)std::min(chunks, max_blocks));
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return set_err(DG_E_HIP, "evals launch: %s", hipGetErrorString(e));
    return DG_OK;
}

extern "C" {

int dg_evals_create(dg_ctx *c, const uint16_t *kinds, uint32_t K, const int16_t *field_ids, dg_evals **out)
{
    return write_plan_create(c, kinds, K, field_ids, [](uint32_t kind) { return ev_kind_ok(kind); }, out);
}

void dg_evals_destroy(dg_evals *p) { delete p; }

uint32_t dg_evals_count(const dg_evals *p) { return p ? p->K : 0; }

uint8_t dg_evals_wire_type(const dg_evals *p, uint32_t k) { return p && k < p->K ? (uint8_t)ev_wire(p->kinds[k]) : 0; }

uint64_t dg_evals_work_bytes(const dg_evals *p, uint64_t n, const uint64_t *n_ent)
{
    if (!p || !n_ent || n > 0xFFFFFFFFull) return 0;
    for (uint32_t k = 0; k < p->K; k++)
        if (n_ent[k] > DG_EVALS_MAX_ENT) return 0;
    return ev_work(p, n, n_ent).bytes;
}

int dg_evals_batch_device(dg_ctx *c, const dg_evals *ep, const dg_eval_col *cols, uint64_t n, uint64_t out_base, uint8_t *d_out,
                          uint64_t cap, uint64_t *d_out_off, uint8_t *d_status, void *d_work, uint64_t work_bytes, void *stream)
{
    Entry g(c, c && ep && ep->ctx == c, stream, "null ctx/plan, or a plan of another context");
    if (g.rc) return g.rc;
    return evals_launch(c, ep, cols, WriteCall{n, out_base, d_out, cap, d_out_off, d_status}, d_work, work_bytes, g.s);
}

int dg_evals_batch_host(dg_ctx *c, const dg_evals *ep, const dg_eval_col *cols, uint64_t n, uint8_t *out, uint64_t cap,
                        uint64_t *out_off, uint8_t *status, uint64_t *need)
{
    int rc = write_host_prologue(c, ep, cols, n, out_off, need);
    if (rc || !n) return rc;
    const uint32_t K = ep->K;
    uint64_t n_ent[DG_VALS_MAX_COLS];
    for (uint32_t k = 0; k < K; k++) n_ent[k] = cols[k].n_ent;
    Entry g(c, true);
    if (g.rc) return g.rc;
    /* the inputs on the device: offsets and per-entry arrays whole, the
     * payloads from the first to the last byte an entry of an OK cell reads
     * (the cells' statuses by the device's own ev_cell, over a host scan) */
    struct ColDev {
        DevArr<uint64_t> ent_off, key, val;
        DevArr<uint32_t> key_len, val_len;
        DevArr<uint8_t> key_src, val_src, present;
    };
    std::vector<ColDev> dev(K);
    std::vector<dg_eval_col> dc(K);
    for (uint32_t k = 0; k < K; k++) {
        const dg_eval_col &h = cols[k];
        const uint32_t kind = ep->kinds[k], kt = ev_kt(kind), vt = ev_vt(kind);
        const uint64_t ne = h.n_ent;
        memset(&dc[k], 0, sizeof dc[k]);
        dc[k].n_ent = ne;
        if (ev_col_null(h, kt, vt)) return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (h.d_present) {
            if ((rc = to_device(dev[k].present, h.d_present, n))) return rc;
            dc[k].d_present = dev[k].present;
        }
        if ((rc = to_device(dev[k].ent_off, h.d_ent_off, n + 1))) return rc;
        dc[k].d_ent_off = dev[k].ent_off;
        if (!ne) continue;
        if (kt == TT_STRING && (rc = to_device(dev[k].key_len, h.d_key_len, ne))) return rc;
        if (vt == TT_STRING && (rc = to_device(dev[k].val_len, h.d_val_len, ne))) return rc;
        dc[k].d_key_len = dev[k].key_len, dc[k].d_val_len = dev[k].val_len;
        if (kt && kt != TT_STRING) {
            if ((rc = to_device(dev[k].key, h.d_key, ne))) return rc;
            dc[k].d_key = dev[k].key;
        }
        if (vt != TT_STRING) {
            if ((rc = to_device(dev[k].val, h.d_val, ne))) return rc;
            dc[k].d_val = dev[k].val;
        }
        if (ev_stride(kind)) continue;
        std::vector<uint64_t> pos(ne + 1, 0);
        for (uint64_t e = 0; e < ne; e++)
            pos[e + 1] = pos[e] + ev_entry_size(kt, vt, kt == TT_STRING ? h.d_key_len[e] : 0u, vt == TT_STRING ? h.d_val_len[e] : 0u);
        std::vector<uint8_t> owned(ne, 0);
        for (uint64_t i = 0; i < n; i++) {
            if (h.d_present && !h.d_present[i]) continue;
            const uint64_t a = h.d_ent_off[i], b = h.d_ent_off[i + 1];
            if (ev_cell(kind, ep->ids ? 3u : 0u, ep->ids && k == K - 1, true, a, b, ne, pos.data()).cnt)
                std::fill(owned.begin() + a, owned.begin() + b, 1);
        }
        const auto live = [&owned](uint64_t e) { return owned[e] != 0; }; /* an OK cell owns the entry */
        if (kt == TT_STRING) {
            if ((rc = payloads_to_device(h.d_key, h.d_key_len, h.d_key_src, ne, live, dev[k].key, dev[k].key_src))) return rc;
            dc[k].d_key = dev[k].key, dc[k].d_key_src = dev[k].key_src;
        }
        if (vt == TT_STRING) {
            if ((rc = payloads_to_device(h.d_val, h.d_val_len, h.d_val_src, ne, live, dev[k].val, dev[k].val_src))) return rc;
            dc[k].d_val = dev[k].val, dc[k].d_val_src = dev[k].val_src;
        }
    }
    DevArr<uint8_t> d_work;
    const uint64_t work = ev_work(ep, n, n_ent).bytes;
    if ((rc = d_work.alloc(work + 8))) return rc;
    const hipStream_t s = g.s;
    const auto launch = [&](uint8_t *d_out, uint64_t d_cap, uint64_t *d_off, uint8_t *d_status) {
        return evals_launch(c, ep, dc.data(), WriteCall{n, 0, d_out, d_cap, d_off, d_status}, d_work, work, s);
    };
    return write_host_tail(s, n * K, out, cap, out_off, status, need, launch);
}

}  // extern "C"
