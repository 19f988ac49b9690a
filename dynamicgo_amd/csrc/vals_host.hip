/*
 * vals_host.hip — the C ABI of typed column writes (include/dgj2t.h dg_vals_*;
 * the reference's NewNode* constructors, thrift/generic/node.go:92-201).
 * Kernels: vals_device.h, vals_kern.hip; the scan is cols' (cols_kern.hip).
 */
#include <string.h>

#include <hip/hip_runtime.h>

/* the size and kind helpers of vals_device.h serve the host here too */
#define TGI __host__ __device__ __forceinline__
#include "host_internal.h"
#include "vals_device.h"

using namespace dg;

/* One batch on stream s (ctx mutex held). The lengths the scan reads and its
 * tile sums are the component's own, one set per context: a launch on another
 * stream than the previous one waits for it (StreamOrder). A plan of scalars
 * with every field present takes neither: its offsets are a closed form. */
static int vals_launch(dg_ctx *c, const dg_vals *vp, const dg_val_col *cols, uint64_t n, uint64_t out_base, uint8_t *d_out,
                       uint64_t cap, uint64_t *d_out_off, uint8_t *d_status, hipStream_t s)
{
    const uint32_t K = vp->K;
    if (!cols) return set_err(DG_E_INVALID, "null columns");
    bool closed = vp->scalars;
    for (uint32_t k = 0; k < K; k++) {
        const dg_val_col &v = cols[k];
        const uint32_t kind = vp->kinds[k];
        if (v.d_present && !vp->ids) return set_err(DG_E_ARG, "column %u: d_present in a plan without field ids", k);
        if (v.d_present) closed = false;
        if (n == 0) continue;
        /* d_elems and d_src may be null: a column of empty lists or empty strings reads neither */
        if (kind & VL_CONTAINER ? !v.d_elem_off : !v.d_val || (kind == TT_STRING && !v.d_len))
            return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (((uintptr_t)v.d_val & 7) || ((uintptr_t)v.d_elem_off & 7) || ((uintptr_t)v.d_elems & 7) || ((uintptr_t)v.d_len & 3))
            return set_err(DG_E_INVALID, "column %u: values, offsets or elements not aligned", k);
    }
    if (n == 0) return DG_OK;
    if (!d_out_off || ((uintptr_t)d_out_off & 7)) return set_err(DG_E_INVALID, "d_out_off null or not 8-byte aligned");
    const uint64_t pairs = n * K;
    if (n > 0xFFFFFFFFull || pairs > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %u columns", (unsigned long long)n, K);
    VLParams A;
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, K * sizeof *cols);
    memcpy(A.kinds, vp->kinds, sizeof A.kinds);
    memcpy(A.ids, vp->field_ids, sizeof A.ids);
    A.K = K, A.has_ids = vp->ids, A.pairs = pairs, A.base = out_base, A.cap = cap;
    A.off = d_out_off, A.status = d_status, A.out = d_out;
    const bool emit = d_out && cap > out_base;
    const bool lane = c->knobs.vals_lane_emit == 1;
    const uint32_t max_blocks = (uint32_t)std::max(c->n_cu, 1) * 8u;
    if (closed) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < K; k++) {
            A.pre[k] = (uint8_t)at; /* at most 15 items of 11 bytes before it */
            at += (vp->ids ? 3u : 0u) + tg_fixed(vp->kinds[k]);
        }
        A.msg = at + (vp->ids ? 1u : 0u);
        if (!emit) A.out = nullptr;
        launch_vals_size(s, A, true);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return set_err(DG_E_HIP, "vals launch: %s", hipGetErrorString(e));
        return DG_OK;
    }
    int rc;
    if ((rc = c->vals.grow(c->vals_len, pairs)) || (rc = c->vals.grow(c->vals_sums, (pairs + CL_SCAN_TILE - 1) / CL_SCAN_TILE)))
        return rc;
    HIPCHK(c->vals.acquire(s));
    A.len = c->vals_len;
    launch_vals_size(s, A, false);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        launch_cols_scan(s, A.len, pairs, c->vals_sums, d_out_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess && out_base) {
        launch_vals_rebase(s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && emit) {
        launch_vals_emit(s, A, max_blocks, lane, !vp->scalars);
        e = hipGetLastError();
    }
    HIPCHK(c->vals.publish(s));
    if (e != hipSuccess) return set_err(DG_E_HIP, "vals launch: %s", hipGetErrorString(e));
    return DG_OK;
}

extern "C" {

int dg_vals_create(dg_ctx *c, const uint8_t *kinds, uint32_t K, const int16_t *field_ids, dg_vals **out)
{
    if (!c || !kinds || !out) return set_err(DG_E_INVALID, "null ctx/kinds/out");
    if (K < 1 || K > DG_VALS_MAX_COLS) return set_err(DG_E_ARG, "%u columns (1 to %u)", K, DG_VALS_MAX_COLS);
    std::unique_ptr<dg_vals> vp(new dg_vals());
    memset(vp.get(), 0, sizeof(dg_vals));
    vp->ctx = c, vp->K = K, vp->ids = field_ids != nullptr, vp->scalars = true;
    for (uint32_t k = 0; k < K; k++) {
        if (!vl_kind_ok(kinds[k])) return set_err(DG_E_ARG, "column %u: unknown kind %u", k, kinds[k]);
        vp->kinds[k] = kinds[k];
        vp->scalars &= vl_scalar_kind(kinds[k]);
        if (field_ids) vp->field_ids[k] = field_ids[k];
    }
    *out = vp.release();
    return DG_OK;
}

void dg_vals_destroy(dg_vals *p) { delete p; }

uint32_t dg_vals_count(const dg_vals *p) { return p ? p->K : 0; }

uint8_t dg_vals_wire_type(const dg_vals *p, uint32_t k) { return p && k < p->K ? (uint8_t)vl_wire(p->kinds[k]) : 0; }

int dg_vals_batch_device(dg_ctx *c, const dg_vals *vp, const dg_val_col *cols, uint64_t n, uint64_t out_base, uint8_t *d_out,
                         uint64_t cap, uint64_t *d_out_off, uint8_t *d_status, void *stream)
{
    Entry g(c, c && vp && vp->ctx == c, stream, "null ctx/plan, or a plan of another context");
    if (g.rc) return g.rc;
    return vals_launch(c, vp, cols, n, out_base, d_out, cap, d_out_off, d_status, g.s);
}

int dg_vals_batch_host(dg_ctx *c, const dg_vals *vp, const dg_val_col *cols, uint64_t n, uint8_t *out, uint64_t cap,
                       uint64_t *out_off, uint8_t *status, uint64_t *need)
{
    if (!c || !vp || vp->ctx != c || !cols) return set_err(DG_E_INVALID, "null ctx/plan/columns, or a plan of another context");
    const uint32_t K = vp->K;
    for (uint32_t k = 0; k < K; k++)
        if (cols[k].d_present && !vp->ids) return set_err(DG_E_ARG, "column %u: d_present in a plan without field ids", k);
    if (n == 0) return empty_batch(out_off, need);
    if (!out_off) return set_err(DG_E_INVALID, "null buffer");
    const uint64_t pairs = n * K;
    if (n > 0xFFFFFFFFull || pairs > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %u columns", (unsigned long long)n, K);
    Entry g(c, true);
    if (g.rc) return g.rc;
    /* the inputs on the device: a string column's payloads from the first to
     * the last byte any row reads, a container's elements likewise; offsets
     * are rebased to what was uploaded */
    struct ColDev {
        DevArr<uint64_t> val, elem_off, elems;
        DevArr<uint32_t> len;
        DevArr<uint8_t> src, present;
    };
    std::vector<ColDev> dev(K);
    std::vector<dg_val_col> dc(K);
    std::vector<uint64_t> tmp;
    int rc;
    for (uint32_t k = 0; k < K; k++) {
        const dg_val_col &h = cols[k];
        const uint32_t kind = vp->kinds[k];
        memset(&dc[k], 0, sizeof dc[k]);
        if (h.d_present) {
            if ((rc = to_device(dev[k].present, h.d_present, n))) return rc;
            dc[k].d_present = dev[k].present;
        }
        if (kind & VL_CONTAINER) {
            if (!h.d_elem_off) return set_err(DG_E_INVALID, "column %u: null buffer", k);
            uint64_t lo = ~0ull, hi = 0; /* the elements rows of a legal count read */
            for (uint64_t i = 0; i < n; i++) {
                const uint64_t a = h.d_elem_off[i], cnt = h.d_elem_off[i + 1] - a;
                if (!vl_size(kind, 0, 0, true, cnt).cnt) continue;
                lo = std::min(lo, a), hi = std::max(hi, a + cnt);
            }
            if (hi <= lo) lo = hi = 0;
            tmp.assign(h.d_elem_off, h.d_elem_off + n + 1);
            for (uint64_t &o : tmp) o -= lo; /* differences, and so counts and flags, stay */
            if ((rc = to_device(dev[k].elem_off, tmp.data(), n + 1)) || (rc = to_device(dev[k].elems, h.d_elems + lo, hi - lo)))
                return rc;
            dc[k].d_elem_off = dev[k].elem_off, dc[k].d_elems = dev[k].elems;
            continue;
        }
        if (!h.d_val) return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (kind != TT_STRING) {
            if ((rc = to_device(dev[k].val, h.d_val, n))) return rc;
            dc[k].d_val = dev[k].val;
            continue;
        }
        if (!h.d_len) return set_err(DG_E_INVALID, "column %u: null buffer", k);
        uint64_t lo = ~0ull, hi = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (!h.d_len[i] || h.d_len[i] > 0x7FFFFFFFu) continue;
            lo = std::min(lo, h.d_val[i]), hi = std::max(hi, h.d_val[i] + h.d_len[i]);
        }
        if (hi <= lo) lo = hi = 0;
        tmp.assign(h.d_val, h.d_val + n);
        for (uint64_t i = 0; i < n; i++) tmp[i] = h.d_len[i] && h.d_len[i] <= 0x7FFFFFFFu ? tmp[i] - lo : 0;
        if ((rc = to_device(dev[k].val, tmp.data(), n)) || (rc = to_device(dev[k].len, h.d_len, n)) ||
            (rc = to_device(dev[k].src, h.d_src + lo, hi - lo, 16)))
            return rc;
        dc[k].d_val = dev[k].val, dc[k].d_len = dev[k].len, dc[k].d_src = dev[k].src;
    }
    DevArr<uint64_t> d_off;
    DevArr<uint8_t> d_status, d_out;
    if ((rc = d_off.alloc(pairs + 1)) || (rc = d_status.alloc(pairs))) return rc;
    const hipStream_t s = g.s;
    if ((rc = vals_launch(c, vp, dc.data(), n, 0, nullptr, 0, d_off, d_status, s))) return rc; /* sizing */
    HIPCHK(hipMemcpyAsync(out_off, d_off.p, (pairs + 1) * 8, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status.p, pairs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t want = out_off[pairs];
    if (need) *need = want;
    if (!out && !cap) return DG_OK; /* sizing */
    if (want > cap || (!out && want)) return set_err(DG_E_NOMEM, "values need %llu bytes", (unsigned long long)want);
    if (!want) return DG_OK;
    if ((rc = d_out.alloc(want + 16)) || (rc = vals_launch(c, vp, dc.data(), n, 0, d_out, want, d_off, nullptr, s))) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out.p, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return DG_OK;
}

}  // extern "C"
