/*
 * vals_host.hip — the C ABI of typed column writes (include/dgj2t.h dg_vals_*;
 * the reference's NewNode* constructors, thrift/generic/node.go:92-201).
 * Kernels: vals_device.h, vals_kern.hip; the scan is cols' (cols_kern.hip).
 */
#include <string.h>

#include <hip/hip_runtime.h>

/* the size and kind helpers of vals_device.h serve the host here too */
#define TGI __host__ __device__ __forceinline__
#include "vals_device.h"
#include "write_internal.h"

using namespace dg;

/* One batch on stream s (ctx mutex held). The lengths the scan reads and its
 * tile sums are the component's own, one set per context: a launch on another
 * stream than the previous one waits for it (StreamOrder). A plan of scalars
 * with every field present takes neither: its offsets are a closed form. */
static int vals_launch(dg_ctx *c, const dg_vals *vp, const dg_val_col *cols, const WriteCall &w, hipStream_t s)
{
    const uint32_t K = vp->K;
    int rc = write_prologue(vp, cols, w);
    if (rc || !w.n) return rc;
    bool closed = vp->scalars;
    for (uint32_t k = 0; k < K; k++) {
        const dg_val_col &v = cols[k];
        const uint32_t kind = vp->kinds[k];
        if (v.d_present) closed = false;
        /* d_elems and d_src may be null: a column of empty lists or empty strings reads neither */
        if (kind & VL_CONTAINER ? !v.d_elem_off : !v.d_val || (kind == TT_STRING && !v.d_len))
            return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (((uintptr_t)v.d_val & 7) || ((uintptr_t)v.d_elem_off & 7) || ((uintptr_t)v.d_elems & 7) || ((uintptr_t)v.d_len & 3))
            return set_err(DG_E_INVALID, "column %u: values, offsets or elements not aligned", k);
    }
    VLParams A;
    write_params(A, vp, cols, w);
    const uint64_t pairs = A.pairs;
    const bool emit = w.d_out && w.cap > w.out_base;
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
    if ((rc = c->vals.grow(c->vals_len, pairs)) || (rc = c->vals.grow(c->vals_sums, (pairs + CL_SCAN_TILE - 1) / CL_SCAN_TILE)))
        return rc;
    HIPCHK(c->vals.acquire(s));
    A.len = c->vals_len;
    launch_vals_size(s, A, false);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        launch_cols_scan(s, A.len, pairs, c->vals_sums, w.d_out_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess && w.out_base) {
        launch_vals_rebase(s, w.d_out_off, pairs + 1, w.out_base);
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
    const int rc = write_plan_create(c, kinds, K, field_ids, [](uint32_t kind) { return vl_kind_ok(kind); }, out);
    if (rc) return rc;
    (*out)->scalars = true;
    for (uint32_t k = 0; k < K; k++) (*out)->scalars &= vl_scalar_kind(kinds[k]);
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
    return vals_launch(c, vp, cols, WriteCall{n, out_base, d_out, cap, d_out_off, d_status}, g.s);
}

int dg_vals_batch_host(dg_ctx *c, const dg_vals *vp, const dg_val_col *cols, uint64_t n, uint8_t *out, uint64_t cap,
                       uint64_t *out_off, uint8_t *status, uint64_t *need)
{
    int rc = write_host_prologue(c, vp, cols, n, out_off, need);
    if (rc || !n) return rc;
    const uint32_t K = vp->K;
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
        const auto live = [&h](uint64_t i) { return h.d_len[i] <= 0x7FFFFFFFu; }; /* not flagged DG_VAL_E_SIZE */
        if ((rc = payloads_to_device(h.d_val, h.d_len, h.d_src, n, live, dev[k].val, dev[k].src)) ||
            (rc = to_device(dev[k].len, h.d_len, n)))
            return rc;
        dc[k].d_val = dev[k].val, dc[k].d_len = dev[k].len, dc[k].d_src = dev[k].src;
    }
    const hipStream_t s = g.s;
    const auto launch = [&](uint8_t *d_out, uint64_t d_cap, uint64_t *d_off, uint8_t *d_status) {
        return vals_launch(c, vp, dc.data(), WriteCall{n, 0, d_out, d_cap, d_off, d_status}, s);
    };
    return write_host_tail(s, n * K, out, cap, out_off, status, need, launch);
}

}  // extern "C"
