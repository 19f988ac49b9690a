/*
 * rvals_host.hip — the C ABI of row column writes (include/dgj2t.h dg_rvals_*;
 * the reference's NewNodeList / NewNodeSet over struct elements,
 * thrift/generic/node.go:154-187). Kernels: rvals_device.h, rvals_kern.hip; the
 * scans are cols' (cols_kern.hip), the rebase vals' (vals_kern.hip).
 */
#include <string.h>

#include <hip/hip_runtime.h>

/* the size and kind helpers of vals_device.h and rvals_device.h serve the host here too */
#define TGI __host__ __device__ __forceinline__
#include "rvals_device.h"
#include "write_internal.h"

using namespace dg;

/* the plan: vals' kinds, always with field ids, and the outer container's wire type */
struct dg_rvals : WritePlan {
    bool scalars; /* no STRING, list or set column */
    uint8_t container;
    uint8_t kinds[DG_VALS_MAX_COLS];
};

/* where the parts of d_work lie, in bytes from its start (8-byte aligned each) */
struct RVWork {
    uint64_t mlen, mcnt, cnt_off, len, pos, sums, bytes;
};

static uint64_t scan_tiles(uint64_t n) { return (n + CL_SCAN_TILE - 1) / CL_SCAN_TILE; }

/* The launches are serial on one stream, so one set of tile sums serves every
 * scan. The fixed-stride route holds neither the cells' lengths nor pos. */
static RVWork rv_work(uint32_t K, uint64_t n, uint64_t n_rows, bool fixed)
{
    RVWork w;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t a = at;
        at += (bytes + 7) & ~7ull;
        return a;
    };
    const uint64_t cells = n_rows * K;
    w.mlen = take(n * 4), w.mcnt = take(n * 4), w.cnt_off = take((n + 1) * 8);
    w.len = w.pos = ~0ull;
    if (!fixed) w.len = take(cells * 4), w.pos = take((cells + 1) * 8);
    w.sums = take(std::max(scan_tiles(n), fixed ? 0 : scan_tiles(cells)) * 8);
    w.bytes = at;
    return w;
}

/* a buffer the column's kind reads is null; d_elems and d_src may be: a column of empty lists or strings reads neither */
static bool rv_col_null(const dg_val_col &v, uint32_t kind)
{
    return kind & VL_CONTAINER ? !v.d_elem_off : !v.d_val || (kind == TT_STRING && !v.d_len);
}

/* every field present and every item of a fixed width: a row's cells lie at closed-form offsets */
static bool rv_fixed(const dg_rvals *rp, const dg_val_col *cols, uint64_t n_rows)
{
    if (!n_rows) return true;
    if (!rp->scalars) return false;
    for (uint32_t k = 0; k < rp->K; k++)
        if (cols[k].d_present) return false;
    return true;
}

/* what the call gives besides WriteCall's */
struct RVCall {
    const uint64_t *d_row_off;
    uint64_t n_rows;
    uint8_t *d_cell_status; /* may be null */
};

/* One batch on stream s (ctx mutex held). Everything proportional to the
 * messages or the cells lies in the caller's d_work. */
static int rvals_launch(dg_ctx *c, const dg_rvals *rp, const dg_val_col *cols, const WriteCall &call, const RVCall &rows,
                        void *d_work, uint64_t work_bytes, hipStream_t s)
{
    const uint32_t K = rp->K;
    const uint64_t n = call.n, n_rows = rows.n_rows;
    const WriteRows owners{n_rows, "rows"}; /* the cells are the rows', not the messages' */
    if (int rc = write_prologue(rp, cols, call, &owners); rc || !n) return rc;
    if (!rows.d_row_off || ((uintptr_t)rows.d_row_off & 7)) return set_err(DG_E_INVALID, "d_row_off null or not 8-byte aligned");
    for (uint32_t k = 0; k < K && n_rows; k++) {
        const dg_val_col &v = cols[k];
        if (rv_col_null(v, rp->kinds[k])) return set_err(DG_E_INVALID, "column %u: null buffer", k);
        if (((uintptr_t)v.d_val & 7) || ((uintptr_t)v.d_elem_off & 7) || ((uintptr_t)v.d_elems & 7) || ((uintptr_t)v.d_len & 3))
            return set_err(DG_E_INVALID, "column %u: values, offsets or elements not aligned", k);
    }
    const bool fixed = rv_fixed(rp, cols, n_rows);
    const RVWork w = rv_work(K, n, n_rows, fixed);
    if (!d_work || ((uintptr_t)d_work & 7)) return set_err(DG_E_INVALID, "d_work null or not 8-byte aligned");
    if (work_bytes < w.bytes)
        return set_err(DG_E_NOMEM, "d_work of %llu bytes, %llu needed", (unsigned long long)work_bytes, (unsigned long long)w.bytes);
    uint8_t *const wk = (uint8_t *)d_work;
    uint64_t *const sums = (uint64_t *)(wk + w.sums);
    RVParams A;
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, K * sizeof *cols);
    memcpy(A.kinds, rp->kinds, sizeof A.kinds);
    memcpy(A.ids, rp->field_ids, sizeof A.ids);
    A.K = K, A.has_ids = 1, A.fixed = fixed;
    A.n = n, A.n_rows = n_rows, A.cells = n_rows * K, A.base = call.out_base, A.cap = call.cap;
    A.row_off = rows.d_row_off, A.off = call.d_out_off, A.status = call.d_status, A.cell_status = rows.d_cell_status;
    A.out = call.d_out;
    A.mlen = (uint32_t *)(wk + w.mlen), A.mcnt = (uint32_t *)(wk + w.mcnt), A.cnt_off = (uint64_t *)(wk + w.cnt_off);
    hipError_t e = hipSuccess;
    if (fixed) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < K; k++) {
            A.pre[k] = (uint8_t)at; /* at most 15 items of 11 bytes before it */
            at += 3u + tg_fixed(rp->kinds[k]);
        }
        A.stride = at + 1u;
        if (A.cell_status && A.cells) e = hipMemsetAsync(A.cell_status, DG_VAL_OK, A.cells, s);
    } else {
        A.len = (uint32_t *)(wk + w.len), A.pos = (uint64_t *)(wk + w.pos);
        launch_rvals_size(s, A);
        e = hipGetLastError();
        if (e == hipSuccess) {
            launch_cols_scan(s, A.len, A.cells, sums, A.pos);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        launch_rvals_msgs(s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_cols_scan(s, A.mlen, n, sums, call.d_out_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess && call.out_base) {
        launch_vals_rebase(s, call.d_out_off, n + 1, call.out_base);
        e = hipGetLastError();
    }
    if (e == hipSuccess && call.d_out && call.cap > call.out_base) {
        launch_cols_scan(s, A.mcnt, n, sums, A.cnt_off);
        e = hipGetLastError();
        if (e == hipSuccess) {
            /* the emitted rows are not known here: as many blocks as all rows' cells could fill, one at least for
             * the list headers */
            const uint64_t chunks = std::max<uint64_t>((A.cells + RV_CHUNK - 1) / RV_CHUNK, 1);
            const uint64_t max_blocks = (uint64_t)std::max(c->n_cu, 1) * 8u;
            launch_rvals_emit(s, A, (uint32_t)std::min(chunks, max_blocks), (uint32_t)max_blocks, !rp->scalars && n_rows);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return set_err(DG_E_HIP, "rvals launch: %s", hipGetErrorString(e));
    return DG_OK;
}

extern "C" {

int dg_rvals_create(dg_ctx *c, const uint8_t *kinds, uint32_t K, const int16_t *field_ids, uint8_t container, dg_rvals **out)
{
    if (c && kinds && out && !field_ids) return set_err(DG_E_ARG, "no field ids: the elements are structs");
    if (c && kinds && out && container != TT_LIST && container != TT_SET)
        return set_err(DG_E_ARG, "container %u (15 list or 14 set)", container);
    const int rc = write_plan_create(c, kinds, K, field_ids, [](uint32_t kind) { return vl_kind_ok(kind); }, out);
    if (rc) return rc;
    (*out)->container = container, (*out)->scalars = true;
    for (uint32_t k = 0; k < K; k++) (*out)->scalars &= vl_scalar_kind(kinds[k]);
    return DG_OK;
}

void dg_rvals_destroy(dg_rvals *p) { delete p; }

uint32_t dg_rvals_count(const dg_rvals *p) { return p ? p->K : 0; }

uint8_t dg_rvals_wire_type(const dg_rvals *p) { return p ? p->container : 0; }

uint64_t dg_rvals_work_bytes(const dg_rvals *p, uint64_t n, uint64_t n_rows)
{
    if (!p || n > 0xFFFFFFFFull || n_rows > 0xFFFFFFFFull || n_rows * p->K > 0xFFFFFFFFull) return 0;
    return rv_work(p->K, n, n_rows, !n_rows).bytes;
}

int dg_rvals_batch_device(dg_ctx *c, const dg_rvals *rp, const dg_val_col *cols, const uint64_t *d_row_off, uint64_t n,
                          uint64_t n_rows, uint64_t out_base, uint8_t *d_out, uint64_t cap, uint64_t *d_out_off, uint8_t *d_status,
                          uint8_t *d_cell_status, void *d_work, uint64_t work_bytes, void *stream)
{
    Entry g(c, c && rp && rp->ctx == c, stream, "null ctx/plan, or a plan of another context");
    if (g.rc) return g.rc;
    return rvals_launch(c, rp, cols, WriteCall{n, out_base, d_out, cap, d_out_off, d_status}, RVCall{d_row_off, n_rows, d_cell_status},
                        d_work, work_bytes, g.s);
}

int dg_rvals_batch_host(dg_ctx *c, const dg_rvals *rp, const dg_val_col *cols, const uint64_t *row_off, uint64_t n, uint64_t n_rows,
                        uint8_t *out, uint64_t cap, uint64_t *out_off, uint8_t *status, uint8_t *cell_status, uint64_t *need)
{
    const WriteRows owners{n_rows, "rows"};
    int rc = write_host_prologue(c, rp, cols, n, out_off, need, &owners);
    if (rc || !n) return rc;
    if (!row_off) return set_err(DG_E_INVALID, "null buffer");
    const uint32_t K = rp->K;
    for (uint32_t k = 0; k < K && n_rows; k++)
        if (rv_col_null(cols[k], rp->kinds[k])) return set_err(DG_E_INVALID, "column %u: null buffer", k);
    Entry g(c, true);
    if (g.rc) return g.rc;
    /* The rows an OK message owns, by the device's own rules over a host scan:
     * only their cells are live. */
    std::vector<uint64_t> rpos(n_rows + 1, 0);
    for (uint64_t r = 0; r < n_rows; r++) {
        uint64_t bytes = 0;
        for (uint32_t k = 0; k < K; k++) {
            const dg_val_col &h = cols[k];
            const uint32_t kind = rp->kinds[k];
            const bool present = !h.d_present || h.d_present[r];
            uint64_t cnt = 0;
            if (present && (kind & VL_CONTAINER)) cnt = h.d_elem_off[r + 1] - h.d_elem_off[r];
            if (present && kind == TT_STRING) cnt = h.d_len[r];
            bytes += vl_size(kind, 3, k == K - 1, present, cnt).len;
        }
        rpos[r + 1] = rpos[r] + bytes;
    }
    std::vector<uint8_t> owned(n_rows, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t a = row_off[i], b = row_off[i + 1];
        if (a > b || b > n_rows || b - a > 0x7FFFFFFFull || RV_HDR + (rpos[b] - rpos[a]) > 0xFFFFFFFFull) continue;
        std::fill(owned.begin() + a, owned.begin() + b, 1);
    }
    /* the inputs on the device: the per-row arrays whole, a string column's
     * payloads from the first to the last byte a live cell reads, a container's
     * elements likewise; offsets are rebased to what was uploaded */
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
        const uint32_t kind = rp->kinds[k];
        memset(&dc[k], 0, sizeof dc[k]);
        if (!n_rows) continue;
        const auto live = [&](uint64_t r) { return owned[r] && (!h.d_present || h.d_present[r]); };
        if (h.d_present) {
            if ((rc = to_device(dev[k].present, h.d_present, n_rows))) return rc;
            dc[k].d_present = dev[k].present;
        }
        if (kind & VL_CONTAINER) {
            uint64_t lo = ~0ull, hi = 0; /* the elements live cells of a legal count read */
            for (uint64_t r = 0; r < n_rows; r++) {
                const uint64_t a = h.d_elem_off[r], cnt = h.d_elem_off[r + 1] - a;
                if (!live(r) || !vl_size(kind, 3, 0, true, cnt).cnt) continue;
                lo = std::min(lo, a), hi = std::max(hi, a + cnt);
            }
            if (hi <= lo) lo = hi = 0;
            tmp.assign(h.d_elem_off, h.d_elem_off + n_rows + 1);
            for (uint64_t &o : tmp) o -= lo; /* differences, and so counts and flags, stay */
            if ((rc = to_device(dev[k].elem_off, tmp.data(), n_rows + 1)) || (rc = to_device(dev[k].elems, h.d_elems + lo, hi - lo)))
                return rc;
            dc[k].d_elem_off = dev[k].elem_off, dc[k].d_elems = dev[k].elems;
            continue;
        }
        if (kind != TT_STRING) {
            if ((rc = to_device(dev[k].val, h.d_val, n_rows))) return rc;
            dc[k].d_val = dev[k].val;
            continue;
        }
        const auto live_str = [&](uint64_t r) { return live(r) && h.d_len[r] <= 0x7FFFFFFFu; }; /* not flagged DG_VAL_E_SIZE */
        if ((rc = payloads_to_device(h.d_val, h.d_len, h.d_src, n_rows, live_str, dev[k].val, dev[k].src)) ||
            (rc = to_device(dev[k].len, h.d_len, n_rows)))
            return rc;
        dc[k].d_val = dev[k].val, dc[k].d_len = dev[k].len, dc[k].d_src = dev[k].src;
    }
    DevArr<uint64_t> d_row_off;
    DevArr<uint8_t> d_work, d_cell;
    const uint64_t cells = n_rows * K;
    const uint64_t work = rv_work(K, n, n_rows, !n_rows).bytes;
    if ((rc = to_device(d_row_off, row_off, n + 1)) || (rc = d_work.alloc(work + 8)) || (rc = d_cell.alloc(cells + 1))) return rc;
    const hipStream_t s = g.s;
    const auto launch = [&](uint8_t *d_out, uint64_t d_cap, uint64_t *d_off, uint8_t *d_status) {
        const bool sizing = d_status != nullptr; /* write_host_tail's first launch: the statuses are its answer */
        const int lrc = rvals_launch(c, rp, dc.data(), WriteCall{n, 0, d_out, d_cap, d_off, d_status},
                                     RVCall{d_row_off, n_rows, sizing ? d_cell.p : nullptr}, d_work, work, s);
        if (lrc || !sizing || !cell_status || !cells) return lrc;
        HIPCHK(hipMemcpyAsync(cell_status, d_cell.p, cells, hipMemcpyDeviceToHost, s)); /* the tail waits for s */
        return DG_OK;
    };
    return write_host_tail(s, n, out, cap, out_off, status, need, launch);
}

}  // extern "C"
