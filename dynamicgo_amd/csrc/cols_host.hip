/*
 * cols_host.hip — the C ABI of typed column reads (include/dgj2t.h dg_cols_*;
 * the reference's thrift/generic casts behind GetByPath, cast.go:50-224).
 * Kernels: cols_device.h, cols_kern.hip.
 */
#include <string.h>

#include "cols_device.h"
#include "plan_internal.h"

using namespace dg;

static const uint64_t COLS_WS = (uint64_t)TG_DEEP_DEPTH * TG_DEEP_LANES * 8;

static const PlanKinds COLS_KINDS{col_kind_ok, "cols", "paths", "kind"};

/* one batch (device pointers) */
struct ColsBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    uint64_t *val;
    dg_col_cell *cell;
    uint32_t *len;
};

/* the cell pass of one batch on stream s (ctx mutex held), on the component's
 * pass state */
static int cols_launch(dg_ctx *c, const dg_cols *cp, uint8_t root_type, const ColsBatch &b, hipStream_t s)
{
    const uint64_t n = b.n, P = cp->hdr.n_paths;
    if (n == 0) return DG_OK;
    if (!b.src || !b.in_off || !b.val || !b.cell) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)b.val & 7) || ((uintptr_t)b.cell & 7) || ((uintptr_t)b.len & 3))
        return set_err(DG_E_INVALID, "values or cells not 8-byte aligned"); /* one store each */
    if (wants_len(cp->kinds, P) && !b.len) return set_err(DG_E_INVALID, "a STR or list column needs d_len");
    const uint64_t pairs = n * P;
    if (n > 0xFFFFFFFFull || pairs > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %llu columns", (unsigned long long)n, (unsigned long long)P);
    PassState &st = c->cols;
    int rc;
    if ((rc = st.first_use(COLS_WS, 1)) || (rc = st.room(pairs))) return rc;
    CLParams A;
    memset(&A, 0, sizeof A);
    A.tg.src = b.src, A.tg.in_off = b.in_off, A.tg.pairs = pairs, A.tg.P = (uint32_t)P, A.tg.root_type = root_type;
    A.tg.blob = cp->d_blob, A.tg.off_steps = cp->hdr.off_steps, A.tg.off_pool = cp->hdr.off_pool;
    A.tg.deep_list = st.list;
    A.tg.ws = (uint64_t *)(void *)st.ws;
    A.n = n, A.kinds = pack_kinds(cp->kinds, P);
    A.val = b.val, A.cell = (uint64_t *)(void *)b.cell, A.len = b.len;
    return st.enqueue(s, "cols", [&] {
        return st.pass(s, [&](uint32_t *mine, uint32_t *other) {
            A.tg.deep_count = mine, A.tg.reset_count = other;
            launch_cols_pass(s, A);
        });
    });
}

int dg_i_list_launch(dg_ctx *c, PassState &st, bool full_search, bool rows, const ListCol &l, hipStream_t s)
{
    const uint64_t n = l.n;
    if (!l.elem_off) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)l.elem_off & 7) || ((uintptr_t)l.elems & 7)) return set_err(DG_E_INVALID, "offsets or elements not 8-byte aligned");
    if (n > 0xFFFFFFFFull)
        return rows ? set_err(DG_E_INVALID, "%llu rows", (unsigned long long)n)
                    : set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    if (n == 0) { /* the total, so that a reader of d_elem_off[n] finds 0 */
        HIPCHK(hipMemsetAsync(l.elem_off, 0, 8, s));
        return DG_OK;
    }
    if (!l.src || !l.val || !l.cell || !l.len) return set_err(DG_E_INVALID, "null buffer");
    if (int rc = st.grow(st.sums, (n + SCAN_TILE - 1) / SCAN_TILE)) return rc;
    return st.enqueue(s, rows ? "rows list" : "cols list", [&] {
        launch_cols_scan(s, l.len, n, st.sums, l.elem_off);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && l.elems && l.cap) {
            const CLEmit E{l.src, n, l.val, (const uint64_t *)(const void *)l.cell, l.elem_off, l.elems, l.cap};
            launch_cols_emit(s, E, (uint32_t)std::max(c->n_cu, 1) * 8u, full_search);
            e = hipGetLastError();
        }
        return e;
    });
}

/* list column k of plan cp (see dg_i_list_launch) */
static int cols_list_launch(dg_ctx *c, const dg_cols *cp, uint32_t k, const ListCol &l, hipStream_t s)
{
    if (k >= cp->hdr.n_paths || !kind_is_list(cp->kinds[k])) return set_err(DG_E_ARG, "column %u is no list column", k);
    return dg_i_list_launch(c, c->cols, c->knobs.cols_full_search == 1, false, l, s);
}

extern "C" {

int dg_cols_create(dg_ctx *c, const void *blob, size_t len, const uint8_t *kinds, uint32_t n_kinds, dg_cols **out)
{
    return plan_create(c, blob, len, kinds, n_kinds, COLS_KINDS, out);
}

void dg_cols_destroy(dg_cols *p) { destroy_with_blob(p); }

uint32_t dg_cols_count(const dg_cols *p) { return p ? p->hdr.n_paths : 0; }

int dg_cols_batch_device(dg_ctx *c, const dg_cols *cp, uint8_t root_type, const uint8_t *d_thrift, const uint64_t *d_in_off,
                         uint64_t n, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len, void *stream, uint64_t max_len)
{
    (void)max_len; /* dense lanes at every length, as the lookup measured */
    Entry g(c, c && cp && cp->ctx == c, stream, "null ctx/columns, or columns of another context");
    if (g.rc) return g.rc;
    return cols_launch(c, cp, root_type, ColsBatch{d_thrift, d_in_off, n, d_val, d_cell, d_len}, g.s);
}

int dg_cols_list_device(dg_ctx *c, const dg_cols *cp, uint32_t k, const uint8_t *d_thrift, uint64_t n,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k, uint64_t *d_elem_off,
                        uint64_t *d_elems, uint64_t elem_cap, void *stream)
{
    Entry g(c, c && cp && cp->ctx == c, stream, "null ctx/columns, or columns of another context");
    if (g.rc) return g.rc;
    return cols_list_launch(c, cp, k, ListCol{d_thrift, n, d_val_k, d_cell_k, d_len_k, d_elem_off, d_elems, elem_cap}, g.s);
}

int dg_cols_batch_host(dg_ctx *c, const dg_cols *cp, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, uint64_t *val, dg_col_cell *cell, uint32_t *len, uint64_t *elem_off, uint64_t *elems,
                       uint64_t elem_cap, uint64_t *need)
{
    if (!c || !cp || cp->ctx != c) return set_err(DG_E_INVALID, "null ctx/columns, or columns of another context");
    const uint64_t P = cp->hdr.n_paths;
    std::vector<uint32_t> lists; /* the list columns */
    for (uint32_t k = 0; k < P; k++)
        if (kind_is_list(cp->kinds[k])) lists.push_back(k);
    const uint64_t L = lists.size();
    if (L && !elem_off) return set_err(DG_E_INVALID, "null buffer");
    if (n == 0) {
        for (uint64_t j = 0; j < L; j++) elem_off[j] = 0;
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
    /* d_out: values, cells, lengths; d_ret: the list columns' offsets; d_pack: the elements */
    if ((rc = hb.messages(in_off, n, false)) || (rc = c->d_out.grow(cells * 20 + 64)) ||
        (rc = c->d_ret.grow(L * (n + 1) + 1)) || (rc = hb.upload_messages(thrift, in_off)))
        return rc;
    uint64_t *d_val = (uint64_t *)(void *)c->d_out.p;
    dg_col_cell *d_cell = (dg_col_cell *)(void *)(d_val + cells);
    uint32_t *d_len = (uint32_t *)(void *)(d_cell + cells);
    if ((rc = cols_launch(c, cp, root_type, ColsBatch{c->d_json, c->d_in_off, n, d_val, d_cell, d_len}, s))) return rc;
    for (uint64_t j = 0; j < L && !rc; j++) { /* sizing */
        const uint64_t at = lists[j] * n;
        rc = cols_list_launch(c, cp, lists[j],
                              ListCol{c->d_json, n, d_val + at, d_cell + at, d_len + at, c->d_ret + j * (n + 1), nullptr, 0}, s);
    }
    if (rc || (rc = hb.copy(val, d_val, cells * 8, hipMemcpyDeviceToHost)) ||
        (rc = hb.copy(cell, d_cell, cells * 8, hipMemcpyDeviceToHost)) ||
        (L && (rc = hb.copy(elem_off, c->d_ret, L * (n + 1) * 8, hipMemcpyDeviceToHost))) ||
        (rc = hb.download(len, d_len, cells * 4)))
        return rc;
    /* offsets relative to the caller's arena: the upload began at in_off[0] */
    for (uint32_t k = 0; k < P; k++)
        if (cp->kinds[k] == DG_COL_STR || kind_is_list(cp->kinds[k]))
            for (uint64_t i = k * n; i < (k + 1) * n; i++)
                if (cell[i].status == DG_TGET_OK) val[i] += in_off[0];
    const std::vector<uint64_t> base = chain_columns(elem_off, L, n); /* the columns' elements one after the other */
    const uint64_t want = base[L];
    if (need) *need = want;
    if (!elems && !elem_cap) return DG_OK; /* sizing */
    if (want > elem_cap || (!elems && want)) return set_err(DG_E_NOMEM, "columns need %llu elements", (unsigned long long)want);
    if (!want) return DG_OK;
    if ((rc = c->d_pack.grow(want * 8 + 64))) return rc;
    uint64_t *d_elems = (uint64_t *)(void *)c->d_pack.p;
    for (uint64_t j = 0; j < L; j++) {
        const uint64_t at = lists[j] * n, cnt = base[j + 1] - base[j];
        const ListCol l{c->d_json, n, d_val + at, d_cell + at, d_len + at, c->d_ret + j * (n + 1), d_elems + base[j], cnt};
        if (cnt && (rc = cols_list_launch(c, cp, lists[j], l, s))) return rc;
    }
    return hb.download(elems, c->d_pack, want * 8);
}

}  // extern "C"
