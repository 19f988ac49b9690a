/*
 * rows_host.hip — the C ABI of row columns (include/dgj2t.h dg_rows_*: the
 * reference's Children of a list followed by GetByPath and a cast per
 * element; under a map plan, dg_rows_create_map, the Children of a map with
 * every entry's key beside its row). Kernels: rows_device.h, rows_kern.hip; the
 * scan and the list emit are cols' (cols_device.h).
 */
#include <string.h>

#include "plan_internal.h"
#include "rows_device.h"

using namespace dg;

static const uint64_t ROWS_WS = (uint64_t)TG_DEEP_DEPTH * TG_DEEP_LANES * 8;

static const PlanKinds ROWS_KINDS{col_kind_ok, "rows", "sub-paths", "kind"};

/* one batch (device pointers) */
struct RowsBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    dg_rows_head *head;
    uint64_t *row_off;
    dg_row_ent *index; /* null: the component's scratch */
    uint64_t *val;     /* null with cell: the sizing call */
    dg_col_cell *cell;
    uint32_t *len;
    uint64_t row_cap;
    uint64_t *key = nullptr; /* map plans: the rows' keys and key lengths, each may be null */
    uint32_t *key_len = nullptr;
};

/* one batch on stream s (ctx mutex held): head pass -> scan -> index pass ->
 * cell pass, each lane pass followed by its deep pass. counted: head and
 * row_off come from an earlier launch with the same batch (the host entry's
 * second launch). All on the component's pass state (the counters alternate
 * per pass), which also orders the counts and the scratch index. A map plan
 * (rp->key_kind) takes its own head and index operations; the rest is shared. */
static int rows_launch(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const RowsBatch &b, bool counted, hipStream_t s)
{
    const uint64_t n = b.n, P = rp->sub_hdr.n_paths;
    if (!b.row_off) return set_err(DG_E_INVALID, "null buffer");
    if (n == 0) { /* the total, so that a reader of d_row_off[n] finds 0 */
        HIPCHK(hipMemsetAsync(b.row_off, 0, 8, s));
        return DG_OK;
    }
    if (!b.src || !b.in_off || !b.head) return set_err(DG_E_INVALID, "null buffer");
    if (((uintptr_t)b.head & 15) || ((uintptr_t)b.index & 15) || ((uintptr_t)b.row_off & 7))
        return set_err(DG_E_INVALID, "heads or index not 16-byte aligned"); /* 16-byte stores */
    if (((uintptr_t)b.val & 7) || ((uintptr_t)b.cell & 7) || ((uintptr_t)b.len & 3))
        return set_err(DG_E_INVALID, "values or cells not 8-byte aligned");
    if (((uintptr_t)b.key & 7) || ((uintptr_t)b.key_len & 3)) return set_err(DG_E_INVALID, "keys not 8-byte aligned");
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    if (!b.val != !b.cell) return set_err(DG_E_INVALID, "values without cells, or cells without values");
    const bool cells = b.val && b.row_cap;
    const bool indexed = cells || (b.index && b.row_cap); /* an index without cells: the caller's own row walk */
    if (cells && wants_len(rp->kinds, P) && !b.len) return set_err(DG_E_INVALID, "a STR or list column needs d_len");
    if (indexed && (b.row_cap > 0xFFFFFFFFull || b.row_cap * P > 0xFFFFFFFFull))
        return set_err(DG_E_INVALID, "%llu rows x %llu columns: 2^32 pairs or more", (unsigned long long)b.row_cap,
                       (unsigned long long)P);
    PassState &st = c->rows;
    int rc;
    /* the previous launch may still use the old queue, counts, sums and index */
    if ((rc = st.first_use(ROWS_WS, 1)) ||
        (rc = st.room(std::max(n, cells ? b.row_cap * P : 0), (n + SCAN_TILE - 1) / SCAN_TILE)) ||
        (rc = st.grow(c->rows_counts, n)) || (cells && !b.index && (rc = st.grow(c->rows_index, b.row_cap))))
        return rc;
    const bool map = rp->key_kind != 0;
    RWMapParams A; /* a list plan's launches read its RWParams part only */
    memset(&A, 0, sizeof A);
    A.key = b.key, A.key_len = b.key_len, A.key_kind = rp->key_kind;
    A.par.src = b.src, A.par.in_off = b.in_off, A.par.root_type = root_type;
    A.par.blob = rp->d_blob, A.par.off_steps = rp->hdr.off_steps, A.par.off_pool = rp->hdr.off_pool;
    A.sub.blob = rp->d_sub, A.sub.off_steps = rp->sub_hdr.off_steps, A.sub.off_pool = rp->sub_hdr.off_pool;
    A.sub.P = (uint32_t)P;
    A.n = n, A.n_steps = rp->hdr.n_steps, A.kinds = pack_kinds(rp->kinds, P); /* one parent path: all the steps are its own */
    A.head = b.head, A.count = c->rows_counts, A.row_off = b.row_off;
    A.idx = b.index ? b.index : (dg_row_ent *)c->rows_index, A.row_cap = b.row_cap;
    A.val = b.val, A.cell = (uint64_t *)(void *)b.cell, A.len = b.len;
    A.deep_list = st.list, A.ws = (uint64_t *)(void *)st.ws;
    return st.enqueue(s, "rows", [&] {
        const auto pass = [&](auto launch) {
            return st.pass(s, [&](uint32_t *mine, uint32_t *other) {
                A.cnt = mine, A.reset = other;
                launch(s, A);
            });
        };
        hipError_t e = hipSuccess;
        if (!counted) {
            e = map ? pass(launch_rows_map_head) : pass(launch_rows_head);
            if (e == hipSuccess) {
                launch_cols_scan(s, c->rows_counts, n, st.sums, b.row_off);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess && indexed) e = map ? pass(launch_rows_map_index) : pass(launch_rows_index);
        if (e == hipSuccess && cells) e = pass(launch_rows_cells);
        return e;
    });
}

/* takes: the plans the entry takes. A list entry takes list plans only and a map entry (dg_rows_map_*) map plans
 * only; dg_rows_list_device, which only reads cells, takes both. */
enum RowsTakes { ROWS_LIST, ROWS_MAP, ROWS_BOTH };
static int rows_args(const dg_ctx *c, const dg_rows *rp, RowsTakes takes)
{
    if (!c || !rp || rp->ctx != c) return set_err(DG_E_INVALID, "null ctx/rows, or rows of another context");
    if (takes == ROWS_MAP && !rp->key_kind) return set_err(DG_E_ARG, "rows: a list plan at a map entry (use dg_rows_batch_*)");
    if (takes == ROWS_LIST && rp->key_kind) return set_err(DG_E_ARG, "rows: a map plan at a list entry (use dg_rows_map_batch_*)");
    return DG_OK;
}

static int rows_create(dg_ctx *c, const void *parent_blob, size_t parent_len, const void *sub_blob, size_t sub_len,
                       const uint8_t *kinds, uint32_t n_kinds, uint32_t key_kind, dg_rows **out)
{
    if (!c || !parent_blob || !sub_blob || !kinds || !out) return set_err(DG_E_INVALID, "null ctx/blob/kinds/out");
    dg_path_hdr h, sh;
    int rc;
    if ((rc = dg_i_path_validate(parent_blob, parent_len, h)) || (rc = dg_i_path_validate(sub_blob, sub_len, sh))) return rc;
    if (h.n_paths != 1) return set_err(DG_E_ARG, "rows: %u parent paths (exactly 1)", h.n_paths);
    if ((rc = plan_kinds_check(sh, kinds, n_kinds, ROWS_KINDS))) return rc;
    Entry g(c, true);
    if (g.rc) return g.rc;
    std::unique_ptr<dg_rows> rp;
    if ((rc = plan_new(c, h, parent_blob, kinds, n_kinds, "rows", rp))) return rc;
    rp->sub_hdr = sh;
    rp->key_kind = key_kind;
    if ((rc = upload_blob(rp->d_sub, sub_blob, sh.total_len, "rows"))) return rc;
    *out = rp.release();
    return DG_OK;
}

/* dg_rows_batch_host and dg_rows_map_batch_host: size first, then fill. key and key_len (map plans) may be null. */
static int rows_host(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                     uint64_t n, dg_rows_head *head, uint64_t *row_off, dg_row_ent *index, uint64_t *key, uint32_t *key_len,
                     uint64_t *val, dg_col_cell *cell, uint32_t *len, uint64_t row_cap, uint64_t *need)
{
    if (n == 0) return row_off ? empty_batch(row_off, need) : set_err(DG_E_INVALID, "null buffer");
    if (!thrift || !in_off || !head || !row_off) return set_err(DG_E_INVALID, "null buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    const hipStream_t s = g.s;
    HostBatch hb(c, s);
    const uint64_t P = rp->sub_hdr.n_paths;
    int rc;
    if ((rc = hb.messages(in_off, n, false)) || (rc = c->d_aux.grow(2 * n + 2)) || (rc = c->d_ret.grow(n + 1)) ||
        (rc = hb.upload_messages(thrift, in_off)))
        return rc;
    dg_rows_head *d_head = (dg_rows_head *)(void *)c->d_aux.p;
    RowsBatch b{c->d_json, c->d_in_off, n, d_head, c->d_ret, nullptr, nullptr, nullptr, nullptr, 0};
    if ((rc = rows_launch(c, rp, root_type, b, false, s)) || /* heads and scan */
        (rc = hb.copy(row_off, c->d_ret, (n + 1) * 8, hipMemcpyDeviceToHost)) ||
        (rc = hb.download(head, d_head, n * sizeof(dg_rows_head))))
        return rc;
    for (uint64_t i = 0; i < n; i++) /* offsets relative to the caller's arena: the upload began at in_off[0] */
        if (head[i].status == DG_TGET_OK) head[i].first += in_off[0];
    const uint64_t R = row_off[n];
    if (need) *need = R;
    if (!index && !key && !key_len && !val && !cell && !len && !row_cap) return DG_OK; /* sizing */
    if (R > row_cap) return set_err(DG_E_NOMEM, "rows need %llu entries", (unsigned long long)R);
    if (R * P > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "%llu rows x %llu columns: 2^32 pairs or more", (unsigned long long)R, (unsigned long long)P);
    if (!R) return DG_OK;
    if (!val || !cell || !len) return set_err(DG_E_INVALID, "null buffer");
    /* d_out: values, cells, lengths, column-major over R; d_pack: the index, then the keys and their lengths */
    const uint64_t cells = R * P;
    if ((rc = c->d_out.grow(cells * 20 + 64)) || (rc = c->d_pack.grow(R * (sizeof(dg_row_ent) + 12) + 64))) return rc;
    uint64_t *d_val = (uint64_t *)(void *)c->d_out.p;
    dg_col_cell *d_cell = (dg_col_cell *)(void *)(d_val + cells);
    uint32_t *d_len = (uint32_t *)(void *)(d_cell + cells);
    b.index = (dg_row_ent *)(void *)c->d_pack.p, b.val = d_val, b.cell = d_cell, b.len = d_len, b.row_cap = R;
    if (key) b.key = (uint64_t *)(void *)(b.index + R);
    if (key_len) b.key_len = (uint32_t *)(void *)((uint64_t *)(void *)(b.index + R) + R);
    if ((rc = rows_launch(c, rp, root_type, b, true, s))) return rc;
    for (uint64_t k = 0; k < P; k++) /* the caller's columns are row_cap apart */
        if ((rc = hb.copy(val + k * row_cap, d_val + k * R, R * 8, hipMemcpyDeviceToHost)) ||
            (rc = hb.copy(cell + k * row_cap, d_cell + k * R, R * 8, hipMemcpyDeviceToHost)) ||
            (rc = hb.copy(len + k * row_cap, d_len + k * R, R * 4, hipMemcpyDeviceToHost)))
            return rc;
    if ((index && (rc = hb.copy(index, b.index, R * sizeof(dg_row_ent), hipMemcpyDeviceToHost))) ||
        (key && (rc = hb.copy(key, b.key, R * 8, hipMemcpyDeviceToHost))) ||
        (key_len && (rc = hb.copy(key_len, b.key_len, R * 4, hipMemcpyDeviceToHost))) || (rc = hb.sync()))
        return rc;
    for (uint64_t g2 = 0; index && g2 < R; g2++) index[g2].off += in_off[0];
    for (uint64_t g2 = 0; key && rp->key_kind == DG_ROWS_KEY_STR && g2 < R; g2++) key[g2] += in_off[0];
    for (uint32_t k = 0; k < P; k++)
        if (rp->kinds[k] == DG_COL_STR || kind_is_list(rp->kinds[k]))
            for (uint64_t g2 = k * row_cap; g2 < k * row_cap + R; g2++)
                if (cell[g2].status == DG_TGET_OK) val[g2] += in_off[0];
    return DG_OK;
}

extern "C" {

int dg_rows_create(dg_ctx *c, const void *parent_blob, size_t parent_len, const void *sub_blob, size_t sub_len,
                   const uint8_t *kinds, uint32_t n_kinds, dg_rows **out)
{
    return rows_create(c, parent_blob, parent_len, sub_blob, sub_len, kinds, n_kinds, 0, out);
}

int dg_rows_create_map(dg_ctx *c, const void *parent_blob, size_t parent_len, const void *sub_blob, size_t sub_len,
                       const uint8_t *kinds, uint32_t n_kinds, uint32_t key_kind, dg_rows **out)
{
    if (key_kind != DG_ROWS_KEY_STR && key_kind != DG_ROWS_KEY_INT) return set_err(DG_E_ARG, "rows: unknown key kind %u", key_kind);
    return rows_create(c, parent_blob, parent_len, sub_blob, sub_len, kinds, n_kinds, key_kind, out);
}

void dg_rows_destroy(dg_rows *p) { destroy_with_blob(p); }

uint32_t dg_rows_count(const dg_rows *p) { return p ? p->sub_hdr.n_paths : 0; }

uint32_t dg_rows_key_kind(const dg_rows *p) { return p ? p->key_kind : 0; }

int dg_rows_batch_device(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const uint8_t *d_thrift, const uint64_t *d_in_off,
                         uint64_t n, dg_rows_head *d_head, uint64_t *d_row_off, dg_row_ent *d_index, uint64_t *d_val,
                         dg_col_cell *d_cell, uint32_t *d_len, uint64_t row_cap, void *stream, uint64_t max_len)
{
    if (int rc = rows_args(c, rp, ROWS_LIST)) return rc;
    (void)max_len; /* dense lanes at every length, as cols */
    Entry g(c, true, stream);
    if (g.rc) return g.rc;
    const RowsBatch b{d_thrift, d_in_off, n, d_head, d_row_off, d_index, d_val, d_cell, d_len, row_cap};
    return rows_launch(c, rp, root_type, b, false, g.s);
}

int dg_rows_list_device(dg_ctx *c, const dg_rows *rp, uint32_t k, const uint8_t *d_thrift, uint64_t n_rows,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k, uint64_t *d_elem_off,
                        uint64_t *d_elems, uint64_t elem_cap, void *stream)
{
    if (int rc = rows_args(c, rp, ROWS_BOTH)) return rc;
    Entry g(c, true, stream);
    if (g.rc) return g.rc;
    if (k >= rp->sub_hdr.n_paths || !kind_is_list(rp->kinds[k])) return set_err(DG_E_ARG, "column %u is no list column", k);
    return dg_i_list_launch(c, c->rows, false, true,
                            ListCol{d_thrift, n_rows, d_val_k, d_cell_k, d_len_k, d_elem_off, d_elems, elem_cap}, g.s);
}

int dg_rows_batch_host(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, dg_rows_head *head, uint64_t *row_off, dg_row_ent *index, uint64_t *val, dg_col_cell *cell,
                       uint32_t *len, uint64_t row_cap, uint64_t *need)
{
    if (int rc = rows_args(c, rp, ROWS_LIST)) return rc;
    return rows_host(c, rp, root_type, thrift, in_off, n, head, row_off, index, nullptr, nullptr, val, cell, len, row_cap, need);
}

int dg_rows_map_batch_device(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const uint8_t *d_thrift, const uint64_t *d_in_off,
                             uint64_t n, dg_rows_head *d_head, uint64_t *d_row_off, dg_row_ent *d_index, uint64_t *d_key,
                             uint32_t *d_key_len, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len, uint64_t row_cap,
                             void *stream, uint64_t max_len)
{
    if (int rc = rows_args(c, rp, ROWS_MAP)) return rc;
    (void)max_len;
    Entry g(c, true, stream);
    if (g.rc) return g.rc;
    const RowsBatch b{d_thrift, d_in_off, n, d_head, d_row_off, d_index, d_val, d_cell, d_len, row_cap, d_key, d_key_len};
    return rows_launch(c, rp, root_type, b, false, g.s);
}

int dg_rows_map_batch_host(dg_ctx *c, const dg_rows *rp, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                           uint64_t n, dg_rows_head *head, uint64_t *row_off, dg_row_ent *index, uint64_t *key,
                           uint32_t *key_len, uint64_t *val, dg_col_cell *cell, uint32_t *len, uint64_t row_cap, uint64_t *need)
{
    if (int rc = rows_args(c, rp, ROWS_MAP)) return rc;
    return rows_host(c, rp, root_type, thrift, in_off, n, head, row_off, index, key, key_len, val, cell, len, row_cap, need);
}

}  // extern "C"
