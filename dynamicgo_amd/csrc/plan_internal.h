/* plan_internal.h — what cols_host.hip, ents_host.hip and rows_host.hip share: the kind helpers, the checks and
 * the making of a plan (PlanRec, host_internal.h), the chaining of per-column offsets and the list column's scan +
 * emit launch. */
#pragma once
#include "host_internal.h"

/* ---- what the typed-column plans share (cols, ents, rows) ---- */

inline bool kind_is_list(uint32_t kind) { return (kind & DG_COL_LIST) != 0; }
/* a DG_COL_* kind a column of cols or rows may have */
inline bool col_kind_ok(uint32_t kind)
{
    return (kind >= DG_COL_BOOL && kind <= DG_COL_LEN) || kind == (DG_COL_LIST | DG_COL_INT) ||
           kind == (DG_COL_LIST | DG_COL_F64);
}
/* the kinds of P columns as the kernels take them: byte k = column k's */
inline uint64_t pack_kinds(const uint8_t *kinds, uint64_t P)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < P; k++) w |= (uint64_t)kinds[k] << (k * 8);
    return w;
}
inline bool wants_len(const uint8_t *kinds, uint64_t P)
{
    bool w = false;
    for (uint32_t k = 0; k < P; k++) w |= kinds[k] == DG_COL_STR || kind_is_list(kinds[k]);
    return w;
}

/* what differs between the creates: the predicate and the words of the texts */
struct PlanKinds {
    bool (*ok)(uint32_t);
    const char *name;  /* "cols": the upload's error text */
    const char *paths; /* "paths" or "sub-paths" */
    const char *kind;  /* "kind" or "entry kind" */
};

/* n_kinds kinds against a checked path set h: the count, then every kind */
inline int plan_kinds_check(const dg_path_hdr &h, const uint8_t *kinds, uint32_t n_kinds, const PlanKinds &w)
{
    if (n_kinds != h.n_paths) return set_err(DG_E_ARG, "%u kinds for %u %s", n_kinds, h.n_paths, w.paths);
    for (uint32_t k = 0; k < n_kinds; k++)
        if (!w.ok(kinds[k])) return set_err(DG_E_ARG, "column %u: unknown %s %u", k, w.kind, kinds[k]);
    return DG_OK;
}

/* a new plan of context c with its kinds and path set h, blob uploaded (under Entry) */
template <class P>
int plan_new(dg_ctx *c, const dg_path_hdr &h, const void *blob, const uint8_t *kinds, uint32_t n_kinds, const char *name,
             std::unique_ptr<P> &p)
{
    p.reset(new P());
    p->ctx = c;
    p->hdr = h;
    memset(p->kinds, 0, sizeof p->kinds);
    memcpy(p->kinds, kinds, n_kinds); /* n_kinds == h.n_paths <= DG_TGET_MAX_PATHS: dg_i_path_validate and plan_kinds_check */
    return upload_blob(p->d_blob, blob, h.total_len, name);
}

/* dg_cols_create and dg_ents_create: the null checks, the path set's, the
 * count, the kinds, then the plan on the device */
template <class P>
int plan_create(dg_ctx *c, const void *blob, size_t len, const uint8_t *kinds, uint32_t n_kinds, const PlanKinds &w, P **out)
{
    if (!c || !blob || !kinds || !out) return set_err(DG_E_INVALID, "null ctx/blob/kinds/out");
    dg_path_hdr h;
    int rc;
    if ((rc = dg_i_path_validate(blob, len, h)) || (rc = plan_kinds_check(h, kinds, n_kinds, w))) return rc;
    Entry g(c, true);
    if (g.rc) return g.rc;
    std::unique_ptr<P> p;
    if ((rc = plan_new(c, h, blob, kinds, n_kinds, w.name, p))) return rc;
    *out = p.release();
    return DG_OK;
}

/* the offsets of L columns, each n + 1 long and starting at 0, made one run:
 * column j's are moved up by the totals of the columns before it. Answers
 * base[0..L]: base[j] = where column j's elements start, base[L] = the total. */
inline std::vector<uint64_t> chain_columns(uint64_t *off, uint64_t L, uint64_t n)
{
    std::vector<uint64_t> base(L + 1, 0);
    for (uint64_t j = 0; j < L; j++) {
        uint64_t *eo = off + j * (n + 1);
        base[j + 1] = base[j] + eo[n];
        for (uint64_t i = 0; i <= n; i++) eo[i] += base[j];
    }
    return base;
}

/* One list column's scan and (with elems and cap) emit on stream s (ctx mutex
 * held) for dg_cols_list_device, dg_cols_batch_host and dg_rows_list_device
 * (cols_host.hip): n counts in len, the tile sums in st. */
struct ListCol {
    const uint8_t *src;
    uint64_t n;
    const uint64_t *val;
    const dg_col_cell *cell;
    const uint32_t *len;
    uint64_t *elem_off, *elems, cap;
};
/* rows: the counts are rows, not messages (the too-many text and the launch error's name) */
__attribute__((visibility("hidden"))) int dg_i_list_launch(dg_ctx *c, PassState &st, bool full_search, bool rows, const ListCol &l,
                                                           hipStream_t s);
