/* write_internal.h — what vals_host.hip, evals_host.hip and rvals_host.hip share: the plan record and its making, the
 * checks before a launch's per-column ones, the filling of the kernel record's common fields (vals and evals, whose
 * cells are the messages'), the payload upload and the two-pass tail of the host entries. */
#pragma once
#include "host_internal.h"

/* a plan of columns to write: K kinds (the component's own width) and, in struct mode, K field ids */
struct WritePlan {
    dg_ctx *ctx;
    uint32_t K;
    bool ids; /* struct mode */
    int16_t field_ids[DG_VALS_MAX_COLS];
};
struct dg_vals : WritePlan {
    bool scalars; /* no STRING, list or set column */
    uint8_t kinds[DG_VALS_MAX_COLS];
};
struct dg_evals : WritePlan {
    uint16_t kinds[DG_VALS_MAX_COLS];
};

/* dg_vals_create and dg_evals_create: the null checks, the count, every kind by the component's `ok` */
template <class P, class T, class Ok>
int write_plan_create(dg_ctx *c, const T *kinds, uint32_t K, const int16_t *field_ids, Ok ok, P **out)
{
    if (!c || !kinds || !out) return set_err(DG_E_INVALID, "null ctx/kinds/out");
    if (K < 1 || K > DG_VALS_MAX_COLS) return set_err(DG_E_ARG, "%u columns (1 to %u)", K, DG_VALS_MAX_COLS);
    std::unique_ptr<P> p(new P());
    memset(p.get(), 0, sizeof(P));
    p->ctx = c, p->K = K, p->ids = field_ids != nullptr;
    for (uint32_t k = 0; k < K; k++) {
        if (!ok(kinds[k])) return set_err(DG_E_ARG, "column %u: unknown kind %u", k, kinds[k]);
        p->kinds[k] = kinds[k];
        if (field_ids) p->field_ids[k] = field_ids[k];
    }
    *out = p.release();
    return DG_OK;
}

/* what a batch's caller gives besides the columns: device pointers at the launches */
struct WriteCall {
    uint64_t n, out_base;
    uint8_t *d_out; /* null: sizing */
    uint64_t cap;
    uint64_t *d_out_off;
    uint8_t *d_status; /* may be null */
};

/* what is wrong with a column whatever n is: d_present in a plan without field ids, evals' entry count */
template <class Col>
int write_check_cols(const WritePlan *p, const Col *cols)
{
    for (uint32_t k = 0; k < p->K; k++) {
        if (cols[k].d_present && !p->ids) return set_err(DG_E_ARG, "column %u: d_present in a plan without field ids", k);
        if constexpr (std::is_same<Col, dg_eval_col>::value)
            if (cols[k].n_ent > DG_EVALS_MAX_ENT)
                return set_err(DG_E_ARG, "column %u: %llu entries (at most %llu)", k, (unsigned long long)cols[k].n_ent,
                               (unsigned long long)DG_EVALS_MAX_ENT);
    }
    return DG_OK;
}

/* the cells fit the scan: n messages (vals, evals) or n rows (rvals) of K columns */
inline int write_check_pairs(const WritePlan *p, uint64_t n, const char *unit = "messages")
{
    const bool fits = n <= 0xFFFFFFFFull && n * p->K <= 0xFFFFFFFFull;
    return fits ? DG_OK : set_err(DG_E_INVALID, "batch of %llu %s x %u columns", (unsigned long long)n, unit, p->K);
}

/* the columns' owners when they are not the messages: rvals' rows */
struct WriteRows {
    uint64_t count;
    const char *unit;
};

/* what the launches check before their per-column buffers; n == 0 is DG_OK with nothing else looked at. The cells are
 * the messages' unless `rows` says whose they are. */
template <class Col>
int write_prologue(const WritePlan *p, const Col *cols, const WriteCall &w, const WriteRows *rows = nullptr)
{
    if (!cols) return set_err(DG_E_INVALID, "null columns");
    if (int rc = write_check_cols(p, cols)) return rc;
    if (w.n == 0) return DG_OK;
    if (!w.d_out_off || ((uintptr_t)w.d_out_off & 7)) return set_err(DG_E_INVALID, "d_out_off null or not 8-byte aligned");
    if (!rows) return write_check_pairs(p, w.n);
    if (w.n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)w.n);
    return write_check_pairs(p, rows->count, rows->unit);
}

/* the fields VLParams and EVParams share, from the plan and the call; every other field 0 */
template <class R, class P, class Col>
void write_params(R &A, const P *p, const Col *cols, const WriteCall &w)
{
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, p->K * sizeof *cols);
    memcpy(A.kinds, p->kinds, sizeof A.kinds);
    memcpy(A.ids, p->field_ids, sizeof A.ids);
    A.K = p->K, A.has_ids = p->ids, A.pairs = w.n * p->K, A.base = w.out_base, A.cap = w.cap;
    A.off = w.d_out_off, A.status = w.d_status, A.out = w.d_out;
}

/* String payloads of a host column on the device: from the first to the last byte read by an entry that is `live`
 * (the component's rule) and not empty; those entries' offsets are rebased to what was uploaded, every other one is 0
 * and neither its offset nor its payload is looked at. */
template <class Live>
int payloads_to_device(const uint64_t *off, const uint32_t *len, const uint8_t *src, uint64_t n_ent, Live live,
                       DevArr<uint64_t> &d_off, DevArr<uint8_t> &d_src)
{
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t e = 0; e < n_ent; e++)
        if (live(e) && len[e]) lo = std::min(lo, off[e]), hi = std::max(hi, off[e] + len[e]);
    if (hi <= lo) lo = hi = 0;
    std::vector<uint64_t> tmp(n_ent);
    for (uint64_t e = 0; e < n_ent; e++) tmp[e] = live(e) && len[e] ? off[e] - lo : 0;
    if (int rc = to_device(d_off, tmp.data(), n_ent)) return rc;
    return to_device(d_src, src + lo, hi - lo, 16);
}

/* what a host entry does first; n == 0 is answered here (off[0] = 0, *need = 0) */
template <class Col>
int write_host_prologue(dg_ctx *c, const WritePlan *p, const Col *cols, uint64_t n, uint64_t *out_off, uint64_t *need,
                        const WriteRows *rows = nullptr)
{
    if (!c || !p || p->ctx != c || !cols) return set_err(DG_E_INVALID, "null ctx/plan/columns, or a plan of another context");
    if (int rc = write_check_cols(p, cols)) return rc;
    if (n == 0) return empty_batch(out_off, need);
    if (!out_off) return set_err(DG_E_INVALID, "null buffer");
    if (!rows) return write_check_pairs(p, n);
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    return write_check_pairs(p, rows->count, rows->unit);
}

/* The tail of a host entry, the inputs staged: launch(d_out, cap, d_off, d_status) once for the sizes (d_out null),
 * whose offsets and statuses are the answer and give *need, and unless `out` is null and cap 0 (a sizing call) once more
 * into an arena of exactly that size. */
template <class Launch>
int write_host_tail(hipStream_t s, uint64_t pairs, uint8_t *out, uint64_t cap, uint64_t *out_off, uint8_t *status, uint64_t *need,
                    Launch launch)
{
    DevArr<uint64_t> d_off;
    DevArr<uint8_t> d_status, d_out;
    int rc;
    if ((rc = d_off.alloc(pairs + 1)) || (rc = d_status.alloc(pairs)) || (rc = launch(nullptr, 0, d_off, d_status))) return rc;
    HIPCHK(hipMemcpyAsync(out_off, d_off.p, (pairs + 1) * 8, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status.p, pairs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t want = out_off[pairs];
    if (need) *need = want;
    if (!out && !cap) return DG_OK; /* sizing */
    if (want > cap || (!out && want)) return set_err(DG_E_NOMEM, "values need %llu bytes", (unsigned long long)want);
    if (!want) return DG_OK;
    if ((rc = d_out.alloc(want + 16)) || (rc = launch(d_out, want, d_off, nullptr))) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out.p, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return DG_OK;
}
