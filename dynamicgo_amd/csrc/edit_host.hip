/*
 * edit_host.hip — the C ABI of batched SetByPath / UnsetByPath (include/dgj2t.h
 * dg_edit_*; the reference's thrift/generic SetByPath / UnsetByPath). Decision
 * and splice: edit_device.h; the lookup in front of them: tget_host.hip.
 */
#include <string.h>

#include "edit_device.h"
#include "host_internal.h"

using namespace dg;

struct dg_edit {
    dg_ctx *ctx = nullptr;
    dg_path *ps = nullptr; /* the (parent, full) set, on the context's device */
    EditStep step = {};    /* val_type is the launch's */
    uint32_t key_off = 0;  /* the last step's key in ps->d_blob (key kinds) */
    uint32_t extra = 0;    /* what a SET can add besides the value */
};

/* one batch (device pointers) */
struct EditBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    uint8_t val_type;
    const uint8_t *val;
    const uint64_t *val_off;
    uint64_t val_len;
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint64_t *ret;
    uint64_t max_len;
};

/* one batch on stream s (ctx mutex held): the lookup of (parent, full) into the
 * context's record scratch, then the splice's two routes, back to back. The
 * scratch is one per context: a launch on another stream than the previous one
 * waits for it (StreamOrder). */
static int edit_launch(dg_ctx *c, const dg_edit *e, uint8_t root_type, const EditBatch &b, hipStream_t s)
{
    const uint64_t n = b.n;
    if (n == 0) return DG_OK;
    const bool set = e->step.op == DG_EDIT_SET;
    if (!b.src || !b.in_off || !b.out || !b.out_off || !b.out_len || !b.ret || (set && !b.val && (b.val_off || b.val_len)))
        return set_err(DG_E_INVALID, "null buffer");
    if (n * 2 > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    int rc = c->edit.grow(c->edit_rec, 2 * n); /* the previous launch may still read the old records */
    if (rc) return rc;
    HIPCHK(c->edit.acquire(s));
    if (!(c->knobs.edit_reuse_rec == 1 && c->edit_rec_n == n)) { /* the knob: time the splice alone */
        rc = tget_launch(c, e->ps, root_type, TGetBatch{b.src, b.in_off, n, c->edit_rec, nullptr, nullptr, b.max_len}, s);
        c->edit_rec_n = rc == DG_OK ? n : 0;
    }
    hipError_t err = hipSuccess;
    if (rc == DG_OK) {
        EditParams A;
        memset(&A, 0, sizeof A);
        A.step = e->step;
        A.step.val_type = b.val_type;
        A.key = e->ps->d_blob + e->key_off;
        A.src = b.src, A.in_off = b.in_off, A.n = n;
        A.rec = c->edit_rec;
        A.val = set ? b.val : nullptr, A.val_off = set ? b.val_off : nullptr, A.val_len = set ? b.val_len : 0;
        A.out = b.out, A.out_off = b.out_off, A.out_len = b.out_len, A.ret = b.ret;
        A.wave_min = c->knobs.edit_wave_min < 0 ? 0 : (uint64_t)c->knobs.edit_wave_min;
        /* the hints bound every output (per-message values: val_len is the longest value, 0 = unknown) */
        const bool hinted = b.max_len && !(set && b.val_off && !b.val_len);
        const bool no_wave = hinted && dg_edit_slot_bound(e, b.max_len, b.val_len) < A.wave_min;
        err = launch_splice_routes(
            c, n, ED_WAVES, no_wave, [&](uint32_t lanes) { launch_edit_lane(s, A, lanes); },
            [&](uint32_t blocks) { launch_edit_wave(s, A, blocks); });
    }
    HIPCHK(c->edit.publish(s));
    if (rc) return rc;
    if (err != hipSuccess) return set_err(DG_E_HIP, "edit launch: %s", hipGetErrorString(err));
    return DG_OK;
}

extern "C" {

int dg_edit_create(dg_ctx *c, const void *blob, size_t len, uint32_t op, dg_edit **out)
{
    /* the blob is judged before the context is looked at: a refusal does not need a device */
    if (!blob || !out) return set_err(DG_E_INVALID, "null blob/out");
    if (op != DG_EDIT_SET && op != DG_EDIT_UNSET) return set_err(DG_E_INVALID, "unknown edit op %u", op);
    dg_path_hdr h;
    if (int rc = dg_i_path_validate(blob, len, h)) return rc;
    if (h.n_paths != 1) return set_err(DG_E_ARG, "edit: %u paths (exactly 1)", h.n_paths);
    const uint8_t *b = (const uint8_t *)blob;
    dg_path_ent pe;
    memcpy(&pe, b + sizeof(dg_path_hdr), sizeof pe);
    if (pe.count < 1) return set_err(DG_E_ARG, "edit: the empty path");
    if (!c) return set_err(DG_E_INVALID, "null ctx");
    /* the (parent, full) set: both paths over the same steps */
    dg_path_hdr g = h;
    g.n_paths = 2, g.n_steps = pe.count;
    g.off_steps = (uint32_t)(sizeof(dg_path_hdr) + 2 * sizeof(dg_path_ent));
    g.off_pool = g.off_steps + pe.count * (uint32_t)sizeof(dg_path_step);
    g.total_len = g.off_pool + h.pool_len;
    std::vector<uint8_t> set(g.total_len);
    const dg_path_ent ents[2] = {{0, pe.count - 1}, {0, pe.count}};
    memcpy(set.data(), &g, sizeof g);
    memcpy(set.data() + sizeof g, ents, sizeof ents);
    memcpy(set.data() + g.off_steps, b + h.off_steps + (uint64_t)pe.first * sizeof(dg_path_step),
           pe.count * sizeof(dg_path_step));
    if (h.pool_len) memcpy(set.data() + g.off_pool, b + h.off_pool, h.pool_len);
    dg_path_step last;
    memcpy(&last, set.data() + g.off_steps + (uint64_t)(pe.count - 1) * sizeof last, sizeof last);
    std::unique_ptr<dg_edit> e(new dg_edit());
    e->ctx = c;
    e->step.op = op, e->step.n_steps = pe.count;
    e->step.kind = last.kind, e->step.key_len = last.key_len, e->step.kval = last.val;
    const bool pooled = last.kind == DG_PS_STRKEY || last.kind == DG_PS_BINKEY;
    e->key_off = g.off_pool + (pooled ? (uint32_t)last.val : 0u);
    e->extra = edit_step_extra(last.kind, last.key_len);
    if (int rc = dg_path_create(c, set.data(), set.size(), &e->ps)) return rc;
    *out = e.release();
    return DG_OK;
}

void dg_edit_destroy(dg_edit *e)
{
    if (!e) return;
    dg_path_destroy(e->ps);
    delete e;
}

uint64_t dg_edit_slot_bound(const dg_edit *e, uint64_t len, uint64_t val_len)
{
    if (!e) return 0;
    return e->step.op == DG_EDIT_SET ? len + val_len + e->extra : len;
}

int dg_edit_batch_device(dg_ctx *c, const dg_edit *e, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, uint8_t val_type, const uint8_t *d_val,
                         const uint64_t *d_val_off, uint64_t val_len, uint8_t *d_out, const uint64_t *d_out_off,
                         uint32_t *d_out_len, uint64_t *d_ret, void *stream, uint64_t max_len)
{
    Entry g(c, c && e && e->ctx == c, stream, "null ctx/edit, or an edit of another context");
    if (g.rc) return g.rc;
    return edit_launch(c, e, root_type,
                       EditBatch{d_thrift, d_in_off, n, val_type, d_val, d_val_off, val_len, d_out, d_out_off, d_out_len,
                                 d_ret, max_len},
                       g.s);
}

/* every message in a slot of its exact bound (rounded up to 16: the packing
 * reads its slots as aligned words), one launch, packed on the device */
int dg_edit_batch_host(dg_ctx *c, const dg_edit *e, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, uint8_t val_type, const uint8_t *val, const uint64_t *val_off, uint64_t val_len,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need)
{
    if (!c || !e || e->ctx != c) return set_err(DG_E_INVALID, "null ctx/edit, or an edit of another context");
    if (n == 0) return empty_batch(out_off, out_need);
    const bool set = e->step.op == DG_EDIT_SET;
    if (!thrift || !in_off || !out_off || !ret) return set_err(DG_E_INVALID, "null buffer");
    if (!set) val = nullptr, val_off = nullptr, val_len = 0;
    if (!val && (val_off || val_len)) return set_err(DG_E_INVALID, "null value buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    HostBatch hb(c, g.s);
    uint64_t max_val = val_len;
    int rc;
    if ((val_off && (rc = hb.values(val_off, n, 1, &max_val))) ||
        (rc = hb.layout(in_off, nullptr, n, [&](uint64_t i, uint64_t len) {
            return dg_edit_slot_bound(e, len, val_off ? hb.vo[i + 1] - hb.vo[i] : val_len);
        })) ||
        (rc = hb.upload_messages(thrift, in_off)) || (rc = hb.upload_slots()) ||
        (rc = hb.upload_values(val, val_off, val_len)))
        return rc;
    const EditBatch b{c->d_json, c->d_in_off, n, val_type, set ? (const uint8_t *)c->d_cb : nullptr,
                      val_off ? (const uint64_t *)c->d_aux : nullptr, max_val, c->d_out, c->d_out_off, c->d_out_len,
                      c->d_ret, hb.max_len};
    if ((rc = edit_launch(c, e, root_type, b, g.s))) return rc;
    return hb.pack_and_download(HostOut{out, out_cap, out_off, out_need}, ret);
}

}  // extern "C"
