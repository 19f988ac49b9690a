/*
 * editm_host.hip — the C ABI of batched SetMany (include/dgj2t.h dg_editm_*; the
 * reference's thrift/generic Node.SetMany) and of batched SetByPath / UnsetByPath
 * (dg_edit_*), which is the many-edit with one item: dg_edit_create keeps its own
 * refusals, every other dg_edit_* entry is its dg_editm_* twin with K = 1.
 * Decision, combine and splice: editm_device.h; the lookup in front of them:
 * tget_host.hip.
 */
#include <string.h>

#include "editm_device.h"
#include "host_internal.h"

using namespace dg;

struct dg_editm {
    dg_ctx *ctx = nullptr;
    dg_path *ps = nullptr; /* {parent, full_1 .. full_K}, on the context's device */
    uint32_t op = 0, n_steps = 0, K = 0;
    EmItem it[EM_MAX] = {}; /* val_type, val_pos and val_len are the launch's */
    uint64_t extra = 0;     /* what a SET can add besides the values */
};

/* the single edit: a many-edit of one item */
struct dg_edit : dg_editm {};

/* one batch (device pointers; val_types and val_lens on the host) */
struct EmBatch {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    const uint8_t *val_types;
    const uint8_t *val;
    const uint64_t *val_off;
    const uint64_t *val_lens;
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint64_t *ret;
    uint64_t max_len;
};

static uint32_t step_class(uint32_t kind) { return kind == DG_PS_FIELD ? 0u : kind == DG_PS_INDEX ? 1u : 2u; }

/* one batch on stream s (ctx mutex held): the lookup of the K + 1 paths into the
 * context's record scratch, then the splice's two routes, back to back. The
 * scratch is one per context: a launch on another stream than the previous one
 * waits for it (StreamOrder). */
static int editm_launch(dg_ctx *c, const dg_editm *e, uint8_t root_type, const EmBatch &b, hipStream_t s)
{
    const uint64_t n = b.n, K = e->K;
    if (n == 0) return DG_OK;
    const bool set = e->op == DG_EDIT_SET;
    if (!b.src || !b.in_off || !b.out || !b.out_off || !b.out_len || !b.ret) return set_err(DG_E_INVALID, "null buffer");
    if (set && (!b.val_types || !b.val_lens)) return set_err(DG_E_INVALID, "null value types / lengths");
    if (n * (K + 1) > 0xFFFFFFFFull)
        return set_err(DG_E_INVALID, "batch of %llu messages x %llu items", (unsigned long long)n, (unsigned long long)K);
    EmParams A;
    memset(&A, 0, sizeof A);
    A.op = e->op, A.n_steps = e->n_steps, A.K = e->K;
    uint64_t val_total = 0;
    bool known = true; /* every value's length, or its longest, is given */
    for (uint32_t j = 0; j < K; j++) {
        A.it[j] = e->it[j];
        if (!set) continue;
        A.it[j].val_type = b.val_types[j];
        A.it[j].val_pos = val_total, A.it[j].val_len = b.val_lens[j];
        val_total += b.val_lens[j];
        known = known && !(b.val_off && !b.val_lens[j]);
    }
    if (set && !b.val && (b.val_off || val_total)) return set_err(DG_E_INVALID, "null buffer");
    int rc = c->edit.grow(c->edit_rec, (K + 1) * n); /* the previous launch may still read the old records */
    if (rc) return rc;
    HIPCHK(c->edit.acquire(s));
    if (!(c->knobs.edit_reuse_rec == 1 && c->edit_rec_n == n && c->edit_rec_k == K)) { /* the knob: time the splice alone */
        rc = tget_launch(c, e->ps, root_type, TGetBatch{b.src, b.in_off, n, c->edit_rec, nullptr, nullptr, b.max_len}, s);
        c->edit_rec_n = rc == DG_OK ? n : 0, c->edit_rec_k = K;
    }
    hipError_t err = hipSuccess;
    if (rc == DG_OK) {
        A.pool = e->ps->d_blob;
        A.src = b.src, A.in_off = b.in_off, A.n = n;
        A.rec = c->edit_rec;
        A.val = set ? b.val : nullptr, A.val_off = set ? b.val_off : nullptr;
        A.out = b.out, A.out_off = b.out_off, A.out_len = b.out_len, A.ret = b.ret;
        A.wave_min = c->knobs.edit_wave_min < 0 ? 0 : (uint64_t)c->knobs.edit_wave_min;
        const bool hinted = b.max_len && (!set || known); /* the hints bound every output */
        const bool no_wave = hinted && dg_editm_slot_bound(e, b.max_len, val_total) < A.wave_min;
        err = launch_splice_routes(
            c, n, ED_WAVES, no_wave, [&](uint32_t lanes) { launch_editm_lane(s, A, lanes); },
            [&](uint32_t blocks) { launch_editm_wave(s, A, blocks); });
    }
    HIPCHK(c->edit.publish(s));
    if (rc) return rc;
    if (err != hipSuccess) return set_err(DG_E_HIP, "edit launch: %s", hipGetErrorString(err));
    return DG_OK;
}

/* what both creates refuse first (the blob is judged before the context is looked at: a refusal does not
 * need a device); h = the blob's header */
static int edit_blob(const void *blob, size_t len, uint32_t op, const void *out, dg_path_hdr &h)
{
    if (!blob || !out) return set_err(DG_E_INVALID, "null blob/out");
    if (op != DG_EDIT_SET && op != DG_EDIT_UNSET) return set_err(DG_E_INVALID, "unknown edit op %u", op);
    return dg_i_path_validate(blob, len, h);
}

static dg_path_step step_at(const uint8_t *b, const dg_path_hdr &h, const dg_path_ent &pe, uint32_t k)
{
    dg_path_step st;
    memcpy(&st, b + h.off_steps + (uint64_t)(pe.first + k) * sizeof st, sizeof st);
    return st;
}

/* e from a judged blob of K paths of cnt >= 1 steps each: the {parent, full_1 .. full_K} set on c's device
 * (every path's steps copied in turn, the parent over the first one's) and the items' last steps */
static int edit_build(dg_ctx *c, const uint8_t *b, const dg_path_hdr &h, const dg_path_ent *pe, uint32_t op, dg_editm *e)
{
    if (!c) return set_err(DG_E_INVALID, "null ctx");
    const uint32_t K = h.n_paths, cnt = pe[0].count;
    dg_path_hdr g = h;
    g.n_paths = K + 1, g.n_steps = K * cnt;
    g.off_steps = (uint32_t)((sizeof(dg_path_hdr) + (K + 1) * sizeof(dg_path_ent) + 7) & ~7ull);
    g.off_pool = g.off_steps + g.n_steps * (uint32_t)sizeof(dg_path_step);
    g.total_len = g.off_pool + h.pool_len;
    std::vector<uint8_t> set(g.total_len);
    memcpy(set.data(), &g, sizeof g);
    e->ctx = c, e->op = op, e->n_steps = cnt, e->K = K;
    const dg_path_ent parent{0, cnt - 1};
    memcpy(set.data() + sizeof g, &parent, sizeof parent);
    for (uint32_t j = 0; j < K; j++) {
        const dg_path_ent ent{j * cnt, cnt};
        memcpy(set.data() + sizeof g + (j + 1) * sizeof ent, &ent, sizeof ent);
        memcpy(set.data() + g.off_steps + (uint64_t)j * cnt * sizeof(dg_path_step),
               b + h.off_steps + (uint64_t)pe[j].first * sizeof(dg_path_step), cnt * sizeof(dg_path_step));
        const dg_path_step last = step_at(b, h, pe[j], cnt - 1);
        const bool pooled = last.kind == DG_PS_STRKEY || last.kind == DG_PS_BINKEY;
        e->it[j].kind = last.kind, e->it[j].key_len = last.key_len, e->it[j].kval = last.val;
        e->it[j].key_off = g.off_pool + (pooled ? (uint32_t)last.val : 0u);
        e->extra += edit_step_extra(last.kind, last.key_len);
    }
    if (h.pool_len) memcpy(set.data() + g.off_pool, b + h.off_pool, h.pool_len);
    return dg_path_create(c, set.data(), set.size(), &e->ps); /* 16 zero bytes after the pool */
}

extern "C" {

int dg_editm_create(dg_ctx *c, const void *blob, size_t len, uint32_t op, dg_editm **out)
{
    dg_path_hdr h;
    if (int rc = edit_blob(blob, len, op, out, h)) return rc;
    const uint32_t K = h.n_paths;
    if (K > DG_EDITM_MAX_ITEMS) return set_err(DG_E_ARG, "editm: %u items (1 to %u)", K, DG_EDITM_MAX_ITEMS);
    const uint8_t *b = (const uint8_t *)blob;
    dg_path_ent pe[EM_MAX];
    memcpy(pe, b + sizeof(dg_path_hdr), K * sizeof(dg_path_ent));
    const uint32_t cnt = pe[0].count;
    if (cnt < 1) return set_err(DG_E_ARG, "editm: the empty path");
    const uint8_t *pool = b + h.off_pool;
    for (uint32_t j = 1; j < K; j++) {
        if (pe[j].count != cnt) return set_err(DG_E_ARG, "editm: paths of unequal length (%u and %u steps)", cnt, pe[j].count);
        for (uint32_t k = 0; k + 1 < cnt; k++) {
            const dg_path_step x = step_at(b, h, pe[0], k), y = step_at(b, h, pe[j], k);
            const bool pooled = x.kind == DG_PS_STRKEY || x.kind == DG_PS_BINKEY;
            if (x.kind != y.kind || x.key_len != y.key_len ||
                (pooled ? memcmp(pool + x.val, pool + y.val, x.key_len) != 0 : x.val != y.val))
                return set_err(DG_E_ARG, "editm: paths differ before their last step (path %u, step %u)", j, k);
        }
        if (step_class(step_at(b, h, pe[j], cnt - 1).kind) != step_class(step_at(b, h, pe[0], cnt - 1).kind))
            return set_err(DG_E_ARG, "editm: mixed step classes (item %u)", j);
    }
    std::unique_ptr<dg_editm> e(new dg_editm());
    if (int rc = edit_build(c, b, h, pe, op, e.get())) return rc;
    *out = e.release();
    return DG_OK;
}

/* the single edit's own refusals, then the many-edit's plan of one item */
int dg_edit_create(dg_ctx *c, const void *blob, size_t len, uint32_t op, dg_edit **out)
{
    dg_path_hdr h;
    if (int rc = edit_blob(blob, len, op, out, h)) return rc;
    if (h.n_paths != 1) return set_err(DG_E_ARG, "edit: %u paths (exactly 1)", h.n_paths);
    dg_path_ent pe;
    memcpy(&pe, (const uint8_t *)blob + sizeof(dg_path_hdr), sizeof pe);
    if (pe.count < 1) return set_err(DG_E_ARG, "edit: the empty path");
    std::unique_ptr<dg_edit> e(new dg_edit());
    if (int rc = edit_build(c, (const uint8_t *)blob, h, &pe, op, e.get())) return rc;
    *out = e.release();
    return DG_OK;
}

void dg_editm_destroy(dg_editm *e)
{
    if (!e) return;
    dg_path_destroy(e->ps);
    delete e;
}

void dg_edit_destroy(dg_edit *e) { dg_editm_destroy(e); }

uint32_t dg_editm_items(const dg_editm *e) { return e ? e->K : 0; }

uint64_t dg_editm_slot_bound(const dg_editm *e, uint64_t len, uint64_t val_total)
{
    if (!e) return 0;
    return e->op == DG_EDIT_SET ? len + val_total + e->extra : len;
}

uint64_t dg_edit_slot_bound(const dg_edit *e, uint64_t len, uint64_t val_len) { return dg_editm_slot_bound(e, len, val_len); }

int dg_editm_batch_device(dg_ctx *c, const dg_editm *e, uint8_t root_type, const uint8_t *d_thrift,
                          const uint64_t *d_in_off, uint64_t n, const uint8_t *val_types, const uint8_t *d_val,
                          const uint64_t *d_val_off, const uint64_t *val_lens, uint8_t *d_out,
                          const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, void *stream,
                          uint64_t max_len)
{
    Entry g(c, c && e && e->ctx == c, stream, "null ctx/edit, or an edit of another context");
    if (g.rc) return g.rc;
    return editm_launch(c, e, root_type,
                        EmBatch{d_thrift, d_in_off, n, val_types, d_val, d_val_off, val_lens, d_out, d_out_off,
                                d_out_len, d_ret, max_len},
                        g.s);
}

/* K = 1: the call's val_type and val_len are item 0's */
int dg_edit_batch_device(dg_ctx *c, const dg_edit *e, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, uint8_t val_type, const uint8_t *d_val,
                         const uint64_t *d_val_off, uint64_t val_len, uint8_t *d_out, const uint64_t *d_out_off,
                         uint32_t *d_out_len, uint64_t *d_ret, void *stream, uint64_t max_len)
{
    return dg_editm_batch_device(c, e, root_type, d_thrift, d_in_off, n, &val_type, d_val, d_val_off, &val_len, d_out,
                                 d_out_off, d_out_len, d_ret, stream, max_len);
}

/* every message in a slot of its exact bound (rounded up to 16: the packing
 * reads its slots as aligned words), one launch, packed on the device */
int dg_editm_batch_host(dg_ctx *c, const dg_editm *e, uint8_t root_type, const uint8_t *thrift,
                        const uint64_t *in_off, uint64_t n, const uint8_t *val_types, const uint8_t *val,
                        const uint64_t *val_off, const uint64_t *val_lens, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_off, uint64_t *ret, uint64_t *out_need)
{
    if (!c || !e || e->ctx != c) return set_err(DG_E_INVALID, "null ctx/edit, or an edit of another context");
    if (n == 0) return empty_batch(out_off, out_need);
    const bool set = e->op == DG_EDIT_SET;
    const uint64_t K = e->K;
    if (!thrift || !in_off || !out_off || !ret) return set_err(DG_E_INVALID, "null buffer");
    if (set && (!val_types || !val_lens)) return set_err(DG_E_INVALID, "null value types / lengths");
    if (!set) val = nullptr, val_off = nullptr;
    uint64_t shared = 0; /* the K values together when every message gets them */
    uint64_t max_val[EM_MAX] = {};
    if (set && !val_off)
        for (uint64_t j = 0; j < K; j++) shared += val_lens[j], max_val[j] = val_lens[j];
    if (!val && (val_off || shared)) return set_err(DG_E_INVALID, "null value buffer");
    Entry g(c, true);
    if (g.rc) return g.rc;
    HostBatch hb(c, g.s);
    int rc;
    if ((val_off && (rc = hb.values(val_off, n, K, max_val))) ||
        (rc = hb.layout(in_off, nullptr, n, [&](uint64_t i, uint64_t len) {
            return dg_editm_slot_bound(e, len, val_off ? hb.vo[(i + 1) * K] - hb.vo[i * K] : shared);
        })) ||
        (rc = hb.upload_messages(thrift, in_off)) || (rc = hb.upload_slots()) ||
        (rc = hb.upload_values(val, val_off, shared)))
        return rc;
    const EmBatch b{c->d_json, c->d_in_off, n, val_types, set ? (const uint8_t *)c->d_cb : nullptr,
                    val_off ? (const uint64_t *)c->d_aux : nullptr, max_val, c->d_out, c->d_out_off, c->d_out_len,
                    c->d_ret, hb.max_len};
    if ((rc = editm_launch(c, e, root_type, b, g.s))) return rc;
    return hb.pack_and_download(HostOut{out, out_cap, out_off, out_need}, ret);
}

int dg_edit_batch_host(dg_ctx *c, const dg_edit *e, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, uint8_t val_type, const uint8_t *val, const uint64_t *val_off, uint64_t val_len,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need)
{
    return dg_editm_batch_host(c, e, root_type, thrift, in_off, n, &val_type, val, val_off, &val_len, out, out_cap,
                               out_off, ret, out_need);
}

}  // extern "C"
