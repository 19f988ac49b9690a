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
    int rc;
    if (c->edit_rec.cap < 2 * n) { /* the previous launch may still read the old records */
        HIPCHK(c->edit.wait_host());
        if ((rc = c->edit_rec.grow(2 * n))) return rc;
    }
    HIPCHK(c->edit.acquire(s));
    rc = DG_OK;
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
        /* a route no message can take is not launched: the lane route when
         * every output takes the wave route, the wave route when the hints
         * bound every output below wave_min (per-message values: val_len is
         * the longest value, 0 = unknown) */
        const bool hinted = b.max_len && !(set && b.val_off && !b.val_len);
        const bool no_wave = hinted && dg_edit_slot_bound(e, b.max_len, b.val_len) < A.wave_min;
        if (A.wave_min) {
            const int64_t g = c->knobs.edit_lanes;
            launch_edit_lane(s, A, g == 4 || g == 16 ? (uint32_t)g : 1u);
            err = hipGetLastError();
        }
        if (err == hipSuccess && !no_wave) {
            const uint64_t want = (n + ED_WAVES - 1) / ED_WAVES;
            launch_edit_wave(s, A, (uint32_t)std::min<uint64_t>(want, (uint64_t)c->n_cu * 8));
            err = hipGetLastError();
        }
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
    e->extra = last.kind == DG_PS_FIELD ? 3u : last.kind == DG_PS_INDEX ? 0u : last.kind == DG_PS_STRKEY ? 4u + last.key_len
               : last.kind == DG_PS_BINKEY ? last.key_len : 8u;
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
    if (n == 0) {
        if (out_off) out_off[0] = 0;
        if (out_need) *out_need = 0;
        return DG_OK;
    }
    const bool set = e->step.op == DG_EDIT_SET;
    if (!thrift || !in_off || !out_off || !ret) return set_err(DG_E_INVALID, "null buffer");
    if (!set) val = nullptr, val_off = nullptr, val_len = 0;
    if (!val && (val_off || val_len)) return set_err(DG_E_INVALID, "null value buffer");
    std::vector<uint64_t> io(n + 1), so(n + 1), vo;
    uint64_t max_len = 0, max_val = val_len;
    io[0] = so[0] = 0;
    if (val_off) {
        vo.resize(n + 1);
        max_val = 0;
    }
    for (uint64_t i = 0; i < n; i++) {
        if (in_off[i + 1] < in_off[i]) return set_err(DG_E_INVALID, "in_off not ascending");
        if (val_off && val_off[i + 1] < val_off[i]) return set_err(DG_E_INVALID, "val_off not ascending");
        const uint64_t len = in_off[i + 1] - in_off[i], vl = val_off ? val_off[i + 1] - val_off[i] : val_len;
        const uint64_t cap = dg_edit_slot_bound(e, len, vl);
        if (cap > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "message %llu: an output of %llu bytes", (unsigned long long)i,
                                                (unsigned long long)cap);
        io[i + 1] = io[i] + len;
        so[i + 1] = so[i] + ((cap + 15) & ~15ull);
        if (val_off) vo[i] = val_off[i] - val_off[0], vo[i + 1] = val_off[i + 1] - val_off[0];
        max_len = std::max(max_len, len), max_val = std::max(max_val, vl);
    }
    const uint64_t vtotal = val_off ? vo[n] : val_len;
    Entry g(c, true);
    if (g.rc) return g.rc;
    const hipStream_t s = g.s;
    int rc;
    if ((rc = c->d_json.grow(io[n] + 64)) || (rc = c->d_in_off.grow(n + 1)) || (rc = c->d_out.grow(so[n] + 64)) ||
        (rc = c->d_out_off.grow(n + 1)) || (rc = c->d_out_len.grow(n + 1)) || (rc = c->d_ret.grow(n + 1)) ||
        (rc = c->d_pack.grow(so[n] + 64)) || (rc = c->d_pack_off.grow(n + 1)) || (rc = c->d_cb.grow(vtotal + 64)) ||
        (rc = c->d_aux.grow(n + 1)))
        return rc;
    if (io[n]) HIPCHK(hipMemcpyAsync(c->d_json, thrift + in_off[0], io[n], hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->d_json + io[n], 0, 64, s));
    if (vtotal) HIPCHK(hipMemcpyAsync(c->d_cb, val + (val_off ? val_off[0] : 0), vtotal, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->d_cb + vtotal, 0, 64, s));
    if (val_off) HIPCHK(hipMemcpyAsync(c->d_aux, vo.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_in_off, io.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_out_off, so.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    const EditBatch b{c->d_json, c->d_in_off, n, val_type, set ? (const uint8_t *)c->d_cb : nullptr,
                      val_off ? (const uint64_t *)c->d_aux : nullptr, val_off ? max_val : val_len, c->d_out,
                      c->d_out_off, c->d_out_len, c->d_ret, max_len};
    if ((rc = edit_launch(c, e, root_type, b, s))) {
        (void)hipStreamSynchronize(s); /* the uploads read locals */
        return rc;
    }
    BatchArgs pb; /* the packing goes by the lengths: 0 for every failed message (no slot can overflow) */
    pb.out = c->d_out, pb.out_off = c->d_out_off, pb.out_len = c->d_out_len, pb.n = n;
    if ((rc = dg_i_pack_scan(c, s, pb, c->d_pack, c->d_pack_off))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    HIPCHK(hipMemcpyAsync(ret, c->d_ret, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_off, c->d_pack_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t total = out_off[n];
    if (out_need) *out_need = total;
    if (total > out_cap || (!out && total)) return set_err(DG_E_NOMEM, "output needs %llu bytes", (unsigned long long)total);
    if (total) {
        HIPCHK(hipMemcpyAsync(out, c->d_pack, total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return DG_OK;
}

}  // extern "C"
