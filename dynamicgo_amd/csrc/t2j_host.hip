/*
 * t2j_host.hip — the C ABI of the reverse path, Thrift binary -> JSON
 * (include/dgj2t.h dg_desc_attach_t2j / dg_t2j_*; the reference's
 * t2j.BinaryConv.Do / DoInto, conv/t2j/conv.go:50-95). Kernels: t2j_device.h.
 */
#include <string.h>

#include "host_internal.h"
#include "t2j_device.h"

using namespace dg;

static const uint64_t T2J_DEEP_WS =
    (uint64_t)T2J_DEEP_BLOCKS * T2J_BLOCK * (T2J_DEEP_DEPTH * sizeof(T2JFrame) + (uint64_t)T2J_WIDE_WORDS * 8);

/* lanes per message of the LDS-frame pass (t2j_kern.hip) from the batch's
 * longest message: short messages want full waves, ~1 KB ones sparse waves;
 * unknown or huge (a mixed batch) keep the middle. the t2j_spread knob (1|2|4) forces. */
static uint32_t t2j_spread(const dg_ctx *c, uint64_t max_len)
{
    const int64_t v = c->knobs.t2j_spread;
    if (v) return v == 1 || v == 4 ? (uint32_t)v : 2u;
    if (max_len == 0 || max_len > 16384) return 2;
    return max_len <= 512 ? 1 : 4;
}

/* one batch on stream s. With the wave path (a descriptor that fits LDS and
 * messages that may be long): the lane pass converts the short messages and
 * lists the long ones, the wave kernel converts those (t2j_wave.h), the lane
 * pass in list mode converts the wave kernel's bails. Then the deep pass over
 * what the lane passes queued (it also zeroes the counter set the previous
 * launch used); the scratch's `done`
 * event after. */
static int t2j_launch(dg_ctx *c, const dg_desc *d, uint32_t root, const BatchArgs &b, hipStream_t s)
{
    const uint64_t n = b.n, opts = b.flags;
    if (n == 0) return DG_OK;
    if (!d->d_side) return set_err(DG_E_DESC, "descriptor has no t2j side table (dg_desc_attach_t2j)");
    if (root >= d->hdr.n_types) return set_err(DG_E_INVALID, "root type %u out of range", root);
    if (n > 0xFFFFFFFFull) return set_err(DG_E_INVALID, "batch of %llu messages", (unsigned long long)n);
    Scratch *x;
    int rc = scratch_for(c, s, &x);
    if (rc) return rc;
    if ((rc = x->grow(x->t2j_list, n))) return rc;
    if (!c->t2j_deep.ws && (rc = c->t2j_deep.ws.alloc(T2J_DEEP_WS))) return rc;
    const uint64_t wmin = (uint64_t)c->knobs.t2j_wave_min;
    /* the root-level Go-side options run on the lane kernel only */
    const bool wave = !(opts & (DG_T2J_CONVERT_EXC | DG_T2J_SKIP_RESP_BASE | DG_T2J_HM)) && wmin > 0 && d->hdr.total_len <= 16384 && d->hdr.n_fields <= 1024 && /* T2W_FX */
                      d->hdr.n_types < 4096 && /* a token's type index */
                      d->side_len <= 12288 /* T2W_SIDE */ && (b.max_len == 0 || b.max_len > wmin);
    if (wave) {
        if ((rc = x->grow(x->t2j_big, n))) return rc;
        if ((rc = x->grow(x->t2j_bail, n))) return rc;
        if (!c->t2j_tok.ws && (rc = c->t2j_tok.ws.alloc(t2j_wave_ws_bytes((uint32_t)c->n_cu * T2W_BPC)))) return rc;
    }
    /* overlapped form: the wave kernel (and its bails' list pass) on the
     * scratch's second stream, beside the lane pass over the short ones, so
     * the lane pass fills the CUs the persistent wave grid leaves idle */
    const bool ovl = wave && c->knobs.t2j_overlap != 0;
    if (ovl && !x->side) {
        HIPCHK(x->side.create(hipStreamNonBlocking));
        HIPCHK(x->side_go.create(hipEventDisableTiming));
        HIPCHK(x->side_done.create(hipEventDisableTiming));
    }
    hipStream_t ws = ovl ? (hipStream_t)x->side : s; /* the wave kernel's stream */
    /* one token workspace per context, like the deep workspace: a wave
     * pass on another stream waits for the previous one */
    if (wave) HIPCHK(c->t2j_tok.acquire(ws));
    /* this launch's counter set; its deep pass zeroes the other one */
    uint32_t *const cnt = x->t2j_cnt.mine();
    T2JParams P;
    memset(&P, 0, sizeof P);
    P.root = root;
    P.opts = opts;
    P.src = b.src;
    P.in_off = b.in_off;
    P.n = n;
    P.out = b.out;
    P.out_off = b.out_off;
    P.out_len = b.out_len;
    P.ret = b.ret;
    P.blob = d->d_blob;
    P.hdr = d->hdr;
    P.side = d->d_side;
    P.deep_list = x->t2j_list;
    P.deep_count = cnt + T2J_DEEPQ;
    P.reset_counts = x->t2j_cnt.other();
    P.ws = c->t2j_deep.ws;
    P.stats = c->d_stats;
    P.aux = (opts & DG_T2J_SKIP_RESP_BASE) ? b.aux : nullptr;
    P.ans_tab = (opts & DG_T2J_HM) ? b.hm.vm : nullptr;
    P.ans_bytes = b.hm.bytes;
    hipError_t e = hipSuccess;
    if (wave) {
        T2JParams P1 = P;
        P1.big_list = x->t2j_big;
        P1.big_count = cnt + T2J_BIG;
        P1.big_min = wmin;
        if (ovl) {
            launch_t2j_route(n, s, P1); /* the long ones, by length */
            if ((e = hipGetLastError()) == hipSuccess) e = hipEventRecord(x->side_go, s);
            if (e == hipSuccess) e = hipStreamWaitEvent(ws, x->side_go, 0);
            P1.skip_big = 1;
            P1.big_list = nullptr;
            P1.big_count = nullptr;
        }
        if (e == hipSuccess) launch_t2j_pass(n, s, P1, 1); /* the short ones: full waves */
        T2WParams W;
        W.list = x->t2j_big;
        W.count = cnt + T2J_BIG;
        W.queue = cnt + T2J_WAVEQ;
        W.bail_list = x->t2j_bail;
        W.bail_count = cnt + T2J_BAIL;
        const uint32_t wblocks = (uint32_t)c->n_cu * T2W_BPC; /* the token regions are sized for it */
        W.tok = c->t2j_tok.ws;
        W.side_len = (uint32_t)d->side_len;
        if (e == hipSuccess && (e = hipGetLastError()) == hipSuccess) {
            launch_t2j_wave(wblocks, ws, P, W);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            T2JParams P3 = P;
            P3.list = x->t2j_bail;
            P3.list_count = W.bail_count;
            launch_t2j_list(64, ws, P3);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = c->t2j_tok.publish(ws);
        if (ovl && e == hipSuccess) { /* the deep pass takes both passes' queue */
            e = hipEventRecord(x->side_done, ws);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, x->side_done, 0);
        }
    } else {
        launch_t2j_pass(n, s, P, t2j_spread(c, b.max_len));
        e = hipGetLastError();
    }
    /* the deep workspace is one per context: a deep pass on another stream
     * than the previous one waits for it (deep messages are rare; the LDS
     * passes of different streams still overlap) */
    if (e == hipSuccess) e = c->t2j_deep.acquire(s);
    if (e == hipSuccess) {
        launch_t2j_deep(s, P);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = c->t2j_deep.publish(s);
    x->t2j_cnt.finish(e == hipSuccess, s);
    HIPCHK(x->publish(s));
    if (e != hipSuccess) return set_err(DG_E_HIP, "t2j launch: %s", hipGetErrorString(e));
    return DG_OK;
}

extern "C" {

int dg_desc_attach_t2j(dg_desc *d, const void *side, size_t len)
{
    if (!d || !side || len < sizeof(dg_t2j_hdr)) return set_err(DG_E_INVALID, "bad args");
    dg_t2j_hdr h;
    memcpy(&h, side, sizeof h);
    if (h.magic != DG_T2J_MAGIC || h.version != 1 || h.total_len > len || h.n_fields != d->hdr.n_fields ||
        (uint64_t)h.off_fields + (uint64_t)h.n_fields * sizeof(dg_t2j_field) > len ||
        (uint64_t)h.off_pool + h.pool_len > len || (h.off_pool & 7))
        return set_err(DG_E_DESC, "bad t2j side table");
    /* every key range inside the pool (the kernel reads them unchecked) */
    const dg_t2j_field *f = (const dg_t2j_field *)((const uint8_t *)side + h.off_fields);
    for (uint32_t k = 0; k < h.n_fields; k++)
        if ((uint64_t)f[k].key_off + f[k].key_len > h.pool_len || (uint64_t)f[k].name_off + f[k].name_len > h.pool_len ||
            (f[k].key_off & 7) || (f[k].name_off & 7))
            return set_err(DG_E_DESC, "t2j side table: field %u key out of range", k);
    Entry g(d->ctx, true);
    if (g.rc) return g.rc;
    DevArr<uint8_t> p;
    if (int rc = p.alloc(len + 16)) return rc; /* the kernel reads whole words past a key's end */
    HIPCHK(hipMemcpy(p, side, len, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(p + len, 0, 16));
    HIPCHK(hipDeviceSynchronize()); /* before launches on non-blocking streams read it */
    if (d->d_side) HIPCHK(hipDeviceSynchronize()); /* launches in flight may read the old table */
    d->d_side = std::move(p); /* the old table, if any, is freed when p goes */
    d->side_len = len;
    return DG_OK;
}

/* 128-byte slots, like dg_slot_bound: t2j-c2's writes were 380 B per
 * message (every line its 208 B of JSON touched) at 8-byte alignment */
uint64_t dg_t2j_slot_bound(uint64_t len) { return (3 * len + 64 + 127) & ~127ull; }

int dg_t2j_batch_device_cb(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *d_thrift,
                           const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                           const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, uint64_t *d_aux,
                           const dg_cb_entry *d_ans, const uint8_t *d_ans_bytes, void *stream, uint64_t max_len)
{
    Entry g(c, c && d && !((opts & DG_T2J_SKIP_RESP_BASE) && !d_aux) && !(d_ans && !d_ans_bytes), stream);
    if (g.rc) return g.rc;
    BatchArgs b;
    b.src = d_thrift, b.in_off = d_in_off, b.n = n, b.flags = opts, b.max_len = max_len;
    b.out = d_out, b.out_off = d_out_off, b.out_len = d_out_len, b.ret = d_ret;
    b.aux = d_aux, b.hm.vm = d_ans, b.hm.bytes = d_ans_bytes;
    return t2j_launch(c, d, root, b, g.s);
}

/* the forms without callback answers, without spans, without max_len */
int dg_t2j_batch_device_aux(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *d_thrift,
                            const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                            const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, uint64_t *d_aux,
                            void *stream, uint64_t max_len)
{
    return dg_t2j_batch_device_cb(c, d, root, d_thrift, d_in_off, n, opts, d_out, d_out_off, d_out_len, d_ret, d_aux,
                                  nullptr, nullptr, stream, max_len);
}

int dg_t2j_batch_device_ml(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *d_thrift,
                           const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                           const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, void *stream,
                           uint64_t max_len)
{
    Entry g(c, c && d, stream, "null ctx/desc");
    if (g.rc) return g.rc;
    BatchArgs b;
    b.src = d_thrift, b.in_off = d_in_off, b.n = n, b.flags = opts, b.max_len = max_len;
    b.out = d_out, b.out_off = d_out_off, b.out_len = d_out_len, b.ret = d_ret;
    return t2j_launch(c, d, root, b, g.s);
}

int dg_t2j_batch_device(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *d_thrift, const uint64_t *d_in_off,
                        uint64_t n, uint64_t opts, uint8_t *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                        uint64_t *d_ret, void *stream)
{
    return dg_t2j_batch_device_ml(c, d, root, d_thrift, d_in_off, n, opts, d_out, d_out_off, d_out_len, d_ret, stream,
                                  0);
}

/* in: host pointers (src, in_off, n, flags = the options, ret, aux) */
static int t2j_batch_host(dg_ctx *c, const dg_desc *d, uint32_t root, const BatchArgs &in, const HostOut &o,
                          const dg_cb_tables *cb)
{
    const uint8_t *const thrift = in.src;
    const uint64_t *const in_off = in.in_off, n = in.n, opts = in.flags;
    uint8_t *const out = o.out;
    uint64_t *const out_off = o.out_off, *const ret = in.ret, *const aux = in.aux;
    if (!c || !d || (!thrift && n) || !in_off || !out_off || (!ret && n) ||
        ((opts & DG_T2J_SKIP_RESP_BASE) && n && !aux) || (cb && cb->ans_tab && cb->len && !cb->bytes))
        return set_err(DG_E_INVALID, "bad args");
    const dg_cb_entry *ans = cb && (opts & DG_T2J_HM) ? cb->ans_tab : nullptr;
    for (uint64_t i = 0; ans && i < n; i++) /* one byte per answer, inside the bytes (read unchecked) */
        if (ans[i].off + ans[i].count > cb->len)
            return set_err(DG_E_INVALID, "callback answers of message %llu outside the bytes", (unsigned long long)i);
    Entry g(c, true);
    if (g.rc) return g.rc;
    if (n == 0) return empty_batch(out_off, o.out_need);
    /* what a copy reads or writes is declared before the batch, whose destructor waits for the copies */
    std::vector<uint64_t> todo, slot_of(n, 0), r, ax; /* slot_of: stage offset of message i's final bytes */
    std::vector<uint32_t> olen(n, 0), l;
    std::vector<uint8_t> stage;
    std::vector<dg_cb_entry> e; /* the rerun's answer entries */
    HostBatch hb(c, g.s);
    int rc;
    /* pass 0: every message in a dg_t2j_slot_bound slot; pass 1: the
     * overflowed ones again, each in a slot of the size it reported + 64.
     * Each pass downloads its whole slot arena: which statuses keep their bytes
     * is t2j's own rule, and an overflowed message's length is what it needs. */
    for (int pass = 0; pass < 2 && (pass == 0 || !todo.empty()); pass++) {
        const uint64_t m = pass ? todo.size() : n;
        r.resize(m), l.resize(m), ax.resize(aux ? m : 0);
        if ((rc = hb.layout(in_off, pass ? todo.data() : nullptr, m, [&](uint64_t i, uint64_t len) -> uint64_t {
                return pass == 0 ? dg_t2j_slot_bound(len) : (uint64_t)olen[i] + 64;
            })) ||
            (rc = hb.upload_messages(thrift, in_off)) || (rc = hb.upload_slots(false)) ||
            (aux && (rc = c->d_aux.grow(m + 1))))
            return rc;
        BatchArgs b;
        b.src = c->d_json, b.in_off = c->d_in_off, b.n = m, b.flags = opts, b.max_len = hb.max_len;
        b.out = c->d_out, b.out_off = c->d_out_off, b.out_len = c->d_out_len, b.ret = c->d_ret;
        if (aux) b.aux = c->d_aux;
        if (ans) { /* [m entries | the answer bytes]; the rerun's entries gathered */
            e.resize(pass ? m : 0);
            for (uint64_t k = 0; k < e.size(); k++) e[k] = ans[todo[k]];
            if ((rc = c->d_cb.grow(8 * m + cb->len + 8)) ||
                (rc = hb.copy(c->d_cb, pass ? e.data() : ans, 8 * m, hipMemcpyHostToDevice)) ||
                (rc = hb.copy(c->d_cb + 8 * m, cb->bytes, cb->len, hipMemcpyHostToDevice)))
                return rc;
            b.hm.vm = (const dg_cb_entry *)(const void *)(uint8_t *)c->d_cb, b.hm.bytes = c->d_cb + 8 * m;
        }
        if ((rc = t2j_launch(c, d, root, b, g.s))) return rc;
        const uint64_t off0 = stage.size(), slots = hb.so[m];
        stage.resize(off0 + slots);
        if ((rc = hb.copy(ax.data(), c->d_aux, ax.size() * 8, hipMemcpyDeviceToHost)) ||
            (rc = hb.copy(r.data(), c->d_ret, m * 8, hipMemcpyDeviceToHost)) ||
            (rc = hb.copy(l.data(), c->d_out_len, m * 4, hipMemcpyDeviceToHost)) ||
            (rc = hb.copy(stage.data() + off0, c->d_out, slots, hipMemcpyDeviceToHost)) || (rc = hb.sync()))
            return rc;
        std::vector<uint64_t> next;
        for (uint64_t k = 0; k < m; k++) {
            const uint64_t i = pass ? todo[k] : k;
            ret[i] = r[k];
            olen[i] = l[k];
            if (aux) aux[i] = ax[k];
            slot_of[i] = off0 + hb.so[k];
            if ((uint8_t)r[k] == DG_ST_OUT_OVERFLOW) {
                if (pass == 1)
                    return set_err(DG_E_NOMEM, "message %llu overflowed its exact-size slot", (unsigned long long)i);
                next.push_back(i);
            }
        }
        todo.swap(next);
    }
    uint64_t total = 0;
    out_off[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (ret[i] != 0 && (uint8_t)ret[i] != DG_T2J_E_EXCEPTION && (uint8_t)ret[i] != DG_T2J_E_CALLBACK)
            olen[i] = 0; /* kept: the exception's JSON, a stop's record */
        total += olen[i];
        out_off[i + 1] = total;
    }
    if (o.out_need) *o.out_need = total;
    if (total > o.out_cap || (!out && total)) return set_err(DG_E_NOMEM, "output needs %llu bytes", (unsigned long long)total);
    for (uint64_t i = 0; i < n; i++)
        if (olen[i]) memcpy(out + out_off[i], stage.data() + slot_of[i], olen[i]);
    return DG_OK;
}

int dg_t2j_batch_host_cb(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *thrift, const uint64_t *in_off,
                         uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret,
                         uint64_t *out_need, uint64_t *aux, const dg_cb_tables *cb)
{
    BatchArgs in;
    in.src = thrift, in.in_off = in_off, in.n = n, in.flags = opts, in.ret = ret, in.aux = aux;
    return t2j_batch_host(c, d, root, in, HostOut{out, out_cap, out_off, out_need}, cb);
}

int dg_t2j_batch_host_aux(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *thrift, const uint64_t *in_off,
                          uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret,
                          uint64_t *out_need, uint64_t *aux)
{
    return dg_t2j_batch_host_cb(c, d, root, thrift, in_off, n, opts, out, out_cap, out_off, ret, out_need, aux, nullptr);
}

int dg_t2j_batch_host(dg_ctx *c, const dg_desc *d, uint32_t root, const uint8_t *thrift, const uint64_t *in_off,
                      uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret,
                      uint64_t *out_need)
{
    return dg_t2j_batch_host_cb(c, d, root, thrift, in_off, n, opts, out, out_cap, out_off, ret, out_need, nullptr,
                                nullptr);
}

}  // extern "C"
