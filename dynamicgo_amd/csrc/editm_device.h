/*
 * editm_device.h — batched SetMany (include/dgj2t.h dg_editm_*): the device
 * restatement of the reference's SetMany + replaceMany (thrift/generic/
 * node.go:930-1007) and its UNSET counterpart over K + 1 records of the path
 * lookup: `parent` and the K full paths, each the parent plus one last step.
 *
 * editm_decide calls edit_decide (edit_device.h) once per item, orders the K
 * cuts by where they start in the message (inserts, which are empty cuts, before
 * a cut that starts at the same byte; equal keys in item order), refuses cuts
 * that overlap, folds the inserts' or drops' count patches into one and lays out
 * the segment table. The output of a message is then, for each cut c in order,
 *
 *   msg[g_c, a1_c) | generated (<= 8 bytes, in a register) | key (path pool) | value
 *
 * (g_0 = 0, g_c = the end of cut c - 1) and at last msg[g_K, len), with the
 * container's 4-byte count, which lies in front of the first cut, replaced.
 * em_splice writes it in 16-byte units aligned on the DESTINATION, each
 * assembled by em_fetch from every run that covers it (up to 4 K + 1; the
 * patched count is folded in before the store), so a store never mixes lanes
 * and no byte is stored twice. The head up to the first boundary and the tail
 * after the last are clipped to the byte.
 *
 * Everything is a template over K: every index into the table is a constant once
 * the loops are unrolled, so the table lives in registers (a private array
 * indexed by a variable goes to scratch memory). The K cuts are sorted by a
 * bubble network of compare-exchanges for the same reason. The lanes that share
 * a message are a template parameter too (1, 4 or 16: the lane route, 64: the
 * wave route). Compiles for the host like edit_device.h (EDI, TGI).
 *
 * Bounds: as edit_device.h. Reads run at most 15 bytes past a run's end (message
 * and value arenas readable 16 bytes past their ends, 16 zero bytes after the
 * path blob); writes are exactly [dst, dst + out_len), and only when out_len
 * fits the slot.
 */
#pragma once
#include "edit_device.h"

namespace dg {

constexpr uint32_t EM_MAX = DG_EDITM_MAX_ITEMS;

/* item j of the many-edit: its last step and its value (val_pos / val_len: where
 * it lies in `val` when every message gets the same values) */
struct EmItem {
    uint32_t kind, key_len;
    int64_t kval;
    uint32_t val_type, key_off; /* key_off: the step's key bytes in the path blob (key kinds) */
    uint64_t val_pos, val_len;
};

struct EmParams {
    uint32_t op, n_steps, K; /* n_steps of a full path (>= 1) */
    EmItem it[EM_MAX];
    const uint8_t *pool; /* the path blob on the device, 16 zero bytes after it */
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    const dg_tget_rec *rec; /* (K + 1) n: parent, full_1 .. full_K per message */
    const uint8_t *val;
    const uint64_t *val_off; /* n K + 1, message-major; null: it[j].val_pos / val_len for every message */
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint64_t *ret;
    uint64_t wave_min;
};

/* one cut: msg[a1, suf) becomes gen[0, gl) + pool[koff, koff + kl) + vp[0, vl) */
struct EmCut {
    uint32_t a1, suf, gl, kl, koff, vl, idx;
    uint64_t gen;
    const uint8_t *vp;
};

/* the segment table of one message: cut c's gap msg[g[c], c[c].a1) starts at
 * output offset o[c]; the final suffix msg[g[K], len) at o[K]; total bytes */
template <uint32_t KT>
struct EmSrc {
    const uint8_t *msg, *pool;
    uint32_t g[KT + 1], o[KT + 1];
    EmCut c[KT];
    uint32_t total, patch, cpos;
    uint64_t cntb; /* the new count's four bytes, first byte lowest */
};

struct EmDec {
    uint32_t status, aux, item, mask;
    uint64_t need;
};

/* the wave route: one message per wave, so the table is the same in every lane. Read back through
 * readfirstlane it is a scalar to the compiler and lives in SGPRs (the ones that do not fit are kept in the
 * lanes of a few VGPRs), not in one VGPR per entry */
#if defined(__HIP_DEVICE_COMPILE__)
EDI uint32_t em_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
#else
EDI uint32_t em_u32(uint32_t x) { return x; }
#endif
EDI uint64_t em_u64(uint64_t x) { return em_u32((uint32_t)x) | (uint64_t)em_u32((uint32_t)(x >> 32)) << 32; }
EDI const uint8_t *em_up(const uint8_t *p) { return (const uint8_t *)(uintptr_t)em_u64((uint64_t)(uintptr_t)p); }

EDI TGRes em_ures(const TGRes &r)
{
    return TGRes{em_u32(r.start), em_u32(r.end), em_u32(r.type), em_u32(r.status), em_u32(r.step), em_u32(r.aux)};
}

template <uint32_t KT>
EDI void em_uniform(EmSrc<KT> &S)
{
    S.msg = em_up(S.msg), S.pool = em_up(S.pool);
    S.total = em_u32(S.total), S.patch = em_u32(S.patch), S.cpos = em_u32(S.cpos), S.cntb = em_u64(S.cntb);
#pragma unroll
    for (uint32_t c = 0; c <= KT; c++) S.g[c] = em_u32(S.g[c]), S.o[c] = em_u32(S.o[c]);
#pragma unroll
    for (uint32_t c = 0; c < KT; c++) {
        EmCut &x = S.c[c];
        x.a1 = em_u32(x.a1), x.suf = em_u32(x.suf), x.gl = em_u32(x.gl), x.kl = em_u32(x.kl), x.koff = em_u32(x.koff);
        x.vl = em_u32(x.vl), x.idx = em_u32(x.idx), x.gen = em_u64(x.gen), x.vp = em_up(x.vp);
    }
}

/* x comes after y: it starts later, or at the same byte and y is an insert while x is not.
 * "Inserts first" is needed beside (a1, item index): a list's or map's header ends where its
 * first entry starts, so an insert (a1 = suf = that byte) and a replace or drop of entry 0
 * (a1 = that byte, suf behind it) share a1. Were the replace given first it would sort in
 * front, the new entries would land behind the replaced one instead of at the front, and
 * suf > the insert's a1 would report the legal pair as DG_EDITM_E_SAME. */
EDI bool em_after(const EmCut &x, const EmCut &y)
{
    return x.a1 > y.a1 || (x.a1 == y.a1 && x.suf > x.a1 && y.suf == y.a1);
}

template <uint32_t KT>
EDI EmDec editm_decide(const EmParams &A, const TGRes &par, const TGRes (&full)[KT], const uint8_t *b, uint64_t len,
                       const uint8_t *const (&vp)[KT], const uint64_t (&vl)[KT], EmSrc<KT> &S)
{
    EmDec R = {};
    uint32_t np = 0, cnt0 = 0;
    uint64_t add = 0;
    bool failed = false;
    S.msg = b, S.pool = A.pool, S.cpos = 0;
#pragma unroll
    for (uint32_t j = 0; j < KT; j++) {
        const EditStep st{A.op, A.n_steps, A.it[j].kind, A.it[j].key_len, A.it[j].kval, A.it[j].val_type};
        const EditDec D = edit_decide(st, par, full[j], b, len);
        if (D.status != DG_EDIT_OK && !failed) failed = true, R.status = D.status, R.aux = D.aux, R.item = j;
        R.mask |= D.existed << j;
        if (D.patch) {
            if (!np) S.cpos = D.cpos, cnt0 = D.cnt;
            np++;
        }
        const uint64_t v = D.use_val ? vl[j] : 0;
        add += v;
        S.c[j] = EmCut{D.a1, D.suf, D.gen_len, D.key_len, A.it[j].key_off, (uint32_t)v, j, D.gen, vp[j]};
    }
    if (failed) {
        R.mask = 0;
        return R;
    }
    /* by (a1, inserts first), stable: a bubble network, every index a constant */
#pragma unroll
    for (uint32_t p = 0; p + 1 < KT; p++) {
#pragma unroll
        for (uint32_t q = 0; q + 1 < KT - p; q++) {
            const EmCut x = S.c[q], y = S.c[q + 1];
            const bool sw = em_after(x, y);
            S.c[q] = sw ? y : x;
            S.c[q + 1] = sw ? x : y;
        }
    }
    bool same = false;
#pragma unroll
    for (uint32_t c = 0; c + 1 < KT; c++)
        if (S.c[c].suf > S.c[c + 1].a1 && !same) same = true, R.item = S.c[c + 1].idx;
    if (same) {
        R.status = DG_EDITM_E_SAME, R.mask = 0;
        return R;
    }
    /* the offsets are 32 bits wide: they are used only when `need`, summed in 64 bits, fits a slot */
    uint32_t g = 0, o = 0;
    uint64_t kept = 0;
#pragma unroll
    for (uint32_t c = 0; c < KT; c++) {
        S.g[c] = g, S.o[c] = o;
        const uint64_t fix = (uint64_t)(S.c[c].a1 - g) + S.c[c].gl + S.c[c].kl;
        o += (uint32_t)fix + S.c[c].vl, kept += fix;
        g = S.c[c].suf;
    }
    S.g[KT] = g, S.o[KT] = o;
    R.need = kept + add + (len - g);
    S.total = (uint32_t)R.need;
    S.patch = np != 0;
    S.cntb = __builtin_bswap32(cnt0 + (np - (np != 0)) * (A.op == DG_EDIT_SET ? 1u : ~0u));
    return R;
}

/* the output bytes [o, o + 16) (those at or past total are not defined) */
template <uint32_t KT>
EDI TGWin em_fetch(const EmSrc<KT> &S, uint64_t o)
{
    TGWin r{0, 0};
    if (o + 16 <= S.c[0].a1) {
        r = tg_ld(S.msg + o);
    } else if (o >= S.o[KT]) {
        r = tg_ld(S.msg + S.g[KT] + (o - S.o[KT]));
    } else {
#pragma unroll
        for (uint32_t c = 0; c < KT; c++) {
            if (S.o[c + 1] <= o || o + 16 <= S.o[c]) continue;
            uint64_t x = S.o[c], e = x + (S.c[c].a1 - S.g[c]);
            ed_run(r, o, x, e, S.msg + S.g[c]);
            x = e, e += S.c[c].gl;
            ed_reg(r, o, x, e, S.c[c].gen);
            x = e, e += S.c[c].kl;
            ed_run(r, o, x, e, S.pool + S.c[c].koff);
            x = e, e += S.c[c].vl;
            ed_run(r, o, x, e, S.c[c].vp);
        }
        ed_run(r, o, S.o[KT], S.total, S.msg + S.g[KT]);
    }
    if (S.patch) ed_reg(r, o, S.cpos, (uint64_t)S.cpos + 4, S.cntb);
    return r;
}

/* lane `lane` of LANES writes its share of the output to d[0, total): the
 * aligned units in strides of LANES, then, as two more pieces of the same loop,
 * the head up to d's next 16-byte boundary and the tail after the last unit */
template <uint32_t KT, uint32_t LANES>
EDI void em_splice(const EmSrc<KT> &S, uint8_t *d, uint32_t lane)
{
    const uint64_t n = S.total;
    uint64_t h = (16 - ((uintptr_t)d & 15)) & 15;
    if (h > n) h = n;
    const uint64_t body = (n - h) >> 4, t0 = h + body * 16;
    for (uint64_t c = lane; c < body + 2; c += LANES) {
        const uint64_t off = c < body ? h + c * 16 : c == body ? 0 : t0;
        const uint32_t nb = c < body ? 16u : c == body ? (uint32_t)h : (uint32_t)(n - t0);
        if (!nb) continue;
        const TGWin w = em_fetch(S, off);
        if (nb == 16) __builtin_memcpy(__builtin_assume_aligned(d + off, 16), &w, 16);
        else ed_store(d + off, w, nb);
    }
}

/* message i for lane `lane` of the LANES that share it (WAVE: the wave route,
 * else the lane route with 1, 4 or 16 lanes a message); a message whose route
 * is the other one is left to it. Lane 0 stores out_len and ret. */
template <uint32_t KT, uint32_t LANES, bool WAVE>
EDI void editm_message(const EmParams &A, uint64_t i, uint32_t lane)
{
    const uint64_t a = WAVE ? em_u64(A.in_off[i]) : A.in_off[i], len = (WAVE ? em_u64(A.in_off[i + 1]) : A.in_off[i + 1]) - a;
    const uint8_t *b = A.src + a;
    const uint64_t q = i * (KT + 1);
    const TGRes par = WAVE ? em_ures(ed_rec(A.rec, q)) : ed_rec(A.rec, q);
    TGRes full[KT];
    const uint8_t *vp[KT];
    uint64_t vl[KT];
    /* the lookup's spans lie inside the message; records of another batch (the
     * edit_reuse_rec knob misused) must not take a read outside it */
    bool sane = par.start <= par.end && par.end <= len;
#pragma unroll
    for (uint32_t j = 0; j < KT; j++) {
        full[j] = WAVE ? em_ures(ed_rec(A.rec, q + 1 + j)) : ed_rec(A.rec, q + 1 + j);
        sane = sane && full[j].start <= full[j].end && full[j].end <= len;
        if (A.val_off) {
            const uint64_t v0 = WAVE ? em_u64(A.val_off[i * KT + j]) : A.val_off[i * KT + j];
            vp[j] = A.val + v0, vl[j] = (WAVE ? em_u64(A.val_off[i * KT + j + 1]) : A.val_off[i * KT + j + 1]) - v0;
        } else {
            vp[j] = A.val + A.it[j].val_pos, vl[j] = A.it[j].val_len;
        }
    }
    EmSrc<KT> S;
    EmDec D = {};
    if (sane) D = editm_decide<KT>(A, par, full, b, len, vp, vl, S);
    else D.status = DG_EDIT_E_READ;
    const uint64_t need = D.status == DG_EDIT_OK ? D.need : 0;
    if ((need >= A.wave_min) != WAVE) return;
    const uint64_t cap = A.out_off[i + 1] - A.out_off[i];
    uint64_t ret = D.status | (uint64_t)D.item << 16 | (uint64_t)D.aux << 32;
    uint32_t olen = 0;
    if (D.status == DG_EDIT_OK) {
        if (need > cap || need > 0xFFFFFFFFull) {
            olen = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)need;
            ret = DG_EDIT_E_OVERFLOW | (uint64_t)olen << 32;
        } else {
            olen = (uint32_t)need;
            ret |= (uint64_t)D.mask << 8;
            if (WAVE) em_uniform(S);
            em_splice<KT, LANES>(S, A.out + A.out_off[i], lane);
        }
    }
    if (lane == 0) {
        A.out_len[i] = olen;
        A.ret[i] = ret;
    }
}

void launch_editm_lane(hipStream_t s, const EmParams &A, uint32_t lanes); /* lanes a message: 1, 4 or 16 */
void launch_editm_wave(hipStream_t s, const EmParams &A, uint32_t blocks);

}  // namespace dg
