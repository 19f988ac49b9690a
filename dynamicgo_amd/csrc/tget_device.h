/*
 * tget_device.h — batched GetByPath over Thrift binary (include/dgj2t.h
 * dg_tget_*): the device restatement of the reference's path search
 * (thrift/generic/node.go:292-484 with value.go:113-143's LIST/SET rule) over
 * its Read*Begin checks (thrift/binary.go:562-649,737-791) and skipType
 * (thrift/binary_skip.go:109-204).
 *
 * One lane walks one (message, path) pair. The walk is a chain of dependent
 * loads, one per field header: every header is read as ONE 16-byte window at
 * the read position, which also holds the header of the value behind it (a
 * string's size, a list's or map's header), so a skipped field costs one load.
 * The skipper is iterative: a frame per open container (element wire types +
 * entries left; a struct needs no count) in LDS, TG_LDS_DEPTH per lane; a value
 * nested deeper ends the lane with TG_ST_DEEP and the pair is rerun by the deep
 * kernel with TG_DEEP_DEPTH frames in device memory.
 *
 * Bounds: the read position p never passes the message length (every advance
 * is checked against it first), and a window reads 16 bytes at p, so at most 16
 * bytes past the message: the arena is readable that far past its end.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dgj2t.h"

namespace dg {

#ifndef TGI /* a host build of the walk (a CPU check against the checker) defines it as `inline` */
#define TGI __device__ __forceinline__
#endif

constexpr uint32_t TG_BLOCK = 256;
constexpr uint32_t TG_LDS_DEPTH = 8;      /* skip frames per lane in LDS (16 KB a block) */
constexpr uint32_t TG_DEEP_DEPTH = 1024;  /* ... per lane of the deep pass: MaxSkipDepth 1023 opens at most 1023 */
constexpr uint32_t TG_DEEP_BLOCK = 64, TG_DEEP_BLOCKS = 64;
constexpr uint32_t TG_DEEP_LANES = TG_DEEP_BLOCK * TG_DEEP_BLOCKS;
constexpr uint32_t TG_MAX_SKIP = 1023;    /* thrift.MaxSkipDepth (binary_skip.go:24) */
constexpr uint32_t TG_ST_DEEP = 0xF1;     /* internal: rerun with the deep frames */

enum : uint8_t { TT_STOP = 0, TT_BYTE = 3, TT_I16 = 6, TT_I32 = 8, TT_I64 = 10, TT_STRING = 11, TT_STRUCT = 12,
                 TT_MAP = 13, TT_SET = 14, TT_LIST = 15 };

struct TGParams {
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t pairs;        /* n * P */
    uint32_t P;
    uint32_t root_type;
    const uint8_t *blob;   /* the path set (dg_path_hdr ...), 16 zero bytes after it */
    uint32_t off_steps, off_pool;
    dg_tget_rec *rec;
    uint64_t *val_off;
    uint32_t *val_len;
    uint32_t *deep_list;   /* pairs queued for the deep pass */
    uint32_t *deep_count;
    uint32_t *reset_count; /* the other launch's counter, zeroed by the deep pass */
    uint64_t *ws;          /* deep frames: [level * TG_DEEP_LANES + lane] */
};

/* typeSize (binary_skip.go:26-41): > 0 for BOOL, I08, DOUBLE, I16, I32, I64 */
TGI uint32_t tg_fixed(uint32_t t)
{
    const uint64_t tab = (1ull << 8) | (1ull << 12) | (8ull << 16) | (2ull << 24) | (4ull << 32) | (8ull << 40);
    return t < 16 ? (uint32_t)(tab >> (t * 4)) & 15u : 0u;
}

/* Type.Valid (thrift/descriptor.go:60-67) */
TGI bool tg_valid(uint32_t t) { return t < 18 && ((0x3FD5Fu >> t) & 1u); }

/* 16 bytes at any alignment, as two little-endian words */
struct TGWin {
    uint64_t lo, hi;
};
TGI TGWin tg_ld(const uint8_t *b)
{
    TGWin w;
    __builtin_memcpy(&w, b, 16);
    return w;
}
/* the window's bytes from k on (k <= 8: eight of them; k <= 12: at least four) */
TGI uint64_t tg_at(const TGWin &w, uint32_t k)
{
    if (k == 0) return w.lo;
    if (k >= 8) return w.hi >> ((k - 8) * 8);
    return (w.lo >> (k * 8)) | (w.hi << (64 - k * 8));
}
TGI uint32_t tg_u8(const TGWin &w, uint32_t k) { return (uint32_t)tg_at(w, k) & 0xFFu; }
TGI uint32_t tg_be32(const TGWin &w, uint32_t k) { return __builtin_bswap32((uint32_t)tg_at(w, k)); }
TGI int32_t tg_be16(const TGWin &w, uint32_t k) { return (int16_t)__builtin_bswap16((uint16_t)tg_at(w, k)); }

/* n bytes at a and b equal (both readable 16 bytes past their n) */
TGI bool tg_eq(const uint8_t *a, const uint8_t *b, uint64_t n)
{
    for (uint64_t q = 0; q < n; q += 16) {
        const TGWin x = tg_ld(a + q), y = tg_ld(b + q);
        const uint64_t r = n - q;
        uint64_t dl = x.lo ^ y.lo, dh = x.hi ^ y.hi;
        if (r < 8) {
            dl &= (1ull << (r * 8)) - 1;
            dh = 0;
        } else if (r < 16) {
            dh &= r == 8 ? 0ull : (1ull << ((r - 8) * 8)) - 1;
        }
        if (dl | dh) return false;
    }
    return true;
}

/* a lane's frames: bits 0-31 the entries left (a map counts keys and values:
 * even = a key is next), 32-39 / 40-47 the key and value wire types (a list:
 * its element type twice), bit 48 clear for a struct */
struct TGLdsFrames {
    static constexpr uint32_t cap = TG_LDS_DEPTH;
    uint64_t *base; /* &frames[threadIdx.x]; level l at base[l * TG_BLOCK] */
    TGI uint64_t &at(uint32_t l) const { return base[l * TG_BLOCK]; }
};
struct TGDeepFrames {
    static constexpr uint32_t cap = TG_DEEP_DEPTH;
    uint64_t *base;
    TGI uint64_t &at(uint32_t l) const { return base[(uint64_t)l * TG_DEEP_LANES]; }
};

enum : uint32_t { TG_R_OK = 0, TG_R_FAIL = 1, TG_R_DEEP = 2 };

/* One value of wire type t at b[p], met with sp frames open; w = the window
 * loaded at p - k (k <= 3). Fixed sizes and, inside a list or map (direct),
 * strings are skipped without the depth test; everything else is
 * skipType(t, MaxSkipDepth - sp) (binary_skip.go:109-204): containers that do
 * not reduce to a multiplication open a frame. */
template <class FR>
TGI uint32_t tg_value(const uint8_t *b, uint64_t len, uint64_t &p, uint32_t t, bool direct, uint32_t &sp, const FR &fr,
                      const TGWin &w, uint32_t k)
{
    const uint32_t fs = tg_fixed(t);
    if (fs) {
        if (p + fs > len) return TG_R_FAIL;
        p += fs;
        return TG_R_OK;
    }
    if (!(direct && t == TT_STRING) && sp >= TG_MAX_SKIP) return TG_R_FAIL; /* errExceedDepthLimit */
    if (t == TT_STRING) { /* skipstr: the size as uint32 in an int */
        if (p + 4 > len) return TG_R_FAIL;
        const uint64_t e = p + 4 + (uint64_t)tg_be32(w, k);
        if (e > len) return TG_R_FAIL;
        p = e;
        return TG_R_OK;
    }
    if (t == TT_STRUCT) {
        if (sp >= FR::cap) return TG_R_DEEP;
        fr.at(sp++) = 0;
        return TG_R_OK;
    }
    if (t == TT_MAP) {
        if (p + 6 > len) return TG_R_FAIL;
        const uint32_t kt = tg_u8(w, k), vt = tg_u8(w, k + 1);
        const int32_t sz = (int32_t)tg_be32(w, k + 2);
        if (sz < 0) return TG_R_FAIL;
        p += 6;
        const uint32_t ks = tg_fixed(kt), vs = tg_fixed(vt);
        if (ks && vs) {
            const uint64_t e = p + (uint64_t)sz * (ks + vs);
            if (e > len) return TG_R_FAIL;
            p = e;
            return TG_R_OK;
        }
        if (sp >= FR::cap) return TG_R_DEEP;
        fr.at(sp++) = (uint64_t)(uint32_t)sz * 2 | (uint64_t)kt << 32 | (uint64_t)vt << 40 | 1ull << 48;
        return TG_R_OK;
    }
    if (t == TT_LIST || t == TT_SET) {
        if (p + 5 > len) return TG_R_FAIL;
        const uint32_t vt = tg_u8(w, k);
        const int32_t sz = (int32_t)tg_be32(w, k + 1);
        if (sz < 0) return TG_R_FAIL;
        p += 5;
        const uint32_t vs = tg_fixed(vt);
        if (vs) {
            const uint64_t e = p + (uint64_t)sz * vs;
            if (e > len) return TG_R_FAIL;
            p = e;
            return TG_R_OK;
        }
        if (sp >= FR::cap) return TG_R_DEEP;
        fr.at(sp++) = (uint64_t)(uint32_t)sz | (uint64_t)vt << 32 | (uint64_t)vt << 40 | 1ull << 48;
        return TG_R_OK;
    }
    return TG_R_FAIL; /* default: errInvalidDataSize */
}

/* SkipType(t) at b[p] (w = the window loaded at p - k). sp0: the value sits
 * inside sp0 containers that a caller's own skip has open (kids_device.h): its
 * depth budget is MaxSkipDepth - sp0 and its frames start at level sp0. */
template <class FR>
TGI uint32_t tg_skip(const uint8_t *b, uint64_t len, uint64_t &p, uint32_t t, const FR &fr, const TGWin &w0, uint32_t k0,
                     uint32_t sp0 = 0)
{
    uint32_t sp = sp0;
    uint32_t r = tg_value(b, len, p, t, false, sp, fr, w0, k0);
    while (r == TG_R_OK && sp > sp0) {
        const uint64_t f = fr.at(sp - 1);
        if (!(f >> 48)) { /* a struct: the next field header */
            if (p + 1 > len) return TG_R_FAIL;
            const TGWin w = tg_ld(b + p);
            const uint32_t ft = tg_u8(w, 0);
            p += 1;
            if (ft == TT_STOP) {
                sp--;
                continue;
            }
            if (p + 2 > len) return TG_R_FAIL;
            p += 2;
            r = tg_value(b, len, p, ft, false, sp, fr, w, 3);
        } else {
            const uint32_t left = (uint32_t)f;
            if (!left) {
                sp--;
                continue;
            }
            fr.at(sp - 1) = f - 1;
            const uint32_t et = (uint32_t)(f >> (left & 1 ? 40 : 32)) & 0xFFu;
            const uint32_t fs = tg_fixed(et);
            if (fs) { /* no window needed */
                if (p + fs > len) return TG_R_FAIL;
                p += fs;
            } else {
                r = tg_value(b, len, p, et, true, sp, fr, tg_ld(b + p), 0);
            }
        }
    }
    return r;
}

struct TGRes {
    uint32_t start, end, type, status, step, aux;
};
TGI TGRes tg_res(uint32_t status, uint32_t step, uint32_t type = 0, uint64_t start = 0, uint64_t end = 0,
                 uint64_t aux = 0)
{
    return TGRes{(uint32_t)start, (uint32_t)end, type, status, step, (uint32_t)aux};
}

/* ReadMapBegin (binary.go:585-617) at p: kt, vt, size; false = ErrRead */
TGI bool tg_map_begin(const uint8_t *b, uint64_t len, uint64_t &p, uint32_t &kt, uint32_t &vt, int64_t &size)
{
    if (p + 1 > len) return false;
    const TGWin w = tg_ld(b + p);
    kt = tg_u8(w, 0);
    if (!tg_valid(kt)) return false;
    if (p + 2 > len) return false;
    vt = tg_u8(w, 1);
    if (!tg_valid(vt)) return false;
    if (p + 6 > len) return false;
    size = (int32_t)tg_be32(w, 2);
    if (size < 0) return false;
    p += 6;
    return true;
}

/* path `path` of the set on the message b[0, len), up to where its last step
 * lands: DG_TGET_OK = a value of wire type `type` starts at `start` (nothing of
 * it is read), step = the path's length; anything else is the lookup's result */
template <class FR>
TGI TGRes tg_seek(const TGParams &A, const uint8_t *b, uint64_t len, uint32_t path, const FR &fr)
{
    if (len > 0xFFFFFFFFull) return tg_res(DG_TGET_E_READ, 0, 0, 0, 0, 0xFFFFFFFFull);
    const dg_path_ent pe = ((const dg_path_ent *)(const void *)(A.blob + sizeof(dg_path_hdr)))[path];
    const dg_path_step *steps = (const dg_path_step *)(const void *)(A.blob + A.off_steps) + pe.first;
    const uint8_t *pool = A.blob + A.off_pool;
    uint64_t p = 0, start = 0;
    uint32_t tt = A.root_type;
    bool is_list = tt == TT_LIST;
    for (uint32_t s = 0; s < pe.count; s++) {
        const dg_path_step st = steps[s];
        if (st.kind == DG_PS_FIELD) { /* searchFieldId */
            for (;;) {
                if (p + 1 > len) return tg_res(DG_TGET_E_READ, s);
                const TGWin w = tg_ld(b + p);
                const uint32_t ft = tg_u8(w, 0);
                if (!tg_valid(ft)) return tg_res(DG_TGET_E_READ, s);
                p += 1;
                if (ft == TT_STOP) return tg_res(DG_TGET_NOT_FOUND, s, TT_STRUCT, 0, 0, p);
                if (p + 2 > len) return tg_res(DG_TGET_E_READ, s);
                p += 2;
                if (tg_be16(w, 1) == (int32_t)st.val) {
                    start = p;
                    tt = ft;
                    break;
                }
                const uint32_t r = tg_skip(b, len, p, ft, fr, w, 3);
                if (r == TG_R_DEEP) return tg_res(TG_ST_DEEP, s);
                if (r) return tg_res(DG_TGET_E_READ, s);
            }
            is_list = tt == TT_LIST;
        } else if (st.kind == DG_PS_INDEX) { /* searchIndex over ReadListBegin */
            if (p + 1 > len) return tg_res(DG_TGET_E_READ, s);
            const TGWin w = tg_ld(b + p);
            const uint32_t et = tg_u8(w, 0);
            if (!tg_valid(et) || p + 5 > len) return tg_res(DG_TGET_E_READ, s);
            const int64_t size = (int32_t)tg_be32(w, 1);
            if (size < 0) return tg_res(DG_TGET_E_READ, s);
            p += 5;
            if (st.val >= size) return tg_res(DG_TGET_NOT_FOUND, s, is_list ? TT_LIST : TT_SET, p, p, p);
            const uint32_t fs = tg_fixed(et);
            if (fs) { /* st.val SkipTypes of a fixed size */
                p += (uint64_t)st.val * fs;
                if (p > len) return tg_res(DG_TGET_E_READ, s);
            } else {
                for (int64_t i = 0; i < st.val; i++) {
                    const uint32_t r = tg_skip(b, len, p, et, fr, tg_ld(b + p), 0);
                    if (r == TG_R_DEEP) return tg_res(TG_ST_DEEP, s);
                    if (r) return tg_res(DG_TGET_E_READ, s);
                }
            }
            start = p;
            tt = et;
        } else { /* searchStrKey / searchIntKey / searchBinKey */
            uint32_t kt, vt;
            int64_t size;
            if (!tg_map_begin(b, len, p, kt, vt, size)) return tg_res(DG_TGET_E_READ, s);
            if (st.kind == DG_PS_STRKEY && kt != TT_STRING) return tg_res(DG_TGET_E_TYPE, s, 0, 0, 0, kt);
            if (st.kind == DG_PS_INTKEY && kt != TT_BYTE && kt != TT_I16 && kt != TT_I32 && kt != TT_I64)
                return tg_res(DG_TGET_E_TYPE, s, 0, 0, 0, kt);
            const uint64_t after_hdr = p;
            bool found = false;
            for (int64_t i = 0; i < size; i++) {
                bool hit;
                if (st.kind == DG_PS_STRKEY) { /* ReadString (binary.go:767-791) */
                    if (p + 4 > len) return tg_res(DG_TGET_E_READ, s);
                    const int32_t sz = (int32_t)tg_be32(tg_ld(b + p), 0);
                    p += 4;
                    if (sz < 0 || (uint64_t)sz > len - p) return tg_res(DG_TGET_E_READ, s);
                    hit = (uint32_t)sz == st.key_len && tg_eq(b + p, pool + st.val, (uint64_t)sz);
                    p += (uint64_t)sz;
                } else if (st.kind == DG_PS_INTKEY) { /* ReadInt (binary.go:737-754): a byte is unsigned */
                    const uint32_t ks = tg_fixed(kt);
                    if (p + ks > len) return tg_res(DG_TGET_E_READ, s);
                    const uint64_t raw = __builtin_bswap64(tg_ld(b + p).lo);
                    const int64_t key = kt == TT_BYTE ? (int64_t)(raw >> 56)
                                                      : (int64_t)raw >> (64 - 8 * ks);
                    p += ks;
                    hit = key == st.val;
                } else { /* the key's bytes as SkipType(kt) delimits them */
                    const uint64_t ks = p;
                    const uint32_t r = tg_skip(b, len, p, kt, fr, tg_ld(b + p), 0);
                    if (r == TG_R_DEEP) return tg_res(TG_ST_DEEP, s);
                    if (r) return tg_res(DG_TGET_E_READ, s);
                    hit = p - ks == st.key_len && tg_eq(b + ks, pool + st.val, p - ks);
                }
                if (hit) {
                    found = true;
                    break;
                }
                const uint32_t r = tg_skip(b, len, p, vt, fr, tg_ld(b + p), 0);
                if (r == TG_R_DEEP) return tg_res(TG_ST_DEEP, s);
                if (r) return tg_res(DG_TGET_E_READ, s);
            }
            if (!found) return tg_res(DG_TGET_NOT_FOUND, s, TT_MAP, after_hdr, after_hdr, p);
            start = p;
            tt = vt;
        }
    }
    return tg_res(DG_TGET_OK, pe.count, tt, start, start);
}

/* path `path` of the set on the message b[0, len): the lookup, then the skip
 * that finds the value's end */
template <class FR>
TGI TGRes tg_walk(const TGParams &A, const uint8_t *b, uint64_t len, uint32_t path, const FR &fr)
{
    const TGRes at = tg_seek(A, b, len, path, fr);
    if (at.status != DG_TGET_OK) return at;
    uint64_t p = at.start;
    const uint32_t r = tg_skip(b, len, p, at.type, fr, tg_ld(b + p), 0);
    if (r == TG_R_DEEP) return tg_res(TG_ST_DEEP, at.step);
    if (r) return tg_res(DG_TGET_E_READ, at.step);
    return tg_res(DG_TGET_OK, at.step, at.type, at.start, p);
}

/* pair q's record (one 16-byte store) and its packing entries */
TGI void tg_store(const TGParams &A, uint64_t q, uint64_t a, const TGRes &r)
{
    uint4 v;
    v.x = r.start;
    v.y = r.end;
    v.z = (r.type & 0xFFu) | (r.status & 0xFFu) << 8 | (r.step & 0xFFFFu) << 16;
    v.w = r.aux;
    ((uint4 *)(void *)A.rec)[q] = v;
    if (A.val_off) A.val_off[q] = a + r.start;
    if (A.val_len) A.val_len[q] = r.status == DG_TGET_OK ? r.end - r.start : 0u;
}

void launch_tget_pass(hipStream_t s, const TGParams &A, uint32_t spread);
void launch_tget_deep(hipStream_t s, const TGParams &A);

}  // namespace dg
