/*
 * ents_device.h — entry columns (include/dgj2t.h dg_ents_*): GetByPath followed
 * by the reference's Node.List with String per element, Node.StrMap and
 * Node.IntMap (thrift/generic/cast.go:198-286 over iter.go:41-68 and
 * ReadMapBegin / ReadListBegin, thrift/binary.go:585-649), the values through
 * Node.Interface's arms for BOOL, the ints, DOUBLE and STRING (cast.go:342-356).
 *
 * The cell pass is cols' (cols_device.h): one lane per (message, column) pair
 * around tg_walk, the container's header in cl_cell's one unaligned 8-byte
 * load. The lookup's final skip has walked the whole container, so an OK cell
 * knows its end (span) and every entry inside it is whole.
 *
 * The emit has two routes. Entries of a fixed stride (int keys with BOOL, int
 * or DOUBLE values) are element-parallel like cols' list emit: a lane finds
 * the message of entry g in the scanned counts and reads its key and value at
 * g's own position. Entries of a variable stride (a string key, a string value
 * or a string element) can only be found by reading every length prefix before
 * them: one lane walks one OK cell, a chain of dependent 4-byte loads, and
 * either stores each entry as it meets it or stages R of them in LDS for the
 * wave to write out in runs.
 *
 * Bounds: a walk never reads an entry that would pass the cell's end, and a
 * load of 8 bytes starts before that end, so it stays inside the 16 spare
 * bytes the lookup's windows already need.
 */
#pragma once
#include "cols_device.h"

namespace dg {

constexpr uint32_t EN_BLOCK = 256;
constexpr uint32_t EN_EMIT_CHUNK = 8 * EN_BLOCK; /* entries a block of the fixed-stride emit takes a round */
constexpr uint32_t EN_WAVE = 64;                 /* the staged emit: one wave a block */

struct ENCell {
    CLCell c;
    uint32_t span; /* an OK cell: the bytes from c.val to the container's end */
};

struct ENParams {
    TGParams tg;    /* the lookup's part (rec, val_off and val_len stay null) */
    uint64_t n;
    uint64_t kinds; /* byte k: column k's kind */
    uint64_t *val;  /* column-major, as CLParams */
    uint64_t *cell;
    uint32_t *len, *span;
};

struct ENEmit {
    const uint8_t *src;
    uint64_t n;
    const uint64_t *val, *cell;
    const uint32_t *len, *span;
    const uint64_t *off;
    uint64_t *key;  /* any of the four may be null */
    uint32_t *klen;
    uint64_t *v;
    uint32_t *vlen;
    uint64_t cap;
    uint32_t kind;
};

/* Type.IsInt (thrift/descriptor.go): I08, I16, I32, I64 */
TGI bool en_is_int(uint32_t t) { return t == TT_BYTE || t == TT_I16 || t == TT_I32 || t == TT_I64; }

/* Node.Interface on a value of wire type vt gives what value kind v reads */
TGI bool en_takes(uint32_t v, uint32_t vt)
{
    return v == DG_ENT_INT ? en_is_int(vt) : v == DG_ENT_F64 ? vt == CL_T_DOUBLE : v == DG_ENT_BOOL ? vt == CL_T_BOOL
                                                                                                    : vt == TT_STRING;
}

/* the cast of a column of kind `kind` on the lookup's result r in the message
 * at b (its first byte at arena offset a) */
TGI ENCell en_cell(uint32_t kind, const TGRes &r, const uint8_t *b, uint64_t a)
{
    ENCell o{{0, 0, r.status, r.type, r.step, r.aux}, 0};
    CLCell &c = o.c;
    if (r.status != DG_TGET_OK) return o;
    const uint32_t t = r.type;
    const uint64_t raw = cl_be64(b + r.start);
    uint32_t hdr, size;
    bool ok;
    if (kind == DG_ENT_LISTSTR) { /* should2(LIST, SET), cast.go:202 */
        if (t != TT_LIST && t != TT_SET) {
            c.status = DG_COL_E_UNSUPPORTED;
            return o;
        }
        const uint32_t et = (uint32_t)(raw >> 56);
        hdr = 5, size = (uint32_t)(raw >> 24);
        if (!tg_valid(et)) { /* iterElems -> ReadListBegin */
            c.status = DG_TGET_E_READ, c.type = 0;
            return o;
        }
        ok = size == 0 || et == TT_STRING;
        if (ok) c.type = et;
        else c.aux = et;
    } else {
        if (t != TT_MAP) { /* should(MAP), cast.go:231, 262 */
            c.status = DG_COL_E_UNSUPPORTED;
            return o;
        }
        const uint32_t kt = (uint32_t)(raw >> 56), vt = (uint32_t)(raw >> 48) & 0xFFu;
        hdr = 6, size = (uint32_t)(raw >> 16);
        if (kind & DG_ENT_INTMAP) {
            if (!en_is_int(kt)) { /* cast.go:265, before iterPairs: the raw key byte (node.go:66-68) */
                c.status = DG_COL_E_UNSUPPORTED, c.aux = kt;
                return o;
            }
            if (!tg_valid(vt)) { /* iterPairs -> ReadMapBegin */
                c.status = DG_TGET_E_READ, c.type = 0;
                return o;
            }
            c.aux = kt | vt << 8;
        } else {
            if (!tg_valid(kt) || !tg_valid(vt)) { /* iterPairs first, cast.go:234 */
                c.status = DG_TGET_E_READ, c.type = 0;
                return o;
            }
            c.aux = kt | vt << 8;
            if (kt != TT_STRING) { /* cast.go:238, whatever the size */
                c.status = DG_COL_E_UNSUPPORTED;
                return o;
            }
        }
        ok = size == 0 || en_takes(kind & 15u, vt);
    }
    if (ok) c.val = a + r.start + hdr, c.len = size, o.span = r.end - r.start - hdr;
    else c.status = DG_COL_E_UNSUPPORTED;
    return o;
}

/* a value of kind v (not STR) and wire type vt (one v takes), raw = its bytes from the top */
TGI uint64_t en_scalar(uint32_t v, uint32_t vt, uint64_t raw)
{
    if (v == DG_ENT_BOOL) return (raw >> 56) == 1; /* DecodeBool */
    if (v == DG_ENT_F64) return raw;
    uint64_t x = 0;
    (void)cl_int(vt, raw, x);
    return x;
}

struct ENEntry {
    uint64_t key, val;
    uint32_t klen, vlen;
};

/* entry j of an OK cell of a fixed-stride kind whose entry 0 is at src + val:
 * two loads of 8 bytes, each from a byte of the entry */
TGI ENEntry en_fixed(const uint8_t *src, uint64_t val, uint32_t v, uint32_t kt, uint32_t vt, uint64_t j)
{
    const uint32_t kw = tg_fixed(kt), vw = tg_fixed(vt);
    const uint8_t *p = src + val + j * (kw + vw);
    ENEntry o{0, 0, 0, 0};
    (void)cl_int(kt, cl_be64(p), o.key); /* ReadInt: a byte is unsigned */
    o.val = en_scalar(v, vt, cl_be64(p + kw));
    return o;
}

/* a string at arena position p: its payload's offset and length; false = it would pass e */
TGI bool en_str(const uint8_t *src, uint64_t &p, uint64_t e, uint64_t &off, uint32_t &len)
{
    if (p + 4 > e) return false;
    uint32_t l;
    __builtin_memcpy(&l, src + p, 4);
    l = __builtin_bswap32(l);
    if (p + 4 + (uint64_t)l > e) return false;
    off = p + 4, len = l, p += 4 + (uint64_t)l;
    return true;
}

/* the entry at arena position p of a cell that ends at e, p moved behind it;
 * false = the entry would pass e (nothing of it is to be stored) */
TGI bool en_next(const uint8_t *src, uint64_t &p, uint64_t e, uint32_t kind, uint32_t kt, uint32_t vt, ENEntry &o)
{
    o = ENEntry{0, 0, 0, 0};
    if (kind & DG_ENT_STRMAP) {
        if (!en_str(src, p, e, o.key, o.klen)) return false;
    } else if (kind & DG_ENT_INTMAP) {
        const uint32_t kw = tg_fixed(kt);
        if (!kw || p + kw > e) return false;
        (void)cl_int(kt, cl_be64(src + p), o.key);
        p += kw;
    }
    if (kind == DG_ENT_LISTSTR || (kind & 15u) == DG_ENT_STR) return en_str(src, p, e, o.val, o.vlen);
    const uint32_t vw = tg_fixed(vt);
    if (!vw || p + vw > e) return false;
    o.val = en_scalar(kind & 15u, vt, cl_be64(src + p));
    p += vw;
    return true;
}

void launch_ents_pass(hipStream_t s, const ENParams &A);
/* stage: 0 = every lane stores its entries itself; 4, 8 or 16 = that many entries a lane staged in LDS a round */
void launch_ents_emit(hipStream_t s, const ENEmit &E, uint32_t max_blocks, uint32_t stage);

}  // namespace dg
