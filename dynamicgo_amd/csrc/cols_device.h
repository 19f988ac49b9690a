/*
 * cols_device.h — typed column reads (include/dgj2t.h dg_cols_*): GetByPath
 * followed by the reference's casts Node.Bool / Byte / Int / Float64 / String /
 * Binary / Len and List (thrift/generic/cast.go:50-224) over the decoders of
 * thrift/binary.go (DecodeBool 2152, DecodeByte, DecodeInt16/32/64,
 * DecodeDouble).
 *
 * The cell pass: one lane takes one (message, column) pair in tget's
 * geometry (the pair pass, walk_kern.h), runs tg_walk (tget_device.h,
 * unchanged) and decodes at the found position with ONE unaligned 8-byte load and a byte swap: every scalar, a
 * list's header (type byte + count) and a map's (two type bytes + count) lie
 * in those 8 bytes. The load starts at most at the message's end, so it stays
 * inside the 16 spare bytes tg_walk's windows already need.
 *
 * The list emit is element-parallel: a lane finds the message of element g in
 * the scanned counts (elem_off) and writes elems[g], so a wave stores 512
 * contiguous bytes whatever the lists' lengths are.
 */
#pragma once
#include "scan_defs.h"
#include "tget_device.h"

namespace dg {

constexpr uint32_t CL_BLOCK = 256;
constexpr uint32_t CL_SCAN_TILE = SCAN_TILE; /* counts per block of the scan (vals and evals size their sums by this name) */
constexpr uint32_t CL_EMIT_CHUNK = 8 * CL_BLOCK; /* elements a block of the emit takes a round */
constexpr uint32_t CL_T_BOOL = 2, CL_T_DOUBLE = 4;

/* one cell before it is stored */
struct CLCell {
    uint64_t val;
    uint32_t len, status, type, step, aux;
};

struct CLParams {
    TGParams tg;      /* the lookup's part (rec, val_off and val_len stay null) */
    uint64_t n;
    uint64_t kinds;   /* byte k: column k's kind */
    uint64_t *val;    /* column-major: column k at [k * n, k * n + n) */
    uint64_t *cell;   /* dg_col_cell as one word: status | type << 8 | step << 16 | aux << 32 */
    uint32_t *len;    /* may be null */
};

struct CLEmit {
    const uint8_t *src;
    uint64_t n;
    const uint64_t *val, *cell;
    const uint64_t *elem_off;
    uint64_t *elems;
    uint64_t cap;
};

/* 8 bytes at any alignment, read big-endian: the first byte is the top one */
TGI uint64_t cl_be64(const uint8_t *b)
{
    uint64_t v;
    __builtin_memcpy(&v, b, 8);
    return __builtin_bswap64(v);
}

/* Node.int (cast.go:124-138) on wire type t, raw = the value's bytes from the
 * top: I08 through DecodeByte, unsigned (int(byte)); I16 / I32 / I64
 * sign-extended. false: the cast does not take t (ErrUnsupportedType). */
TGI bool cl_int(uint32_t t, uint64_t raw, uint64_t &v)
{
    if (t == TT_BYTE) {
        v = raw >> 56;
        return true;
    }
    if (t != TT_I16 && t != TT_I32 && t != TT_I64) return false;
    v = (uint64_t)((int64_t)raw >> (64 - 8 * tg_fixed(t)));
    return true;
}

/* the cast of a column of kind `kind` on the lookup's result r in the message
 * at b (its first byte at arena offset a) */
TGI CLCell cl_cell(uint32_t kind, const TGRes &r, const uint8_t *b, uint64_t a)
{
    CLCell c{0, 0, r.status, r.type, r.step, r.aux};
    if (r.status != DG_TGET_OK) return c;
    const uint32_t t = r.type;
    const uint64_t raw = cl_be64(b + r.start);
    bool ok = false;
    if (kind & DG_COL_LIST) { /* Node.List: should2(LIST, SET), cast.go:202 */
        if (t == TT_LIST || t == TT_SET) {
            const uint32_t et = (uint32_t)(raw >> 56), size = (uint32_t)(raw >> 24);
            if (!tg_valid(et)) { /* ReadListBegin (binary.go:625-649) */
                c.status = DG_TGET_E_READ, c.type = 0;
                return c;
            }
            uint64_t unused;
            ok = size == 0 || ((kind & 15u) == DG_COL_INT ? cl_int(et, 0, unused) : et == CL_T_DOUBLE);
            if (ok) c.val = a + r.start + 5, c.len = size, c.type = et;
            else c.aux = et;
        }
    } else if (kind == DG_COL_BOOL) { /* DecodeBool: int8(b[0]) == 1 */
        ok = t == CL_T_BOOL;
        c.val = (raw >> 56) == 1;
    } else if (kind == DG_COL_BYTE) {
        ok = t == TT_BYTE;
        c.val = raw >> 56;
    } else if (kind == DG_COL_INT) {
        ok = cl_int(t, raw, c.val);
    } else if (kind == DG_COL_F64) {
        ok = t == CL_T_DOUBLE;
        c.val = raw;
    } else if (kind == DG_COL_STR) {
        ok = t == TT_STRING;
        c.val = a + r.start + 4, c.len = r.end - r.start - 4;
    } else if (kind == DG_COL_LEN) { /* Node.len, cast.go:57-68 */
        ok = t == TT_LIST || t == TT_SET || t == TT_MAP;
        c.val = (uint32_t)(raw >> (t == TT_MAP ? 16 : 24));
    }
    if (!ok) c.status = DG_COL_E_UNSUPPORTED, c.val = 0, c.len = 0;
    return c;
}

TGI uint64_t cl_cell_word(const CLCell &c)
{
    return (uint64_t)(c.status & 0xFFu) | (uint64_t)(c.type & 0xFFu) << 8 | (uint64_t)(c.step & 0xFFFFu) << 16 |
           (uint64_t)c.aux << 32;
}

/* element j of an OK list cell whose element 0 is at src + val and whose
 * element type is et (one the cast takes): 8 bytes, INT extended per width,
 * DOUBLE bit for bit. Reads 8 bytes from the element's first. */
TGI uint64_t cl_elem(const uint8_t *src, uint64_t val, uint32_t et, uint64_t j)
{
    const uint64_t raw = cl_be64(src + val + j * tg_fixed(et));
    uint64_t v = raw;
    if (et != CL_T_DOUBLE) (void)cl_int(et, raw, v);
    return v;
}

/* the message m in [lo, hi) with off[m] <= g < off[m + 1], given off[lo] <= g < off[hi] */
TGI uint64_t cl_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t g)
{
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

void launch_cols_pass(hipStream_t s, const CLParams &A);
void launch_cols_scan(hipStream_t s, const uint32_t *cnt, uint64_t n, uint64_t *sums, uint64_t *off);
void launch_cols_emit(hipStream_t s, const CLEmit &E, uint32_t max_blocks, bool full_search);

}  // namespace dg
