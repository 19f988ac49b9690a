/*
 * evals_device.h — entry column writes (include/dgj2t.h dg_evals_*), the
 * inverse of ents_device.h and the container half of vals_device.h: the
 * reference's NewNodeList / NewNodeSet / NewNodeMap (thrift/generic/node.go:154-187)
 * over WriteAny (thrift/binary.go:1480-1660) for list<string>, set<string> and
 * maps with int or string keys and scalar or string values.
 *
 * A cell is one (message, column) pair q = i * K + j as in vals; its item is
 * the container's header, its entries and, in struct mode, the field header
 * before and, behind a message's last item, the STOP byte. When writing, every
 * length is an input, so nothing is walked:
 *   entry size  variable-stride kinds (a string key, a string value, list
 *               elements): one lane per entry writes the entry's encoded bytes
 *               (ev_entry_size), cols' scan turns them into positions. An entry
 *               that trips a size rule counts as EV_BAD = 2^32 - 1 bytes, which
 *               alone makes its cell an item of 2^32 bytes or more: the cell
 *               pass flags it from the sum, with no search and no store.
 *               Fixed-stride kinds (int keys, scalar values) take neither
 *               launch: entry r of a cell lies at r * stride.
 *   cell size   one lane per cell (ev_cell): the item's length, the status and
 *               the count the emit writes (0 for an absent or flagged cell);
 *               cols' scan of the lengths gives the offsets, of the counts the
 *               emit's index space.
 *   head        one lane per cell: field header, container header, STOP.
 *   emit        entry-parallel over the scanned counts of all columns at once:
 *               lane t of a round takes emitted entry base + r * 256 + t, finds
 *               its cell between the chunk's two end searches (cl_find) and
 *               writes the key and the value at the cell's offset + header +
 *               the entry's position. Only entries of OK, present cells have an
 *               index, so no entry and no payload of any other cell is read.
 * Nothing at an index >= cap is stored: every store is cut at cap.
 */
#pragma once
#include "vals_device.h"

namespace dg {

constexpr uint32_t EV_BLOCK = CL_BLOCK;
constexpr uint32_t EV_CHUNK = CL_EMIT_CHUNK; /* emitted entries a block takes a round */
constexpr uint32_t EV_BAD = 0xFFFFFFFFu;     /* the size of an entry that trips a size rule */

struct EVParams {
    dg_eval_col col[DG_VALS_MAX_COLS];
    const uint64_t *pos[DG_VALS_MAX_COLS]; /* variable-stride columns: the scanned entry sizes, n_ent + 1 */
    uint16_t kinds[DG_VALS_MAX_COLS];
    int16_t ids[DG_VALS_MAX_COLS];
    uint32_t K, has_ids;
    uint64_t pairs, base, cap;
    uint32_t *len, *cnt; /* per cell: the item's bytes, the entries to emit */
    uint64_t *cnt_off;   /* pairs + 1: the scanned counts */
    uint64_t *off;       /* pairs + 1 */
    uint8_t *status;     /* may be null */
    uint8_t *out;        /* null: sizing */
};

TGI bool ev_is_map(uint32_t kind) { return (kind & DG_EVAL_MAP) != 0; }
TGI uint32_t ev_kt(uint32_t kind) { return ev_is_map(kind) ? (kind >> 4) & 15u : 0u; } /* 0: a list has no keys */
TGI uint32_t ev_vt(uint32_t kind) { return ev_is_map(kind) ? kind & 15u : (uint32_t)TT_STRING; }
TGI bool ev_kind_ok(uint32_t kind)
{
    if (kind == (DG_VAL_LIST | TT_STRING) || kind == (DG_VAL_SET | TT_STRING)) return true;
    if ((kind & ~0xFFu) != DG_EVAL_MAP) return false;
    const uint32_t kt = (kind >> 4) & 15u, vt = kind & 15u;
    const bool key = kt == TT_STRING || kt == TT_BYTE || kt == TT_I16 || kt == TT_I32 || kt == TT_I64;
    return key && (vt == TT_STRING || tg_fixed(vt) != 0);
}
TGI uint32_t ev_wire(uint32_t kind) { return ev_is_map(kind) ? TT_MAP : kind & DG_VAL_LIST ? TT_LIST : TT_SET; }
TGI uint32_t ev_hdr(uint32_t kind) { return ev_is_map(kind) ? 6u : 5u; }
/* an entry's bytes when they do not depend on the entry, else 0 */
TGI uint32_t ev_stride(uint32_t kind)
{
    const uint32_t kw = tg_fixed(ev_kt(kind)), vw = tg_fixed(ev_vt(kind));
    return kw && vw ? kw + vw : 0u;
}

/* one entry's encoded bytes for the scan; klen / vlen count only where the type is STRING */
TGI uint32_t ev_entry_size(uint32_t kt, uint32_t vt, uint32_t klen, uint32_t vlen)
{
    uint64_t b = 0;
    if (kt == TT_STRING) {
        if (klen > 0x7FFFFFFFu) return EV_BAD;
        b += 4ull + klen;
    } else {
        b += tg_fixed(kt);
    }
    if (vt == TT_STRING) {
        if (vlen > 0x7FFFFFFFu) return EV_BAD;
        b += 4ull + vlen;
    } else {
        b += tg_fixed(vt);
    }
    return b < EV_BAD ? (uint32_t)b : EV_BAD;
}

/* one cell's item */
struct EVCell {
    uint32_t len, status;
    uint32_t cnt; /* the entries written; 0 when absent or flagged */
};

/* the item of a cell of kind `kind` that owns the entries [a, b) of n_ent: fh =
 * 3 in struct mode, stop = 1 behind a message's last item, pos = the scanned
 * entry sizes of a variable-stride kind (not read by an empty or flagged cell) */
TGI EVCell ev_cell(uint32_t kind, uint32_t fh, uint32_t stop, bool present, uint64_t a, uint64_t b, uint64_t n_ent,
                   const uint64_t *pos)
{
    EVCell z{stop, DG_VAL_OK, 0};
    if (!present) return z;
    const uint32_t hdr = fh + ev_hdr(kind);
    uint64_t cnt = 0, bytes = 0;
    if (a > b || b > n_ent) {
        z.status = DG_EVAL_E_RANGE;
    } else if (b - a > 0x7FFFFFFFull) {
        z.status = DG_VAL_E_SIZE;
    } else if (b > a) {
        const uint32_t stride = ev_stride(kind);
        cnt = b - a;
        bytes = stride ? cnt * stride : pos[b] - pos[a];
        if (hdr + bytes + stop > 0xFFFFFFFFull) z.status = DG_VAL_E_SIZE, cnt = 0, bytes = 0;
    }
    z.cnt = (uint32_t)cnt, z.len = hdr + (uint32_t)bytes + stop;
    return z;
}

/* cell q decoded from the inputs (vl_cell, vals_device.h), and its item */
using EVPair = VLCell;
TGI EVPair ev_pair(const EVParams &A, uint64_t q) { return vl_cell(A, q); }
TGI EVCell ev_pair_cell(const EVParams &A, const EVPair &p)
{
    const dg_eval_col &c = A.col[p.j];
    uint64_t a = 0, b = 0;
    if (p.present) a = c.d_ent_off[p.i], b = c.d_ent_off[p.i + 1];
    return ev_cell(p.kind, p.fh, p.stop, p.present, a, b, c.n_ent, A.pos[p.j]);
}

/* what precedes the entries of the item of `len` bytes and `cnt` entries at
 * out + pos, and the STOP byte, nothing of it at cap or beyond. An item of
 * `stop` bytes is an absent cell's. */
TGI void ev_head(uint32_t kind, int32_t id, uint32_t fh, uint32_t stop, uint32_t len, uint32_t cnt, uint8_t *out, uint64_t pos,
                 uint64_t cap)
{
    VLBytes h{0, 0, 0};
    if (len > stop) {
        vl_field(h, fh, ev_wire(kind), id);
        if (ev_is_map(kind))
            vl_push(h, (uint64_t)ev_kt(kind) | (uint64_t)ev_vt(kind) << 8 | (uint64_t)__builtin_bswap32(cnt) << 16, 6);
        else vl_push(h, (uint64_t)TT_STRING | (uint64_t)__builtin_bswap32(cnt) << 8, 5);
    }
    vl_close(h, stop, len, out, pos, cap);
}

/* a payload of len bytes at out + at in 8-byte units, one unaligned 8-byte load each (vl_unit: up to 7 bytes past it) */
TGI void ev_payload(const uint8_t *pay, uint32_t len, uint8_t *out, uint64_t at, uint64_t cap)
{
    for (uint64_t u = 0; u * VL_UNIT < len && at + u * VL_UNIT < cap; u++)
        vl_unit(TT_STRING, pay, nullptr, u, len, out, at + u * VL_UNIT, cap);
}

/* entry e of column c, key then value, at out + at */
TGI void ev_entry(const dg_eval_col &c, uint32_t kt, uint32_t vt, uint64_t e, uint8_t *out, uint64_t at, uint64_t cap)
{
    VLBytes h{0, 0, 0};
    if (kt == TT_STRING) {
        const uint32_t kl = c.d_key_len[e];
        vl_push(h, __builtin_bswap32(kl), 4);
        if (kl) {
            at = vl_flush(h, out, at, cap);
            ev_payload(c.d_key_src + c.d_key[e], kl, out, at, cap);
            at += kl;
        }
    } else if (kt) {
        vl_push(h, vl_scalar(kt, c.d_key[e]), tg_fixed(kt));
    }
    if (vt == TT_STRING) {
        const uint32_t vl = c.d_val_len[e];
        vl_push(h, __builtin_bswap32(vl), 4);
        at = vl_flush(h, out, at, cap);
        if (vl) ev_payload(c.d_val_src + c.d_val[e], vl, out, at, cap);
    } else {
        vl_push(h, vl_scalar(vt, c.d_val[e]), tg_fixed(vt));
        (void)vl_flush(h, out, at, cap);
    }
}

/* The emit's lane: emitted entry t, which lies in cell q (cnt_off[q] <= t <
 * cnt_off[q + 1], so q is OK, present and not empty). */
TGI void ev_emit(const EVParams &A, uint64_t q, uint64_t t)
{
    const EVPair p = ev_pair(A, q);
    const dg_eval_col &c = A.col[p.j];
    const uint64_t e0 = c.d_ent_off[p.i], r = t - A.cnt_off[q];
    const uint32_t stride = ev_stride(p.kind);
    const uint64_t rel = stride ? r * stride : A.pos[p.j][e0 + r] - A.pos[p.j][e0];
    ev_entry(c, ev_kt(p.kind), ev_vt(p.kind), e0 + r, A.out, A.off[q] + p.fh + ev_hdr(p.kind) + rel, A.cap);
}

void launch_evals_entry_size(hipStream_t s, const dg_eval_col &c, uint32_t kt, uint32_t vt, uint32_t *elen);
void launch_evals_cells(hipStream_t s, const EVParams &A);
void launch_evals_emit(hipStream_t s, const EVParams &A, uint32_t blocks);

}  // namespace dg
