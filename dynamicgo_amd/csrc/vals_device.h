/*
 * vals_device.h — typed column writes (include/dgj2t.h dg_vals_*), the inverse
 * of cols_device.h: the reference's NewNodeBool ... NewNodeString /
 * NewNodeList / NewNodeSet / NewNodeStruct (thrift/generic/node.go:92-201) over
 * BinaryEncoding.Encode* (thrift/binary.go:2101-2149).
 *
 * A cell is one (message, column) pair q = i * K + j; its item is the value's
 * bytes and, in struct mode, the 3-byte field header before them and, behind a
 * message's last item, the STOP byte. Three steps:
 *   size   one lane per cell (vl_size): the item's length and the status. A
 *          plan of scalars only has closed-form offsets, so that launch also
 *          writes the offsets and the bytes and nothing follows it.
 *   scan   cols' scan (launch_cols_scan) of the lengths into the offsets.
 *   emit   head: one lane per cell writes what precedes a body (field header,
 *          string length, list header, a scalar's bytes) and STOP in at most
 *          two unaligned stores (vl_head); body: string payloads and list
 *          elements in units of VL_UNIT output bytes (vl_unit). A block takes
 *          VL_CHUNK neighbouring bytes of the arena, narrows the cells to those
 *          that touch its chunk by two searches of full depth, and lane t takes
 *          the aligned 8 bytes [p, p + 8): it emits every unit that BEGINS
 *          there (at most one per cell, at most 8 cells), so a wave stores
 *          512 contiguous bytes whatever the cells' lengths are.
 * Nothing at an index >= cap is stored: every store is cut at cap.
 */
#pragma once
#include "cols_device.h"

namespace dg {

constexpr uint32_t VL_BLOCK = CL_BLOCK;
constexpr uint32_t VL_UNIT = 8;                       /* output bytes of one body unit */
constexpr uint32_t VL_CHUNK = 8 * VL_BLOCK * VL_UNIT; /* output bytes a block of the body pass takes a round */
constexpr uint32_t VL_CONTAINER = DG_VAL_LIST | DG_VAL_SET;

struct VLParams {
    dg_val_col col[DG_VALS_MAX_COLS];
    uint8_t kinds[DG_VALS_MAX_COLS];
    int16_t ids[DG_VALS_MAX_COLS];
    uint8_t pre[DG_VALS_MAX_COLS]; /* closed form: where item j begins in its message */
    uint32_t msg;                  /* closed form: a message's bytes */
    uint32_t K, has_ids;
    uint64_t pairs, base, cap;
    uint32_t *len;   /* the lengths for the scan (not in closed form) */
    uint64_t *off;   /* pairs + 1 */
    uint8_t *status; /* may be null */
    uint8_t *out;    /* null: sizing */
};

/* one cell's item */
struct VLSize {
    uint32_t len, status;
    uint32_t hdr;     /* bytes before the body: field header + string length or list header (a scalar: the field header) */
    uint32_t present; /* the item holds a value */
    uint64_t cnt;     /* a string's bytes, a container's elements; 0 when flagged */
};

TGI bool vl_scalar_kind(uint32_t kind) { return tg_fixed(kind) != 0; }
TGI bool vl_kind_ok(uint32_t kind)
{
    if (kind & VL_CONTAINER) return (kind & VL_CONTAINER) != VL_CONTAINER && vl_scalar_kind(kind & 0x3Fu);
    return kind == TT_STRING || vl_scalar_kind(kind);
}
TGI uint32_t vl_wire(uint32_t kind) { return kind & DG_VAL_LIST ? TT_LIST : kind & DG_VAL_SET ? TT_SET : kind; }

/* the item of a cell of kind `kind`: fh = 3 in struct mode, stop = 1 behind a
 * message's last item, cnt = the string's length or the container's count as
 * the inputs give it */
TGI VLSize vl_size(uint32_t kind, uint32_t fh, uint32_t stop, bool present, uint64_t cnt)
{
    VLSize z{stop, DG_VAL_OK, 0, 0, 0};
    if (!present) return z;
    z.present = 1;
    if (vl_scalar_kind(kind)) {
        z.hdr = fh, z.len = fh + tg_fixed(kind) + stop;
        return z;
    }
    const uint32_t w = kind == TT_STRING ? 1u : tg_fixed(kind & 0x3Fu);
    z.hdr = fh + (kind == TT_STRING ? 4u : 5u);
    if (cnt > 0x7FFFFFFFull || z.hdr + cnt * w + stop > 0xFFFFFFFFull) z.status = DG_VAL_E_SIZE, cnt = 0;
    z.cnt = cnt, z.len = z.hdr + (uint32_t)(cnt * w) + stop;
    return z;
}

/* the low w bytes of v big-endian, as the low w bytes of a word in memory order; BOOL: 1 or 0 */
TGI uint64_t vl_scalar(uint32_t t, uint64_t v)
{
    if (t == CL_T_BOOL) return v != 0;
    return __builtin_bswap64(v << (64 - 8 * tg_fixed(t)));
}

/* nb <= 8 bytes of w, in memory order, at o: one store of each of 8 / 4 / 2 / 1 bytes at most */
TGI void vl_put(uint8_t *o, uint64_t w, uint32_t nb)
{
    if (nb >= 8) {
        __builtin_memcpy(o, &w, 8);
        return;
    }
    if (nb & 4) {
        const uint32_t x = (uint32_t)w;
        __builtin_memcpy(o, &x, 4);
        o += 4, w >>= 32;
    }
    if (nb & 2) {
        const uint16_t x = (uint16_t)w;
        __builtin_memcpy(o, &x, 2);
        o += 2, w >>= 16;
    }
    if (nb & 1) *o = (uint8_t)w;
}

/* up to 16 bytes gathered in memory order */
struct VLBytes {
    uint64_t lo, hi;
    uint32_t n;
};
TGI void vl_push(VLBytes &h, uint64_t v, uint32_t nb) /* the low nb <= 8 bytes of v; the others are 0 */
{
    const uint32_t s = 8 * h.n;
    if (s < 64) {
        h.lo |= v << s;
        if (s && s + 8 * nb > 64) h.hi |= v >> (64 - s);
    } else {
        h.hi |= v << (s - 64);
    }
    h.n += nb;
}

/* h at out + at in at most two stores, nothing of it at cap or beyond; h is
 * empty afterwards and the answer is the position behind it */
TGI uint64_t vl_flush(VLBytes &h, uint8_t *out, uint64_t at, uint64_t cap)
{
    if (at < cap && h.n) {
        const uint64_t room = cap - at;
        const uint32_t nb = h.n < room ? h.n : (uint32_t)room;
        vl_put(out + at, h.lo, nb < 8 ? nb : 8);
        if (nb > 8) vl_put(out + at + 8, h.hi, nb - 8);
    }
    at += h.n;
    h.lo = h.hi = 0, h.n = 0;
    return at;
}

/* the 3-byte field header of struct mode (fh): the wire type and the id big-endian */
TGI void vl_field(VLBytes &h, uint32_t fh, uint32_t wire, int32_t id)
{
    if (fh) vl_push(h, (uint64_t)wire | (uint64_t)__builtin_bswap16((uint16_t)id) << 8, 3);
}

/* The item of len bytes at out + pos closed, h holding what precedes its body: STOP goes with h when nothing lies
 * between (a near stop), else behind the body (a far stop); nothing is stored at cap or beyond. */
TGI void vl_close(VLBytes &h, uint32_t stop, uint32_t len, uint8_t *out, uint64_t pos, uint64_t cap)
{
    const bool far_stop = stop && len != h.n + 1;
    if (stop && !far_stop) vl_push(h, 0, 1);
    (void)vl_flush(h, out, pos, cap);
    if (far_stop && pos + len - 1 < cap) out[pos + len - 1] = 0;
}

/* what precedes the body of the item z at out + pos, a scalar's bytes (v) and
 * the STOP byte, nothing of it at cap or beyond */
TGI void vl_head(uint32_t kind, int32_t id, uint32_t fh, uint32_t stop, const VLSize &z, uint64_t v, uint8_t *out,
                 uint64_t pos, uint64_t cap)
{
    VLBytes h{0, 0, 0};
    if (z.present) {
        vl_field(h, fh, vl_wire(kind), id);
        if (kind & VL_CONTAINER) vl_push(h, (uint64_t)(kind & 0x3Fu) | (uint64_t)__builtin_bswap32((uint32_t)z.cnt) << 8, 5);
        else if (kind == TT_STRING) vl_push(h, __builtin_bswap32((uint32_t)z.cnt), 4);
        else vl_push(h, vl_scalar(kind, v), tg_fixed(kind));
    }
    vl_close(h, stop, z.len, out, pos, cap);
}

/* unit u of a body of cnt bytes (STRING, from pay) or cnt elements (a
 * container, from el), stored at out + at = the body's byte 8 u, cut at cap.
 * A string unit reads 8 bytes from its first, so up to 7 past the payload. */
TGI void vl_unit(uint32_t kind, const uint8_t *pay, const uint64_t *el, uint64_t u, uint64_t cnt, uint8_t *out, uint64_t at,
                 uint64_t cap)
{
    uint64_t w = 0;
    uint32_t nb;
    if (kind == TT_STRING) {
        __builtin_memcpy(&w, pay + u * VL_UNIT, 8);
        const uint64_t rem = cnt - u * VL_UNIT;
        nb = rem < VL_UNIT ? (uint32_t)rem : VL_UNIT;
    } else {
        const uint32_t et = kind & 0x3Fu, ew = tg_fixed(et), per = VL_UNIT / ew;
        const uint64_t e0 = u * per, rem = cnt - e0;
        const uint32_t m = rem < per ? (uint32_t)rem : per;
        for (uint32_t k = 0; k < m; k++) w |= vl_scalar(et, el[e0 + k]) << (8 * ew * k);
        nb = m * ew;
    }
    if (at >= cap) return;
    if (cap - at < nb) nb = (uint32_t)(cap - at);
    vl_put(out + at, w, nb);
}

/* the body units of a cell's item */
TGI uint64_t vl_units(uint32_t kind, uint64_t cnt)
{
    const uint64_t bytes = kind == TT_STRING ? cnt : kind & VL_CONTAINER ? cnt * tg_fixed(kind & 0x3Fu) : 0;
    return (bytes + VL_UNIT - 1) / VL_UNIT;
}

/* Cell q of either parameter record (VLParams; EVParams, evals_device.h): fh = 3 in struct mode, stop = 1 behind a
 * message's last item, present: the inputs hold a value for it */
struct VLCell {
    uint32_t i, j, kind, fh, stop;
    int32_t id;
    bool present;
};
template <class P>
TGI VLCell vl_cell(const P &A, uint64_t q)
{
    VLCell p;
    p.i = (uint32_t)q / A.K, p.j = (uint32_t)q - p.i * A.K;
    p.kind = A.kinds[p.j], p.id = A.ids[p.j];
    p.fh = A.has_ids ? 3u : 0u, p.stop = A.has_ids && p.j == A.K - 1;
    p.present = !(A.has_ids && A.col[p.j].d_present) || A.col[p.j].d_present[p.i] != 0;
    return p;
}

/* a cell of vals with its item */
struct VLPair : VLCell {
    VLSize z;
    uint64_t v; /* a scalar's value; a string's payload offset */
};
TGI VLPair vl_pair(const VLParams &A, uint64_t q)
{
    VLPair p;
    static_cast<VLCell &>(p) = vl_cell(A, q);
    const dg_val_col &c = A.col[p.j];
    uint64_t cnt = 0;
    p.v = 0;
    if (p.present) {
        if (p.kind & VL_CONTAINER) cnt = c.d_elem_off[p.i + 1] - c.d_elem_off[p.i];
        else p.v = c.d_val[p.i];
        if (p.kind == TT_STRING) cnt = c.d_len[p.i];
    }
    p.z = vl_size(p.kind, p.fh, p.stop, p.present, cnt);
    return p;
}

/* the whole body of cell p at out + pos by its own lane (the lane-per-value emit) */
TGI void vl_body_loop(const VLParams &A, const VLPair &p, uint64_t pos)
{
    const dg_val_col &c = A.col[p.j];
    const uint64_t units = vl_units(p.kind, p.z.cnt);
    if (!units) return;
    const uint8_t *pay = p.kind == TT_STRING ? c.d_src + p.v : nullptr;
    const uint64_t *el = p.kind == TT_STRING ? nullptr : c.d_elems + c.d_elem_off[p.i];
    for (uint64_t u = 0; u < units; u++) vl_unit(p.kind, pay, el, u, p.z.cnt, A.out, pos + p.z.hdr + u * VL_UNIT, A.cap);
}

/* The body pass's lane: every body unit that begins in the aligned 8 bytes
 * [p, p + 8) of the arena, below total = min(the arena's end, cap). The cells
 * [lo, hi) hold every cell that touches the lane's chunk. Offsets alone tell a
 * body: an absent or flagged cell's item ends where its body would begin. */
TGI void vl_granule(const VLParams &A, uint64_t lo, uint64_t hi, uint64_t p, uint64_t total)
{
    const uint64_t pe = p + VL_UNIT < total ? p + VL_UNIT : total;
    const uint64_t g = p > A.base ? p : A.base;
    if (g >= pe) return;
    for (uint64_t q = cl_find(A.off, lo, hi, g); q < hi; q++) {
        const uint64_t a = A.off[q];
        if (a >= pe) break;
        const uint64_t e = A.off[q + 1];
        const uint32_t i = (uint32_t)q / A.K, j = (uint32_t)q - i * A.K, kind = A.kinds[j];
        if (vl_scalar_kind(kind)) continue;
        const uint64_t bs = a + (A.has_ids ? 3u : 0u) + (kind == TT_STRING ? 4u : 5u);
        const uint64_t be = e - (A.has_ids && j == A.K - 1);
        if (bs >= be) continue;
        const uint64_t u = bs >= p ? 0 : (p - bs + VL_UNIT - 1) / VL_UNIT, at = bs + u * VL_UNIT;
        if (at >= pe || at >= be) continue;
        const dg_val_col &c = A.col[j];
        if (kind == TT_STRING) vl_unit(kind, c.d_src + c.d_val[i], nullptr, u, be - bs, A.out, at, A.cap);
        else vl_unit(kind, nullptr, c.d_elems + c.d_elem_off[i], u, (be - bs) / tg_fixed(kind & 0x3Fu), A.out, at, A.cap);
    }
}

inline dim3 cell_grid(uint64_t pairs) { return dim3((uint32_t)((pairs + VL_BLOCK - 1) / VL_BLOCK)); } /* one lane per cell */

void launch_vals_size(hipStream_t s, const VLParams &A, bool closed);
void launch_vals_rebase(hipStream_t s, uint64_t *off, uint64_t entries, uint64_t base); /* evals' too */
void launch_vals_emit(hipStream_t s, const VLParams &A, uint32_t max_blocks, bool lane_emit, bool bodies);

}  // namespace dg
