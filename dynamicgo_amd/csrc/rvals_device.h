/*
 * rvals_device.h — row column writes (include/dgj2t.h dg_rvals_*), the inverse
 * of rows_device.h and a component beside vals_device.h and evals_device.h: the
 * reference's NewNodeList / NewNodeSet over []interface{} of
 * map[FieldID]interface{} (thrift/generic/node.go:154-187; WriteAny,
 * thrift/binary.go:1504-1528 and :1661) for list<struct> and set<struct> whose
 * elements hold scalar, string and numeric-list fields.
 *
 * A cell is one (row, column) pair q = g * K + j; its item is vals' item in
 * struct mode: the 3-byte field header, the value and, behind a row's last
 * item, the STOP byte. Message i owns the rows [row_off[i], row_off[i + 1]);
 * its item is 0C, the i32 count and its rows' cells. Every length is an input,
 * so nothing is walked:
 *   cell size  one lane per cell (rv_size_lane): the item's length and the cell
 *              status; cols' scan turns the lengths into pos[cells + 1], 64-bit
 *              and relative to row 0. A plan of scalars with every field
 *              present takes neither: cell (g, j) lies at g * stride + pre[j]
 *              (rv_pos answers both).
 *   message    one lane per message (rv_msg_lane): RANGE, then the count, then
 *              the length 5 + pos[row_off[i + 1] K] - pos[row_off[i] K] and
 *              SIZE; the length and the rows to emit (0 when flagged) go to two
 *              scans: d_out_off and the emitted rows' index space cnt_off.
 *   head       one lane per message writes the 5-byte list header
 *              (rv_list_head); one lane per emitted cell, the K cells of a row
 *              in neighbouring lanes, writes vals' head (rv_head_lane). Only
 *              rows of OK messages have an index, so no payload byte and no
 *              element of any other row is read.
 *   body       vals' body pass over the arena's bytes (rv_granule): a lane owns
 *              8 aligned bytes, finds its message in d_out_off and its cell in
 *              pos between that message's rows, and emits every unit that
 *              begins in its bytes, so whole waves store contiguous runs
 *              whatever the mix of row and payload lengths is.
 * Nothing at an index >= cap is stored: every store is cut at cap.
 */
#pragma once
#include "vals_device.h"

namespace dg {

constexpr uint32_t RV_BLOCK = VL_BLOCK;
constexpr uint32_t RV_CHUNK = 8 * RV_BLOCK; /* emitted cells a block of the head pass takes a round */
constexpr uint32_t RV_HDR = 5;              /* 0C and the i32 count */

struct RVParams {
    dg_val_col col[DG_VALS_MAX_COLS];
    uint8_t kinds[DG_VALS_MAX_COLS];
    int16_t ids[DG_VALS_MAX_COLS];
    uint8_t pre[DG_VALS_MAX_COLS]; /* fixed stride: where item j begins in its row */
    uint32_t stride;               /* fixed stride: a row's bytes */
    uint32_t fixed;                /* the fixed-stride route: no len, no pos */
    uint32_t K, has_ids;           /* has_ids = 1: vl_cell reads it */
    uint64_t n, n_rows, cells, base, cap;
    const uint64_t *row_off; /* n + 1 */
    uint32_t *len;           /* cells: the items' lengths for the scan */
    uint64_t *pos;           /* cells + 1: the scanned lengths */
    uint32_t *mlen, *mcnt;   /* n: a message's bytes, its rows to emit */
    uint64_t *cnt_off;       /* n + 1: the scanned counts */
    uint64_t *off;           /* n + 1 */
    uint8_t *status;         /* n, may be null */
    uint8_t *cell_status;    /* cells, may be null */
    uint8_t *out;            /* null: sizing */
};

/* where cell q begins, relative to row 0's first cell; q = cells is the end */
TGI uint64_t rv_pos(const RVParams &A, uint64_t q)
{
    if (!A.fixed) return A.pos[q];
    const uint64_t g = q / A.K;
    return g * A.stride + A.pre[q - g * A.K];
}

/* cell q with its item, vals' vl_pair over this record: row q / K, column q % K */
TGI VLPair rv_pair(const RVParams &A, uint64_t q)
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
    p.z = vl_size(p.kind, 3, p.stop, p.present, cnt);
    return p;
}

/* the cell-size pass's lane */
TGI void rv_size_lane(const RVParams &A, uint64_t q)
{
    const VLPair p = rv_pair(A, q);
    A.len[q] = p.z.len;
    if (A.cell_status) A.cell_status[q] = (uint8_t)p.z.status;
}

/* one message's item */
struct RVMsg {
    uint32_t len, status;
    uint32_t cnt; /* the rows written; 0 when flagged */
};

/* the item of the message that owns the rows [a, b) of n_rows */
TGI RVMsg rv_msg(const RVParams &A, uint64_t a, uint64_t b)
{
    RVMsg z{RV_HDR, DG_VAL_OK, 0};
    if (a > b || b > A.n_rows) {
        z.status = DG_EVAL_E_RANGE;
    } else if (b - a > 0x7FFFFFFFull) {
        z.status = DG_VAL_E_SIZE;
    } else if (b > a) {
        const uint64_t bytes = rv_pos(A, b * A.K) - rv_pos(A, a * A.K);
        if (RV_HDR + bytes > 0xFFFFFFFFull) z.status = DG_VAL_E_SIZE;
        else z.cnt = (uint32_t)(b - a), z.len = RV_HDR + (uint32_t)bytes;
    }
    return z;
}

/* the message pass's lane */
TGI void rv_msg_lane(const RVParams &A, uint64_t i)
{
    const RVMsg z = rv_msg(A, A.row_off[i], A.row_off[i + 1]);
    A.mlen[i] = z.len, A.mcnt[i] = z.cnt;
    if (A.status) A.status[i] = (uint8_t)z.status;
}

/* message i's list header: the element type STRUCT and the count */
TGI void rv_list_head(const RVParams &A, uint64_t i)
{
    VLBytes h{0, 0, 0};
    vl_push(h, (uint64_t)TT_STRUCT | (uint64_t)__builtin_bswap32(A.mcnt[i]) << 8, RV_HDR);
    (void)vl_flush(h, A.out, A.off[i], A.cap);
}

/* The head pass's lane: emitted cell t = e * K + j of emitted row e, which lies
 * in message m (cnt_off[m] <= e < cnt_off[m + 1], so m is OK and not empty). */
TGI void rv_head_lane(const RVParams &A, uint64_t m, uint64_t t)
{
    const uint64_t e = t / A.K, j = t - e * A.K;
    const uint64_t a = A.row_off[m], g = a + (e - A.cnt_off[m]);
    const uint64_t q = g * A.K + j;
    const VLPair p = rv_pair(A, q);
    const uint64_t at = A.off[m] + RV_HDR + (rv_pos(A, q) - rv_pos(A, a * A.K));
    vl_head(p.kind, p.id, 3, p.stop, p.z, p.v, A.out, at, A.cap);
}

/* The body pass's lane, vals' vl_granule over messages of rows: every body unit
 * that begins in the aligned 8 bytes [p, p + 8) of the arena, below total =
 * min(the arena's end, cap). The messages [mlo, mhi) hold every message that
 * touches the lane's chunk. A cell's end is pos[q + 1] in relative coordinates,
 * so the 5 header bytes between two messages never count as body; offsets alone
 * tell a body: an absent or flagged cell's item ends where its body would begin. */
TGI void rv_granule(const RVParams &A, uint64_t mlo, uint64_t mhi, uint64_t p, uint64_t total)
{
    const uint64_t pe = p + VL_UNIT < total ? p + VL_UNIT : total;
    const uint64_t g0 = p > A.base ? p : A.base;
    if (g0 >= pe) return;
    for (uint64_t m = cl_find(A.off, mlo, mhi, g0); m < mhi; m++) {
        const uint64_t ms = A.off[m];
        if (ms >= pe) break;
        const uint64_t rows = A.mcnt[m];
        if (!rows) continue;
        const uint64_t qa = A.row_off[m] * A.K, qb = qa + rows * A.K;
        const uint64_t rel = A.pos[qa], first = ms + RV_HDR; /* cell q begins at first + pos[q] - rel */
        uint64_t q = qa;
        if (g0 > first) {
            const uint64_t want = g0 - first + rel;
            if (want >= A.pos[qb]) continue; /* the lane begins behind this message */
            q = cl_find(A.pos, qa, qb, want);
        }
        for (; q < qb; q++) {
            const uint64_t s = first + (A.pos[q] - rel);
            if (s >= pe) break;
            const uint64_t e = first + (A.pos[q + 1] - rel);
            const uint64_t i = q / A.K;
            const uint32_t j = (uint32_t)(q - i * A.K), kind = A.kinds[j];
            if (vl_scalar_kind(kind)) continue;
            const uint64_t bs = s + 3u + (kind == TT_STRING ? 4u : 5u);
            const uint64_t be = e - (j == A.K - 1);
            if (bs >= be) continue;
            const uint64_t u = bs >= p ? 0 : (p - bs + VL_UNIT - 1) / VL_UNIT, at = bs + u * VL_UNIT;
            if (at >= pe || at >= be) continue;
            const dg_val_col &c = A.col[j];
            if (kind == TT_STRING) vl_unit(kind, c.d_src + c.d_val[i], nullptr, u, be - bs, A.out, at, A.cap);
            else vl_unit(kind, nullptr, c.d_elems + c.d_elem_off[i], u, (be - bs) / tg_fixed(kind & 0x3Fu), A.out, at, A.cap);
        }
    }
}

void launch_rvals_size(hipStream_t s, const RVParams &A);
void launch_rvals_msgs(hipStream_t s, const RVParams &A);
void launch_rvals_emit(hipStream_t s, const RVParams &A, uint32_t head_blocks, uint32_t max_blocks, bool bodies);

}  // namespace dg
