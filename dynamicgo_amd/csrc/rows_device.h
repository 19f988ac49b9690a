/*
 * rows_device.h — row columns (include/dgj2t.h dg_rows_*): the fields of every
 * element of a list or set as ragged columns, the device restatement of
 *     v.GetByPath(parent...).Children(&kids, false, opts)
 *     for each kid: kid.Node.GetByPath(sub...) and a cast
 * over the pieces the other components own: tg_seek / tg_walk / tg_skip
 * (tget_device.h), kd_scan with its sink template (kids_device.h), cl_cell and
 * the scan of the counts (cols_device.h). Nothing of them is restated here.
 *
 * Four passes on one stream:
 *   head    one lane per message: tg_seek to the parent, kd_scan one level with
 *           the counting sink (a list of fixed-size elements is a
 *           multiplication), the head and the count;
 *   scan    launch_cols_scan over the counts: row_off;
 *   index   one lane per message: the same walk with RWStore, one 16-byte entry
 *           per element at row_off[i] + j (a list of fixed-size elements: by
 *           arithmetic, without the walk);
 *   cells   one lane per (row, column) pair, the P pairs of a row in
 *           neighbouring lanes: tg_walk over the element's own bytes with the
 *           list's element type as the root type, then cl_cell.
 * Work of the cell pass is balanced over elements, not over messages.
 *
 * Frames: TG_LDS_DEPTH levels per lane in LDS in every lane pass; what nests
 * deeper is queued and rerun with TG_DEEP_DEPTH levels in device memory. The
 * head and index walks never recurse (kd_scan's recurse is false), so S stays 0
 * and a level's second word (aux) is never touched: it aliases the first.
 *
 * Bounds: as tget_device.h over the message (head, index) and over the
 * element (cells): the read position never passes the element's length, and a
 * window reads 16 bytes at it. No index entry and no cell of a row >= row_cap
 * is stored.
 *
 * Map plans (dg_rows_create_map): the parent is a MAP, a row is an entry, its
 * index entry the VALUE's span, its key stored beside it. The head
 * (rw_map_head_msg) and the index (rw_map_index_msg) are operations of their
 * own over RWMapParams with a storing sink of their own (RWMapStore) behind the
 * same kd_scan; the list operations above, the cell pass, the scan, the queues
 * and the frames are shared unchanged. A map whose key and value are both of
 * fixed size gets its entries and keys by arithmetic. Key loads are windows of
 * 16 bytes at a position that never passes the message's length.
 */
#pragma once
#include "cols_device.h"
#include "kids_device.h"

namespace dg {

constexpr uint32_t RW_BLOCK = 256;

struct RWParams {
    TGParams par;          /* src, in_off, root_type and the parent path's blob: what tg_seek reads */
    TGParams sub;          /* the sub-paths' blob, P; root_type is set per row */
    uint64_t n;
    uint32_t n_steps;      /* the parent path's length; 0 = the message's root */
    uint64_t kinds;        /* byte k: column k's kind */
    dg_rows_head *head;
    uint32_t *count;       /* n: the heads' counts, what the scan reads */
    uint64_t *row_off;     /* n + 1 */
    dg_row_ent *idx;
    uint64_t row_cap;
    uint64_t *val;         /* column-major over row_cap */
    uint64_t *cell;        /* dg_col_cell as one word (cl_cell_word) */
    uint32_t *len;         /* may be null */
    uint32_t *deep_list;   /* messages (head, index) or pairs (cells) queued for the deep pass */
    uint32_t *cnt;         /* this pass's queue counter */
    uint32_t *reset;       /* the other pass's, zeroed by the deep pass */
    uint64_t *ws;          /* deep frames: [level * TG_DEEP_LANES + lane] */
};

struct RWLdsFrames : TGLdsFrames {
    TGI uint64_t &aux(uint32_t l) const { return at(l); }
};
struct RWDeepFrames : TGDeepFrames {
    TGI uint64_t &aux(uint32_t l) const { return at(l); }
};

/* kd_scan's storing sink for rows: element k's index entry, one 16-byte store.
 * Nothing is stored at or past cap, the message's own count cut at row_cap. */
struct RWStore {
    static constexpr bool emit = true;
    dg_row_ent *out; /* the message's first entry */
    uint32_t cap;
    uint64_t base;   /* the message's arena offset */
    uint32_t msg;
    uint32_t k = 0;
    TGI uint32_t add(uint64_t start, uint64_t end, uint64_t, uint32_t, int64_t, uint32_t, uint32_t, uint32_t)
    {
        if (k < cap) {
            const uint64_t o = base + start;
            uint4 v;
            v.x = (uint32_t)o, v.y = (uint32_t)(o >> 32), v.z = (uint32_t)(end - start), v.w = msg;
            *(uint4 *)(void *)(out + k) = v;
        }
        return k++;
    }
    TGI void close(uint32_t, uint64_t) {}
};

TGI void rw_put_head(const RWParams &A, uint64_t i, uint64_t first, uint32_t count, uint32_t status, uint32_t type,
                     uint32_t et, uint32_t step)
{
    uint4 v; /* one 16-byte store */
    v.x = (uint32_t)first, v.y = (uint32_t)(first >> 32), v.z = count;
    v.w = (status & 0xFFu) | (type & 0xFFu) << 8 | (et & 0xFFu) << 16 | (step & 0xFFu) << 24;
    *(uint4 *)(void *)(A.head + i) = v;
    A.count[i] = count;
}

/* the head of message i: GetByPath up to the parent, then Children one level,
 * counted. true = the message needs the deep frames (nothing is written) */
template <class FR>
TGI bool rw_head_msg(const RWParams &A, uint64_t i, const FR &fr)
{
    const uint64_t a = A.par.in_off[i], len = A.par.in_off[i + 1] - a;
    const uint8_t *b = A.par.src + a;
    const TGRes at = tg_seek(A.par, b, len, 0, fr);
    if (at.status == TG_ST_DEEP) return true;
    if (at.status != DG_TGET_OK) {
        rw_put_head(A, i, 0, 0, at.status, 0, 0, at.step);
        return false;
    }
    if (at.type != TT_LIST && at.type != TT_SET) { /* GetByPath's SkipType(node) comes before the type test */
        uint64_t p = at.start;
        const uint32_t r = A.n_steps ? tg_skip(b, len, p, at.type, fr, tg_ld(b + p), 0) : (uint32_t)TG_R_OK;
        if (r == TG_R_DEEP) return true;
        if (r) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
        else rw_put_head(A, i, 0, 0, DG_COL_E_UNSUPPORTED, at.type, 0, A.n_steps);
        return false;
    }
    KDCount sk;
    uint32_t direct;
    uint64_t cn;
    const uint32_t r = kd_scan(b, len, at.start, at.type, A.n_steps == 0, false, fr, sk, direct, cn);
    if (r == TG_R_DEEP) return true;
    if (r) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
    else rw_put_head(A, i, a + at.start + 5, direct, DG_TGET_OK, at.type, (uint32_t)(cn >> 40), A.n_steps);
    return false;
}

/* the index entries of message i (rows [row_off[i], row_off[i] + count) below
 * row_cap). true = the walk needs the deep frames */
template <class FR>
TGI bool rw_index_msg(const RWParams &A, uint64_t i, const FR &fr)
{
    const dg_rows_head h = A.head[i];
    const uint64_t r0 = A.row_off[i];
    if (h.status != DG_TGET_OK || !h.count || r0 >= A.row_cap) return false;
    const uint64_t room = A.row_cap - r0;
    const uint32_t take = h.count < room ? h.count : (uint32_t)room;
    dg_row_ent *out = A.idx + r0;
    const uint32_t fs = tg_fixed(h.elem_type);
    if (fs) { /* element j at first + j * fs: the count pass has checked that all of them lie inside the message */
        for (uint32_t j = 0; j < take; j++) {
            const uint64_t o = h.first + (uint64_t)j * fs;
            uint4 v;
            v.x = (uint32_t)o, v.y = (uint32_t)(o >> 32), v.z = fs, v.w = (uint32_t)i;
            *(uint4 *)(void *)(out + j) = v;
        }
        return false;
    }
    const uint64_t a = A.par.in_off[i], len = A.par.in_off[i + 1] - a;
    RWStore sk{out, take, a, (uint32_t)i};
    uint32_t direct;
    uint64_t cn;
    return kd_scan(A.par.src + a, len, h.first - a - 5, h.type, A.n_steps == 0, false, fr, sk, direct, cn) == TG_R_DEEP;
}

/* ---- map plans: the entries of a map<K, V> as rows, with their keys ---- */

struct RWMapParams : RWParams {
    uint64_t *key;      /* row_cap; may be null */
    uint32_t *key_len;  /* row_cap; may be null */
    uint32_t key_kind;  /* DG_ROWS_KEY_STR or DG_ROWS_KEY_INT */
};

/* a map's key type under a plan's key kind: StrMap's and IntMap's restriction */
TGI bool rw_key_ok(uint32_t key_kind, uint32_t kt)
{
    if (key_kind == DG_ROWS_KEY_STR) return kt == TT_STRING;
    return kt == TT_BYTE || kt == TT_I16 || kt == TT_I32 || kt == TT_I64;
}

/* one row of a map: 16 + 8 + 4 bytes */
TGI void rw_put_entry(dg_row_ent *out, uint64_t *key, uint32_t *key_len, uint32_t k, uint64_t off, uint32_t len,
                      uint32_t msg, uint64_t kv, uint32_t kl)
{
    uint4 v;
    v.x = (uint32_t)off, v.y = (uint32_t)(off >> 32), v.z = len, v.w = msg;
    *(uint4 *)(void *)(out + k) = v;
    if (key) key[k] = kv;
    if (key_len) key_len[k] = kl;
}

/* kd_scan's storing sink for map rows: entry k's index entry (the value's
 * span), its key and its key length. A string key is the arena offset of its
 * payload and the payload's length; an int key is ReadInt's value and its
 * width, the bytes between the key's start and the value's. Nothing is stored
 * at or past cap. */
struct RWMapStore {
    static constexpr bool emit = true;
    dg_row_ent *out; /* the message's first entry */
    uint64_t *key;   /* ... first key, or null */
    uint32_t *key_len;
    uint32_t cap;
    uint64_t base;   /* the message's arena offset */
    uint32_t msg;
    uint32_t k = 0;
    TGI uint32_t add(uint64_t start, uint64_t end, uint64_t key_start, uint32_t, int64_t kv, uint32_t, uint32_t kind, uint32_t)
    {
        if (k < cap) {
            const bool str = kind == DG_PS_STRKEY;
            rw_put_entry(out, key, key_len, k, base + start, (uint32_t)(end - start), msg,
                         str ? base + key_start + 4 : (uint64_t)kv, str ? (uint32_t)kv : (uint32_t)(start - key_start));
        }
        return k++;
    }
    TGI void close(uint32_t, uint64_t) {}
};

/* the head of message i under a map plan: GetByPath up to the parent, the
 * map's header, the key type against the plan's key kind, then Children one
 * level, counted. true = the message needs the deep frames (nothing is
 * written) */
template <class FR>
TGI bool rw_map_head_msg(const RWMapParams &A, uint64_t i, const FR &fr)
{
    const uint64_t a = A.par.in_off[i], len = A.par.in_off[i + 1] - a;
    const uint8_t *b = A.par.src + a;
    const TGRes at = tg_seek(A.par, b, len, 0, fr);
    if (at.status == TG_ST_DEEP) return true;
    if (at.status != DG_TGET_OK) {
        rw_put_head(A, i, 0, 0, at.status, 0, 0, at.step);
        return false;
    }
    uint32_t kt = 0, vt = 0;
    bool hdr = true;
    if (at.type == TT_MAP) {
        uint64_t p = at.start;
        int64_t size;
        hdr = tg_map_begin(b, len, p, kt, vt, size);
    }
    if (at.type != TT_MAP || (hdr && !rw_key_ok(A.key_kind, kt))) { /* GetByPath's SkipType(node) comes before both tests */
        uint64_t p = at.start;
        const uint32_t r = A.n_steps ? tg_skip(b, len, p, at.type, fr, tg_ld(b + p), 0) : (uint32_t)TG_R_OK;
        if (r == TG_R_DEEP) return true;
        if (r) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
        else rw_put_head(A, i, 0, 0, DG_COL_E_UNSUPPORTED, at.type, at.type == TT_MAP ? kt : 0u, A.n_steps);
        return false;
    }
    if (!hdr) { /* ReadMapBegin refuses it; so does the node's skip, or Children behind it */
        rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
        return false;
    }
    KDCount sk;
    uint32_t direct;
    uint64_t cn;
    const uint32_t r = kd_scan(b, len, at.start, TT_MAP, A.n_steps == 0, false, fr, sk, direct, cn);
    if (r == TG_R_DEEP) return true;
    if (r) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
    else rw_put_head(A, i, a + at.start + 6, direct, DG_TGET_OK, TT_MAP, vt, A.n_steps);
    return false;
}

/* the index entries and the keys of message i under a map plan (rows
 * [row_off[i], row_off[i] + count) below row_cap). true = the walk needs the
 * deep frames */
template <class FR>
TGI bool rw_map_index_msg(const RWMapParams &A, uint64_t i, const FR &fr)
{
    const dg_rows_head h = A.head[i];
    const uint64_t r0 = A.row_off[i];
    if (h.status != DG_TGET_OK || !h.count || r0 >= A.row_cap) return false;
    const uint64_t room = A.row_cap - r0;
    const uint32_t take = h.count < room ? h.count : (uint32_t)room;
    dg_row_ent *out = A.idx + r0;
    uint64_t *key = A.key ? A.key + r0 : nullptr;
    uint32_t *key_len = A.key_len ? A.key_len + r0 : nullptr;
    const uint64_t a = A.par.in_off[i], len = A.par.in_off[i + 1] - a;
    const uint8_t *b = A.par.src + a;
    const uint64_t p0 = h.first - a; /* entry 0's key; the header lies 6 bytes before it */
    const uint32_t kt = tg_u8(tg_ld(b + (p0 - 6)), 0);
    const uint32_t ks = tg_fixed(kt), vs = tg_fixed(h.elem_type);
    if (ks && vs) { /* entry j at first + j * (ks + vs): the count pass has checked that all of them lie inside the message */
        for (uint32_t j = 0; j < take; j++) {
            const uint64_t p = p0 + (uint64_t)j * (ks + vs);
            const uint64_t raw = __builtin_bswap64(tg_ld(b + p).lo); /* ReadInt: a byte is unsigned */
            const uint64_t kv = kt == TT_BYTE ? raw >> 56 : (uint64_t)((int64_t)raw >> (64 - 8 * ks));
            rw_put_entry(out, key, key_len, j, a + p + ks, vs, (uint32_t)i, kv, ks);
        }
        return false;
    }
    RWMapStore sk{out, key, key_len, take, a, (uint32_t)i};
    uint32_t direct;
    uint64_t cn;
    return kd_scan(b, len, p0 - 6, TT_MAP, A.n_steps == 0, false, fr, sk, direct, cn) == TG_R_DEEP;
}

/* the rows whose cells are written */
TGI uint64_t rw_rows(const RWParams &A)
{
    const uint64_t R = A.row_off[A.n];
    return R < A.row_cap ? R : A.row_cap;
}

/* pair q = (row g, column k): the lookup on the element's own bytes. The
 * result's status is TG_ST_DEEP when the walk needs the deep frames. */
template <class FR>
TGI CLCell rw_cell(const RWParams &A, uint64_t g, uint32_t k, const FR &fr)
{
    const dg_row_ent e = A.idx[g];
    TGParams T = A.sub;
    T.root_type = A.head[e.msg].elem_type;
    const uint8_t *b = A.par.src + e.off;
    const TGRes r = tg_walk(T, b, e.len, k, fr);
    /* cl_cell's 8-byte load starts at b + r.start <= b + e.len, the element's
     * end at the latest: the element lies inside a message, so the load stays
     * inside the arena or the 16 spare bytes behind it. */
    return cl_cell((uint32_t)(A.kinds >> (k * 8)) & 0xFFu, r, b, e.off);
}

/* cell (g, k): 8 + 8 (+ 4) bytes, column-major over row_cap */
TGI void rw_store(const RWParams &A, uint64_t g, uint32_t k, const CLCell &c)
{
    const uint64_t at = (uint64_t)k * A.row_cap + g;
    A.val[at] = c.val;
    A.cell[at] = cl_cell_word(c);
    if (A.len) A.len[at] = c.len;
}

void launch_rows_head(hipStream_t s, const RWParams &A);
void launch_rows_index(hipStream_t s, const RWParams &A);
void launch_rows_cells(hipStream_t s, const RWParams &A);
void launch_rows_map_head(hipStream_t s, const RWMapParams &A);
void launch_rows_map_index(hipStream_t s, const RWMapParams &A);

}  // namespace dg
