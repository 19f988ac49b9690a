/*
 * kids_device.h — batched Children over Thrift binary (include/dgj2t.h
 * dg_kids_*): the device restatement of the reference's Node.Children /
 * PathNode.scanChildren + handleChild (thrift/generic/node.go:1133-1154,
 * path.go:796-836, 1121-1248) behind GetByPath (tget_device.h).
 *
 * One lane takes one message, twice: the count pass walks to the node
 * (tg_seek: it stops at the node's start), scans it and writes the message's
 * head; after a scan of the counts the emit pass resumes at head.start and
 * stores the records. Both passes run kd_scan, with a sink that counts or one
 * that stores.
 *
 * The Go skips every child (SkipType with a budget of its own) and, in
 * recursive mode, scans the child's bytes again, level by level: quadratic in
 * depth. kd_scan makes ONE walk. The containers it scans are open frames of its
 * own; a value it does not scan (a scalar, a map key, every child in one-level
 * mode) is skipped by tg_skip from the depth it sits at. The only depth limit
 * that can fail is the outermost skip's (every later one covers fewer levels
 * with the same 1023): GetByPath's skip of the node for a non-empty path, each
 * direct child's for the empty path. So a value inside S scanned containers
 * below the node is met at skip depth S + 1 (non-empty path) or S (empty path).
 *
 * Frames: the innermost scanned container lives in registers (c0, c1), the S
 * enclosing ones in frame levels [0, S), two 64-bit words a level; a skip
 * started at depth D uses the first word of levels [D, ...). D >= S, so it
 * never touches a scanned level. KD_LDS_DEPTH levels per lane in LDS; a message
 * that needs more ends TG_R_DEEP and is rerun with KD_DEEP_DEPTH levels in
 * device memory.
 *
 * Bounds: as tget_device.h (p never passes len; windows read 16 bytes at p).
 * The storing sink never writes a record at or past the message's count.
 */
#pragma once
#include "scan_defs.h"
#include "tget_device.h"

namespace dg {

constexpr uint32_t KD_BLOCK = 256;
constexpr uint32_t KD_LDS_DEPTH = 8;     /* levels per lane in LDS: 2 words each, 32 KB a block */
constexpr uint32_t KD_DEEP_DEPTH = 1024; /* ... per lane of the deep pass */
constexpr uint32_t KD_DEEP_BLOCK = 64, KD_DEEP_BLOCKS = 32;
constexpr uint32_t KD_DEEP_LANES = KD_DEEP_BLOCK * KD_DEEP_BLOCKS;
constexpr uint32_t KD_WIDE_BLOCK = 256;

struct KDParams {
    TGParams tg;          /* src, in_off, root_type, blob, off_steps, off_pool: what tg_seek reads */
    uint64_t n;
    uint32_t n_steps;     /* the path's length; 0 = the message's root */
    uint32_t recurse;
    dg_kids_head *head;
    uint64_t *rec_off;
    dg_kid_rec *recs;
    uint64_t rec_cap;
    uint64_t wide_min;    /* 0: no wide route */
    uint32_t *deep_list;  /* messages queued for the deep pass */
    uint32_t *wide_list;  /* ... for the wide kernel */
    uint32_t *cnt;        /* this stage's counters: [0] deep, [1] wide */
    uint32_t *reset;      /* the other stage's, zeroed by the deep pass */
    uint64_t *ws;         /* deep frames: [word * KD_DEEP_DEPTH + level][lane] */
    unsigned long long *stats; /* the context's counters: [KD_STAT_DEEP] += messages a deep pass reran */
};
constexpr uint32_t KD_STAT_DEEP = 12;

/* a lane's levels: at() is the word tg_skip uses too */
struct KDLdsFrames {
    static constexpr uint32_t cap = KD_LDS_DEPTH;
    uint64_t *base; /* &frames[threadIdx.x] */
    TGI uint64_t &at(uint32_t l) const { return base[l * KD_BLOCK]; }
    TGI uint64_t &aux(uint32_t l) const { return base[(KD_LDS_DEPTH + l) * KD_BLOCK]; }
};
struct KDDeepFrames {
    static constexpr uint32_t cap = KD_DEEP_DEPTH;
    uint64_t *base;
    TGI uint64_t &at(uint32_t l) const { return base[(uint64_t)l * KD_DEEP_LANES]; }
    TGI uint64_t &aux(uint32_t l) const { return base[(uint64_t)(KD_DEEP_DEPTH + l) * KD_DEEP_LANES]; }
};

TGI bool kd_complex(uint32_t t) { return t >= TT_STRUCT && t <= TT_LIST; }

/* the sinks of kd_scan: add() takes a child in wire order and returns its
 * index among the message's records; close() completes a container's record */
struct KDCount {
    static constexpr bool emit = false;
    uint32_t k = 0;
    TGI uint32_t add(uint64_t, uint64_t, uint64_t, uint32_t, int64_t, uint32_t, uint32_t, uint32_t) { return k++; }
    TGI void close(uint32_t, uint64_t) {}
};
struct KDStore {
    static constexpr bool emit = true;
    dg_kid_rec *out; /* the message's first record */
    uint32_t cap;    /* its count: nothing is stored at or past it */
    uint32_t k = 0;
    TGI uint32_t add(uint64_t start, uint64_t end, uint64_t key_start, uint32_t parent, int64_t key, uint32_t type,
                     uint32_t kind, uint32_t depth)
    {
        if (k < cap) { /* two 16-byte stores */
            uint4 lo, hi;
            lo.x = (uint32_t)start, lo.y = (uint32_t)end, lo.z = (uint32_t)key_start, lo.w = parent;
            hi.x = (uint32_t)(uint64_t)key, hi.y = (uint32_t)((uint64_t)key >> 32);
            hi.z = (type & 0xFFu) | (kind & 0xFFu) << 8 | (depth & 0xFFFFu) << 16, hi.w = 0;
            uint4 *r = (uint4 *)(void *)(out + k);
            r[0] = lo, r[1] = hi;
        }
        return k++;
    }
    TGI void close(uint32_t idx, uint64_t end)
    {
        if (idx >= cap) return;
        out[idx].end = (uint32_t)end;
        out[idx].n_desc = k - idx - 1;
    }
};

/* the strict header of a scanned container at b[p]: ReadListBegin /
 * ReadMapBegin (binary.go:585-649; a struct has none). c0 = entries left
 * (bits 0-31; a map counts entries) | key type << 32 | value type << 40 |
 * kind << 48 (0 struct, 1 list or set, 2 map); false = ErrRead */
TGI bool kd_open(const uint8_t *b, uint64_t len, uint64_t &p, uint32_t t, uint64_t &c0)
{
    if (t == TT_STRUCT) {
        c0 = 0;
        return true;
    }
    if (t == TT_MAP) {
        uint32_t kt, vt;
        int64_t size;
        if (!tg_map_begin(b, len, p, kt, vt, size)) return false;
        c0 = (uint64_t)size | (uint64_t)kt << 32 | (uint64_t)vt << 40 | 2ull << 48;
        return true;
    }
    if (p + 1 > len) return false;
    const TGWin w = tg_ld(b + p);
    const uint32_t et = tg_u8(w, 0);
    if (!tg_valid(et) || p + 5 > len) return false;
    const int32_t size = (int32_t)tg_be32(w, 1);
    if (size < 0) return false;
    p += 5;
    c0 = (uint64_t)(uint32_t)size | (uint64_t)et << 32 | (uint64_t)et << 40 | 1ull << 48;
    return true;
}

/* scanChildren of the node of wire type tt (a struct, list, set or map) at
 * b[p]; empty: the path is empty (see the depth rule above). TG_R_OK: the
 * children went to sk, direct = how many are the node's own, c_node = the
 * node's frame word (its types). TG_R_FAIL = ErrRead. */
template <class FR, class SK>
TGI uint32_t kd_scan(const uint8_t *b, uint64_t len, uint64_t p, uint32_t tt, uint32_t empty, bool recurse,
                     const FR &fr, SK &sk, uint32_t &direct, uint64_t &c_node)
{
    uint32_t S = 0;
    uint64_t c0, c1;
    if (!kd_open(b, len, p, tt, c0)) return TG_R_FAIL;
    c_node = c0;
    c1 = (uint64_t)DG_KIDS_NO_PARENT | (c0 & 0xFFFFFFFFull) << 32; /* the record's index | the size */
    direct = 0;
    for (;;) {
        const uint32_t kind = (uint32_t)(c0 >> 48);
        const uint32_t D = S + 1 - empty;
        uint32_t ct, pk = 0, k = 0;
        int64_t key = 0;
        uint64_t key_start = p;
        TGWin w;
        bool closes = false;
        if (kind == 0) { /* ReadFieldBegin (binary.go:562-577) */
            if (p + 1 > len) return TG_R_FAIL;
            w = tg_ld(b + p);
            ct = tg_u8(w, 0);
            if (!tg_valid(ct)) return TG_R_FAIL;
            p += 1;
            if (ct == TT_STOP) {
                closes = true;
            } else {
                if (p + 2 > len) return TG_R_FAIL;
                p += 2;
                key = tg_be16(w, 1), pk = DG_PS_FIELD, k = 3;
            }
        } else {
            const uint32_t left = (uint32_t)c0;
            const uint32_t kt = (uint32_t)(c0 >> 32) & 0xFFu;
            ct = (uint32_t)(c0 >> 40) & 0xFFu;
            const uint32_t ks = kind == 2 ? tg_fixed(kt) : 0u, vs = tg_fixed(ct);
            if (!left) {
                closes = true;
            } else if (!SK::emit && vs && (kind == 1 || ks)) { /* counting: entries of one size are a multiplication */
                const uint64_t e = p + (uint64_t)left * (ks + vs);
                if (e > len) return TG_R_FAIL;
                p = e;
                sk.k += left;
                if (!S) direct += left;
                c0 -= left;
                continue;
            } else {
                c0 -= 1;
                if (kind == 1) {
                    key = (int64_t)((uint32_t)(c1 >> 32) - left), pk = DG_PS_INDEX;
                } else if (kt == TT_STRING) { /* ReadString (binary.go:767-791) */
                    if (p + 4 > len) return TG_R_FAIL;
                    const int32_t sz = (int32_t)tg_be32(tg_ld(b + p), 0);
                    p += 4;
                    if (sz < 0 || (uint64_t)sz > len - p) return TG_R_FAIL;
                    p += (uint64_t)sz;
                    key = sz, pk = DG_PS_STRKEY;
                } else if (kt == TT_BYTE || kt == TT_I16 || kt == TT_I32 || kt == TT_I64) { /* ReadInt: a byte is unsigned */
                    if (p + ks > len) return TG_R_FAIL;
                    const uint64_t raw = __builtin_bswap64(tg_ld(b + p).lo);
                    key = kt == TT_BYTE ? (int64_t)(raw >> 56) : (int64_t)raw >> (64 - 8 * ks);
                    p += ks;
                    pk = DG_PS_INTKEY;
                } else { /* the bytes SkipType(kt) delimits; a key is never descended into */
                    const uint32_t r = tg_skip(b, len, p, kt, fr, tg_ld(b + p), 0, D);
                    if (r) return r;
                    key = (int64_t)(p - key_start), pk = DG_PS_BINKEY;
                }
                w = tg_ld(b + p);
            }
        }
        if (closes) {
            if (!S) return TG_R_OK;
            sk.close((uint32_t)c1, p);
            S--;
            c0 = fr.at(S), c1 = fr.aux(S);
            continue;
        }
        /* handleChild: the value of wire type ct at p */
        const uint64_t start = p;
        const uint32_t fs = tg_fixed(ct);
        if (fs) {
            if (p + fs > len) return TG_R_FAIL;
            p += fs;
        } else if (ct == TT_STRING) { /* a struct's field pays the depth test, an element does not (tg_value) */
            if (kind == 0 && D >= TG_MAX_SKIP) return TG_R_FAIL;
            if (p + 4 > len) return TG_R_FAIL;
            const uint64_t e = p + 4 + (uint64_t)tg_be32(w, k);
            if (e > len) return TG_R_FAIL;
            p = e;
        } else if (!kd_complex(ct)) {
            return TG_R_FAIL; /* skipType's default */
        } else if (!recurse) {
            const uint32_t r = tg_skip(b, len, p, ct, fr, w, k, D);
            if (r) return r;
        } else { /* scanned in place of skip-then-scan: its record is completed when it closes */
            if (D >= TG_MAX_SKIP) return TG_R_FAIL; /* errExceedDepthLimit */
            if (S >= FR::cap) return TG_R_DEEP;
            const uint32_t idx = sk.add(start, 0, key_start, (uint32_t)c1, key, ct, pk, S + 1);
            if (!S) direct++;
            fr.at(S) = c0, fr.aux(S) = c1;
            S++;
            if (!kd_open(b, len, p, ct, c0)) return TG_R_FAIL;
            c1 = (uint64_t)idx | (c0 & 0xFFFFFFFFull) << 32;
            continue;
        }
        sk.add(start, p, key_start, (uint32_t)c1, key, ct, pk, S + 1);
        if (!S) direct++;
    }
}

TGI void kd_put_head(dg_kids_head *dst, uint32_t count, uint32_t direct, uint64_t start, uint32_t type, uint32_t kt,
                     uint32_t et, uint32_t status)
{
    uint4 v; /* one 16-byte store */
    v.x = count, v.y = direct, v.z = (uint32_t)start;
    v.w = (type & 0xFFu) | (kt & 0xFFu) << 8 | (et & 0xFFu) << 16 | (status & 0xFFu) << 24;
    *(uint4 *)(void *)dst = v;
}

/* the count pass of message i: GetByPath up to the node, the scan, the head.
 * true = the message needs the deep frames (nothing is written) */
template <class FR>
TGI bool kd_count_msg(const KDParams &A, uint64_t i, const FR &fr)
{
    const uint64_t a = A.tg.in_off[i], len = A.tg.in_off[i + 1] - a;
    const uint8_t *b = A.tg.src + a;
    const TGRes at = tg_seek(A.tg, b, len, 0, fr);
    if (at.status == TG_ST_DEEP) return true;
    dg_kids_head *h = A.head + i;
    if (at.status != DG_TGET_OK) {
        kd_put_head(h, 0, at.step, 0, 0, 0, 0, at.status);
        return false;
    }
    if (!kd_complex(at.type)) { /* GetByPath's SkipType(node) comes before Children's default case */
        uint64_t p = at.start;
        if (A.n_steps && tg_skip(b, len, p, at.type, fr, tg_ld(b + p), 0))
            kd_put_head(h, 0, A.n_steps, 0, 0, 0, 0, DG_TGET_E_READ);
        else kd_put_head(h, 0, A.n_steps, at.start, at.type, 0, 0, DG_KIDS_E_UNSUPPORTED);
        return false;
    }
    KDCount sk;
    uint32_t direct;
    uint64_t cn;
    const uint32_t r = kd_scan(b, len, at.start, at.type, A.n_steps == 0, A.recurse != 0, fr, sk, direct, cn);
    if (r == TG_R_DEEP) return true;
    if (r) kd_put_head(h, 0, A.n_steps, 0, 0, 0, 0, DG_TGET_E_READ);
    else kd_put_head(h, sk.k, direct, at.start, at.type, (cn >> 48) == 2 ? (uint32_t)(cn >> 32) : 0u,
                     (cn >> 48) ? (uint32_t)(cn >> 40) : 0u, DG_TGET_OK);
    return false;
}

/* the emit pass of message i (head OK, cnt records at rec_off[i], which fit):
 * the scan again from head.start. true = it needs the deep frames */
template <class FR>
TGI bool kd_emit_msg(const KDParams &A, uint64_t i, uint32_t cnt, const FR &fr)
{
    const uint64_t a = A.tg.in_off[i], len = A.tg.in_off[i + 1] - a;
    const dg_kids_head h = A.head[i];
    KDStore sk{A.recs + A.rec_off[i], cnt};
    uint32_t direct;
    uint64_t cn;
    return kd_scan(A.tg.src + a, len, h.start, h.type, A.n_steps == 0, A.recurse != 0, fr, sk, direct, cn) == TG_R_DEEP;
}

/* a node the wide kernel can emit: every child at a computable position */
TGI bool kd_wide_ok(const dg_kids_head &h)
{
    if (h.type == TT_MAP) return tg_fixed(h.key_type) && tg_fixed(h.elem_type);
    return (h.type == TT_LIST || h.type == TT_SET) && tg_fixed(h.elem_type);
}

void launch_kids_count(hipStream_t s, const KDParams &A);
void launch_kids_scan(hipStream_t s, const KDParams &A, uint64_t *sums);
void launch_kids_emit(hipStream_t s, const KDParams &A, uint32_t wide_blocks);

}  // namespace dg
