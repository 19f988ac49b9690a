/*
 * cut_device.h — batched MarshalTo ("cutting", include/dgj2t.h dg_cut_*): the
 * device restatement of the reference's Value.MarshalTo / marshalTo /
 * handleUnsets (thrift/generic/value.go:375-552) over RequiresBitmap.CheckRequires
 * (thrift/utils.go:110-141), BinaryProtocol.WriteEmpty (thrift/binary.go:483-515),
 * the Read*Begin checks (thrift/binary.go:562-649) and SkipType (tget_device.h
 * tg_skip).
 *
 * Every byte the reference writes for a kept value is a byte of the source (it
 * echoes the headers it read), so the output of a message is a concatenation
 * of source spans and the plan's unset literals. The walk keeps ONE open kept
 * run [run, p) of source bytes and hands it to the sink only when a dropped
 * value, a literal or the end of the message interrupts it: neighbouring kept
 * fields are one copy. The walk is a template over the frame stores (one frame
 * per open cut container; the skipper's frames are tget's) and the sink, and
 * compiles for the host too (CUTI, like TGI).
 *
 * Bounds. Reads: the read position never passes the message length and a
 * window reads 16 bytes at it, so at most 16 bytes past the message (the arena
 * rule of tget); a sink reads at most 15 bytes past a run's or a literal's end
 * (the plan blob has 16 zero bytes after it). Writes: a sink writes
 * [dst + o, dst + o + n) and nothing else, and only while o + n <= cap; past
 * that it counts without writing (DG_CUT_E_OVERFLOW with the needed size).
 * Neither sink rounds a store up: no byte at or beyond out_len is written on
 * success.
 */
#pragma once
#include "tget_device.h"

namespace dg {

#ifndef CUTI /* a host build of the walk defines it (and TGI) as `inline` */
#define CUTI __device__ __forceinline__
#endif

constexpr uint32_t CUT_BLOCK = 256;
constexpr uint32_t CUT_LDS_DEPTH = 8;   /* cut frames per lane of the lane route (32 KB a block) */
constexpr uint32_t CUT_WAVES = 4;       /* waves per block of the wave route */
constexpr uint32_t CUT_ST_DEEP = 0xF1;  /* internal: more cut frames than the store has */
constexpr uint32_t CUT_ST_SKIPDEEP = 0xF2; /* internal: a skipped or copied value nests beyond the skip frames */

struct CutPlanView {
    const dg_cut_node *nodes;
    const dg_cut_field *fields;
    const dg_cut_lit *lits;
    const uint8_t *pool;
    uint32_t root;
};

struct CutParams {
    CutPlanView plan;
    /* the plan's tables once more, as bytes blob[0, tab_len) with the tables at
     * these offsets: a block copies them to LDS when they fit (cut_kern.hip) */
    const uint8_t *blob;
    uint32_t tab_len, off_nodes, off_fields, off_lits;
    uint64_t opts;
    const uint8_t *src;
    const uint64_t *in_off;
    uint64_t n;
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint64_t *ret;
    uint64_t wave_min;     /* the lane route declines messages at least this long */
    uint32_t *wave_list;   /* messages queued for the wave route */
    uint32_t *wave_count;
    uint32_t *reset_count; /* the other launch's counter, zeroed by the wave route */
};

/* a store of cut frames: meta = node | entries left << 32 (a map counts keys
 * and values: even = a key is next), mask = a struct's live tracked bits */
struct CutLdsFrames {
    static constexpr uint32_t cap = CUT_LDS_DEPTH;
    uint64_t *m, *k; /* &meta[threadIdx.x], &mask[threadIdx.x]; level l at [l * CUT_BLOCK] */
    CUTI uint64_t &meta(uint32_t l) const { return m[l * CUT_BLOCK]; }
    CUTI uint64_t &mask(uint32_t l) const { return k[l * CUT_BLOCK]; }
};
struct CutWaveFrames { /* one wave's: every lane reads and writes the same words */
    static constexpr uint32_t cap = DG_CUT_MAX_DEPTH;
    uint64_t *m, *k;
    CUTI uint64_t &meta(uint32_t l) const { return m[l]; }
    CUTI uint64_t &mask(uint32_t l) const { return k[l]; }
};
struct CutWaveSkipFrames { /* tg_skip's frames of one wave: MaxSkipDepth fits */
    static constexpr uint32_t cap = TG_DEEP_DEPTH;
    uint64_t *base;
    CUTI uint64_t &at(uint32_t l) const { return base[l]; }
};

/* The lane route's copy engine: one lane copies [s, s + n) to dst + o in
 * 16-byte windows, source and destination at any alignment, the tail clipped
 * to the byte (8 + 4 + 2 + 1). */
struct CutLaneSink {
    uint8_t *dst;
    uint64_t cap, o;
    bool ovf;
    CUTI void put(const uint8_t *s, uint64_t n)
    {
        if (!n) return;
        if (ovf || o + n > cap) {
            ovf = true;
            o += n;
            return;
        }
        uint8_t *d = dst + o;
        o += n;
        uint64_t q = 0;
        for (; q + 16 <= n; q += 16) {
            const TGWin w = tg_ld(s + q);
            __builtin_memcpy(d + q, &w, 16);
        }
        const uint32_t r = (uint32_t)(n - q);
        if (!r) return;
        const TGWin w = tg_ld(s + q);
        uint8_t *t = d + q;
        uint64_t v = w.lo;
        if (r & 8) {
            __builtin_memcpy(t, &v, 8);
            t += 8;
            v = w.hi;
        }
        if (r & 4) {
            const uint32_t x = (uint32_t)v;
            __builtin_memcpy(t, &x, 4);
            t += 4;
            v >>= 32;
        }
        if (r & 2) {
            const uint16_t x = (uint16_t)v;
            __builtin_memcpy(t, &x, 2);
            t += 2;
            v >>= 16;
        }
        if (r & 1) *t = (uint8_t)v;
    }
};

/* The wave route's copy engine: all 64 lanes call put with the same
 * arguments. The head up to the destination's next 16-byte boundary goes byte
 * by byte (a lane each), the body as aligned 16-byte stores in strides of
 * 64 x 16 bytes (the loads are unaligned), the tail byte by byte again. */
struct CutWaveSink {
    uint8_t *dst;
    uint64_t cap, o;
    bool ovf;
    uint32_t lane;
    CUTI void put(const uint8_t *s, uint64_t n)
    {
        if (!n) return;
        if (ovf || o + n > cap) {
            ovf = true;
            o += n;
            return;
        }
        uint8_t *d = dst + o;
        o += n;
        uint64_t h = (16 - ((uintptr_t)d & 15)) & 15;
        if (h > n) h = n;
        if (lane < h) d[lane] = s[lane];
        const uint64_t body = (n - h) >> 4;
        for (uint64_t c = lane; c < body; c += 64) {
            const TGWin w = tg_ld(s + h + c * 16);
            __builtin_memcpy(__builtin_assume_aligned(d + h + c * 16, 16), &w, 16);
        }
        const uint64_t t0 = h + body * 16;
        if (lane < n - t0) d[t0 + lane] = s[t0 + lane];
    }
};

struct CutRes {
    uint32_t status, aux;
};

/* One message b[0, len) under the plan: the bytes go to sk (sk.o = their
 * count, sk.ovf = they did not fit); fr = the cut frames, sf = tg_skip's. */
template <class FR, class SF, class SK>
CUTI CutRes cut_walk(const CutPlanView &P, uint64_t opts, const uint8_t *b, uint64_t len, const FR &fr, const SF &sf,
                     SK &sk)
{
    if (len > 0xFFFFFFFFull) return CutRes{DG_CUT_E_READ, 0xFFFFFFFFu};
    const bool check = !(opts & DG_CUT_NOT_CHECK_REQ);
    uint64_t p = 0, run = 0;
    uint32_t sp = 0, nd = P.root;
    bool have = true; /* a value of node nd begins at p */
    for (;;) {
        if (!have) {
            if (!sp) break;
            const uint64_t f = fr.meta(sp - 1);
            const dg_cut_node &N = P.nodes[(uint32_t)f];
            if (N.kind == DG_CUT_STRUCT) { /* ReadFieldBegin */
                if (p + 1 > len) return CutRes{DG_CUT_E_READ, 0};
                const TGWin w = tg_ld(b + p);
                const uint32_t ft = tg_u8(w, 0);
                if (!tg_valid(ft)) return CutRes{DG_CUT_E_READ, 0};
                p += 1;
                if (ft == TT_STOP) { /* handleUnsets, then the STOP byte stays in the run */
                    const uint64_t live = fr.mask(sp - 1);
                    if (live) {
                        const uint64_t miss = live & N.required;
                        if (miss) /* ascending id = ascending bit: the lowest one */
                            return CutRes{DG_CUT_E_REQUIRED,
                                          (uint32_t)(int32_t)P.lits[N.lit0 + (uint32_t)__builtin_ctzll(miss)].id};
                        if (opts & DG_CUT_WRITE_DEFAULT) {
                            sk.put(b + run, p - 1 - run);
                            for (uint64_t m = live; m; m &= m - 1) {
                                const dg_cut_lit L = P.lits[N.lit0 + (uint32_t)__builtin_ctzll(m)];
                                sk.put(P.pool + L.off, L.len);
                            }
                            run = p - 1;
                        }
                    }
                    sp--;
                    continue;
                }
                if (p + 2 > len) return CutRes{DG_CUT_E_READ, 0};
                p += 2;
                const int32_t id = tg_be16(w, 1);
                /* from.Struct().FieldById: the struct's range of the field table, sorted by id */
                uint32_t lo = N.a, hi = N.a + N.n_fields;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (P.fields[mid].id < id) lo = mid + 1;
                    else hi = mid;
                }
                const bool known = lo < N.a + N.n_fields && P.fields[lo].id == id;
                if (!known && (opts & DG_CUT_DISALLOW_UNKNOWN)) return CutRes{DG_CUT_E_UNKNOWN, (uint32_t)id};
                const dg_cut_field F = known ? P.fields[lo] : dg_cut_field{0, 0, DG_CUT_NO_BIT, DG_CUT_DROP};
                if (known && ft != F.type) return CutRes{DG_CUT_E_TYPE, (uint32_t)id};
                if (F.child == DG_CUT_DROP) { /* SkipType(tt): the run ends before the field header */
                    sk.put(b + run, p - 3 - run);
                    const uint32_t r = tg_skip(b, len, p, ft, sf, w, 3);
                    if (r == TG_R_DEEP) return CutRes{CUT_ST_SKIPDEEP, 0};
                    if (r) return CutRes{DG_CUT_E_READ, 0};
                    run = p;
                    continue;
                }
                if (check && F.bit != DG_CUT_NO_BIT) fr.mask(sp - 1) &= ~(1ull << F.bit);
                nd = F.child;
            } else {
                const uint32_t left = (uint32_t)(f >> 32);
                if (!left) {
                    sp--;
                    continue;
                }
                fr.meta(sp - 1) = f - (1ull << 32);
                nd = N.kind == DG_CUT_MAP && (left & 1) ? N.b : N.a;
            }
        }
        have = false;
        const dg_cut_node &N = P.nodes[nd];
        if (N.kind == DG_CUT_COPY) { /* skip_val: SkipType(to.Type()), the span stays in the run */
            const uint32_t r = tg_skip(b, len, p, N.a, sf, tg_ld(b + p), 0);
            if (r == TG_R_DEEP) return CutRes{CUT_ST_SKIPDEEP, 0};
            if (r) return CutRes{DG_CUT_E_READ, 0};
        } else if (N.kind == DG_CUT_STRUCT) {
            if (sp >= FR::cap) return CutRes{CUT_ST_DEEP, 0};
            fr.meta(sp) = nd;
            fr.mask(sp) = check ? N.tracked : 0;
            sp++;
        } else if (N.kind == DG_CUT_LIST) { /* ReadListBegin; the wire element type is not checked */
            if (p + 1 > len) return CutRes{DG_CUT_E_READ, 0};
            const TGWin w = tg_ld(b + p);
            if (!tg_valid(tg_u8(w, 0)) || p + 5 > len) return CutRes{DG_CUT_E_READ, 0};
            const int32_t size = (int32_t)tg_be32(w, 1);
            if (size < 0) return CutRes{DG_CUT_E_READ, 0};
            p += 5;
            if (size) {
                if (sp >= FR::cap) return CutRes{CUT_ST_DEEP, 0};
                fr.meta(sp) = nd | (uint64_t)(uint32_t)size << 32;
                fr.mask(sp) = 0;
                sp++;
            }
        } else if (N.kind == DG_CUT_MAP) { /* ReadMapBegin */
            uint32_t kt, vt;
            int64_t size;
            if (!tg_map_begin(b, len, p, kt, vt, size)) return CutRes{DG_CUT_E_READ, 0};
            if (size) {
                if (sp >= FR::cap) return CutRes{CUT_ST_DEEP, 0};
                fr.meta(sp) = nd | (uint64_t)(uint32_t)size * 2 << 32;
                fr.mask(sp) = 0;
                sp++;
            }
        } else {
            return CutRes{DG_CUT_E_TYPE, 0};
        }
    }
    sk.put(b + run, p - run);
    return CutRes{DG_CUT_OK, 0};
}

/* message i's out_len and ret from the walk's result */
CUTI void cut_store(const CutParams &A, uint64_t i, CutRes r, uint64_t o, bool ovf)
{
    uint32_t ol = 0;
    if (r.status == DG_CUT_OK) {
        ol = o > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)o;
        if (ovf || o > 0xFFFFFFFFull) r = CutRes{DG_CUT_E_OVERFLOW, ol};
    }
    A.out_len[i] = ol;
    A.ret[i] = (uint64_t)r.status | (uint64_t)r.aux << 32;
}

void launch_cut_lane(hipStream_t s, const CutParams &A);
void launch_cut_wave(hipStream_t s, const CutParams &A, uint32_t blocks);

}  // namespace dg
