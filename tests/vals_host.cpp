/* The typed-column encode (dynamicgo_amd/csrc/vals_device.h) built for the host:
 * the per-cell size function behind vl_pair, the head writer, the body-unit
 * function and the cell search, driven cell by cell and 8 bytes by 8 bytes in
 * the order of the kernels of vals_kern.hip. test_vals_host.py loads it; with
 * -DVALS_MAIN it is a program that runs corpus files with every input array and
 * every output in a heap block of its own, for a sanitizer to watch. */
#define TGI inline
#include "../dynamicgo_amd/csrc/vals_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace dg;

/* One batch: sizes and statuses, offsets (closed: by the formula of a plan of
 * scalars; else the running sum), then with `out` the head of every cell and
 * the bodies: lane_emit 1 by the cell's own loop, 0 chunk by chunk as
 * vals_body_kernel walks the arena with `blocks` blocks. */
extern "C" int vals_run(const uint8_t *kinds, const int16_t *ids, uint32_t K, const dg_val_col *cols, uint64_t n,
                        uint64_t base, uint8_t *out, uint64_t cap, uint64_t *off, uint8_t *status, int lane_emit, int closed,
                        uint32_t blocks)
{
    VLParams A;
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, K * sizeof *cols);
    memcpy(A.kinds, kinds, K);
    if (ids) memcpy(A.ids, ids, 2 * K);
    A.K = K, A.has_ids = ids != nullptr, A.pairs = n * K, A.base = base, A.cap = cap, A.off = off, A.out = out;
    if (closed) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < K; k++) A.pre[k] = (uint8_t)at, at += (ids ? 3u : 0u) + tg_fixed(kinds[k]);
        A.msg = at + (ids ? 1u : 0u);
    }
    uint64_t pos = base;
    for (uint64_t q = 0; q < A.pairs; q++) {
        const VLPair p = vl_pair(A, q);
        if (status) status[q] = (uint8_t)p.z.status;
        off[q] = closed ? base + (uint64_t)p.i * A.msg + A.pre[p.j] : pos;
        pos = off[q] + p.z.len;
    }
    off[A.pairs] = pos;
    if (!out || cap <= base) return 0;
    for (uint64_t q = 0; q < A.pairs; q++) {
        const VLPair p = vl_pair(A, q);
        vl_head(p.kind, p.id, p.fh, p.stop, p.z, p.v, out, off[q], cap);
        if (lane_emit) vl_body_loop(A, p, off[q]);
    }
    if (lane_emit) return 0;
    const uint64_t need = off[A.pairs], total = need < cap ? need : cap, first = base & ~(uint64_t)(VL_UNIT - 1);
    for (uint32_t b = 0; b < blocks; b++)
        for (uint64_t cb = first + (uint64_t)b * VL_CHUNK; cb < total; cb += (uint64_t)blocks * VL_CHUNK) {
            const uint64_t end = cb + VL_CHUNK < total ? cb + VL_CHUNK : total;
            const uint64_t lo = cl_find(off, 0, A.pairs, cb > base ? cb : base), hi = cl_find(off, 0, A.pairs, end - 1) + 1;
            for (uint64_t p = cb; p < end; p += VL_UNIT) vl_granule(A, lo, hi, p, total);
        }
    return 0;
}

/* vl_size alone: out = len, status, hdr, the count written */
extern "C" void vals_size(uint32_t kind, uint32_t fh, uint32_t stop, int present, uint64_t cnt, uint64_t *out)
{
    const VLSize z = vl_size(kind, fh, stop, present != 0, cnt);
    out[0] = z.len, out[1] = z.status, out[2] = z.hdr, out[3] = z.cnt;
}

extern "C" int vals_kind_ok(uint32_t kind) { return vl_kind_ok(kind); }
extern "C" uint32_t vals_wire(uint32_t kind) { return vl_wire(kind); }

#ifdef VALS_MAIN
static void *block(FILE *fh, uint64_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    if (bytes && fread(p, 1, bytes, fh) != bytes) exit(2);
    return p;
}

static uint64_t fnv(uint64_t h, const void *p, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001B3ull;
    return h;
}

/* corpus (valsgen.corpus_bytes): u32 K, n, has_ids; K kind bytes; K i16 ids; per column six u64 lengths and the arrays.
 * Both emits into blocks of exactly need + 16 bytes with cap = need; prints the cells, the flagged cells, the bytes and a
 * hash of offsets, statuses and bytes. */
int main(int argc, char **argv)
{
    unsigned long long cells = 0, flagged = 0, bytes = 0;
    uint64_t h = 0xCBF29CE484222325ull;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t hd[3];
        if (!fh || fread(hd, 4, 3, fh) != 3) return 2;
        const uint32_t K = hd[0], n = hd[1];
        uint8_t kinds[16];
        int16_t ids[16];
        if (K > 16 || fread(kinds, 1, K, fh) != K || fread(ids, 2, K, fh) != K) return 2;
        dg_val_col cols[16];
        std::vector<void *> held;
        for (uint32_t k = 0; k < K; k++) {
            uint64_t len[6];
            if (fread(len, 8, 6, fh) != 6) return 2;
            const uint32_t width[6] = {8, 4, 1, 8, 8, 1};
            void *p[6];
            for (int a = 0; a < 6; a++) p[a] = len[a] ? block(fh, len[a] * width[a]) : nullptr, held.push_back(p[a]);
            cols[k] = dg_val_col{(const uint64_t *)p[0], (const uint32_t *)p[1], (const uint8_t *)p[2], (const uint64_t *)p[3],
                                 (const uint64_t *)p[4], (const uint8_t *)p[5]};
        }
        fclose(fh);
        const uint64_t pairs = (uint64_t)n * K;
        uint64_t *off = (uint64_t *)malloc((pairs + 1) * 8);
        uint8_t *st = (uint8_t *)malloc(pairs ? pairs : 1);
        vals_run(kinds, hd[2] ? ids : nullptr, K, cols, n, 0, nullptr, 0, off, st, 0, 0, 1);
        const uint64_t need = off[pairs];
        uint8_t *out[2];
        for (int lane = 0; lane < 2; lane++) {
            out[lane] = (uint8_t *)malloc(need + 16);
            memset(out[lane], 0xAA, need + 16);
            vals_run(kinds, hd[2] ? ids : nullptr, K, cols, n, 0, out[lane], need, off, st, lane, 0, 3);
        }
        if (memcmp(out[0], out[1], need + 16)) return 3;
        for (uint64_t q = 0; q < pairs; q++) flagged += st[q] != 0;
        cells += pairs, bytes += need;
        h = fnv(fnv(fnv(h, off, (pairs + 1) * 8), st, pairs), out[0], need + 16);
        free(out[0]), free(out[1]), free(off), free(st);
        for (void *p : held) free(p);
    }
    printf("%llu cells, %llu flagged, %llu bytes, hash %016llx\n", cells, flagged, bytes, (unsigned long long)h);
    return 0;
}
#endif
