/* The row-column encode (dynamicgo_amd/csrc/rvals_device.h) built for the host:
 * the per-lane functions the kernels of rvals_kern.hip run (rv_size_lane,
 * rv_msg_lane, rv_list_head, rv_head_lane and rv_granule over cl_find), driven
 * cell by cell, message by message and chunk by chunk in the kernels' order,
 * with running sums where the device scans. Every part of the work space lies
 * in a heap block of its own between 16 bytes of 0xAA that must stay.
 * test_rvals_host.py loads it; with -DRVALS_MAIN it is a program that runs
 * corpus files with every input array and every output in a heap block of its
 * own, for a sanitizer to watch. */
#define TGI inline
#include "../dynamicgo_amd/csrc/rvals_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace dg;

/* a part of the work space: `bytes` bytes between two guards */
struct Part {
    uint8_t *raw;
    uint64_t bytes;
    explicit Part(uint64_t b) : raw((uint8_t *)malloc(b + 32)), bytes(b) { memset(raw, 0xAA, b + 32); }
    ~Part() { free(raw); }
    template <class T>
    T *as() { return (T *)(raw + 16); }
    bool intact() const
    {
        for (uint32_t k = 0; k < 16; k++)
            if (raw[k] != 0xAA || raw[16 + bytes + k] != 0xAA) return false;
        return true;
    }
};

/* One batch. route 0: the fixed-stride route where the launch takes it (a plan
 * of scalars, no d_present; no rows), 1: the scanned route whatever the plan is.
 * With `out` the head pass walks the scanned counts with `blocks` blocks of
 * RV_CHUNK cells and the body pass the arena's bytes with `blocks` blocks of
 * VL_CHUNK bytes. Answers 0, or 1 when a guard of the work space broke. */
extern "C" int rvals_run(const uint8_t *kinds, const int16_t *ids, uint32_t K, const dg_val_col *cols, const uint64_t *row_off,
                         uint64_t n, uint64_t n_rows, uint64_t base, uint8_t *out, uint64_t cap, uint64_t *off, uint8_t *status,
                         uint8_t *cell_status, uint32_t blocks, uint32_t route)
{
    RVParams A;
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, K * sizeof *cols);
    memcpy(A.kinds, kinds, K);
    memcpy(A.ids, ids, 2 * K);
    bool scalars = true, all_present = true;
    for (uint32_t k = 0; k < K; k++) scalars &= vl_scalar_kind(kinds[k]), all_present &= !cols[k].d_present;
    A.K = K, A.has_ids = 1, A.fixed = !n_rows || (route == 0 && scalars && all_present);
    A.n = n, A.n_rows = n_rows, A.cells = n_rows * K, A.base = base, A.cap = cap;
    A.row_off = row_off, A.off = off, A.status = status, A.cell_status = cell_status, A.out = out;
    Part len(A.fixed ? 0 : A.cells * 4), pos(A.fixed ? 0 : (A.cells + 1) * 8), mlen(n * 4), mcnt(n * 4), cnt_off((n + 1) * 8);
    A.mlen = mlen.as<uint32_t>(), A.mcnt = mcnt.as<uint32_t>(), A.cnt_off = cnt_off.as<uint64_t>();
    if (A.fixed) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < K; k++) A.pre[k] = (uint8_t)at, at += 3u + tg_fixed(kinds[k]);
        A.stride = at + 1u;
        if (cell_status) memset(cell_status, DG_VAL_OK, A.cells);
    } else {
        A.len = len.as<uint32_t>(), A.pos = pos.as<uint64_t>();
        for (uint64_t q = 0; q < A.cells; q++) rv_size_lane(A, q);
        A.pos[0] = 0;
        for (uint64_t q = 0; q < A.cells; q++) A.pos[q + 1] = A.pos[q] + A.len[q];
    }
    for (uint64_t i = 0; i < n; i++) rv_msg_lane(A, i);
    off[0] = base, A.cnt_off[0] = 0;
    for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + A.mlen[i], A.cnt_off[i + 1] = A.cnt_off[i] + A.mcnt[i];
    if (out && cap > base) {
        for (uint64_t i = 0; i < n; i++) rv_list_head(A, i);
        const uint64_t cells = A.cnt_off[n] * K;
        for (uint32_t b = 0; b < blocks; b++)
            for (uint64_t cb = (uint64_t)b * RV_CHUNK; cb < cells; cb += (uint64_t)blocks * RV_CHUNK) {
                const uint64_t end = cb + RV_CHUNK < cells ? cb + RV_CHUNK : cells;
                const uint64_t lo = cl_find(A.cnt_off, 0, n, cb / K), hi = cl_find(A.cnt_off, 0, n, (end - 1) / K) + 1;
                for (uint64_t t = cb; t < end; t++) rv_head_lane(A, cl_find(A.cnt_off, lo, hi, t / K), t);
            }
        if (!scalars && n_rows) {
            const uint64_t need = off[n], total = need < cap ? need : cap, first = base & ~(uint64_t)(VL_UNIT - 1);
            for (uint32_t b = 0; b < blocks; b++)
                for (uint64_t cb = first + (uint64_t)b * VL_CHUNK; cb < total; cb += (uint64_t)blocks * VL_CHUNK) {
                    const uint64_t end = cb + VL_CHUNK < total ? cb + VL_CHUNK : total;
                    const uint64_t lo = cl_find(A.off, 0, n, cb > base ? cb : base), hi = cl_find(A.off, 0, n, end - 1) + 1;
                    for (uint64_t p = cb; p < end; p += VL_UNIT) rv_granule(A, lo, hi, p, total);
                }
        }
    }
    return len.intact() && pos.intact() && mlen.intact() && mcnt.intact() && cnt_off.intact() ? 0 : 1;
}

#ifdef RVALS_MAIN
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

/* corpus (rvalsgen.corpus_bytes). The emit into a block of exactly need + 16 bytes with cap = need, and again with a cap
 * in the middle into a block of that cap; prints the messages, the cells, the flagged of both, the bytes and a hash of
 * offsets, statuses and bytes. */
int main(int argc, char **argv)
{
    unsigned long long msgs = 0, cells = 0, flagged = 0, cell_flagged = 0, bytes = 0;
    uint64_t h = 0xCBF29CE484222325ull;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t hd[2];
        uint64_t n_rows;
        if (!fh || fread(hd, 4, 2, fh) != 2 || fread(&n_rows, 8, 1, fh) != 1) return 2;
        const uint32_t K = hd[0], n = hd[1];
        uint8_t kinds[16];
        int16_t ids[16];
        if (K > 16 || fread(kinds, 1, K, fh) != K || fread(ids, 2, K, fh) != K) return 2;
        uint64_t *row_off = (uint64_t *)block(fh, (uint64_t)(n + 1) * 8);
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
        const uint64_t nc = n_rows * K;
        uint64_t *off = (uint64_t *)malloc((uint64_t)(n + 1) * 8);
        uint8_t *st = (uint8_t *)malloc(n ? n : 1), *cst = (uint8_t *)malloc(nc ? nc : 1);
        if (rvals_run(kinds, ids, K, cols, row_off, n, n_rows, 0, nullptr, 0, off, st, cst, 1, 0)) return 4;
        const uint64_t need = off[n];
        uint8_t *out = (uint8_t *)malloc(need + 16);
        memset(out, 0xAA, need + 16);
        if (rvals_run(kinds, ids, K, cols, row_off, n, n_rows, 0, out, need, off, st, cst, 3, 0)) return 4;
        const uint64_t half = need / 2;
        uint8_t *cut = (uint8_t *)malloc(half ? half : 1);
        if (rvals_run(kinds, ids, K, cols, row_off, n, n_rows, 0, cut, half, off, st, cst, 2, 1)) return 4;
        if (memcmp(out, cut, half)) return 3;
        for (uint64_t i = 0; i < n; i++) flagged += st[i] != 0;
        for (uint64_t q = 0; q < nc; q++) cell_flagged += cst[q] != 0;
        msgs += n, cells += nc, bytes += need;
        h = fnv(fnv(fnv(fnv(h, off, (uint64_t)(n + 1) * 8), st, n), cst, nc), out, need + 16);
        free(out), free(cut), free(off), free(st), free(cst), free(row_off);
        for (void *p : held) free(p);
    }
    printf("%llu messages, %llu flagged, %llu cells, %llu flagged, %llu bytes, hash %016llx\n", msgs, flagged, cells, cell_flagged,
           bytes, (unsigned long long)h);
    return 0;
}
#endif
