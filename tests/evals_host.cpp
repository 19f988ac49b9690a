/* The entry-column encode (dynamicgo_amd/csrc/evals_device.h) built for the
 * host: the per-lane functions the kernels of evals_kern.hip run (ev_entry_size,
 * ev_pair_cell, ev_head, ev_emit over cl_find), driven entry by entry and cell by
 * cell in the kernels' order, with running sums where the device scans.
 * test_evals_host.py loads it; with -DEVALS_MAIN it is a program that runs
 * corpus files with every input array and every output in a heap block of its
 * own, for a sanitizer to watch. */
#define TGI inline
#include "../dynamicgo_amd/csrc/evals_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace dg;

/* One batch: the entry sizes and positions of every variable-stride column (in
 * blocks of exactly n_ent and n_ent + 1 entries), the cells, the offsets, then
 * with `out` the heads and the emit chunk by chunk as evals_emit_kernel walks
 * the scanned counts with `blocks` blocks. */
extern "C" int evals_run(const uint16_t *kinds, const int16_t *ids, uint32_t K, const dg_eval_col *cols, uint64_t n,
                         uint64_t base, uint8_t *out, uint64_t cap, uint64_t *off, uint8_t *status, uint32_t blocks)
{
    EVParams A;
    memset(&A, 0, sizeof A);
    memcpy(A.col, cols, K * sizeof *cols);
    memcpy(A.kinds, kinds, 2 * K);
    if (ids) memcpy(A.ids, ids, 2 * K);
    A.K = K, A.has_ids = ids != nullptr, A.pairs = n * K, A.base = base, A.cap = cap, A.off = off, A.out = out;
    std::vector<uint64_t *> held;
    for (uint32_t k = 0; k < K; k++) {
        const dg_eval_col &c = cols[k];
        if (ev_stride(kinds[k]) || !c.n_ent) continue;
        const uint32_t kt = ev_kt(kinds[k]), vt = ev_vt(kinds[k]);
        uint64_t *pos = (uint64_t *)malloc((c.n_ent + 1) * 8);
        pos[0] = 0;
        for (uint64_t g = 0; g < c.n_ent; g++)
            pos[g + 1] = pos[g] + ev_entry_size(kt, vt, kt == TT_STRING ? c.d_key_len[g] : 0u, vt == TT_STRING ? c.d_val_len[g] : 0u);
        A.pos[k] = pos, held.push_back(pos);
    }
    std::vector<uint32_t> cnt(A.pairs ? A.pairs : 1);
    std::vector<uint64_t> cnt_off(A.pairs + 1);
    A.cnt = cnt.data(), A.cnt_off = cnt_off.data();
    uint64_t pos = base, ents = 0;
    for (uint64_t q = 0; q < A.pairs; q++) {
        const EVCell z = ev_pair_cell(A, ev_pair(A, q));
        if (status) status[q] = (uint8_t)z.status;
        off[q] = pos, cnt[q] = z.cnt, cnt_off[q] = ents;
        pos += z.len, ents += z.cnt;
    }
    off[A.pairs] = pos, cnt_off[A.pairs] = ents;
    if (out && cap > base) {
        for (uint64_t q = 0; q < A.pairs; q++) {
            const EVPair p = ev_pair(A, q);
            ev_head(p.kind, p.id, p.fh, p.stop, (uint32_t)(off[q + 1] - off[q]), cnt[q], out, off[q], cap);
        }
        for (uint32_t b = 0; b < blocks; b++)
            for (uint64_t cb = (uint64_t)b * EV_CHUNK; cb < ents; cb += (uint64_t)blocks * EV_CHUNK) {
                const uint64_t end = cb + EV_CHUNK < ents ? cb + EV_CHUNK : ents;
                const uint64_t lo = cl_find(A.cnt_off, 0, A.pairs, cb), hi = cl_find(A.cnt_off, 0, A.pairs, end - 1) + 1;
                for (uint64_t t = cb; t < end; t++) ev_emit(A, cl_find(A.cnt_off, lo, hi, t), t);
            }
    }
    for (uint64_t *p : held) free(p);
    return 0;
}

extern "C" int evals_kind_ok(uint32_t kind) { return ev_kind_ok(kind); }
extern "C" uint32_t evals_wire(uint32_t kind) { return ev_wire(kind); }
extern "C" uint32_t evals_entry_size(uint32_t kt, uint32_t vt, uint32_t klen, uint32_t vlen) { return ev_entry_size(kt, vt, klen, vlen); }

#ifdef EVALS_MAIN
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

/* corpus (evalsgen.corpus_bytes). The emit into a block of exactly need + 16 bytes with cap = need, and again with a cap
 * in the middle into a block of that cap; prints the cells, the flagged cells, the bytes and a hash of offsets,
 * statuses and bytes. */
int main(int argc, char **argv)
{
    unsigned long long cells = 0, flagged = 0, bytes = 0;
    uint64_t h = 0xCBF29CE484222325ull;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t hd[3];
        if (!fh || fread(hd, 4, 3, fh) != 3) return 2;
        const uint32_t K = hd[0], n = hd[1];
        uint16_t kinds[16];
        int16_t ids[16];
        if (K > 16 || fread(kinds, 2, K, fh) != K || fread(ids, 2, K, fh) != K) return 2;
        dg_eval_col cols[16];
        std::vector<void *> held;
        for (uint32_t k = 0; k < K; k++) {
            uint64_t len[9];
            if (fread(len, 8, 9, fh) != 9) return 2;
            const uint32_t width[8] = {8, 8, 4, 8, 4, 1, 1, 1};
            void *p[8];
            for (int a = 0; a < 8; a++) p[a] = len[a + 1] ? block(fh, len[a + 1] * width[a]) : nullptr, held.push_back(p[a]);
            cols[k] = dg_eval_col{(const uint64_t *)p[0], (const uint64_t *)p[1], (const uint32_t *)p[2], (const uint64_t *)p[3],
                                  (const uint32_t *)p[4], (const uint8_t *)p[5], (const uint8_t *)p[6], (const uint8_t *)p[7],
                                  len[0]};
        }
        fclose(fh);
        const uint64_t pairs = (uint64_t)n * K;
        uint64_t *off = (uint64_t *)malloc((pairs + 1) * 8);
        uint8_t *st = (uint8_t *)malloc(pairs ? pairs : 1);
        evals_run(kinds, hd[2] ? ids : nullptr, K, cols, n, 0, nullptr, 0, off, st, 1);
        const uint64_t need = off[pairs];
        uint8_t *out = (uint8_t *)malloc(need + 16);
        memset(out, 0xAA, need + 16);
        evals_run(kinds, hd[2] ? ids : nullptr, K, cols, n, 0, out, need, off, st, 3);
        const uint64_t half = need / 2;
        uint8_t *cut = (uint8_t *)malloc(half ? half : 1);
        evals_run(kinds, hd[2] ? ids : nullptr, K, cols, n, 0, cut, half, off, st, 2);
        if (memcmp(out, cut, half)) return 3;
        for (uint64_t q = 0; q < pairs; q++) flagged += st[q] != 0;
        cells += pairs, bytes += need;
        h = fnv(fnv(fnv(h, off, (pairs + 1) * 8), st, pairs), out, need + 16);
        free(out), free(cut), free(off), free(st);
        for (void *p : held) free(p);
    }
    printf("%llu cells, %llu flagged, %llu bytes, hash %016llx\n", cells, flagged, bytes, (unsigned long long)h);
    return 0;
}
#endif
