/* The entry-column decode (dynamicgo_amd/csrc/ents_device.h) built for the host:
 * tg_walk with 8 frames, then with 1024 where that ends TG_ST_DEEP, then
 * en_cell, as the two kernels of the cell pass do; en_fixed for the entries of
 * a fixed-stride cell and en_next for the walk of a variable-stride one, as the
 * emit kernels do. test_ents_host.py loads it; with -DENTS_MAIN it is a
 * program that runs corpus files with every message, the blob and every
 * output in a heap block of their own (a message: len + 16 bytes), for a
 * sanitizer to watch the reads and the stores. */
#define TGI inline
#include "../dynamicgo_amd/csrc/ents_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <uint32_t CAP>
struct HostFrames {
    static constexpr uint32_t cap = CAP;
    uint64_t *base;
    uint64_t &at(uint32_t l) const { return base[l]; }
};

/* out: status, type, step, aux, len, span, the value's low and high word; returns whether the pair needed the 1024
 * frames */
extern "C" int cell(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t off_steps, uint32_t off_pool,
                    uint32_t path, uint32_t root_type, uint32_t kind, uint64_t base, uint32_t *out)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    dg::TGParams A = {};
    A.blob = blob, A.off_steps = off_steps, A.off_pool = off_pool, A.root_type = root_type;
    dg::TGRes r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    const int deep = r.status == dg::TG_ST_DEEP;
    if (deep) r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
    const dg::ENCell c = dg::en_cell(kind, r, msg, base);
    const uint64_t w = dg::cl_cell_word(c.c); /* the stored form, taken apart again */
    const uint32_t v[8] = {(uint32_t)(w & 0xFF), (uint32_t)(w >> 8 & 0xFF), (uint32_t)(w >> 16 & 0xFFFF), (uint32_t)(w >> 32),
                           c.c.len,              c.span,                    (uint32_t)c.c.val,            (uint32_t)(c.c.val >> 32)};
    memcpy(out, v, sizeof v);
    return deep;
}

/* the entries of an OK cell (val, count, span and aux as `cell` gave them, val relative to src) into four arrays of
 * `count` slots, by the route its kind takes on the device; returns how many were stored */
extern "C" uint32_t emit(const uint8_t *src, uint64_t val, uint32_t count, uint32_t span, uint32_t aux, uint32_t kind,
                         uint64_t *key, uint32_t *klen, uint64_t *v, uint32_t *vlen)
{
    const uint32_t kt = aux & 0xFF, vt = aux >> 8 & 0xFF;
    uint32_t j = 0;
    if ((kind & DG_ENT_INTMAP) && (kind & 15u) != DG_ENT_STR) {
        for (; j < count && (uint64_t)(j + 1) * (dg::tg_fixed(kt) + dg::tg_fixed(vt)) <= span; j++) {
            const dg::ENEntry e = dg::en_fixed(src, val, kind & 15u, kt, vt, j);
            key[j] = e.key, klen[j] = e.klen, v[j] = e.val, vlen[j] = e.vlen;
        }
        return j;
    }
    uint64_t p = val;
    for (; j < count; j++) {
        dg::ENEntry e;
        if (!dg::en_next(src, p, val + span, kind, kt, vt, e)) break;
        key[j] = e.key, klen[j] = e.klen, v[j] = e.val, vlen[j] = e.vlen;
    }
    return j;
}

#ifdef ENTS_MAIN
/* corpus: u32 n_msgs, n_cols, root_type, off_steps, off_pool, blob_len; 8 kind bytes; the blob; per message u32 len,
 * bytes. Prints the status counts, the entries of all OK cells and the sum of their keys, values and lengths (string
 * keys and values count as their offset from the cell's value). */
int main(int argc, char **argv)
{
    unsigned long cells = 0, deep = 0, by[256] = {}, ents = 0;
    uint64_t sum = 0;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[6], len;
        uint8_t kinds[8];
        if (!fh || fread(h, 4, 6, fh) != 6 || fread(kinds, 1, 8, fh) != 8) return 2;
        uint8_t *blob = (uint8_t *)malloc(h[5] + 16);
        if (fread(blob, 1, h[5], fh) != h[5]) return 2;
        memset(blob + h[5], 0, 16);
        for (uint32_t i = 0; i < h[0]; i++) {
            if (fread(&len, 4, 1, fh) != 1) return 2;
            uint8_t *m = (uint8_t *)malloc(len + 16);
            if (fread(m, 1, len, fh) != len) return 2;
            memset(m + len, 0xAA, 16);
            for (uint32_t k = 0; k < h[1]; k++, cells++) {
                uint32_t out[8];
                deep += cell(m, len, blob, h[3], h[4], k, h[2], kinds[k], 0, out);
                by[out[0] & 255]++;
                if (out[0] != DG_TGET_OK || !out[4]) continue;
                const uint32_t cnt = out[4];
                const uint64_t val = out[6] | (uint64_t)out[7] << 32;
                uint64_t *key = (uint64_t *)malloc(cnt * 8), *v = (uint64_t *)malloc(cnt * 8);
                uint32_t *klen = (uint32_t *)malloc(cnt * 4), *vlen = (uint32_t *)malloc(cnt * 4);
                const uint32_t got = emit(m, val, cnt, out[5], out[3], kinds[k], key, klen, v, vlen);
                const bool sk = kinds[k] & DG_ENT_STRMAP, sv = kinds[k] == DG_ENT_LISTSTR || (kinds[k] & 15) == DG_ENT_STR;
                for (uint32_t j = 0; j < got; j++, ents++)
                    sum += (key[j] - (sk ? val : 0)) + klen[j] + (v[j] - (sv ? val : 0)) + vlen[j];
                free(key), free(v), free(klen), free(vlen);
            }
            free(m);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu cells, %lu deep; OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu; %lu entries, sum %llu\n",
           cells, deep, by[0], by[1], by[2], by[3], by[4], ents, (unsigned long long)sum);
    return 0;
}
#endif
