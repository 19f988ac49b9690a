/* The typed-column decode (dynamicgo_amd/csrc/cols_device.h) built for the host:
 * tg_walk with 8 frames, then with 1024 where that ends TG_ST_DEEP, then cl_cell,
 * as the two kernels do, and cl_elem for a list cell's elements.
 * test_cols_host.py loads it; with -DCOLS_MAIN it is a program that runs a
 * corpus file with every message and the blob in a heap block of their own,
 * len + 16 bytes, for a sanitizer to watch the reads. */
#define TGI inline
#include "../dynamicgo_amd/csrc/cols_device.h"
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

/* out: status, type, step, aux, len, the value's low and high word; returns whether the pair needed the 1024 frames */
extern "C" int cell(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t off_steps, uint32_t off_pool,
                    uint32_t path, uint32_t root_type, uint32_t kind, uint64_t base, uint32_t *out)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    dg::TGParams A = {};
    A.blob = blob, A.off_steps = off_steps, A.off_pool = off_pool, A.root_type = root_type;
    dg::TGRes r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    const int deep = r.status == dg::TG_ST_DEEP;
    if (deep) r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
    const dg::CLCell c = dg::cl_cell(kind, r, msg, base);
    const uint64_t w = dg::cl_cell_word(c); /* the stored form, taken apart again */
    const uint32_t v[7] = {(uint32_t)(w & 0xFF),   (uint32_t)(w >> 8 & 0xFF), (uint32_t)(w >> 16 & 0xFFFF), (uint32_t)(w >> 32),
                           c.len,                  (uint32_t)c.val,           (uint32_t)(c.val >> 32)};
    memcpy(out, v, sizeof v);
    return deep;
}

/* element j of an OK list cell: the list's first element at src + val */
extern "C" uint64_t elem(const uint8_t *src, uint64_t val, uint32_t et, uint64_t j) { return dg::cl_elem(src, val, et, j); }

extern "C" uint64_t find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t g) { return dg::cl_find(off, lo, hi, g); }

#ifdef COLS_MAIN
/* corpus: u32 n_msgs, n_cols, root_type, off_steps, off_pool, blob_len; 8 kind bytes; the blob; per message u32 len,
 * bytes. Prints the status counts, the elements of all OK list cells and the sum of all values and elements. */
int main(int argc, char **argv)
{
    unsigned long cells = 0, deep = 0, by[256] = {}, elems = 0;
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
                uint32_t out[7];
                deep += cell(m, len, blob, h[3], h[4], k, h[2], kinds[k], 0, out);
                by[out[0] & 255]++;
                const uint64_t val = out[5] | (uint64_t)out[6] << 32;
                if ((kinds[k] & DG_COL_LIST) && out[0] == DG_TGET_OK) {
                    for (uint32_t j = 0; j < out[4]; j++, elems++) sum += elem(m, val, out[1], j);
                } else if (kinds[k] != DG_COL_STR) {
                    sum += val;
                }
            }
            free(m);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu cells, %lu deep; OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu; %lu elements, sum %llu\n",
           cells, deep, by[0], by[1], by[2], by[3], by[4], elems, (unsigned long long)sum);
    return 0;
}
#endif
