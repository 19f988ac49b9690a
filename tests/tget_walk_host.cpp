/* The path-lookup walk (dynamicgo_amd/csrc/tget_device.h) built for the host:
 * tg_walk with 8 frames, then with 1024 where that ends TG_ST_DEEP, as the two
 * kernels do. test_tget_walk_host.py loads it; with -DWALK_MAIN it is a program
 * that runs a corpus file with every message and the blob in a heap block of
 * their own, len + 16 bytes, for a sanitizer to watch the reads. */
#define TGI inline
#include "../dynamicgo_amd/csrc/tget_device.h"
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

extern "C" int walk(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t off_steps, uint32_t off_pool,
                    uint32_t path, uint32_t root_type, uint32_t *out)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    dg::TGParams A = {};
    A.blob = blob, A.off_steps = off_steps, A.off_pool = off_pool, A.root_type = root_type;
    dg::TGRes r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    const int deep = r.status == dg::TG_ST_DEEP;
    if (deep) r = dg::tg_walk(A, msg, len, path, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
    const uint32_t v[6] = {r.start, r.end, r.type, r.status, r.step, r.aux};
    memcpy(out, v, sizeof v);
    return deep;
}

#ifdef WALK_MAIN
/* corpus: u32 n_msgs, n_paths, root_type, off_steps, off_pool, blob_len; the blob; per message u32 len, bytes */
int main(int argc, char **argv)
{
    unsigned long pairs = 0, deep = 0, by[256] = {};
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[6], len;
        if (!fh || fread(h, 4, 6, fh) != 6) return 2;
        uint8_t *blob = (uint8_t *)malloc(h[5] + 16);
        if (fread(blob, 1, h[5], fh) != h[5]) return 2;
        memset(blob + h[5], 0, 16);
        for (uint32_t i = 0; i < h[0]; i++) {
            if (fread(&len, 4, 1, fh) != 1) return 2;
            uint8_t *m = (uint8_t *)malloc(len + 16);
            if (fread(m, 1, len, fh) != len) return 2;
            memset(m + len, 0xAA, 16);
            for (uint32_t k = 0; k < h[1]; k++, pairs++) {
                uint32_t out[6];
                deep += walk(m, len, blob, h[3], h[4], k, h[2], out);
                by[out[3] & 255]++;
            }
            free(m);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu pairs, %lu deep; OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu\n", pairs, deep, by[0], by[1], by[2],
           by[3]);
    return 0;
}
#endif
