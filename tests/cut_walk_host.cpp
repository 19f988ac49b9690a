/* The cut walk and both copy engines (dynamicgo_amd/csrc/cut_device.h) built
 * for the host. route 0 is the lane route: cut_walk with 8 cut frames, 8 skip
 * frames and the lane sink, and where that declines (or the message is at
 * least wave_min long) the wave route, as the kernels do; route 1 is the wave
 * route alone: 64 cut frames, 1024 skip frames and the wave sink, run once per
 * lane 0..63 into the same output, each lane writing its share.
 * test_cut_host.py loads it; with -DWALK_MAIN it is a program that runs a
 * corpus file with every message, every slot and the blob in a heap block of
 * their own (len + 16, cap, len + 16 bytes) for a sanitizer to watch. */
#define TGI inline
#define CUTI inline
#include "../dynamicgo_amd/csrc/cut_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <uint32_t CAP>
struct HostCutFrames {
    static constexpr uint32_t cap = CAP;
    uint64_t *m, *k;
    uint64_t &meta(uint32_t l) const { return m[l]; }
    uint64_t &mask(uint32_t l) const { return k[l]; }
};
template <uint32_t CAP>
struct HostSkipFrames {
    static constexpr uint32_t cap = CAP;
    uint64_t *base;
    uint64_t &at(uint32_t l) const { return base[l]; }
};

static dg::CutPlanView view(const uint8_t *blob)
{
    dg_cut_hdr h;
    memcpy(&h, blob, sizeof h);
    return dg::CutPlanView{(const dg_cut_node *)(const void *)(blob + h.off_nodes),
                           (const dg_cut_field *)(const void *)(blob + h.off_fields),
                           (const dg_cut_lit *)(const void *)(blob + h.off_lits), blob + h.off_pool, h.root};
}

/* returns 1 when the lane route declined the message; *ret and *out_len as the kernels store them */
extern "C" int cut_msg(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint64_t opts, int route, uint64_t wave_min,
                       uint8_t *out, uint64_t cap, uint64_t *ret, uint32_t *out_len)
{
    /* garbage a frame must not inherit */
    std::vector<uint64_t> m(DG_CUT_MAX_DEPTH, 0xA5A5A5A5A5A5A5A5ull), k(DG_CUT_MAX_DEPTH, 0x5A5A5A5A5A5A5A5Aull),
        sf(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull);
    const dg::CutPlanView P = view(blob);
    dg::CutParams A = {};
    A.out_len = out_len, A.ret = ret;
    int declined = 0;
    if (route == 0) {
        dg::CutRes r{dg::CUT_ST_DEEP, 0};
        dg::CutLaneSink sk{out, cap, 0, false};
        if (len < wave_min)
            r = dg::cut_walk(P, opts, msg, len, HostCutFrames<dg::CUT_LDS_DEPTH>{m.data(), k.data()},
                             HostSkipFrames<dg::TG_LDS_DEPTH>{sf.data()}, sk);
        if (r.status != dg::CUT_ST_DEEP && r.status != dg::CUT_ST_SKIPDEEP) {
            dg::cut_store(A, 0, r, sk.o, sk.ovf);
            return 0;
        }
        declined = 1;
    }
    for (uint32_t lane = 0; lane < 64; lane++) {
        dg::CutWaveSink sk{out, cap, 0, false, lane};
        dg::CutRes r = dg::cut_walk(P, opts, msg, len, HostCutFrames<DG_CUT_MAX_DEPTH>{m.data(), k.data()},
                                    HostSkipFrames<dg::TG_DEEP_DEPTH>{sf.data()}, sk);
        if (r.status == dg::CUT_ST_DEEP) r = dg::CutRes{DG_CUT_E_DEPTH, 0};
        if (r.status == dg::CUT_ST_SKIPDEEP) r = dg::CutRes{DG_CUT_E_READ, 0};
        if (lane == 0) dg::cut_store(A, 0, r, sk.o, sk.ovf);
    }
    return declined;
}

#ifdef WALK_MAIN
/* corpus: u32 n_msgs, opts, blob_len; the blob; per message u32 len, cap, then the bytes */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, declined = 0, bytes = 0, by[256] = {};
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[3], lc[2];
        if (!fh || fread(h, 4, 3, fh) != 3) return 2;
        uint8_t *blob = (uint8_t *)malloc(h[2] + 16);
        if (fread(blob, 1, h[2], fh) != h[2]) return 2;
        memset(blob + h[2], 0, 16);
        for (uint32_t i = 0; i < h[0]; i++, msgs++) {
            if (fread(lc, 4, 2, fh) != 2) return 2;
            uint8_t *m = (uint8_t *)malloc(lc[0] + 16);
            if (fread(m, 1, lc[0], fh) != lc[0]) return 2;
            memset(m + lc[0], 0xAA, 16);
            uint8_t *o[2];
            uint64_t ret[2];
            uint32_t ol[2];
            for (int route = 0; route < 2; route++) {
                o[route] = (uint8_t *)malloc(lc[1] ? lc[1] : 1);
                const int d = cut_msg(m, lc[0], blob, h[1], route, 1u << 20, o[route], lc[1], &ret[route], &ol[route]);
                if (route == 0) declined += d;
            }
            if (ret[0] != ret[1] || ol[0] != ol[1] || (ret[0] == 0 && memcmp(o[0], o[1], ol[0]))) {
                fprintf(stderr, "message %u: the routes differ\n", i);
                return 3;
            }
            by[ret[0] & 255]++;
            if (ret[0] == 0) bytes += ol[0];
            free(o[0]), free(o[1]), free(m);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu messages, %lu declined; OK %lu, E_READ %lu, E_TYPE %lu, E_UNKNOWN %lu, E_REQUIRED %lu, E_DEPTH %lu, "
           "E_OVERFLOW %lu; %lu bytes\n",
           msgs, declined, by[0], by[1], by[2], by[3], by[4], by[5], by[0xF0], bytes);
    return 0;
}
#endif
