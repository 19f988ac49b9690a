/* The edit's decision function (dynamicgo_amd/csrc/edit_device.h) and the
 * many-edit's splice with one item (editm_device.h), as dg_edit_* runs them,
 * built for the host, behind the lookup's walk (tget_device.h) as the launch
 * sequence runs them: tg_walk on (parent, full) with 8 frames, then 1024 where
 * that ends TG_ST_DEEP, then editm_message<1>. route 0 is the lane route (one lane
 * writes everything), route 1 the wave route, run once per lane 0..63 into the
 * same output, each lane writing its share; routes 2 and 3 are the lane route
 * with 4 and 16 lanes a message, run the same way. test_edit_host.py loads it; with
 * -DEDIT_MAIN it is a program that runs corpus files with every message, value,
 * slot and the blob in a heap block of their own (len + 16, vlen + 16, cap,
 * len + 16 bytes) for a sanitizer to watch. */
#define TGI inline
#define EDI inline
#include "../dynamicgo_amd/csrc/editm_device.h"
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

/* blob: a path set of two paths, parent and full (generic.compile_paths), with
 * 16 zero bytes after it. *ret and *out_len as the kernels store them. */
extern "C" void edit_msg(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t op, uint32_t root_type,
                         uint32_t val_type, const uint8_t *val, uint64_t vlen, int route, uint8_t *out, uint64_t cap,
                         uint64_t *ret, uint32_t *out_len)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    dg_path_hdr h;
    memcpy(&h, blob, sizeof h);
    dg::TGParams T = {};
    T.blob = blob, T.off_steps = h.off_steps, T.off_pool = h.off_pool, T.root_type = root_type;
    alignas(16) dg_tget_rec rec[2];
    for (uint32_t k = 0; k < 2; k++) {
        dg::TGRes r = dg::tg_walk(T, msg, len, k, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
        if (r.status == dg::TG_ST_DEEP) r = dg::tg_walk(T, msg, len, k, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
        rec[k] = dg_tget_rec{r.start, r.end, (uint8_t)r.type, (uint8_t)r.status, (uint16_t)r.step, r.aux};
    }
    dg_path_ent pe;
    memcpy(&pe, blob + sizeof h + sizeof pe, sizeof pe);
    dg_path_step last;
    memcpy(&last, blob + h.off_steps + (uint64_t)(pe.first + pe.count - 1) * sizeof last, sizeof last);
    const bool pooled = last.kind == DG_PS_STRKEY || last.kind == DG_PS_BINKEY;
    const uint64_t in_off[2] = {0, len}, out_off[2] = {0, cap};
    dg::EmParams A = {};
    A.op = op, A.n_steps = pe.count, A.K = 1;
    A.it[0] = dg::EmItem{last.kind, last.key_len, last.val, val_type, h.off_pool + (pooled ? (uint32_t)last.val : 0u), 0, vlen};
    A.pool = blob;
    A.src = msg, A.in_off = in_off, A.n = 1, A.rec = rec;
    A.val = val;
    A.out = out, A.out_off = out_off, A.out_len = out_len, A.ret = ret;
    if (route == 1) {
        A.wave_min = 0;
        for (uint32_t lane = 0; lane < 64; lane++) dg::editm_message<1, 64, true>(A, 0, lane);
        return;
    }
    A.wave_min = ~0ull;
    if (route == 0) dg::editm_message<1, 1, false>(A, 0, 0);
    else if (route == 2)
        for (uint32_t lane = 0; lane < 4; lane++) dg::editm_message<1, 4, false>(A, 0, lane);
    else
        for (uint32_t lane = 0; lane < 16; lane++) dg::editm_message<1, 16, false>(A, 0, lane);
}

#ifdef EDIT_MAIN
/* corpus: u32 n_msgs, op, root_type, val_type, blob_len; the blob; per message u32 len, cap, vlen, the message, the value */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, existed = 0, bytes = 0, by[256] = {};
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[5], lc[3];
        if (!fh || fread(h, 4, 5, fh) != 5) return 2;
        uint8_t *blob = (uint8_t *)malloc(h[4] + 16);
        if (fread(blob, 1, h[4], fh) != h[4]) return 2;
        memset(blob + h[4], 0, 16);
        for (uint32_t i = 0; i < h[0]; i++, msgs++) {
            if (fread(lc, 4, 3, fh) != 3) return 2;
            uint8_t *m = (uint8_t *)malloc(lc[0] + 16), *v = (uint8_t *)malloc(lc[2] + 16);
            if (fread(m, 1, lc[0], fh) != lc[0] || fread(v, 1, lc[2], fh) != lc[2]) return 2;
            memset(m + lc[0], 0xAA, 16);
            memset(v + lc[2], 0xBB, 16);
            uint8_t *o[4];
            uint64_t ret[4];
            uint32_t ol[4];
            for (int route = 0; route < 4; route++) {
                o[route] = (uint8_t *)malloc(lc[1] ? lc[1] : 1);
                edit_msg(m, lc[0], blob, h[1], h[2], h[3], v, lc[2], route, o[route], lc[1], &ret[route], &ol[route]);
            }
            for (int route = 1; route < 4; route++)
                if (ret[0] != ret[route] || ol[0] != ol[route] || ((ret[0] & 0xFF) == 0 && memcmp(o[0], o[route], ol[0]))) {
                    fprintf(stderr, "file %d message %u: route %d differs from route 0\n", f, i, route);
                    return 3;
                }
            by[ret[0] & 255]++;
            if ((ret[0] & 0xFF) == 0) bytes += ol[0], existed += (ret[0] >> 8) & 1;
            free(o[0]), free(o[1]), free(o[2]), free(o[3]), free(m), free(v);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu messages; OK %lu (existed %lu), NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_OVERFLOW %lu; %lu bytes\n", msgs,
           by[0], existed, by[1], by[2], by[3], by[0xF0], bytes);
    return 0;
}
#endif
