/* The many-edit's combine and splice (dynamicgo_amd/csrc/editm_device.h) built
 * for the host, behind the lookup's walk (tget_device.h) as the launch sequence
 * runs them: tg_walk on {parent, full_1 .. full_K} with 8 frames, then 1024 where
 * that ends TG_ST_DEEP, then editm_message. route 0 is the lane route with one
 * lane a message, route 1 the wave route, run once per lane 0..63 into the same
 * output, each lane writing its share; routes 2 and 3 are the lane route with 4
 * and 16 lanes a message, run the same way. test_editm_host.py loads it; with
 * -DEDITM_MAIN it is a program that runs corpus files with every message, value,
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

template <uint32_t KT>
static void run_routes(const dg::EmParams &A0, int route)
{
    dg::EmParams A = A0;
    if (route == 1) {
        A.wave_min = 0;
        for (uint32_t lane = 0; lane < 64; lane++) dg::editm_message<KT, 64, true>(A, 0, lane);
        return;
    }
    A.wave_min = ~0ull;
    if (route == 0) dg::editm_message<KT, 1, false>(A, 0, 0);
    else if (route == 2)
        for (uint32_t lane = 0; lane < 4; lane++) dg::editm_message<KT, 4, false>(A, 0, lane);
    else
        for (uint32_t lane = 0; lane < 16; lane++) dg::editm_message<KT, 16, false>(A, 0, lane);
}

/* blob: a path set of K + 1 paths, parent and the K full paths
 * (generic.compile_paths), with 16 zero bytes after it. vals[j] / vlens[j]: item
 * j's value, each readable 16 bytes past its end. *ret and *out_len as the
 * kernels store them. */
extern "C" void editm_msg(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t op, uint32_t root_type,
                          const uint32_t *val_types, const uint8_t *const *vals, const uint64_t *vlens, int route,
                          uint8_t *out, uint64_t cap, uint64_t *ret, uint32_t *out_len)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    dg_path_hdr h;
    memcpy(&h, blob, sizeof h);
    const uint32_t K = h.n_paths - 1;
    dg::TGParams T = {};
    T.blob = blob, T.off_steps = h.off_steps, T.off_pool = h.off_pool, T.root_type = root_type;
    alignas(16) dg_tget_rec rec[dg::EM_MAX + 1];
    for (uint32_t k = 0; k <= K; k++) {
        dg::TGRes r = dg::tg_walk(T, msg, len, k, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
        if (r.status == dg::TG_ST_DEEP) r = dg::tg_walk(T, msg, len, k, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
        rec[k] = dg_tget_rec{r.start, r.end, (uint8_t)r.type, (uint8_t)r.status, (uint16_t)r.step, r.aux};
    }
    /* every value in a block of its own: the "arena" starts at the lowest of them, val_pos counts from there */
    uintptr_t base = (uintptr_t)vals[0];
    for (uint32_t j = 1; j < K; j++) base = (uintptr_t)vals[j] < base ? (uintptr_t)vals[j] : base;
    const uint64_t in_off[2] = {0, len}, out_off[2] = {0, cap};
    dg::EmParams A = {};
    A.op = op, A.K = K;
    for (uint32_t j = 0; j < K; j++) {
        dg_path_ent pe;
        memcpy(&pe, blob + sizeof h + (j + 1) * sizeof pe, sizeof pe);
        dg_path_step last;
        memcpy(&last, blob + h.off_steps + (uint64_t)(pe.first + pe.count - 1) * sizeof last, sizeof last);
        const bool pooled = last.kind == DG_PS_STRKEY || last.kind == DG_PS_BINKEY;
        A.n_steps = pe.count;
        A.it[j].kind = last.kind, A.it[j].key_len = last.key_len, A.it[j].kval = last.val;
        A.it[j].val_type = val_types[j];
        A.it[j].key_off = h.off_pool + (pooled ? (uint32_t)last.val : 0u);
        A.it[j].val_pos = (uintptr_t)vals[j] - base, A.it[j].val_len = vlens[j];
    }
    A.pool = blob;
    A.src = msg, A.in_off = in_off, A.n = 1, A.rec = rec;
    A.val = (const uint8_t *)base, A.val_off = nullptr;
    A.out = out, A.out_off = out_off, A.out_len = out_len, A.ret = ret;
    switch (K) {
        case 1: run_routes<1>(A, route); break;
        case 2: run_routes<2>(A, route); break;
        case 3: run_routes<3>(A, route); break;
        case 4: run_routes<4>(A, route); break;
        case 5: run_routes<5>(A, route); break;
        case 6: run_routes<6>(A, route); break;
        case 7: run_routes<7>(A, route); break;
        default: *ret = ~0ull, *out_len = 0;
    }
}

#ifdef EDITM_MAIN
/* corpus: u32 n_msgs, op, root_type, K, blob_len; u32 val_types[K]; the blob; per message u32 len, cap, vlen[K],
 * the message, the K values */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, existed = 0, bytes = 0, by[256] = {};
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[5], vt[dg::EM_MAX], lc[2 + dg::EM_MAX];
        if (!fh || fread(h, 4, 5, fh) != 5 || h[3] < 1 || h[3] > dg::EM_MAX) return 2;
        const uint32_t K = h[3];
        if (fread(vt, 4, K, fh) != K) return 2;
        uint8_t *blob = (uint8_t *)malloc(h[4] + 16);
        if (fread(blob, 1, h[4], fh) != h[4]) return 2;
        memset(blob + h[4], 0, 16);
        for (uint32_t i = 0; i < h[0]; i++, msgs++) {
            if (fread(lc, 4, 2 + K, fh) != 2 + K) return 2;
            uint8_t *m = (uint8_t *)malloc(lc[0] + 16), *v[dg::EM_MAX];
            uint64_t vl[dg::EM_MAX];
            if (fread(m, 1, lc[0], fh) != lc[0]) return 2;
            memset(m + lc[0], 0xAA, 16);
            for (uint32_t j = 0; j < K; j++) {
                vl[j] = lc[2 + j];
                v[j] = (uint8_t *)malloc(vl[j] + 16);
                if (fread(v[j], 1, vl[j], fh) != vl[j]) return 2;
                memset(v[j] + vl[j], 0xBB, 16);
            }
            uint8_t *o[4];
            uint64_t ret[4];
            uint32_t ol[4];
            for (int route = 0; route < 4; route++) {
                o[route] = (uint8_t *)malloc(lc[1] ? lc[1] : 1);
                editm_msg(m, lc[0], blob, h[1], h[2], vt, v, vl, route, o[route], lc[1], &ret[route], &ol[route]);
            }
            for (int route = 1; route < 4; route++)
                if (ret[0] != ret[route] || ol[0] != ol[route] || ((ret[0] & 0xFF) == 0 && memcmp(o[0], o[route], ol[0]))) {
                    fprintf(stderr, "file %d message %u: route %d differs from route 0\n", f, i, route);
                    return 3;
                }
            by[ret[0] & 255]++;
            if ((ret[0] & 0xFF) == 0) bytes += ol[0], existed += __builtin_popcountll((ret[0] >> 8) & 0x7F);
            for (int route = 0; route < 4; route++) free(o[route]);
            for (uint32_t j = 0; j < K; j++) free(v[j]);
            free(m);
        }
        free(blob);
        fclose(fh);
    }
    printf("%lu messages; OK %lu (existed %lu), NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_SAME %lu, E_OVERFLOW %lu; %lu bytes\n",
           msgs, by[0], existed, by[1], by[2], by[3], by[5], by[0xF0], bytes);
    return 0;
}
#endif
