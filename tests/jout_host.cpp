/* The lane writers built for the host: Out (dynamicgo_amd/csrc/j2t_device.h)
 * and JOut (t2j_device.h), driven by an op list. test_jout_host.py loads it
 * and compares with a byte-at-a-time model; with -DJOUT_MAIN it is a program
 * that runs seeded op lists against the same model, every buffer a heap block
 * of exactly guard + cap + guard bytes, for a sanitizer to watch the stores.
 *
 * Built as HIP (-x hip): every __device__ function of the headers is made
 * __host__ __device__ here, so the host pass compiles the writers as they
 * stand; the headers are not edited. */
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../dynamicgo_amd/csrc/t2j_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { OP_WLE = 0, OP_W8 = 1, OP_SET_LEN = 2, OP_FINISH = 3 };

template <class W>
static uint64_t run_ops(uint8_t *base, uint64_t cap, const uint64_t *ops, uint32_t nops)
{
    W o;
    o.init(base, cap);
    for (uint32_t k = 0; k < nops; k++) {
        const uint64_t op = ops[3 * k], a = ops[3 * k + 1], v = ops[3 * k + 2];
        switch (op) {
        case OP_WLE: o.wle(v, (uint32_t)a); break;
        case OP_W8: o.w8((uint8_t)v); break;
        case OP_SET_LEN: o.set_len(a); break;
        case OP_FINISH: o.finish(); break;
        }
    }
    return o.len;
}

/* which: 0 = Out, 1 = JOut. ops: nops triples (op, a, v). Returns len. */
extern "C" uint64_t jout_run(int which, uint8_t *base, uint64_t cap, const uint64_t *ops, uint32_t nops)
{
    return which ? run_ops<dg::JOut>(base, cap, ops, nops) : run_ops<dg::Out>(base, cap, ops, nops);
}

#ifdef JOUT_MAIN
static uint64_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 17;
}

int main()
{
    enum { GUARD = 32, MAXCAP = 48, MAXOPS = 14, MAXLOG = MAXOPS * 8 };
    unsigned long runs = 0, overflows = 0, rollbacks = 0;
    uint64_t seed = 1;
    for (int which = 0; which < 2; which++)
        for (uint32_t mis = 0; mis < 17; mis++) /* base % 16: 0 and 8 are the wide phases, the rest byte-wise */
            for (uint64_t cap = 0; cap <= MAXCAP; cap++)
                for (int rep = 0; rep < 6; rep++, runs++) {
                    uint64_t ops[3 * (MAXOPS + 1)];
                    uint8_t model[MAXLOG];
                    uint64_t len = 0;
                    const uint32_t nops = 1 + (uint32_t)(rnd(seed) % MAXOPS);
                    for (uint32_t k = 0; k < nops; k++) {
                        const uint64_t r = rnd(seed) % 16, v = rnd(seed) * 0x9E3779B97F4A7C15ull;
                        uint64_t *q = &ops[3 * k];
                        if (r < 2 && len) { /* truncate */
                            q[0] = OP_SET_LEN, q[1] = rnd(seed) % (len + 1), q[2] = 0;
                            len = q[1];
                            rollbacks++;
                        } else if (r < 5) {
                            q[0] = OP_W8, q[1] = 1, q[2] = v & 0xFF;
                            model[len++] = (uint8_t)v;
                        } else {
                            const uint32_t n = 1 + (uint32_t)(rnd(seed) % 8);
                            q[0] = OP_WLE, q[1] = n, q[2] = v;
                            for (uint32_t j = 0; j < n; j++) model[len++] = (uint8_t)(v >> (8 * j));
                        }
                    }
                    ops[3 * nops] = OP_FINISH, ops[3 * nops + 1] = ops[3 * nops + 2] = 0;
                    /* exactly guard + cap + guard bytes behind a 16-aligned block start + mis */
                    void *blk = nullptr;
                    if (posix_memalign(&blk, 16, mis + 2 * GUARD + cap)) return 2;
                    uint8_t *buf = (uint8_t *)blk + mis;
                    memset(buf, 0xC3, 2 * GUARD + cap);
                    const uint64_t got = jout_run(which, buf + GUARD, cap, ops, nops + 1);
                    const uint64_t keep = len < cap ? len : cap;
                    int bad = got != len || memcmp(buf + GUARD, model, keep) != 0;
                    for (uint32_t j = 0; j < GUARD; j++) bad |= buf[j] != 0xC3 || buf[GUARD + cap + j] != 0xC3;
                    if (bad) {
                        printf("MISMATCH writer %d base%%16 %u cap %lu rep %d: len %lu, model %lu\n", which,
                               (unsigned)(((uintptr_t)(buf + GUARD)) & 15), (unsigned long)cap, rep, (unsigned long)got,
                               (unsigned long)len);
                        return 1;
                    }
                    overflows += len > cap;
                    free(blk);
                }
    printf("%lu runs (%lu overflowing, %lu truncations): buffers and guards match the model\n", runs, overflows,
           rollbacks);
    return 0;
}
#endif
