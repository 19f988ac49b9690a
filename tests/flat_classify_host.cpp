/* The flat kernel's structure-phase classification (fl_classify.h) built for
 * the host, so that a CPU test (test_flat_classify_host.py) can hold it to a
 * byte-at-a-time model: 64 bytes in, the quote, comma, colon and backslash
 * masks and the any-backslash word out.
 *
 * Built as HIP (-x hip), host pass only, the way str_host.cpp is: __device__
 * is defined away and the two device builtins take the header's plain-C++
 * stand-ins.
 *
 * With -DCLS_MAIN the file is a program: every byte value at every position
 * over every background, each block in a heap allocation of exactly 64
 * bytes, against the byte loop below -- for a sanitizer build. */
#ifndef __HIP_DEVICE_COMPILE__
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#undef __device__
#define __device__
#include "../dynamicgo_amd/csrc/fl_classify.h"

namespace {

void load16(const uint8_t *b, uint32_t (&x)[16])
{
    for (int i = 0; i < 16; i++)
        x[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
}

}  // namespace

/* out[5 * i ..]: Q, C, K, B, any-backslash (0 / 1) of block i; the return
 * value counts the blocks on which the instance without the backslash mask
 * disagrees with the one with it */
extern "C" uint64_t cls_blocks(const uint8_t *blocks, uint64_t n, uint64_t *out)
{
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t x[16];
        load16(blocks + 64 * i, x);
        const dg::FlMasks a = dg::fl_classify<true>(x), b = dg::fl_classify<false>(x);
        out[5 * i] = a.Q;
        out[5 * i + 1] = a.C;
        out[5 * i + 2] = a.K;
        out[5 * i + 3] = a.B;
        out[5 * i + 4] = (a.anybs & 0x80808080u) != 0;
        bad += a.Q != b.Q || a.C != b.C || a.K != b.K || ((a.anybs & 0x80808080u) != 0) != ((b.anybs & 0x80808080u) != 0) ||
               (a.anybs & ~0x80808080u) || b.B;
    }
    return bad;
}

/* the builtins' stand-ins and the flag / pack pair on their own */
extern "C" uint32_t cls_eq(uint32_t x, uint32_t cc) { return dg::fl_eq(x, ~x & 0x80808080u, cc); }
extern "C" uint32_t cls_pack8(uint32_t f0, uint32_t f1) { return dg::fl_pack8(f0, f1); }

#ifdef CLS_MAIN
int main()
{
    static const uint8_t bg[] = {'a', 0x22, 0x2C, 0x3A, 0x5C, 0x23, 0x2D, 0x3B, 0x5D, 0xA2, 0xAC, 0xBA, 0xDC, 0x00, 0xFF};
    uint64_t n = 0, bad = 0;
    for (unsigned g = 0; g < sizeof bg; g++)
        for (unsigned p = 0; p < 64; p++)
            for (unsigned c = 0; c < 256; c++) {
                uint8_t *b = (uint8_t *)malloc(64);
                memset(b, bg[g], 64);
                b[p] = (uint8_t)c;
                uint64_t got[5], want[5] = {0, 0, 0, 0, 0};
                bad += cls_blocks(b, 1, got);
                for (unsigned i = 0; i < 64; i++) {
                    want[0] |= (uint64_t)(b[i] == '"') << i;
                    want[1] |= (uint64_t)(b[i] == ',') << i;
                    want[2] |= (uint64_t)(b[i] == ':') << i;
                    want[3] |= (uint64_t)(b[i] == '\\') << i;
                }
                want[4] = want[3] != 0;
                bad += memcmp(got, want, sizeof got) != 0;
                free(b);
                n++;
            }
    printf("%llu blocks, %llu bad\n", (unsigned long long)n, (unsigned long long)bad);
    return bad != 0;
}
#endif
#endif
