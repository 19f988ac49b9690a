/* The flat kernel's per-descriptor image (dynamicgo_amd/csrc/flat_image.h,
 * built by flat_image.hip's flat_image_build) checked on the host, as a
 * stand-alone program for the sanitizers (test_flat_image_host.py):
 *
 *   flat_image_host BLOB...      each file one descriptor blob
 *
 * For each blob, in heap blocks of exactly their sizes: the image's length
 * and 16-byte padding, the blob's bytes and the zero fill behind them, and the
 * three tables against what the kernels read today -- P10 (j2t_device.h), the
 * powers of ten as integers, and the Eisel-Lemire window
 * DG_POW10_M128[EL_WLO + 348 + t][1], t < EL_WN (j2t_fast.h, dg_tables.h).
 *
 * Built as HIP (-x hip) like num_host.cpp: only the host pass sees the
 * headers, with __device__ and __constant__ defined away so that the tables
 * are host arrays; the device-only intrinsics the headers call get host
 * overloads. The headers are not edited. */
#ifndef __HIP_DEVICE_COMPILE__
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b)
{
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
}
inline unsigned int __umul24(unsigned int a, unsigned int b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
inline double __dmul_rn(double a, double b)
{
    volatile double r = a * b;
    return r;
}
inline double __ddiv_rn(double a, double b)
{
    volatile double r = a / b;
    return r;
}
inline int __clzll(long long a) { return a ? __builtin_clzll((unsigned long long)a) : 64; }
inline long long __double_as_longlong(double d)
{
    long long v;
    memcpy(&v, &d, 8);
    return v;
}
inline double __longlong_as_double(long long v)
{
    double d;
    memcpy(&d, &v, 8);
    return d;
}

#undef __device__
#define __device__
#undef __constant__
#define __constant__
#include "../dynamicgo_amd/csrc/j2t_fast.h"
#include "../dynamicgo_amd/csrc/flat_image.hip"

static int fail(const char *file, const char *what, long k)
{
    fprintf(stderr, "%s: %s (%ld)\n", file, what, k);
    return 1;
}

static int check(const char *file)
{
    FILE *fh = fopen(file, "rb");
    if (!fh) return fail(file, "cannot open", 0);
    fseek(fh, 0, SEEK_END);
    const long len = ftell(fh);
    fseek(fh, 0, SEEK_SET);
    uint8_t *blob = (uint8_t *)malloc((size_t)len); /* exactly the blob: a read past it is caught */
    if (len <= 0 || fread(blob, 1, (size_t)len, fh) != (size_t)len) return fail(file, "cannot read", len);
    fclose(fh);
    const uint32_t b16 = ((uint32_t)len + 15) & ~15u, want = b16 + 8 * 20 + 8 * 23 + 8 * dg::EL_WN + 8;
    const uint32_t n = dg::fli_len((uint32_t)len);
    if (n != want || n % 16 || dg::fli_blob16((uint32_t)len) != b16 || dg::FLI_TABS != 864) return fail(file, "length", n);
    uint8_t *img = (uint8_t *)malloc(n); /* exactly the image */
    memset(img, 0xA5, n);
    dg::flat_image_build(blob, (uint32_t)len, img);
    if (memcmp(img, blob, (size_t)len)) return fail(file, "blob bytes", 0);
    for (uint32_t k = (uint32_t)len; k < b16; k++)
        if (img[k]) return fail(file, "padding behind the blob", k);
    const uint8_t *t = img + b16;
    for (int k = 0; k < 20; k++) { /* 10^k, from its decimal text */
        char txt[32] = "1";
        for (int j = 0; j < k; j++) strcat(txt, "0");
        const uint64_t w = strtoull(txt, nullptr, 10);
        if (memcmp(t + 8 * k, &w, 8)) return fail(file, "p10u", k);
    }
    t += 8 * 20;
    for (int k = 0; k < 23; k++) { /* P10, and the correctly rounded 1e<k> */
        char txt[32];
        snprintf(txt, sizeof txt, "1e%d", k);
        const double d = strtod(txt, nullptr);
        if (memcmp(t + 8 * k, &dg::P10[k], 8) || memcmp(t + 8 * k, &d, 8)) return fail(file, "p10d", k);
    }
    t += 8 * 23;
    for (int k = 0; k < dg::EL_WN; k++) /* what el_window_fill reads */
        if (memcmp(t + 8 * k, &DG_POW10_M128[dg::EL_WLO + 348 + k][1], 8)) return fail(file, "window", k);
    t += 8 * dg::EL_WN;
    for (; t < img + n; t++)
        if (*t) return fail(file, "padding behind the tables", t - img);
    printf("blob %ld: image %u bytes, tables at %u: ok\n", len, n, b16);
    free(img);
    free(blob);
    return 0;
}

int main(int argc, char **argv)
{
    int bad = argc < 2;
    for (int k = 1; k < argc; k++) bad |= check(argv[k]);
    return bad;
}
#endif
