/* The kernels' field-name lookups built for the host, so that a CPU test
 * (test_keys_host.py) can hold them to the Python name map on the descriptor
 * families of descgen.py, and so that a sanitizer can watch what they read:
 *
 *   key_eq     the masked word compare against the zero-padded pool key (j2t_fast.h)
 *   fl_lookup  the flat kernel's hash and probe loop (j2t_flat.h)
 *   wv_lookup  the wave kernel's probe loop (j2t_wave.h), given the hash
 *
 * Built as HIP (-x hip), host pass only, as num_host.cpp is: __device__,
 * __constant__, __global__ and __shared__ are defined away, so the headers'
 * free templates are host templates and the kernels plain functions nobody
 * calls; the device intrinsics they name get host stand-ins below (the
 * lookups use none of them). The headers are not edited.
 *
 * The blob sits in a heap block of exactly total_len bytes and the key in one
 * that ends 16 bytes after the key (the arena's documented readable tail), at
 * every offset 0..7 from an 8-byte boundary, so a read beyond either is a
 * heap-buffer-overflow to AddressSanitizer.
 *
 * Left to the GPU tests (test_gpu_descgen.py): fl_field's inline compare of
 * keys up to 16 bytes against the LDS key table, the probe loop inside
 * fast_convert and the exact machine's member find_field.
 *
 * Corpus (little-endian u32 unless noted), written by test_keys_host.py:
 *   n_blobs, then per blob: len, bytes (len is a multiple of 8)
 *   n_queries, then per query: blob, struct index, key length, the field
 *   index the name map gives (i32, -1: none), key bytes, padded to 4
 * With -DKEYS_MAIN: a program that runs a corpus file and reports. */
#ifndef __HIP_DEVICE_COMPILE__
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b)
{
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
}
inline unsigned int __umul24(unsigned int a, unsigned int b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
inline double __dmul_rn(double a, double b) { volatile double r = a * b; return r; }
inline double __ddiv_rn(double a, double b) { volatile double r = a / b; return r; }
inline int __clzll(long long a) { return a ? __builtin_clzll((unsigned long long)a) : 64; }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
/* never called: the kernels that use them are compiled, not run */
inline void __syncthreads() {}
inline void __threadfence() {}
template <class T, class U> inline T atomicAdd(T *p, U v) { T o = *p; *p = (T)(o + v); return o; }
template <class T, class U> inline T atomicOr(T *p, U v) { T o = *p; *p = (T)(o | v); return o; }
template <class T, class U> inline T atomicMax(T *p, U v) { T o = *p; if ((T)v > o) *p = (T)v; return o; }
template <class T> inline T __shfl(T v, int, int = 64) { return v; }
template <class T> inline T __shfl_xor(T v, int, int = 64) { return v; }
template <class T> inline T __shfl_up(T v, unsigned, int = 64) { return v; }
template <class T> inline T __shfl_down(T v, unsigned, int = 64) { return v; }

#undef __device__
#define __device__
#undef __constant__
#define __constant__
#undef __global__
#define __global__
#undef __shared__
#define __shared__
#undef __launch_bounds__
#define __launch_bounds__(...)
#define amdgpu_waves_per_eu(...) unused /* the attribute is for kernels only */
#include "../dynamicgo_amd/csrc/j2t_flat.h"
#include "../dynamicgo_amd/csrc/j2t_wave.h"

namespace {

typedef dg::SrcT<const uint64_t> MemSrc;

struct Blob {
    uint8_t *p;
    dg_desc_hdr h;
};

uint32_t rd32(const uint8_t *&c)
{
    uint32_t v;
    memcpy(&v, c, 4);
    c += 4;
    return v;
}

/* per query, out[4]: fl_lookup, wv_lookup, key_eq disagreements with memcmp
 * over the struct's names of the key's length, names of that length */
long run(const uint8_t *c, size_t len, int32_t *out)
{
    const uint8_t *end = c + len;
    std::vector<Blob> blobs(rd32(c));
    for (Blob &b : blobs) {
        const uint32_t n = rd32(c);
        b.p = (uint8_t *)malloc(n); /* exactly total_len bytes */
        memcpy(b.p, c, n);
        memcpy(&b.h, b.p, sizeof b.h);
        if (b.h.total_len != n) return -1;
        c += n;
    }
    const uint32_t nq = rd32(c);
    long wrong = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t bi = rd32(c), si = rd32(c), kn = rd32(c);
        const int32_t want = (int32_t)rd32(c);
        const uint8_t *key = c;
        c += (kn + 3) & ~3u;
        if (c > end || bi >= blobs.size()) return -1;
        const Blob &b = blobs[bi];
        const auto D = dg::desc_view<1>((const __attribute__((address_space(1))) uint8_t *)b.p, b.h);
        const dg_struct sd = dg::ldrec(&D.S[si]);
        int32_t fl = -3, wv = -3, keq = 0, same = 0;
        for (uint32_t lead = 0; lead < 8; lead++) {
            /* '"' key '"' then 14 more bytes: 16 readable bytes behind the key */
            const size_t sz = lead + 1 + kn + 16;
            uint8_t *buf = (uint8_t *)malloc((sz + 7) & ~(size_t)7);
            memset(buf, '#', lead);
            buf[lead] = '"';
            memcpy(buf + lead + 1, key, kn);
            buf[lead + 1 + kn] = '"';
            memset(buf + lead + 2 + kn, ':', sz - (lead + 2 + kn));
            MemSrc s;
            s.init((const uint64_t *)buf, 0, (int64_t)(lead + 2 + kn + 2));
            const int64_t k0 = lead + 1;
            const int32_t a = dg::fl_lookup(D, sd, s, (uint32_t)k0, kn);
            uint32_t h = DG_NAME_HASH_SEED;
            for (uint32_t j = 0; j < kn; j++) h = DG_NAME_HASH_STEP(h, key[j]);
            const int32_t w = dg::wv_lookup(D, sd, s, k0, kn, h);
            if (lead == 0) {
                fl = a;
                wv = w;
            } else {
                if (a != fl) fl = -4; /* the verdict moved with the alignment */
                if (w != wv) wv = -4;
            }
            if (lead == 0 || lead == 5) {
                for (uint32_t e = 0; e <= sd.name_mask; e++) {
                    const dg_name nm = dg::ldrec(&D.N[sd.name_begin + e]);
                    if (nm.field == DG_NONE || nm.key_len != kn) continue;
                    same += lead == 0;
                    const bool eq = dg::key_eq(s, k0, kn, (decltype(&D.R[0]))(&D.P[nm.key_off]));
                    if (eq != (memcmp(b.p + b.h.off_pool + nm.key_off, key, kn) == 0)) keq++;
                }
            }
            free(buf);
        }
        out[4 * q] = fl;
        out[4 * q + 1] = wv;
        out[4 * q + 2] = keq;
        out[4 * q + 3] = same;
        if (fl != want || wv != want || keq) wrong++;
    }
    for (Blob &b : blobs) free(b.p);
    return wrong;
}

}  // namespace

extern "C" long keys_run(const uint8_t *corpus, size_t len, int32_t *out) { return run(corpus, len, out); }

#ifdef KEYS_MAIN
int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> c;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) c.insert(c.end(), tmp, tmp + n);
    fclose(f);
    const uint8_t *p = c.data();
    uint32_t nb;
    memcpy(&nb, p, 4);
    p += 4;
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t l;
        memcpy(&l, p, 4);
        p += 4 + l;
    }
    uint32_t nq;
    memcpy(&nq, p, 4);
    std::vector<int32_t> out(4 * (size_t)nq + 4);
    const long wrong = run(c.data(), c.size(), out.data());
    printf("%u blobs, %u queries, %ld wrong\n", nb, nq, wrong);
    return wrong != 0;
}
#endif
#endif
