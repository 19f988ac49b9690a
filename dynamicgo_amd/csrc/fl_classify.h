/*
 * fl_classify.h — the flat kernel's structure-phase byte classification:
 * 64 message bytes (sixteen dwords, re-aligned to the message) -> 64-bit
 * masks of the quotes, commas and colons, bit b = byte b.
 *
 * A header of its own, with plain-C++ stand-ins for the two device builtins,
 * so that a host build (tests/flat_classify_host.cpp) holds it to a
 * byte-at-a-time model.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef DGI
#define DGI __device__ __forceinline__
#endif

namespace dg {

/* c + the sum of the four byte products of a and b (v_dot4_u32_u8) */
DGI uint32_t fl_udot4(uint32_t a, uint32_t b, uint32_t c)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (uint32_t i = 0; i < 4; i++) c += ((a >> 8 * i) & 0xFFu) * ((b >> 8 * i) & 0xFFu);
    return c;
#endif
}

/* 0x80 in each byte of x equal to the class byte (< 0x80) replicated in cc;
 * nh = ~x & 0x80808080. Every byte of (x | 0x80..) ^ cc is >= 0x80, so the
 * subtraction of 0x01010101 never borrows across bytes, and bit 7 of a byte
 * survives it unless the low seven bits matched: exact, no false flag beside
 * a match */
DGI uint32_t fl_eq(uint32_t x, uint32_t nh, uint32_t cc)
{
    return nh & ~(((x | 0x80808080u) ^ cc) + 0xFEFEFEFFu);
}

/* the 0x80-per-byte flags of two dwords -> 8 bits, byte i of the pair at bit
 * 7 + i: two dot products, no shift of the inputs, no multiply */
DGI uint32_t fl_pack8(uint32_t f0, uint32_t f1) { return fl_udot4(f1, 0x80402010u, fl_udot4(f0, 0x08040201u, 0u)); }

/* fl_pack8's bits as byte j (0..3) of a mask word */
DGI uint32_t fl_put8(uint32_t m, uint32_t p, uint32_t j) { return m | (j ? p << (8 * j - 7) : p >> 7); }

struct FlMasks {
    uint64_t Q, C, K; /* '"'  ','  ':' */
    uint64_t B;       /* '\\', only with BS */
    uint32_t anybs;   /* non-zero: the 64 bytes hold a backslash */
};

/* x: the lane's 64 bytes as sixteen little-endian dwords */
template <bool BS>
DGI FlMasks fl_classify(const uint32_t (&x)[16])
{
    uint32_t q[2] = {0, 0}, c[2] = {0, 0}, k[2] = {0, 0}, b[2] = {0, 0}, anybs = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t x0 = x[2 * j], x1 = x[2 * j + 1];
        const uint32_t n0 = ~x0 & 0x80808080u, n1 = ~x1 & 0x80808080u;
        const uint32_t b0 = fl_eq(x0, n0, 0x5C5C5C5Cu), b1 = fl_eq(x1, n1, 0x5C5C5C5Cu);
        q[j >> 2] = fl_put8(q[j >> 2], fl_pack8(fl_eq(x0, n0, 0x22222222u), fl_eq(x1, n1, 0x22222222u)), j & 3);
        c[j >> 2] = fl_put8(c[j >> 2], fl_pack8(fl_eq(x0, n0, 0x2C2C2C2Cu), fl_eq(x1, n1, 0x2C2C2C2Cu)), j & 3);
        k[j >> 2] = fl_put8(k[j >> 2], fl_pack8(fl_eq(x0, n0, 0x3A3A3A3Au), fl_eq(x1, n1, 0x3A3A3A3Au)), j & 3);
        anybs |= b0 | b1;
        if (BS) b[j >> 2] = fl_put8(b[j >> 2], fl_pack8(b0, b1), j & 3);
    }
    FlMasks m;
    m.Q = (uint64_t)q[1] << 32 | q[0];
    m.C = (uint64_t)c[1] << 32 | c[0];
    m.K = (uint64_t)k[1] << 32 | k[0];
    m.B = (uint64_t)b[1] << 32 | b[0];
    m.anybs = anybs;
    return m;
}

}  // namespace dg
