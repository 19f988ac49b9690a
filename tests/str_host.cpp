/* The string and base64 routines of the kernels built for the host, so that a
 * CPU test (test_str_host.py) can hold each of them to the reference on the
 * corpora of strgen.py:
 *
 *   j2t  advance_string + unquote and b64decode (decode_block, b64decode_from)
 *        as the exact machine calls them (j2t_device.h); fast_string with
 *        fast_unquote / hex4w and fast_binary with b64_4 / b64_8 and its
 *        up-front length (j2t_fast.h); hexv, b64v
 *        the flat kernel's escape table entries: fl_hex4, fl_escape, esc_in,
 *        esc_out, esc_utf8 (j2t_flat.h); the wave kernel's b64_len and
 *        chunk_b64 (j2t_wave.h)
 *   t2j  emit_quoted, emit_base64 (t2j_device.h) through a plain byte writer;
 *        quote_extra (t2j_wave.h)
 *
 * Built as HIP (-x hip), host pass only, the way keys_host.cpp is:
 * __device__, __constant__, __global__ and __shared__ are defined away, the
 * kernels are plain functions nobody calls, and the device intrinsics they
 * name get host stand-ins (the routines here use none). The headers are not
 * edited.
 *
 * Left to the GPU tests (test_gpu_strings.py): the flat kernel's run writer
 * and fl_esc_in over its LDS table, the wave scan's escape count in tsep and
 * the page's shortcut, the chunk tasks' layout on both kernels -- inline code
 * of the kernels. The corpus reaches each of them on its own route.
 *
 * With -DSTR_MAIN the file is a program: it reads a corpus file (items of
 * u32 length, u8 kind, bytes) and runs every routine on every item with the
 * source in a heap block of exactly the item's length plus 16 bytes, for a
 * sanitizer build. */
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
#include "../dynamicgo_amd/csrc/t2j_device.h"
#include "../dynamicgo_amd/csrc/t2j_wave.h"

namespace {

typedef dg::SrcT<const uint64_t> MemSrc;           /* a message in memory */
typedef dg::SrcT<const uint64_t, int32_t> LdsSrc;  /* the shape of an LDS window: 32-bit positions */

enum { K_MSG = 0, K_SUB = 1, K_LDS = 2 };

/* n bytes at byte offset `off` of 8-byte words; what lies round them is 0xAA
 * up to the readable slack, so that a routine reading past its string sees
 * bytes that are neither zero nor its own */
struct Buf {
    std::vector<uint64_t> w;
    uint32_t off;
    Buf(const uint8_t *m, int64_t n, uint32_t o, uint8_t fill) : w((o + n) / 8 + 4, 0), off(o)
    {
        memset(w.data(), fill, w.size() * 8);
        memcpy((uint8_t *)w.data() + off, m, (size_t)n);
    }
};

struct ByteW { /* emit_*'s writer interface, byte by byte */
    uint8_t *p;
    uint32_t len;
    void wle(uint64_t v, uint32_t n)
    {
        for (uint32_t k = 0; k < n; k++) p[len++] = (uint8_t)(v >> (8 * k));
    }
    void w8(uint8_t v) { p[len++] = v; }
};

/* j2t_string / j2t_binary of the exact machine (j2t_machine.h:362-417) at the
 * body m[s..]: res = {e or -code, l or its negative} */
template <class S>
void exact_on(S &src, int64_t s, int binary, uint8_t *obuf, uint64_t cap, int64_t *res)
{
    dg::Out out;
    out.init(obuf, cap);
    bool esc;
    const int64_t e = dg::advance_string(src, s, esc);
    res[0] = e, res[1] = 0, res[2] = 0;
    if (e < 0) return;
    const int64_t n = e - s - 1;
    if (binary) {
        const uint64_t back = out.alloc(4);
        const int64_t l = dg::b64decode(out, src, s, n);
        res[1] = l;
        if (l >= 0) out.put32(back, (uint32_t)l);
    } else if (esc) {
        const uint64_t lp = out.alloc(4);
        dg::OutSink sink{&out};
        const int64_t l = dg::unquote(src, s, n, sink);
        res[1] = l;
        if (l >= 0) out.put32(lp, (uint32_t)l);
    } else {
        out.w32((uint32_t)n);
        for (int64_t i = 0; i < n; i++) out.w8(src.raw(s + i));
        res[1] = n;
    }
    out.finish();
    res[2] = (int64_t)out.len;
}

template <class S>
int fast_on(S &src, typename S::idx s, int binary, uint8_t *obuf, uint64_t cap, int64_t *res)
{
    dg::Out out;
    out.init(obuf, cap);
    typename S::idx p = s;
    const bool ok = binary ? dg::fast_binary(src, p, out) : dg::fast_string(src, p, out);
    out.finish();
    res[0] = ok ? (int64_t)p : -1, res[1] = 0, res[2] = (int64_t)out.len;
    return ok;
}

/* the branches fast_unquote takes on src[s0, s0+nb), in its own order */
enum {
    U_WORD8 = 1 << 0,    /* a whole word without a backslash */
    U_TAIL = 1 << 1,     /* the last partial word without one */
    U_MASKED = 1 << 2,   /* the rem < 8 mask removed a backslash behind the string's end */
    U_J0 = 1 << 3,       /* bits 3..10: the backslash at byte 0..7 of the loaded word */
    U_SIMPLE = 1 << 11,
    U_U1 = 1 << 12, U_U2 = 1 << 13, U_U3 = 1 << 14, U_PAIR = 1 << 15,
    U_D_END = 1 << 16,   /* declines: a backslash as the last byte */
    U_D_LETTER = 1 << 17,
    U_D_SHORT = 1 << 18, /* \u with fewer than four bytes behind it */
    U_D_HEX0 = 1 << 19,
    U_D_LONE = 1 << 20,  /* a surrogate without its partner */
    U_D_HEX1 = 1 << 21,
    U_D_LOW = 1 << 22,   /* the second \u is no low surrogate */
};

template <class S>
uint32_t classify_unquote(S &src, typename S::idx s0, typename S::idx nb)
{
    typedef typename S::idx SI_;
    uint32_t c = 0;
    SI_ i = s0, end = s0 + nb;
    while (i < end) {
        const uint64_t w = src.get8(i);
        const SI_ rem = end - i;
        uint64_t m = dg::eqbytes(w, '\\');
        if (rem < 8) {
            const uint64_t mm = m & ((1ull << (rem << 3)) - 1);
            if (mm != m) c |= U_MASKED;
            m = mm;
        }
        if (m == 0) {
            c |= rem < 8 ? U_TAIL : U_WORD8;
            i += rem < 8 ? rem : 8;
            continue;
        }
        const uint32_t j = (uint32_t)__builtin_ctzll(m) >> 3;
        c |= U_J0 << j;
        i += j;
        if (end - i < 2) return c | U_D_END;
        const uint8_t l = src.at(i + 1);
        if (l != 'u') {
            if (l != '/' && l != '"' && l != 'b' && l != 'f' && l != 'n' && l != 'r' && l != 't' && l != '\\')
                return c | U_D_LETTER;
            c |= U_SIMPLE;
            i += 2;
            continue;
        }
        if (end - i < 6) return c | U_D_SHORT;
        uint32_t r0, r1;
        if (!dg::hex4w(src, i + 2, r0)) return c | U_D_HEX0;
        i += 6;
        if (r0 <= 0x7f) c |= U_U1;
        else if (r0 <= 0x7ff) c |= U_U2;
        else if (r0 < 0xd800 || r0 > 0xdfff) c |= U_U3;
        else {
            if (end - i < 6 || r0 > 0xdbff || src.at(i) != '\\' || src.at(i + 1) != 'u') return c | U_D_LONE;
            if (!dg::hex4w(src, i + 2, r1)) return c | U_D_HEX1;
            if (r1 < 0xdc00 || r1 > 0xdfff) return c | U_D_LOW;
            i += 6;
            c |= U_PAIR;
        }
    }
    return c;
}

/* the branches fast_binary takes on the body src[s0, s0+nb) (no backslash in it) */
enum {
    B_WANT = 1 << 0,     /* nb % 4 == 0: the length is written up front */
    B_NOWANT = 1 << 1,
    B_PAD1 = 1 << 2, B_PAD2 = 1 << 3,
    B_LOOP8 = 1 << 4,    /* at least one b64_8 step */
    B_BREAK8 = 1 << 5,   /* a b64_8 step refused its word */
    B_TAIL = 1 << 6,     /* b64decode_from finished the body */
    B_D_ERROR = 1 << 7,  /* declines: the exact decoder reports an error */
    B_D_WANT = 1 << 8,   /* declines: decoded, but not to the length written up front */
    B_ESC = 1 << 9,      /* declines: a backslash in the body */
};

template <class S>
uint32_t classify_binary(S &src, int64_t s0, int64_t nb, bool esc)
{
    if (esc) return B_ESC;
    uint32_t c = 0;
    int64_t want = -1;
    if ((nb & 3) == 0) {
        const uint8_t c2 = nb ? src.raw(s0 + nb - 2) : 0, c3 = nb ? src.raw(s0 + nb - 1) : 0;
        want = (int64_t)(nb / 4 * 3) - (c3 == '=' ? (c2 == '=' ? 2 : 1) : 0);
        c |= B_WANT | (c3 == '=' ? (c2 == '=' ? B_PAD2 : B_PAD1) : 0);
    } else {
        c |= B_NOWANT;
    }
    std::vector<uint8_t> scratch((size_t)nb + 64);
    dg::Out out;
    out.init(scratch.data(), scratch.size());
    int64_t ip = 0, op = 0;
    while (ip + 8 <= nb) {
        uint64_t o;
        if (!dg::b64_8(src.get8(s0 + ip), o)) {
            c |= B_BREAK8;
            break;
        }
        c |= B_LOOP8;
        ip += 8;
        op += 6;
    }
    if (ip < nb) {
        c |= B_TAIL;
        op = dg::b64decode_from(out, src, s0, nb, ip, op);
        if (op < 0) return c | B_D_ERROR;
    }
    if (want >= 0 && op != want) c |= B_D_WANT;
    return c;
}

} // namespace

/* the exact machine's string / binary at body offset s of the message m[0, n).
 * res: e (just past the closing quote) or -code; the unquoted / decoded length
 * or the routine's negative result; bytes written (4 of length + body) */
extern "C" void str_exact(const uint8_t *m, int64_t n, int64_t s, int binary, int kind, uint8_t *obuf, uint64_t cap,
                          int64_t *res)
{
    Buf b(m, n, (uint32_t)(n * 3 + kind) & 7, 0);
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    exact_on(src, s, binary, obuf, cap, res);
}

/* fast_string / fast_binary over one source kind. res: the position after the
 * string or -1 (declined); -; bytes written. Returns accepted. fill: the byte
 * round the message (K_MSG, K_LDS) */
extern "C" int str_fast(const uint8_t *m, int64_t n, int64_t s, int binary, int kind, int fill, uint8_t *obuf,
                        uint64_t cap, int64_t *res)
{
    Buf b(m, n, (uint32_t)(n * 5 + kind + s) & 7, (uint8_t)fill);
    if (kind == K_LDS) {
        LdsSrc src;
        src.init(b.w.data(), (int32_t)b.off, (int32_t)n);
        return fast_on(src, (int32_t)s, binary, obuf, cap, res);
    }
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    if (kind == K_SUB) { /* the view starts at the body: positions count from it */
        MemSrc v = src.sub(s, n - s);
        const int ok = fast_on(v, (int64_t)0, binary, obuf, cap, res);
        if (ok) res[0] += s;
        return ok;
    }
    return fast_on(src, s, binary, obuf, cap, res);
}

/* which branches the fast routine takes on this item: a bit set (U_* / B_*) */
extern "C" uint32_t str_class(const uint8_t *m, int64_t n, int64_t s, int binary)
{
    Buf b(m, n, (uint32_t)(n * 7 + s) & 7, '\\'); /* backslashes behind the message: U_MASKED says the mask met them */
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    bool esc;
    const int64_t e = dg::advance_string(src, s, esc);
    if (e < 0) return 0x80000000u;
    if (binary) return classify_binary(src, s, e - 1 - s, esc);
    return classify_unquote(src, s, e - 1 - s);
}

extern "C" int str_quote(const uint8_t *m, int64_t n, uint8_t *obuf)
{
    Buf b(m, n, (uint32_t)(n * 3) & 7, 0x22); /* quotes behind the string: emit_quoted must not count them */
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    ByteW w = {obuf, 0};
    dg::emit_quoted(w, src, (int64_t)0, n);
    return (int)w.len;
}

extern "C" int str_b64enc(const uint8_t *m, int64_t n, uint8_t *obuf)
{
    Buf b(m, n, (uint32_t)(n * 3 + 1) & 7, 0xFF);
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    ByteW w = {obuf, 0};
    dg::emit_base64(w, src, (int64_t)0, n);
    return (int)w.len;
}

extern "C" int str_hexv(int c) { return dg::hexv((uint8_t)c); }
extern "C" int str_b64v(int c) { return dg::b64v((uint8_t)c); }

/* hex4w on the four bytes of w (first lowest): the value, or -1 */
extern "C" int64_t str_hex4w(uint32_t w)
{
    uint64_t words[2] = {w, 0};
    MemSrc src;
    src.init(words, (int64_t)0, 8);
    uint32_t v;
    return dg::hex4w(src, (int64_t)0, v) ? (int64_t)v : -1;
}

/* b64_4 on every word of ws: out[k] = its three bytes (first lowest), or -1 */
extern "C" void str_b64_4_many(const uint32_t *ws, uint64_t n, int64_t *out)
{
    for (uint64_t k = 0; k < n; k++) {
        uint32_t o;
        out[k] = dg::b64_4(ws[k], o) ? (int64_t)o : -1;
    }
}

/* b64_8 on one word: 1 and the six bytes in *o, or 0 */
extern "C" int str_b64_8(uint64_t w, uint64_t *o) { return dg::b64_8(w, *o); }

/* fl_hex4 on the four bytes of w (first lowest): the value, or -1 */
extern "C" int64_t str_fl_hex4(uint32_t w)
{
    uint32_t v;
    return dg::fl_hex4(w, v) ? (int64_t)v : -1;
}

/* fl_escape at position p on each 8 bytes e0[k] (from the backslash on):
 * out[4k..] = the entry (0: left to the exact machine), esc_in, esc_out, esc_utf8 */
extern "C" void str_fl_escape_many(const uint64_t *e0, uint64_t n, uint32_t p, uint32_t *out)
{
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t x = dg::fl_escape(p, e0[k]);
        out[4 * k] = x;
        out[4 * k + 1] = x ? dg::esc_in(x) : 0;
        out[4 * k + 2] = x ? dg::esc_out(x) : 0;
        out[4 * k + 3] = x ? dg::esc_utf8(x) : 0;
        if (x && dg::esc_pos(x) != p) out[4 * k] = 0xFFFFFFFFu;
    }
}

/* chunk_b64 on m[0, n): the bytes written, or -1 where it refuses */
extern "C" int str_chunk_b64(const uint8_t *m, int64_t n, int last, int fill, uint8_t *obuf)
{
    Buf b(m, n, (uint32_t)(n + last) & 7, (uint8_t)fill);
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    ByteW w = {obuf, 0};
    return dg::chunk_b64(src, (int64_t)0, n, last != 0, w) ? (int)w.len : -1;
}

extern "C" int64_t str_b64_len(const uint8_t *m, int64_t n)
{
    Buf b(m, n, 3, 0);
    MemSrc src;
    src.init(b.w.data(), (int64_t)b.off, n);
    return dg::b64_len(src, (int64_t)0, n);
}

/* chunk_b64 as a body's last chunk on every final quantum abcd, abc= and ab==
 * over the alphabet, behind `lead` whole quanta: the number that differ from
 * the exact b64decode of the same bytes in what they write or in b64_len */
extern "C" uint64_t str_chunk_final_mismatches(int lead)
{
    static const char A[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    uint64_t bad = 0;
    uint64_t words[8] = {0};
    uint8_t *m = (uint8_t *)words;
    for (int k = 0; k < 4 * lead; k++) m[k] = (uint8_t)A[(k * 7 + 3) & 63];
    const int64_t n = 4 * lead + 4;
    uint8_t o1[64], o2[64];
    for (int a = 0; a < 64; a++)
        for (int b = 0; b < 64; b++)
            for (int c = 0; c < 65; c++)
                for (int d = c == 64 ? 64 : 0; d < 65; d++) { /* index 64: '=' */
                    uint8_t *q = m + 4 * lead;
                    q[0] = (uint8_t)A[a], q[1] = (uint8_t)A[b], q[2] = c == 64 ? '=' : (uint8_t)A[c], q[3] = d == 64 ? '=' : (uint8_t)A[d];
                    MemSrc s1, s2;
                    s1.init(words, (int64_t)0, n);
                    s2.init(words, (int64_t)0, n);
                    ByteW w = {o1, 0};
                    const bool ok = dg::chunk_b64(s1, (int64_t)0, n, true, w);
                    dg::Out out;
                    out.init(o2, sizeof o2);
                    const int64_t l = dg::b64decode(out, s2, (int64_t)0, n);
                    out.finish();
                    if (!ok || l != (int64_t)w.len || memcmp(o1, o2, (size_t)l) != 0 || dg::b64_len(s1, (int64_t)0, n) != l) bad++;
                }
    return bad;
}

extern "C" uint32_t str_quote_extra(uint64_t w, uint32_t nb) { return dg::quote_extra(w, nb); }

/* the values the headers give the error codes: E_EOF, E_INVAL, E_ESCAPE, E_UNICODE, E_DECODE_BASE64 */
extern "C" void str_consts(int64_t *out)
{
    out[0] = dg::E_EOF, out[1] = dg::E_INVAL, out[2] = dg::E_ESCAPE, out[3] = dg::E_UNICODE, out[4] = dg::E_DECODE_BASE64;
}

#ifdef STR_MAIN
/* every routine on one item whose source is a heap block of exactly n + 16
 * bytes, 8-aligned as the arenas are; j2t items are whole messages (kind 0 / 1:
 * string / binary, body offset in `s`), t2j items raw bytes (kind 2) */
static uint64_t run_item(const uint8_t *m, int64_t n, int64_t s, int kind)
{
    uint64_t sum = 0;
    uint64_t *blk = (uint64_t *)malloc((size_t)n + 16);
    memcpy(blk, m, (size_t)n);
    memset((uint8_t *)blk + n, 0, 16);
    const uint64_t cap = (uint64_t)n * 6 + 64;
    uint8_t *obuf = (uint8_t *)malloc(cap);
    int64_t res[3];
    if (kind < 2) {
        MemSrc a;
        a.init(blk, (int64_t)0, n);
        exact_on(a, s, kind, obuf, cap, res);
        sum += (uint64_t)res[0] + (uint64_t)res[1];
        MemSrc f;
        f.init(blk, (int64_t)0, n);
        sum += (uint64_t)fast_on(f, s, kind, obuf, cap, res);
        MemSrc v0;
        v0.init(blk, (int64_t)0, n);
        MemSrc v = v0.sub(s, n - s);
        sum += (uint64_t)fast_on(v, (int64_t)0, kind, obuf, cap, res);
        LdsSrc l;
        l.init(blk, (int32_t)0, (int32_t)n);
        sum += (uint64_t)fast_on(l, (int32_t)s, kind, obuf, cap, res);
        /* the wave kernel's chunk tasks on a base64 body of whole quanta: as one last chunk, and cut
         * into WV_CHB-character tasks as the page cuts it */
        MemSrc c;
        c.init(blk, (int64_t)0, n);
        bool esc;
        const int64_t e = dg::advance_string(c, s, esc);
        const int64_t nb = e - 1 - s;
        if (kind == 1 && e > 0 && !esc && nb > 0 && (nb & 3) == 0) {
            uint64_t *bb = (uint64_t *)malloc((size_t)nb + 16); /* the body alone: 16 bytes behind its last character */
            memcpy(bb, (const uint8_t *)blk + s, (size_t)nb);
            memset((uint8_t *)bb + nb, 0, 16);
            MemSrc b;
            b.init(bb, (int64_t)0, nb);
            sum += (uint64_t)dg::b64_len(b, (int64_t)0, nb);
            ByteW w = {obuf, 0};
            sum += (uint64_t)dg::chunk_b64(b, (int64_t)0, nb, true, w) + w.len;
            for (int64_t at = 0; at < nb; at += dg::WV_CHB) {
                const int64_t len = nb - at < (int64_t)dg::WV_CHB ? nb - at : (int64_t)dg::WV_CHB;
                ByteW wk = {obuf, 0};
                sum += (uint64_t)dg::chunk_b64(b, at, len, at + len == nb, wk) + wk.len;
            }
            free(bb);
        }
    } else {
        MemSrc a;
        a.init(blk, (int64_t)0, n);
        ByteW w = {obuf, 0};
        dg::emit_quoted(w, a, (int64_t)0, n);
        sum += w.len;
        ByteW w2 = {obuf, 0};
        dg::emit_base64(w2, a, (int64_t)0, n);
        sum += w2.len;
        for (int64_t i = 0; i < n; i += 8) /* the wave page's sizing: a word at a time, the last one partial */
            sum += dg::quote_extra(a.get8(i), (uint32_t)(n - i < 8 ? n - i : 8));
    }
    free(obuf);
    free(blk);
    return sum;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    uint64_t items = 0, sum = 0;
    for (;;) {
        uint32_t hdr[3]; /* length, body offset, kind */
        if (fread(hdr, 4, 3, fh) != 3) break;
        std::vector<uint8_t> m(hdr[0] + 1);
        if (hdr[0] && fread(m.data(), 1, hdr[0], fh) != hdr[0]) return 3;
        sum += run_item(m.data(), hdr[0], hdr[1], (int)hdr[2]);
        items++;
    }
    fclose(fh);
    printf("%llu items, checksum %llu\n", (unsigned long long)items, (unsigned long long)sum);
    return items ? 0 : 4;
}
#endif
#endif
