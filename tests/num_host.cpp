/* The number routines of the kernels built for the host, so that a CPU test
 * (test_num_host.py) can hold each of them to the reference on corpora aimed
 * at their branches (numgen.py):
 *
 *   j2t  fast_vnumber with fast_int_regs / fast_dec_regs / the general loop,
 *        atof_exact_l, eisel_lemire_t with and without the LDS window
 *        (j2t_fast.h); the exact machine's vnumber with atof_native
 *        (j2t_device.h)
 *   t2j  emit_f64 (Schubfach f64_to_dec, Dig24, f64_write_dec), emit_i64
 *        (t2j_device.h) through a plain byte writer
 *
 * Built as HIP (-x hip). Only the host pass sees the headers: there
 * __device__ and __constant__ are defined away, so every routine is a host
 * function and every table (P10, DG_POW10_M128, ...) a host array -- with
 * __device__ kept as an attribute the tables would be uninitialised host
 * shadows of device variables. The device pass compiles nothing. The headers
 * are not edited. The device-only intrinsics the routines call get host
 * overloads of the same meaning below. LDS-qualified pointers (FastTabs) are
 * plain pointers on the host, so FastTabs is built over host arrays.
 *
 * Left to the GPU tests (test_gpu_numbers.py): the register sources RSrc
 * (j2t_wave.h) and RSrcL (j2t_flat.h) themselves -- their headers hold wave
 * code the host cannot compile, so RegSrc below has their shape (five words,
 * a byte shift, the same get8) with RSrc's zero fill or RSrcL's full load --
 * the wave t2j writer t2w_number (t2j_wave.h), and emit_number's cvt32 /
 * cvt64 as the kernels call them. */
#ifndef __HIP_DEVICE_COMPILE__
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b)
{
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
}
inline unsigned int __umul24(unsigned int a, unsigned int b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
inline double __dmul_rn(double a, double b)
{
    volatile double r = a * b; /* one IEEE multiply, never fused */
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
#include "../dynamicgo_amd/csrc/t2j_device.h"

namespace {

using dg::FastTabs;

/* RSrc / RSrcL's shape: the 5 aligned words from the token's first byte on.
 * FULL: every word loaded (RSrcL: the bytes after the token are the
 * message's); otherwise only the words up to get8(n) (RSrc: the rest zero) */
template <class I>
struct RegSrc {
    typedef I idx;
    static constexpr bool kRegs = true;
    uint64_t w0, w1, w2, w3, w4;
    uint32_t sh;
    I n;
    void load(const uint64_t *q, uint32_t shift, I len, bool full)
    {
        sh = shift;
        n = len;
        const uint32_t need = full ? 5u : (sh + (uint32_t)len + 8 + 7) >> 3;
        w0 = q[0];
        w1 = need > 1 ? q[1] : 0;
        w2 = need > 2 ? q[2] : 0;
        w3 = need > 3 ? q[3] : 0;
        w4 = need > 4 ? q[4] : 0;
    }
    uint64_t word(uint32_t j) const { return j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : j == 3 ? w3 : w4; }
    uint8_t raw(I i) const
    {
        const uint32_t b = sh + (uint32_t)i;
        return (uint8_t)(word(b >> 3) >> ((b & 7) << 3));
    }
    uint8_t at(I i) const { return (std::make_unsigned_t<I>)i < (std::make_unsigned_t<I>)n ? raw(i) : 0; }
    uint64_t get8(I i) const
    {
        const uint32_t b = sh + (uint32_t)i, j = b >> 3, s8 = (b & 7) << 3;
        return (word(j) >> s8) | ((word(j + 1) << 1) << (63 - s8));
    }
};

typedef dg::SrcT<const uint64_t> MemSrc;

const char PRE[] = "{\"d\":";
const char TAIL[] = ",\"req\":2}";
enum { NPRE = 5, NTAIL = 9 };

/* prefix + token + tail at byte offset `off` of an 8-aligned, zero-padded buffer */
struct Msg {
    std::vector<uint64_t> w;
    uint32_t off;
    Msg(const uint8_t *tok, int len, uint32_t o) : w((o + NPRE + len + NTAIL) / 8 + 8, 0), off(o)
    {
        uint8_t *b = (uint8_t *)w.data() + off;
        memcpy(b, PRE, NPRE);
        memcpy(b + NPRE, tok, len);
        memcpy(b + NPRE + len, TAIL, NTAIL);
    }
};

struct Tabs {
    uint64_t win[dg::EL_WN];
    FastTabs tb;
    explicit Tabs(bool window)
    {
        for (uint32_t t = 0; t < 64; t++) dg::el_window_fill(win, t);
        tb.p10u = nullptr; /* acc_digits keeps its powers in registers */
        tb.p10d = (dg::lds_f64 *)(const void *)dg::P10;
        tb.pw = window ? (const __attribute__((address_space(3))) uint64_t *)(const void *)win : nullptr;
    }
};

enum { K_MSG = 0, K_SUB = 1, K_RSRC = 2, K_RSRCL = 3 };
enum { R_ERR = 0, R_INT_REGS = 1, R_DEC_REGS = 2, R_INT_LOOP = 3, R_DBL_LOOP = 4 };
enum { C_NONE = 0, C_EXACT = 1, C_EL_WINDOW = 2, C_EL_TABLE = 3, C_EL_FAIL = 4, C_TRUNC = 5 };

/* fast_vnumber's steps in its own order (j2t_fast.h), with the branch taken
 * written down. out: route, conversion, exp10, accepted, man */
template <class S>
void classify(S &src, const FastTabs &tb, int64_t *out)
{
    typedef typename S::idx SI;
    uint64_t man = 0;
    int exp10 = 0, sgn = 1;
    bool trunc = false, regdec = false;
    out[0] = R_ERR, out[1] = C_NONE, out[2] = 0, out[3] = 0, out[4] = 0;
    if constexpr (dg::is_regsrc<S>::value) {
        int64_t iv;
        double dv;
        int32_t e;
        if (dg::fast_int_regs(src, iv, dv, e)) {
            out[0] = R_INT_REGS, out[3] = 1;
            return;
        }
        if (dg::fast_dec_regs(src, man, exp10, sgn)) regdec = true, out[0] = R_DEC_REGS;
    }
    if (!regdec) {
        SI i = 0;
        uint8_t c = src.at(i);
        if (c == '-') sgn = -1, c = src.at(++i);
        if ((uint8_t)(c - '0') > 9) return;
        if (c == '0') {
            const uint8_t c1 = src.at(i + 1);
            if (c1 != '.' && c1 != 'e' && c1 != 'E') {
                out[0] = R_INT_LOOP, out[3] = 1;
                return;
            }
        }
        int nd = 0;
        bool dbl = false;
        uint64_t x;
        for (;;) {
            const uint32_t k = dg::digits8(src, i, x), t = dg::acc_digits(man, nd, x, k, tb);
            exp10 += (int)(k - t);
            i += k;
            if (k < 8) break;
        }
        if (exp10 > 0) trunc = true;
        if (src.at(i) == '.') {
            i++;
            dbl = true;
            if ((uint8_t)(src.at(i) - '0') > 9) return;
        }
        if (man == 0 && exp10 == 0) {
            while (src.at(i) == '0') i++, exp10--;
            nd = 0;
        }
        while (dbl && nd < 19) {
            const uint32_t k = dg::digits8(src, i, x), t = dg::acc_digits(man, nd, x, k, tb);
            exp10 -= (int)t;
            i += t;
            if (t < 8) break;
        }
        while (dbl) {
            const uint32_t k = dg::digits8(src, i, x);
            if (k) trunc = true;
            i += k;
            if (k < 8) break;
        }
        c = src.at(i);
        if (c == 'e' || c == 'E') {
            int esm = 1, e = 0;
            dbl = true;
            c = src.at(++i);
            if (c == '+' || c == '-') esm = c == '+' ? 1 : -1, c = src.at(++i);
            if ((uint8_t)(c - '0') > 9) return;
            while ((uint8_t)(c - '0') <= 9) {
                if (e < 10000) e = e * 10 + (c - '0');
                c = src.at(++i);
            }
            exp10 += e * esm;
        } else if (!dbl) {
            const bool ovf = exp10 != 0 || ((man >> 63) == 1 && (((uint64_t)(int64_t)sgn) & man) != (1ull << 63));
            if (!ovf) {
                out[0] = R_INT_LOOP, out[3] = 1;
                return;
            }
        }
        out[0] = R_DBL_LOOP;
    }
    out[2] = exp10, out[4] = (int64_t)man;
    double val, vu;
    if (dg::atof_exact_l(man, exp10, sgn, val, tb)) {
        out[1] = C_EXACT, out[3] = 1;
        return;
    }
    const bool inwin = tb.pw && (uint32_t)(exp10 - dg::EL_WLO) < (uint32_t)dg::EL_WN;
    if (!dg::eisel_lemire_t(man, exp10, sgn, val, tb)) {
        out[1] = C_EL_FAIL;
        return;
    }
    if (trunc && (!dg::eisel_lemire_t(man + 1, exp10, sgn, vu, tb) || vu != val)) {
        out[1] = C_TRUNC;
        return;
    }
    out[1] = inwin ? C_EL_WINDOW : C_EL_TABLE, out[3] = 1;
}

struct ByteW { /* emit_*'s writer interface, byte by byte */
    uint8_t *p;
    uint32_t len;
    void wle(uint64_t v, uint32_t n)
    {
        for (uint32_t k = 0; k < n; k++) p[len++] = (uint8_t)(v >> (8 * k));
    }
    void w8(uint8_t v) { p[len++] = v; }
};

} // namespace

/* fast_vnumber over one source kind. out: accepted, isint, iv, bits of dv, end
 * (bytes of the token consumed). Returns -1 when the kind does not take this
 * token (a register source holds at most 24 bytes), else accepted. */
extern "C" int num_fast(const uint8_t *tok, int len, int kind, int64_t *out)
{
    const uint32_t off = (uint32_t)(len * 3 + kind) & 7;
    Msg m(tok, len, off);
    Tabs T(kind != K_SUB); /* K_MSG: the flat kernel's long tokens, from LDS with the window; K_SUB: the lane
                            * and small kernels (a map key's sub-view here), no window */
    int64_t iv = 0;
    double dv = 0;
    bool isint = false, ok;
    int64_t end;
    if (kind == K_MSG || kind == K_SUB) {
        MemSrc s;
        s.init(m.w.data(), (int64_t)off, NPRE + len + NTAIL);
        int64_t p = NPRE;
        if (kind == K_SUB) s = s.sub(NPRE, len), p = 0;
        const int64_t p0 = p;
        ok = dg::fast_vnumber(s, p, T.tb, iv, dv, isint);
        end = p - p0;
    } else {
        if (len > 24) return -1;
        const uint32_t b = off + NPRE;
        if (kind == K_RSRC) {
            RegSrc<int64_t> r;
            r.load(m.w.data() + (b >> 3), b & 7, len, false);
            int64_t p = 0;
            ok = dg::fast_vnumber(r, p, T.tb, iv, dv, isint);
            end = p;
        } else {
            RegSrc<int32_t> r;
            r.load(m.w.data() + (b >> 3), b & 7, len, true);
            int32_t p = 0;
            ok = dg::fast_vnumber(r, p, T.tb, iv, dv, isint);
            end = p;
        }
    }
    out[0] = ok, out[1] = isint, out[2] = iv, out[3] = __double_as_longlong(dv), out[4] = end;
    return ok;
}

/* which branches fast_vnumber takes on this token: a register source with
 * the window when it fits one (the flat and wave kernels), else memory.
 * out: route (R_*), conversion (C_*), effective exp10, accepted, mantissa */
extern "C" int num_class(const uint8_t *tok, int len, int64_t *out)
{
    Msg m(tok, len, (uint32_t)(len * 5) & 7);
    Tabs T(true);
    const uint32_t b = m.off + NPRE;
    if (len <= 24) {
        RegSrc<int64_t> r;
        r.load(m.w.data() + (b >> 3), b & 7, len, false);
        classify(r, T.tb, out);
    } else {
        MemSrc s;
        s.init(m.w.data(), (int64_t)m.off, NPRE + len + NTAIL);
        s = s.sub(NPRE, len);
        classify(s, T.tb, out);
    }
    return (int)out[3];
}

/* the exact machine's vnumber (atof_native behind it). framed: the token
 * inside a message (it ends at the first byte that is not the number's),
 * else a sub-view of exactly the token. out: vt, iv, bits of dv, end */
extern "C" void num_exact(const uint8_t *tok, int len, int framed, int64_t *out)
{
    Msg m(tok, len, (uint32_t)(len * 7 + framed) & 7);
    std::vector<uint8_t> dbuf(dg::DCAP + 8);
    MemSrc s;
    s.init(m.w.data(), (int64_t)m.off, NPRE + len + NTAIL);
    int64_t p = NPRE;
    if (!framed) s = s.sub(NPRE, len), p = 0;
    const int64_t p0 = p;
    dg::JState js;
    dg::vnumber(s, p, js, (dg::gu8 *)(void *)dbuf.data());
    out[0] = js.vt, out[1] = js.iv, out[2] = __double_as_longlong(js.dv), out[3] = p - p0;
}

extern "C" int num_f64toa(uint64_t bits, uint8_t *buf)
{
    ByteW w = {buf, 0};
    dg::emit_f64(w, __longlong_as_double((long long)bits));
    return (int)w.len;
}

extern "C" int num_i64toa(int64_t v, uint8_t *buf)
{
    ByteW w = {buf, 0};
    dg::emit_i64(w, v);
    return (int)w.len;
}

/* n doubles at once: text k is buf[32 * k, 32 * k + lens[k]) */
extern "C" void num_f64toa_many(const uint64_t *bits, uint64_t n, uint8_t *buf, uint8_t *lens)
{
    for (uint64_t k = 0; k < n; k++) lens[k] = (uint8_t)num_f64toa(bits[k], buf + 32 * k);
}

/* the values V_INTEGER, V_DOUBLE, E_EOF, E_INVAL, E_FLOAT_INF of the headers */
extern "C" void num_consts(int64_t *out)
{
    out[0] = dg::V_INTEGER, out[1] = dg::V_DOUBLE, out[2] = dg::E_EOF, out[3] = dg::E_INVAL, out[4] = dg::E_FLOAT_INF;
}
#endif
