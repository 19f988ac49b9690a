"""Number corpora aimed at the branches of the number routines, built by
construction (integer / fractions arithmetic, fixed seeds; no GPU and no
reference needed to generate them).

j2t_tokens()  -> [(class, token)]   JSON number tokens (and near-numbers)
t2j_doubles() -> [(class, float)]   doubles for f64toa
t2j_ints()    -> [int]              integers for i64toa

The classes and what each aims at:

  mid     exact decimal midpoints between adjacent doubles, written in full,
          with the last digit +-1 and cut to 19 / 20 / 21 / 40 / 799 / 800 /
          801 digits: atof_native's rounding and its 800-digit cap (DCAP)
  seam    mantissas of 1..20 digits at the effective decimal exponents where
          Eisel-Lemire's power changes source (the LDS window [-40, 24)), where
          it leaves its table (+-348) and where atof_exact ends (+-22, 37)
  exact   atof_exact's own edges: mantissas around 2^52 / 2^53 at each exponent
          edge, and products on both sides of 1e15 after the first multiply
  elfail  tokens Eisel-Lemire gives up on: exact halves of 19 digits or fewer
          (it refuses the ties whose even neighbour is below; the others it
          rounds up, rightly), and longer ones whose truncated mantissa and
          mantissa + 1 round differently
  shape   -?D+.D+ at every length and point position (fast_dec_regs' SWAR
          chunks), integers of 1..40 digits (fast_int_regs) and near-misses
  zeros   leading-zero fractions, zero mantissas, long and huge exponents
  cvt     double tokens at the edges of cvt32 / cvt64 for each integer width
  rand    %.17g of random bit patterns and random a.bEc tokens
"""
import random
import struct

MANT = (1 << 52) - 1


def f2b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def b2f(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def render(digits, k):
    """The decimal int(digits) * 10^-k written positionally, always with a point."""
    if k <= 0:
        return digits + "0" * (-k) + ".0"
    if len(digits) > k:
        return digits[:-k] + "." + digits[-k:]
    return "0." + "0" * (k - len(digits)) + digits


def midpoint(bits):
    """(digits, k): the exact midpoint between the positive doubles with bit
    patterns bits and bits + 1 is int(digits) * 10^-k; digits has no trailing
    zero unless k <= 0. bits + 1 may be the pattern of infinity (2^1024)."""
    e, f = bits >> 52, bits & MANT
    m, q = (f, -1074) if e == 0 else (f | (1 << 52), e - 1075)
    n, q = 2 * m + 1, q - 1  # the midpoint is n * 2^q, n odd
    if q >= 0:
        return str(n << q), 0
    return str(n * 5 ** -q), -q  # n / 2^-q = n * 5^-q / 10^-q


MID_CUTS = (19, 20, 21, 40, 799, 800, 801)


def _mid_bits():
    rng = random.Random(0x4D4944)
    exps = sorted(set([0, 0, 0, 1, 2, 3, 2045, 2046, 1023, 1022, 1024, 1075, 1076, 1074, 971, 972, 1086]) |
                  set(range(5, 2046, 30)))
    out = []
    for e in [0, 0] + exps:
        out.append((e << 52) | rng.getrandbits(52))
    out += [0, 1, rng.getrandbits(20), MANT - 1]  # the smallest subnormals, the largest
    for e in (1, 2, 53, 500, 1000, 1023, 1024, 1075, 1077, 1500, 2000, 2046):
        out.append((e << 52) - 1)  # fraction 0: the midpoint just below 2^(e - 1023)
        out.append(e << 52)        # and just above it
    out.append((2047 << 52) - 1)   # the largest double and 2^1024: rounds to infinity
    return out


def mids():
    """[(bits, digits, k)] of every midpoint of the corpus."""
    return [(b,) + midpoint(b) for b in _mid_bits()]


def _mid_tokens():
    out = []
    for j, (b, d, k) in enumerate(mids()):
        sg = "-" if j % 5 == 4 else ""
        out.append(sg + render(d, k))
        out.append(sg + render(str(int(d) + 1), k))
        out.append(sg + render(str(int(d) - 1).rjust(len(d), "0"), k))
        for n in MID_CUTS:
            if len(d) > n:
                out.append(sg + render(d[:n], k - (len(d) - n)))
    return out


SEAM_EXPS = (-349, -348, -347, -343, -342, -41, -40, -39, -23, -22, -21, 21, 22, 23, 24, 25, 36, 37, 38, 346, 347,
             348, 349)
SEAM_MANTS = ("1", "9007199254740993", "4503599627370497", "12345678901234567", "999999999999999999",
              "1234567890123456789", "12345678901234567891", "18446744073709551615")


def seam_cases():
    """[(token, exp10)]: exp10 is the decimal exponent the parser ends up with
    next to its (at most 19-digit) mantissa."""
    out = []
    for m in SEAM_MANTS:
        kept = min(len(m), 19)  # digits that reach the mantissa; the rest only move the exponent
        for e in SEAM_EXPS:
            out.append(("%se%d" % (m, e - (len(m) - kept)), e))          # integer digits: dropped ones count up
            mm = m if len(m) > 1 else m + "5"
            kk = min(len(mm), 19)
            out.append(("%s.%se%d" % (mm[0], mm[1:], e + kk - 1), e))     # a fraction: kept digits count down
            out.append(("0.000%sE%+d" % (m, e + 3 + kept), e))            # leading zeros count down too
    return out


def _seam_tokens():
    return [t for t, _ in seam_cases()]


EXACT_EXPS = (-23, -22, -21, -1, 0, 1, 15, 21, 22, 23, 24, 25, 36, 37, 38)


def _exact_tokens():
    out = []
    for e in EXACT_EXPS:
        for m in ((1 << 52) - 1, 1 << 52, (1 << 53) - 1, 1 << 53):
            out.append("%de%d" % (m, e))
            out.append("-%d.0e%d" % (m, e))
    for e in range(23, 38):  # val = man * 10^(e - 22) against 1e15
        p = 10 ** (15 - (e - 22))
        for m in (p - 1, p, p + 1):
            out.append("%de%d" % (m, e))
    return out


def _elfail_tokens():
    out = []
    rng = random.Random(0x454C46)
    # integers of at most 19 digits exactly between two doubles: 2^p + odd * 2^(p - 53)
    for p in range(53, 63):
        for _ in range(3):
            n = (1 << p) + (2 * rng.randrange(1 << 20) + 1) * (1 << (p - 53))
            if len(str(n)) <= 19:
                out += [str(n), "%d.0" % n, "-%d" % n, "%de0" % n]
    out += ["9007199254740993", "9007199254740993.0", "9007199254740993e0", "900719925474099.3e1",
            "9007199254740993e1", "9007199254740993e5", "9007199254740993e22", "90071992547409930e-1"]
    # halves of doubles in [2^(53 - j), 2^(54 - j)): (2m + 1) * 5^j has at most 19 digits for j <= 4
    for j in range(1, 5):
        for _ in range(4):
            m = (1 << 52) | rng.getrandbits(52)
            d = str((2 * m + 1) * 5 ** j)
            if len(d) <= 19:
                out += [render(d, j), "-" + render(d, j), "%se-%d" % (d, j)]
    # more than 19 digits: the 19-digit mantissa is below the midpoint and mantissa + 1 above it
    for b, d, k in mids():
        if len(d) < 26 or b >> 52 == 2047 or (b + 1) >> 52 == 2047:
            continue
        for n in (20, 23, 30):
            lo = d[:n]
            hi = str(int(lo) + 1)
            if hi[:19] != lo[:19] or len(hi) != len(lo):
                continue
            out.append(render(lo, k - (len(d) - n)))
            out.append(render(hi, k - (len(d) - n)))
    return out


def _digits(rng, n, first_nonzero=True):
    s = "".join(rng.choice("0123456789") for _ in range(n))
    if first_nonzero and s and s[0] == "0":
        s = rng.choice("123456789") + s[1:]
    return s


def _shape_tokens():
    rng = random.Random(0x534850)
    out = []
    for total in range(3, 24):
        for draw in range(4):
            for pd in range(1, total - 1):  # digits before the point
                for sg in ("", "-"):
                    out.append(sg + _digits(rng, pd) + "." + _digits(rng, total - 1 - pd, False))
            for sg in ("", "-"):
                out.append(sg + "0." + _digits(rng, total - 2, False))
                if total >= 4:
                    out.append(sg + "00." + _digits(rng, total - 3, False))
    for n in range(1, 41):
        for draw in range(4):
            for sg in ("", "-"):
                t = sg + _digits(rng, n)
                out.append(t)
                for c in ".ex":
                    out.append(t[:-1] + c)
    return out


def _zeros_tokens():
    out = []
    for k in list(range(26)) + [340]:
        out.append("0." + "0" * k + str(1 + k % 9))
        out.append("-0." + "0" * k + str(9 - k % 9) + "25")
    out += ["0e999999", "-0.0e-5", "0.0", "1e00000000000000000000001", "1e-0", "1E+00022", "1e10000", "1e9999",
            "1e-10000", "0.0e10000", "0e0", "-0e-0", "0.000e5", "1e-00000000000000000000022"]
    return out


CVT_TOKENS = ["127.9", "128.0", "-128.9", "-129.0", "255.5", "256.0", "32767.5", "32768.0", "-32769.0", "65536.0",
              "2147483647.5", "2147483648.0", "-2147483648.5", "-2147483649.0", "4294967296.0",
              "9223372036854775807.0", "9223372036854774784.0", "-9223372036854775808.0", "-9223372036854777856.0",
              "1e19", "1.8446744073709552e19", "1e300",
              "1.279e2", "1.28e2", "-1.289E2", "2.555e2", "3.27675e4", "65536e0", "2.1474836475e9", "2147483648e0",
              "-2.1474836485e9", "-2147483649e0", "4.294967296e9", "9.223372036854775807e18",
              "-9223372036854775808e0", "-9.223372036854777856e18", "0.9", "-0.9", "1e-300", "-1e300"]


def _rand_tokens():
    rng = random.Random(0x524E44)
    out = []
    while len(out) < 3000:
        b = rng.getrandbits(63)
        if (b >> 52) != 2047:
            out.append("%.17g" % b2f(b))
    for _ in range(2000):
        out.append("%s.%sE%d" % (_digits(rng, rng.randint(1, 11)), _digits(rng, rng.randint(1, 24), False),
                                 rng.randint(-340, 300)))
    return out


_J2T = None


def j2t_tokens():
    global _J2T
    if _J2T is None:
        _J2T = [(c, t) for c, f in (("mid", _mid_tokens), ("seam", _seam_tokens), ("exact", _exact_tokens),
                                    ("elfail", _elfail_tokens), ("shape", _shape_tokens), ("zeros", _zeros_tokens),
                                    ("cvt", lambda: CVT_TOKENS), ("rand", _rand_tokens)) for t in f()]
    return list(_J2T)


def thin(tokens, keep, every):
    """tokens with the classes of `every` ({class: step}) cut to one in step; `keep` classes untouched."""
    seen, out = {}, []
    for c, t in tokens:
        k = seen.get(c, 0)
        seen[c] = k + 1
        if c in keep or k % every.get(c, 1) == 0:
            out.append((c, t))
    return out


# ---------------------------------------------------------------- t2j ----

def _neighbours(x):
    b = f2b(x)
    return [b2f(v) for v in (b - 1, b, b + 1) if 0 < v < (2047 << 52)]


def sig_digits(text):
    """The significant digits of a decimal number's text: sign, point and
    exponent removed, zeros stripped at both ends ("0" for zero)."""
    t = text.lower().lstrip("-+")
    if "e" in t:
        t = t[:t.index("e")]
    return t.replace(".", "").strip("0") or "0"


def _digit_doubles():
    rng = random.Random(0x444947)
    out = []
    for n in range(1, 18):
        for sci in (-300, -200, -100, -30, -10, 30, 100, 200, 300, -7, -6, -1, 0, 8, 17, 20, 21, 22):
            for _ in range(200):  # n <= 15 digits always survive the round trip; 16 and 17 usually
                d = rng.choice("123456789") + _digits(rng, n - 2, False) + (rng.choice("123456789") if n > 1 else "")
                v = float("%se%d" % (d, sci - n + 1))
                if len(sig_digits(repr(v))) == n:
                    out.append(v)
                    break
    for z in range(1, 16):
        for lead in (1, 7, 123, 99999, 4503599, 9007199254):
            if len(str(lead)) + z <= 21:
                out.append(float(lead * 10 ** z))
    return out


_T2J = None


def t2j_doubles():
    global _T2J
    if _T2J is None:
        out = []
        for e in range(-1074, 1024):
            out += [("pow2", v) for v in _neighbours(2.0 ** e)]
        for k in range(-323, 309):
            out += [("pow10", v) for v in _neighbours(float("1e%d" % k))]
        fmt = []
        for x in (1e21, 1e20, 1e-6, 1e-7):
            fmt += _neighbours(x)
        fmt += [123456789012345678901.0, 0.000001234, 5e-324, b2f(MANT), b2f(1 << 52), b2f((2047 << 52) - 1), -0.0,
                0.0]
        out += [("fmt", v) for v in fmt]
        out += [("digits", v) for v in _digit_doubles()]
        _T2J = [(c, -v if j % 7 == 6 else v) for j, (c, v) in enumerate(out)]
    return list(_T2J)


def t2j_ints():
    out = []
    for k in range(19):
        out += [10 ** k, -10 ** k, 10 ** k - 1, -(10 ** k - 1)]
    for w in (8, 16, 32, 64):
        out += [(1 << (w - 1)) - 1, -(1 << (w - 1))]
    for k in range(64):
        out += [1 << k, -(1 << k), (1 << k) - 1, -((1 << k) - 1)]
    return [v for v in out if -(1 << 63) <= v < (1 << 63)]
