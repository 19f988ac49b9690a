"""CPU: the kernels' number routines themselves, built for the host by
num_host.cpp, on the corpora of numgen.py.

j2t: the exact machine's vnumber (atof_native behind it) must give the
reference's and Python's bits on every token; fast_vnumber, wherever it
accepts, must give the exact machine's result on every source kind (a token in
a message, a sub-view, the wave kernel's and the flat kernel's register
sources); where it declines, the token is one it may decline; and every branch
num_class reports is reached by enough tokens -- which is what says the corpus
does what numgen.py claims, seam exponents included.

t2j: emit_f64 / emit_i64 must give the reference's text on the whole corpus,
and repr()'s digits and a float() round trip on a million more doubles."""
import ctypes as C
import math
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

import numgen
import oracle
from dynamicgo_amd import build as B
from test_numbers_oracle import JSON_NUMBER, parse_all, ref_f64_texts, ref_i64_texts

HERE = os.path.dirname(os.path.abspath(__file__))
K_MSG, K_SUB, K_RSRC, K_RSRCL = range(4)
KINDS = {K_MSG: "message", K_SUB: "sub-view", K_RSRC: "RSrc", K_RSRCL: "RSrcL"}
R_ERR, R_INT_REGS, R_DEC_REGS, R_INT_LOOP, R_DBL_LOOP = range(5)
C_NONE, C_EXACT, C_EL_WINDOW, C_EL_TABLE, C_EL_FAIL, C_TRUNC = range(6)
INF = float("inf")


def build_num(out, extra=()):
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-Wno-ignored-attributes", *extra, "-o", out, os.path.join(HERE, "num_host.cpp")], check=True)
    return out


class Num:
    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        p64 = C.POINTER(C.c_int64)
        lib.num_fast.argtypes = [C.c_char_p, C.c_int, C.c_int, p64]
        lib.num_class.argtypes = [C.c_char_p, C.c_int, p64]
        lib.num_exact.argtypes = [C.c_char_p, C.c_int, C.c_int, p64]
        lib.num_f64toa.argtypes = [C.c_uint64, C.c_char_p]
        lib.num_i64toa.argtypes = [C.c_int64, C.c_char_p]
        lib.num_f64toa_many.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.num_consts.argtypes = [p64]
        self.o = (C.c_int64 * 8)()
        lib.num_consts(self.o)
        self.V_INTEGER, self.V_DOUBLE, self.E_EOF, self.E_INVAL, self.E_FLOAT_INF = list(self.o)[:5]
        self.buf = C.create_string_buffer(64)

    def fast(self, tok, kind):
        """None when the kind does not take the token, else (accepted, isint, iv, bits, end)."""
        if self.lib.num_fast(tok, len(tok), kind, self.o) < 0:
            return None
        o = self.o
        return bool(o[0]), bool(o[1]), o[2], o[3] & (2**64 - 1), o[4]

    def cls(self, tok):
        """(route, conversion, exp10, accepted, mantissa)"""
        self.lib.num_class(tok, len(tok), self.o)
        o = self.o
        return o[0], o[1], o[2], bool(o[3]), o[4] & (2**64 - 1)

    def exact(self, tok, framed):
        """(vt, iv, bits, end)"""
        self.lib.num_exact(tok, len(tok), int(framed), self.o)
        o = self.o
        return o[0], o[1], o[2] & (2**64 - 1), o[3]

    def f64toa(self, v):
        n = self.lib.num_f64toa(numgen.f2b(v), self.buf)
        return self.buf.raw[:n].decode()

    def i64toa(self, v):
        n = self.lib.num_i64toa(v, self.buf)
        return self.buf.raw[:n].decode()

    def f64toa_many(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        buf = np.zeros(32 * len(bits), dtype=np.uint8)
        lens = np.zeros(len(bits), dtype=np.uint8)
        self.lib.num_f64toa_many(bits.ctypes.data, len(bits), buf.ctypes.data, lens.ctypes.data)
        raw = buf.tobytes()
        return [raw[32 * k:32 * k + int(lens[k])].decode() for k in range(len(bits))]


@pytest.fixture(scope="module")
def num(tmp_path_factory):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host number routines with" % B.HIPCC)
    return Num(build_num(str(tmp_path_factory.mktemp("num") / "libnum.so"), ("-shared",)))


@pytest.fixture(scope="module")
def tokens():
    return [(c, t.encode()) for c, t in numgen.j2t_tokens()]


@pytest.fixture(scope="module")
def classes(num, tokens):
    return [num.cls(t) for _, t in tokens]


def test_exact_machine_equals_python_and_reference(num, tokens):
    chk = oracle.RefOracle() or oracle.PortOracle()
    ref = parse_all(chk, [t.decode() for _, t in tokens])
    bad = []
    for (c, t), (r, o) in zip(tokens, ref):
        vt, iv, bits, end = num.exact(t, True)
        got = struct.pack(">Q", bits)
        whole = vt >= 0 and end == len(t)
        if JSON_NUMBER.match(t.decode()):
            want = float(t)
            if want in (INF, -INF):
                ok = vt == -num.E_FLOAT_INF
            else:
                ok = whole and got == struct.pack(">d", want)
            if not ok:
                bad.append((c, t[:50], vt, got.hex()))
        if (r == 0) != whole or (r == 0 and got != o):
            bad.append((c, t[:50], vt, end, hex(r), got.hex(), o and o.hex()))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS.values()))
def test_fast_equals_exact_where_it_accepts(num, tokens, classes, kind):
    bad, taken, accepted = [], 0, 0
    for (c, t), k in zip(tokens, classes):
        f = num.fast(t, kind)
        if f is None:
            assert len(t) > 24
            continue
        taken += 1
        ok, isint, iv, bits, end = f
        if ok:
            accepted += 1
            vt, eiv, ebits, eend = num.exact(t, kind == K_MSG)
            if vt < 0 or isint != (vt == num.V_INTEGER) or (isint and iv != eiv) or bits != ebits or end != eend:
                bad.append((c, t[:50], f, (vt, eiv, ebits, eend)))
        else:
            # may decline: Eisel-Lemire gave up, the truncated mantissa is ambiguous, or not a number
            if not (k[1] in (C_EL_FAIL, C_TRUNC) or k[0] == R_ERR):
                bad.append((c, t[:50], "declined", k))
        if kind != K_MSG and ok != k[3]:  # a message's token may be followed by more; the others are the class's own view
            bad.append((c, t[:50], "class says", k, "fast says", ok))
    assert not bad, (len(bad), bad[:6])
    short = sum(len(t) <= 24 for _, t in tokens)  # what a register source holds
    assert taken == (len(tokens) if kind in (K_MSG, K_SUB) else short) and short * 2 > len(tokens)
    assert accepted * 4 >= taken * 3, (taken, accepted)


def test_every_branch_is_reached(num, tokens, classes):
    route = Counter(k[0] for k in classes)
    conv = Counter(k[1] for k in classes)
    for r in (R_ERR, R_INT_REGS, R_DEC_REGS, R_INT_LOOP, R_DBL_LOOP):
        assert route[r] >= 16, ("route", r, route)
    for v in (C_EXACT, C_EL_WINDOW, C_EL_TABLE, C_EL_FAIL, C_TRUNC):
        assert conv[v] >= 16, ("conversion", v, conv)
    # both sides of both seams of the window [EL_WLO, EL_WLO + EL_WN) = [-40, 24)
    at = Counter((k[1], k[2]) for k in classes)
    for c, e in ((C_EL_TABLE, -41), (C_EL_WINDOW, -40), (C_EL_WINDOW, 23), (C_EL_TABLE, 24)):
        assert at[(c, e)] >= 16, (c, e, at[(c, e)])
    assert not any(k[1] == C_EL_WINDOW and not -40 <= k[2] < 24 for k in classes)
    assert not any(k[1] == C_EL_TABLE and -40 <= k[2] < 24 and len(t) <= 24 for k, (_, t) in zip(classes, tokens))
    # Eisel-Lemire's failures: out of its table, and inside it (the ambiguous products)
    assert sum(k[1] == C_EL_FAIL and -348 <= k[2] <= 347 for k in classes) >= 16
    assert sum(k[1] == C_EL_FAIL and not -348 <= k[2] <= 347 for k in classes) >= 16
    # atof_exact's two multiplies and its division
    assert sum(k[1] == C_EXACT and k[2] > 22 for k in classes) >= 16
    assert sum(k[1] == C_EXACT and 0 < k[2] <= 22 for k in classes) >= 16
    assert sum(k[1] == C_EXACT and k[2] < 0 for k in classes) >= 16
    # fast_dec_regs: every point position of every length, both signs
    shapes = {(len(t), t.index(b"."), t[:1] == b"-") for k, (_, t) in zip(classes, tokens) if k[0] == R_DEC_REGS}
    for neg in (False, True):
        for total in range(3, 21):  # digits and the point; 19 digits at the most
            for pd in range(1, total - 1):
                assert (total + neg, pd + neg, neg) in shapes, (total, pd, neg)


def test_seam_tokens_land_on_their_exponents(num):
    """numgen's arithmetic: the parser's exponent next to the mantissa is the
    one the token was built for."""
    for t, e in numgen.seam_cases():
        k = num.cls(t.encode())
        assert k[0] in (R_DEC_REGS, R_DBL_LOOP) and k[2] == e, (t, e, k)


def test_elfail_tokens_fail(num, tokens, classes):
    """The elfail class leaves the fast path both ways: through Eisel-Lemire's
    own refusal (a tie whose even neighbour is below: rounding up would be
    wrong) and through the mantissa + 1 disagreement. A tie whose even
    neighbour is above is accepted, rightly (rounding up is what it does), and
    an integer that fits int64 is an integer first."""
    n = Counter()
    for (c, t), k in zip(tokens, classes):
        if c == "elfail":
            n["int" if k[0] in (R_INT_REGS, R_INT_LOOP) else k[1]] += 1
    assert n[C_EL_FAIL] >= 16 and n[C_TRUNC] >= 16 and n["int"] >= 16, n
    assert n[C_EL_FAIL] + n[C_TRUNC] + n["int"] >= sum(n.values()) * 3 // 4, n


def test_toa_equals_reference(num):
    vals = [v for _, v in numgen.t2j_doubles()]
    got = num.f64toa_many([numgen.f2b(v) for v in vals])
    chk = oracle.RefT2JOracle()
    if chk is not None:
        want = ref_f64_texts(chk, vals)
        bad = [(v.hex(), g, w) for v, g, w in zip(vals, got, want) if g != w]
        assert not bad, (len(bad), bad[:6])
    for v, g in zip(vals, got):
        assert numgen.f2b(float(g)) == numgen.f2b(v) and numgen.sig_digits(g) == numgen.sig_digits(repr(v)), (v.hex(), g)
        assert num.f64toa(v) == g
    ints = numgen.t2j_ints()
    got = [num.i64toa(v) for v in ints]
    assert got == [str(v) for v in ints]
    if chk is not None:
        assert got == ref_i64_texts(chk, ints)


N_EXTRA = 1000000


def test_f64toa_on_a_million_doubles(num):
    """Seeded random bit patterns, half of them with the low 1..52 fraction
    bits cleared (short digit strings, powers of two, integers): repr()'s
    digits and a float() round trip."""
    rng = np.random.default_rng(20240607)
    bits = rng.integers(0, 1 << 64, size=N_EXTRA, dtype=np.uint64)
    clear = rng.integers(1, 53, size=N_EXTRA // 2, dtype=np.uint64)
    bits[:N_EXTRA // 2] &= ~((np.uint64(1) << clear) - np.uint64(1))
    bits = bits[((bits >> np.uint64(52)) & np.uint64(0x7FF)) != np.uint64(0x7FF)]
    texts = num.f64toa_many(bits)
    vals = bits.view(np.float64).tolist()
    sig = numgen.sig_digits
    bad = [(v.hex(), t) for v, t in zip(vals, texts)
           if float(t) != v or sig(t) != sig(repr(v)) or (t[0] == "-") != (math.copysign(1.0, v) < 0)]
    assert not bad, (len(bad), bad[:6])
    assert len(vals) > N_EXTRA * 0.99
