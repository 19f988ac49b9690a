"""CPU: the kernels' string and base64 routines themselves, built for the host
by str_host.cpp, on the corpora of strgen.py.

j2t: the exact machine's advance_string + unquote / b64decode must give the
reference's bytes and status word (code, position, value) on every item;
fast_string / fast_binary, wherever they accept, must give exactly the exact
routine's bytes, length and end position on every source kind (a message in
memory, a sub-view, an LDS-shaped source with 32-bit positions), whatever
bytes lie round the message; where they decline, the item is one they may
decline; and every branch str_class names is reached by at least 16 items --
which is what says the corpus does what strgen.py claims.

t2j: emit_quoted and emit_base64 give the reference's text, and quote_extra
counts exactly what emit_quoted adds on every word and tail, whatever bytes
lie behind the tail.

Exhaustively: hexv, hex4w and fl_hex4 on every byte at every digit position;
fl_escape, esc_in, esc_out and esc_utf8 on all 65 536 code points and all 256
escape letters; b64_4 on every byte at every position and every pair of bytes
at every pair of positions, b64_8 on every byte at its 8 positions; chunk_b64
and b64_len on every final quantum xxxx, xxx= and xx== -- against the
byte-at-a-time routines and the model.

The same file built alone with -DSTR_MAIN under ASan + UBSan runs the corpus
from heap blocks of exactly each source's length plus 16 bytes."""
import ctypes as C
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

import oracle
import strgen
import test_strings_oracle as M
from dynamicgo_amd import build as B, thrift as T

HERE = os.path.dirname(os.path.abspath(__file__))
K_MSG, K_SUB, K_LDS = range(3)
KINDS = {K_MSG: "message", K_SUB: "sub-view", K_LDS: "lds"}

U_WORD8, U_TAIL, U_MASKED = 1, 2, 4
U_J = [8 << j for j in range(8)]
U_SIMPLE, U_U1, U_U2, U_U3, U_PAIR = (1 << k for k in range(11, 16))
U_D_END, U_D_LETTER, U_D_SHORT, U_D_HEX0, U_D_LONE, U_D_HEX1, U_D_LOW = (1 << k for k in range(16, 23))
U_DECLINES = U_D_END | U_D_LETTER | U_D_SHORT | U_D_HEX0 | U_D_LONE | U_D_HEX1 | U_D_LOW
B_WANT, B_NOWANT, B_PAD1, B_PAD2, B_LOOP8, B_BREAK8, B_TAIL, B_D_ERROR, B_D_WANT, B_ESC = (1 << k for k in range(10))
B_DECLINES = B_D_ERROR | B_D_WANT | B_ESC
UNCLOSED = 0x80000000


def build_str(out, extra=()):
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-Wno-ignored-attributes", *extra, "-o", out, os.path.join(HERE, "str_host.cpp")], check=True)
    return out


class Str:
    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        p64 = C.POINTER(C.c_int64)
        lib.str_exact.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_uint64, p64]
        lib.str_fast.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint64, p64]
        lib.str_class.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int]
        lib.str_class.restype = C.c_uint32
        lib.str_quote.argtypes = [C.c_char_p, C.c_int64, C.c_char_p]
        lib.str_b64enc.argtypes = [C.c_char_p, C.c_int64, C.c_char_p]
        lib.str_hex4w.argtypes = [C.c_uint32]
        lib.str_hex4w.restype = C.c_int64
        lib.str_b64_4_many.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        lib.str_b64_8.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
        lib.str_consts.argtypes = [p64]
        self.o = (C.c_int64 * 8)()
        lib.str_consts(self.o)
        assert list(self.o)[:5] == [strgen.ERR_EOF, strgen.ERR_INVAL, strgen.ERR_ESCAPE, strgen.ERR_UNICODE, strgen.ERR_B64]
        self.cap = 1 << 18
        self.buf = C.create_string_buffer(self.cap)

    def exact(self, m, s, binary, kind=0):
        """(e or -code, length or the routine's negative result, the bytes written)"""
        self.lib.str_exact(m, len(m), s, int(binary), kind, self.buf, self.cap, self.o)
        return self.o[0], self.o[1], self.buf.raw[:self.o[2]]

    def fast(self, m, s, binary, kind, fill=0):
        """None where it declines, else (end position, the bytes written)"""
        if not self.lib.str_fast(m, len(m), s, int(binary), kind, fill, self.buf, self.cap, self.o):
            return None
        return self.o[0], self.buf.raw[:self.o[2]]

    def cls(self, m, s, binary):
        return self.lib.str_class(m, len(m), s, int(binary))

    def quote(self, b):
        n = self.lib.str_quote(b, len(b), self.buf)
        return self.buf.raw[:n]

    def b64enc(self, b):
        n = self.lib.str_b64enc(b, len(b), self.buf)
        return self.buf.raw[:n]

    def b64_4(self, words):
        ws = np.ascontiguousarray(words, dtype=np.uint32)
        out = np.zeros(len(ws), dtype=np.int64)
        self.lib.str_b64_4_many(ws.ctypes.data, len(ws), out.ctypes.data)
        return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host string routines with" % B.HIPCC)
    return Str(build_str(str(tmp_path_factory.mktemp("str") / "libstr.so"), ("-shared",)))


def corpus():
    """[(item, message, body offset, binary)]: every j2t item as the last
    value of str_desc(), strings in "str" and base64 bodies in "bin"; the
    count and long families in both."""
    out = []
    for it in M.all_j2t_items():
        for field in ("str", "bin"):
            if (it.fam in M.B64_FAMILIES) == (field == "bin") or it.fam in ("count", "long", "b64len", "b64ws"):
                m, s = M.wrap(it, field, True)
                out.append((it, m, s, field == "bin"))
    return out


@pytest.fixture(scope="module")
def items():
    return corpus()


@pytest.fixture(scope="module")
def classes(lib, items):
    return [lib.cls(m, s, b) for _, m, s, b in items]


def test_exact_routines_equal_the_reference(lib, items):
    chk = oracle.RefOracle() or oracle.PortOracle()
    fl = T.flatten(M.str_desc())
    bad = []
    for binary in (False, True):
        part = [x for x in items if x[3] == binary]
        rets, outs = chk.j2t_batch(fl, [m for _, m, _, _ in part], 0x1, nthreads=8)
        for k, ((it, m, s, _), r, o) in enumerate(zip(part, rets, outs)):
            e, l, got = lib.exact(m, s, binary, k % 3)  # the message at another alignment each time
            r = int(r)
            if e < 0:
                ok = r == (-e | s << 8 | s << 40)
            elif l < 0:
                ok = r == ((strgen.ERR_B64 | e << 8 | (-l - 1) << 40) if binary else (-l | e << 8 | s << 40))
            else:
                # the string's field as the reference wrote it: header, length, bytes; when the body closed
                # its string early the reference may fail further on, but not in this string
                want = M.model_message(it, "bin" if binary else "str", True, 0x1)
                ok = (want is None or (r == 0 and want[0] == 0)) and got[:4] == struct.pack(">i", l) and len(got) == 4 + l
                if r == 0:
                    ok = ok and o[7:7 + 7 + l] == b"\x0b" + struct.pack(">h", M.IDS["bin" if binary else "str"]) + got
            if not ok:
                bad.append((it.fam, m[:60], e, l, hex(r)))
    assert not bad, (len(bad), bad[:6])


MAY_DECLINE = """fast_string declines only where the exact machine reports an
error in the string (unclosed, or one of unquote's four error classes);
fast_binary declines only where the body holds a backslash, the exact decoder
reports an error, or the body decodes to another length than nb / 4 * 3 - pad
promised (\\r \\n inside a body whose length is a multiple of 4, "==" after
whole quanta)."""


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS.values()))
def test_fast_equals_exact_where_it_accepts(lib, items, classes, kind):
    bad, accepted = [], 0
    for (it, m, s, binary), k in zip(items, classes):
        e, l, want = lib.exact(m, s, binary)
        for fill in (0x00, 0x5C, 0x22, 0xAA):  # what lies round the message must not matter
            if kind == K_SUB and fill:
                continue
            f = lib.fast(m, s, binary, kind, fill)
            if f is not None:
                accepted += fill == 0
                if e < 0 or l < 0 or f != (e, want):
                    bad.append((it.fam, m[:60], "accepted", f[0], e, l, f[1][:20], want[:20]))
                if k & (B_DECLINES if binary else U_DECLINES) or k == UNCLOSED:
                    bad.append((it.fam, m[:60], "class says decline", hex(k)))
            else:
                if binary:
                    may = k == UNCLOSED or k & B_ESC or (k & B_D_ERROR and l < 0) or (k & B_D_WANT and l >= 0)
                else:
                    may = e < 0 or l < 0
                if not may or not (k == UNCLOSED or k & (B_DECLINES if binary else U_DECLINES)):
                    bad.append((it.fam, m[:60], "declined", hex(k), e, l))
    assert not bad, (len(bad), bad[:6])
    assert accepted * 2 > len(items), (accepted, len(items))


def test_every_branch_is_reached(lib, items, classes):
    s = Counter()
    b = Counter()
    for (it, m, _, binary), k in zip(items, classes):
        for bit in range(23):
            if k != UNCLOSED and k >> bit & 1:
                (b if binary else s)[1 << bit] += 1
    for bit in [U_WORD8, U_TAIL, U_MASKED] + U_J + [U_SIMPLE, U_U1, U_U2, U_U3, U_PAIR, U_D_LETTER, U_D_SHORT,
                                                   U_D_HEX0, U_D_LONE, U_D_HEX1, U_D_LOW]:
        assert s[bit] >= 16, ("string branch", hex(bit), dict(s))
    # a backslash as the body's last byte cannot come out of advance_string: it takes the quote with it
    # and the string goes on (the "open" items end unclosed, below)
    assert s[U_D_END] == 0
    for bit in (B_WANT, B_NOWANT, B_PAD1, B_PAD2, B_LOOP8, B_BREAK8, B_TAIL, B_D_ERROR, B_D_WANT, B_ESC):
        assert b[bit] >= 16, ("binary branch", hex(bit), dict(b))
    # each escape kind behind a backslash at each byte of the loaded word
    at = Counter((kind, j) for k in classes if k != UNCLOSED for j in range(8) if k & U_J[j]
                 for kind in (U_SIMPLE, U_U1, U_U2, U_U3, U_PAIR) if k & kind)
    for kind in (U_SIMPLE, U_U1, U_U2, U_U3, U_PAIR):
        for j in range(8):
            assert at[(kind, j)] >= 16, (hex(kind), j, at[(kind, j)])
    # a length written up front that the decoding does not keep
    assert sum(bool(k & B_D_WANT) and bool(k & B_WANT) for (_, _, _, bn), k in zip(items, classes) if bn) >= 16
    assert sum(1 for (_, _, _, bn), k in zip(items, classes) if k == UNCLOSED) >= 4


def test_emit_quoted_and_base64_give_the_reference_text(lib):
    chk = oracle.RefT2JOracle()
    fl = T.flatten(M.t2j_desc())
    side = T.flatten_t2j(fl)
    for it in strgen.t2j_strings():
        got = lib.quote(it.body)
        assert b'"' + got + b'"' == it.imp[1] == M.m_quote(it.body), it
        assert b'"' + lib.b64enc(it.body) + b'"' == M.m_b64encode(it.body), it
        if chk is not None:
            m, j0, j1 = M.t2j_messages(it)[0]
            assert chk.t2j(fl, side, m, 0) == (0, b'{"str":"' + got + b'"}'), it
    for it in strgen.t2j_binaries():
        assert b'"' + lib.b64enc(it.body) + b'"' == it.imp[1], it
        assert b'"' + lib.quote(it.body) + b'"' == M.m_quote(it.body), it
        if chk is not None:
            m, j0, j1 = M.t2j_messages(it)[0]
            assert chk.t2j(fl, side, m, 0) == (0, b'{"bin":"' + lib.b64enc(it.body) + b'"}'), it


def test_hex_digits_exhaustively(lib):
    for c in range(256):
        want = int(chr(c), 16) if chr(c) in "0123456789abcdefABCDEF" else -1
        assert lib.lib.str_hexv(c) == want, c
    for base in (b"0000", b"ffff", b"A9c3"):
        for pos in range(4):
            for c in range(256):
                d = base[:pos] + bytes([c]) + base[pos + 1:]
                want = M._hex4(d)
                assert lib.lib.str_hex4w(int.from_bytes(d, "little")) == (-1 if want is None else want), d


def _b64_want(words):
    """b64v's reading of each 4-character word: the three bytes, first lowest, or -1."""
    tab = np.full(256, -1, dtype=np.int64)
    for v, c in enumerate(strgen.B64):
        tab[c] = v
    w = np.asarray(words, dtype=np.uint32)
    s = [tab[(w >> np.uint32(8 * k)) & np.uint32(0xFF)] for k in range(4)]
    bad = (s[0] < 0) | (s[1] < 0) | (s[2] < 0) | (s[3] < 0)
    v = (s[0] << 18) | (s[1] << 12) | (s[2] << 6) | s[3]
    out = (v >> 16) | (v & 0xFF00) | ((v & 0xFF) << 16)
    return np.where(bad, -1, out)


def test_b64_swar_exhaustively(lib):
    for c in range(256):
        assert lib.lib.str_b64v(c) == (strgen.B64.index(c) if c in strgen.B64 else -1), c
    allb = np.arange(256, dtype=np.uint32)
    for base in (b"QUJD", b"+/09", b"zZaA"):
        b = np.uint32(int.from_bytes(base, "little"))
        for p in range(4):
            w = (b & ~np.uint32(0xFF << 8 * p)) | (allb << np.uint32(8 * p))
            assert (lib.b64_4(w) == _b64_want(w)).all(), (base, p)
            for q in range(p + 1, 4):  # every pair of bytes at every pair of positions
                pair = ((b & ~np.uint32((0xFF << 8 * p) | (0xFF << 8 * q))) | (allb[:, None] << np.uint32(8 * p)) |
                        (allb[None, :] << np.uint32(8 * q))).ravel()
                assert (lib.b64_4(pair) == _b64_want(pair)).all(), (base, p, q)
    o = C.c_uint64(0)
    base = int.from_bytes(b"QUJDREVG", "little")
    for p in range(8):
        for c in range(256):
            w = (base & ~(0xFF << 8 * p)) | c << 8 * p
            ok = lib.lib.str_b64_8(w, C.byref(o))
            body = w.to_bytes(8, "little")
            if all(x in strgen.B64 for x in body):
                assert ok and o.value.to_bytes(8, "little")[:6] == strgen._dec_quanta(body), body
            else:
                assert not ok, body


def test_flat_escape_table_exhaustively(lib):
    """fl_hex4 on every byte at every digit position; fl_escape, esc_in,
    esc_out and esc_utf8 on all 65 536 code points (lower and upper case) and
    all 256 escape letters, against the model: an entry where the model
    unquotes without a surrogate, none elsewhere."""
    lib.lib.str_fl_hex4.argtypes = [C.c_uint32]
    lib.lib.str_fl_hex4.restype = C.c_int64
    lib.lib.str_fl_escape_many.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    for base in (b"0000", b"ffff", b"A9c3", b"FfFf"):
        for pos in range(4):
            for c in range(256):
                d = base[:pos] + bytes([c]) + base[pos + 1:]
                want = M._hex4(d)
                assert lib.lib.str_fl_hex4(int.from_bytes(d, "little")) == (-1 if want is None else want), d
    escs = [b"\\u%04x" % cp for cp in range(65536)] + [b"\\u%04X" % cp for cp in range(65536)] + \
           [b"\\" + bytes([c]) + b"0041" for c in range(256)]
    e0 = np.array([int.from_bytes(e.ljust(8, b"\""), "little") for e in escs], dtype=np.uint64)
    for p in (0, 1, 255, 4095):
        out = np.zeros(4 * len(e0), dtype=np.uint32)
        lib.lib.str_fl_escape_many(e0.ctypes.data, len(e0), p, out.ctypes.data)
        out = out.reshape(-1, 4).tolist()
        for e, (x, nin, nout, u8) in zip(escs, out):
            take = e[:6] if e[1:2] == b"u" else e[:2]
            r = M.m_unquote(take)
            if r[0] == "ok":
                assert x not in (0, 0xFFFFFFFF) and x >> 31 and nin == len(take) and nout == len(r[1]) and \
                    u8.to_bytes(4, "little")[:nout] == r[1], (e, hex(x), nin, nout, hex(u8))
            else:
                assert x == 0, (e, hex(x))
        if p == 0:  # every surrogate declines, nothing else under \u does
            assert sum(x == 0 for x, *_ in out[:65536]) == 0x800


def test_chunk_b64_final_quanta_exhaustively(lib):
    lib.lib.str_chunk_final_mismatches.restype = C.c_uint64
    assert lib.lib.str_chunk_final_mismatches(0) == 0
    assert lib.lib.str_chunk_final_mismatches(3) == 0
    lib.lib.str_chunk_b64.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_char_p]
    lib.lib.str_b64_len.argtypes = [C.c_char_p, C.c_int64]
    lib.lib.str_b64_len.restype = C.c_int64
    buf = C.create_string_buffer(1024)
    n = 0
    for it in strgen.j2t_b64():
        b = it.body
        if len(b) % 4 or not b or b"\\" in b or b'"' in b:
            continue
        n += 1
        for fill in (0, 0x3D, 0x41):
            got = lib.lib.str_chunk_b64(b, len(b), 1, fill, buf)
            if got >= 0:  # where the chunk task accepts, the body is canonical: the promised length and the bytes
                assert it.imp == ("ok", buf.raw[:got]) and lib.lib.str_b64_len(b, len(b)) == got, it
            else:
                # it may refuse only what is no canonical padded body: an error, or \r \n / "==" oddities
                assert it.imp[0] == "err" or set(b) - set(strgen.B64 + b"=") or b.endswith(b"==") and \
                    len(it.imp[1]) != len(b) // 4 * 3 - 2, it
    assert n > 1500


def test_quote_extra_equals_what_emit_quoted_adds(lib):
    lib.lib.str_quote_extra.argtypes = [C.c_uint64, C.c_uint32]
    lib.lib.str_quote_extra.restype = C.c_uint32
    n = 0
    for it in strgen.t2j_strings() + strgen.t2j_binaries():
        b = it.body
        for i in range(0, len(b), 8):
            nb = min(8, len(b) - i)
            want = len(M.m_quote(b[i:i + nb])) - 2 - nb
            assert want == len(lib.quote(b[i:i + nb])) - nb
            for behind in (b"\x0b\x00\x05\x00\x00\x00\x22\x5c", b"\x00" * 8, b"\x5c\x22\x0a\x01\x0d\x09\x1f\x00"):
                w = int.from_bytes((b[i:i + nb] + behind)[:8], "little")
                assert lib.lib.str_quote_extra(w, nb) == want, (it, i, behind)
                n += 1
    assert n > 20000


def test_sanitizer_program_reports_nothing(tmp_path, items):
    """str_host.cpp alone with -DSTR_MAIN under ASan + UBSan: every routine on
    every item from a heap block of exactly the source's length plus 16."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s" % B.HIPCC)
    exe = build_str(str(tmp_path / "str_main"), ("-DSTR_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                                 "-fno-sanitize-recover=undefined"))
    path = tmp_path / "corpus.bin"
    n = 0
    with open(path, "wb") as fh:
        for it, m, s, binary in items:
            fh.write(struct.pack("<III", len(m), s, int(binary)) + m)
            n += 1
        for it in strgen.t2j_strings() + strgen.t2j_binaries():
            fh.write(struct.pack("<III", len(it.body), 0, 2) + it.body)
            n += 1
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        (r.returncode, r.stderr[-2000:])
    assert r.stdout.startswith("%d items" % n), r.stdout
