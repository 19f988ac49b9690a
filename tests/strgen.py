"""String and base64 corpora aimed at the seams of the string routines, built
by construction (pieces whose meaning is known, joined; fixed, no random
draws, no GPU and no reference needed to generate them).

Every item is Item(fam, body, imp, lead):

  fam   the family (below)
  body  j2t: the bytes between the quotes of a JSON string, as they stand in
        the message; t2j: the bytes of a Thrift string / binary
  imp   what the construction implies:
          ("ok", bytes)    j2t: the unquoted (or base64-decoded) bytes
          ("err", code)    j2t: the reference's error class (ERR_* below)
          ("open", code)   j2t: the body escapes its own closing quote; as the
                           message's last value it ends in `code`
          ("q", text)      t2j: the quoted text, quotes included
          ("b64", text)    t2j: the padded base64 text, quotes included
          None             the reference decides (the raw family)
  lead  spaces in front of the message (the phase family: every byte phase of
        the aligned words a source loads)

j2t string bodies (j2t_strings):
  esc    a backslash before every byte 0x00..0xFF, at the start, at the end,
         alone and doubled; a backslash as the body's last byte
  uni    \\uXXXX at the UTF-8 length edges in three hex cases; each digit
         replaced by the neighbours of the hex ranges; 0..3 digits before the
         closing quote
  sur    the four corner pairs; a high surrogate before everything that is not
         a low one; lone low surrogates
  phase  one escape of each kind after 0..16 plain bytes, before 0..8 more,
         the message shifted by 0..7 spaces
  count  0..10 escapes in one string (count_messages: over a key and two values)
  raw    every byte but '"' and '\\' raw in a body, alone and at 7, 8, 9 of 17
  long   (long_strings) the wave page's escape count at 32 766 / 32 767 /
         32 768, one escape in 33 000 bytes, escapes across scan chunks

j2t base64 bodies (j2t_b64): b64len, b64alpha, b64ws, b64bits, b64long.
Keys (key_bodies, long_keys). t2j (t2j_strings: q1, qrun, qtail, qutf;
t2j_binaries: b64e)."""
import base64
from collections import namedtuple

ERR_EOF, ERR_INVAL, ERR_ESCAPE, ERR_UNICODE, ERR_B64 = 1, 2, 3, 4, 14

Item = namedtuple("Item", "fam body imp lead")


def _it(fam, body, imp, lead=0):
    return Item(fam, bytes(body), imp, lead)


SIMPLE = {ord('"'): b'"', ord("\\"): b"\\", ord("/"): b"/", ord("b"): b"\b", ord("f"): b"\f", ord("n"): b"\n",
          ord("r"): b"\r", ord("t"): b"\t"}
HEX_NEIGHBOURS = b"/:@G`g \"\x80"


def ok(b):
    return ("ok", bytes(b))


def err(c):
    return ("err", c)


def utf8(cp):
    """UTF-8 of a code point written out (surrogates never come here)."""
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | cp >> 6, 0x80 | cp & 0x3F])
    if cp < 0x10000:
        return bytes([0xE0 | cp >> 12, 0x80 | (cp >> 6) & 0x3F, 0x80 | cp & 0x3F])
    return bytes([0xF0 | cp >> 18, 0x80 | (cp >> 12) & 0x3F, 0x80 | (cp >> 6) & 0x3F, 0x80 | cp & 0x3F])


def _esc():
    out = []
    for c in range(256):
        e = b"\\" + bytes([c])
        if c in SIMPLE:
            v = SIMPLE[c]
            out += [_it("esc", e + b"abc", ok(v + b"abc")), _it("esc", b"abc" + e, ok(b"abc" + v)),
                    _it("esc", e, ok(v)), _it("esc", e + e, ok(v + v))]
        else:
            # \u with fewer than four bytes behind it is the end of input; every other letter is no escape
            code = ERR_EOF if c == ord("u") else ERR_ESCAPE
            out += [_it("esc", e + b"abc", err(code)), _it("esc", b"abc" + e, err(code)), _it("esc", e, err(code)),
                    _it("esc", e + e, err(code))]
    for pre in (b"", b"a", b"abcdefg", b"abcdefgh", b"a\\n"):
        out.append(_it("esc", pre + b"\\", ("open", ERR_EOF)))
    return out


UNI_CPS = (0x0000, 0x007F, 0x0080, 0x07FF, 0x0800, 0xD7FF, 0xE000, 0xFFFF, 0x00E9, 0xABCD, 0xFEDC, 0x0A9F, 0xBEEF)


def _mixed(h):
    return "".join(ch.upper() if k % 2 else ch for k, ch in enumerate(h))


def _uni():
    out = []
    for cp in UNI_CPS:
        for h in sorted({"%04x" % cp, "%04X" % cp, _mixed("%04x" % cp)}):
            e = b"\\u" + h.encode()
            out += [_it("uni", e, ok(utf8(cp))), _it("uni", b"ab" + e + b"cd", ok(b"ab" + utf8(cp) + b"cd")),
                    _it("uni", e + e, ok(utf8(cp) * 2))]
    for base in (b"00e9", b"ABCD", b"09af"):
        for k in range(4):
            for c in HEX_NEIGHBOURS:
                d = base[:k] + bytes([c]) + base[k + 1:]
                # a raw quote closes the string: k digits are left behind \u, fewer than four
                code = ERR_EOF if c == ord('"') else ERR_INVAL
                out += [_it("uni", b"\\u" + d, err(code)), _it("uni", b"xy\\u" + d + b"zw", err(code))]
    for k in range(4):  # 0..3 digits before the closing quote
        out += [_it("uni", b"\\u" + b"00e9"[:k], err(ERR_EOF)), _it("uni", b"plain\\u" + b"ABCD"[:k], err(ERR_EOF))]
    return out


PAIRS = ((0xD800, 0xDC00, 0x10000), (0xD800, 0xDFFF, 0x103FF), (0xDBFF, 0xDC00, 0x10FC00), (0xDBFF, 0xDFFF, 0x10FFFF),
         (0xD83D, 0xDE00, 0x1F600))


def _sur():
    out = []
    for hi, lo, cp in PAIRS:
        assert 0x10000 + ((hi - 0xD800) << 10) + (lo - 0xDC00) == cp
        for fmt in ("\\u%04x\\u%04x", "\\u%04X\\u%04X"):
            e = (fmt % (hi, lo)).encode()
            out += [_it("sur", e, ok(utf8(cp))), _it("sur", b"a" + e + b"b", ok(b"a" + utf8(cp) + b"b")),
                    _it("sur", e + e, ok(utf8(cp) * 2))]
    for hi in (b"\\ud800", b"\\udbff", b"\\uDBFF"):
        follow = [(b"", ERR_UNICODE)]
        follow += [(b"abcdef"[:k], ERR_UNICODE) for k in range(1, 7)]         # fewer than six bytes, then no backslash
        follow += [(b"\\udc00"[:k], ERR_UNICODE) for k in range(2, 6)]        # a low one cut short by the quote
        follow += [(b"\\n", ERR_UNICODE), (b"\\nabcd", ERR_UNICODE), (b"\\\\uabcd", ERR_UNICODE),
                   (b"\\u0041", ERR_UNICODE), (b"\\ud800", ERR_UNICODE), (b"\\udbff", ERR_UNICODE),
                   (b"\\ue000", ERR_UNICODE), (b"\\udbff\\udc00", ERR_UNICODE), (b"\\Udc00", ERR_UNICODE)]
        follow += [(b"\\u" + b"dc00"[:k] + bytes([c]) + b"dc00"[k + 1:], ERR_INVAL) for k in range(4) for c in b"/:@G`g "]
        for f, code in follow:
            out += [_it("sur", hi + f, err(code)), _it("sur", b"ab" + hi + f, err(code))]
    for lo in (b"\\udc00", b"\\udfff", b"\\uDFFF"):
        for f in (b"", b"abcdef", b"\\udc00", b"\\ud800\\udc00"):
            out.append(_it("sur", lo + f, err(ERR_UNICODE)))
    return out


PHASE_KINDS = ((b"\\n", b"\n"), (b"\\u0041", b"A"), (b"\\u00e9", utf8(0xE9)), (b"\\u20ac", utf8(0x20AC)),
               (b"\\ud83d\\ude00", utf8(0x1F600)))
PLAIN = b"abcdefghijklmnopqrstuvwxyz"


def _phase():
    out = []
    for pre in range(17):
        for e, v in PHASE_KINDS:
            for tail in range(9):
                for lead in range(8):
                    out.append(_it("phase", PLAIN[:pre] + e + PLAIN[:tail].upper(), ok(PLAIN[:pre] + v + PLAIN[:tail].upper()),
                                   lead))
    return out


COUNT_ESCAPES = ((b"\\n", b"\n"), (b"\\u00e9", utf8(0xE9)), (b"\\\"", b'"'), (b"\\ud83d\\ude00", utf8(0x1F600)),
                 (b"\\t", b"\t"))


KEPT_ESCAPES = ((b"\\n", b"\n"), (b"\\u00e9", utf8(0xE9)), (b"\\t", b"\t"), (b"\\u0041", b"A"), (b"\\/", b"/"),
                (b"\\u20ac", utf8(0x20AC)))  # what the flat kernel's escape table keeps: one backslash each


def _count_body(n, salt=0, escapes=COUNT_ESCAPES):
    body, val = b"", b""
    for k in range(n):
        e, v = escapes[(k + salt) % len(escapes)]
        body += PLAIN[k:k + 1 + (k + salt) % 3] + e
        val += PLAIN[k:k + 1 + (k + salt) % 3] + v
    return body + b"z", val + b"z"


def _count():
    out = []
    for n in range(11):
        for salt in range(5):
            b, v = _count_body(n, salt)
            out.append(_it("count", b, ok(v)))
            b, v = _count_body(n, salt, KEPT_ESCAPES)
            out.append(_it("count", b, ok(v)))
        out.append(_it("count", b"\\n" * n, ok(b"\n" * n)))
    return out


def count_messages(f1="str", f2="s2"):
    """[(message, [(field name, value)], kept)]: 0..10 escapes spread over the
    key of f1 and the values of f1 and f2, every split of them between the two
    values. kept: the flat kernel's escape table holds the message -- at most
    FL_NESC = 8 backslashes, each a simple escape other than \\" and \\\\ or a
    \\u below the surrogates, none in a key. The others it must decline: more
    than 8 (9 and 10 with the kept kinds alone), an escaped key, or the mixed
    kinds (\\" and a surrogate pair among them)."""
    out = []
    for n in range(11):
        for nk in (0, 1):
            if nk > n:
                continue
            for a in sorted({0, (n - nk) // 2, n - nk}):
                for escapes in (KEPT_ESCAPES, COUNT_ESCAPES):
                    b1, v1 = _count_body(a, 1, escapes)
                    b2, v2 = _count_body(n - nk - a, 2, escapes)
                    key = (b"\\u%04x" % ord(f1[0]) + f1[1:].encode()) if nk else f1.encode()
                    m = b'{"' + key + b'":"' + b1 + b'","req":1,"' + f2.encode() + b'":"' + b2 + b'"}'
                    kept = escapes is KEPT_ESCAPES and nk == 0 and n <= 8
                    # the mixed kinds without an escape of theirs in reach are the kept kinds' own messages
                    if escapes is COUNT_ESCAPES and b'\\"' not in m and b"\\ud" not in m:
                        continue
                    out.append((m, [(f1, v1), ("req", 1), (f2, v2)], kept))
    return out


def _raw():
    out = []
    for c in range(256):
        if c in (0x22, 0x5C):
            continue
        ch = bytes([c])
        out.append(_it("raw", ch, None))
        for p in (7, 8, 9):
            out.append(_it("raw", PLAIN[:p] + ch + PLAIN[:16 - p], None))
    return out


_J2T = None


def j2t_strings():
    global _J2T
    if _J2T is None:
        _J2T = _esc() + _uni() + _sur() + _phase() + _count() + _raw()
    return list(_J2T)


LONG_HDR = 16  # len('{"req":1,"str":"'): the body's offset in the message the long family is laid out for


def long_strings():
    out = [_it("long", b"\\n" * 16383, ok(b"\n" * 16383)), _it("long", b"\\n" * 16383 + b"x", ok(b"\n" * 16383 + b"x")),
           _it("long", b"\\n" * 16384, ok(b"\n" * 16384)),
           _it("long", b"p" * 20000 + b"\\u00e9" + b"q" * 12994, ok(b"p" * 20000 + utf8(0xE9) + b"q" * 12994))]
    # the backslash at message offsets 248..260 and 504..516: every lane seam round a 256-byte scan chunk's end
    for at in list(range(248, 261)) + list(range(504, 517)):
        for e, v in ((b"\\n", b"\n"), (b"\\u00e9", utf8(0xE9)), (b"\\ud83d\\ude00", utf8(0x1F600))):
            pre = b"k" * (at - LONG_HDR)
            out.append(_it("long", pre + e + b"tail", ok(pre + v + b"tail")))
    return out


# ------------------------------------------------------------- keys ----

def key_bodies():
    """esc / uni / sur items that can stand as an object key: the body closes
    its own string (no raw quote, not open)."""
    out = []
    for it in _esc() + _uni() + _sur():
        if it.imp[0] == "open" or _has_raw_quote(it.body):
            continue
        out.append(Item("keys", it.body, it.imp, 0))
    return out


def _has_raw_quote(body):
    i = 0
    while i < len(body):
        if body[i] == 0x5C:
            i += 2
            continue
        if body[i] == 0x22:
            return True
        i += 1
    return False


def long_keys():
    """Escaped keys of unquoted length 1023, 1024, 1025 and 2048 (WS_KEYCAP is 1024)."""
    out = []
    for n in (1023, 1024, 1025, 2048):
        for e, v in ((b"\\u006b", b"k"), (b"\\n", b"\n"), (b"\\u00e9", utf8(0xE9))):
            fill = n - len(v)
            for at in (0, fill // 2, fill):
                out.append(_it("keys", b"k" * at + e + b"k" * (fill - at), ok(b"k" * at + v + b"k" * (fill - at))))
    return out


# ----------------------------------------------------------- base64 ----

B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def payload(n, salt=0):
    return bytes((k * 37 + salt * 101 + 11) & 0xFF for k in range(n))


def enc(b):
    return base64.b64encode(b)


def _dec_quanta(body):
    """Decoding of whole alphabet quanta, written out."""
    assert len(body) % 4 == 0
    out = bytearray()
    for k in range(0, len(body), 4):
        v = 0
        for c in body[k:k + 4]:
            v = v << 6 | B64.index(c)
        out += bytes([v >> 16, (v >> 8) & 0xFF, v & 0xFF])
    return bytes(out)


def _b64len():
    out = []
    alpha = (B64[17:] + B64)[:24]
    for n in range(25):
        body = alpha[:n]
        out.append(_it("b64len", body, ok(_dec_quanta(body)) if n % 4 == 0 else err(ERR_B64)))  # unpadded: an error
        c = enc(payload(n, 1))
        out.append(_it("b64len", c, ok(payload(n, 1))))
        if c.endswith(b"="):
            out.append(_it("b64len", c[:-1], err(ERR_B64)))  # one '=' short
        out.append(_it("b64len", c + b"=", err(ERR_B64)))    # one too many
    for b in (b"=", b"===", b"====", b"A===", b"AA=A", b"AAA=A", b"=AAA", b"A=AA", b"QQ==QUJD", b"QUI=QUJD", b"QQ==QQ==",
              b"QUJDQQ==QUJD", b"==", b"QUJD=", b"QUJD===", b"QUJD===="):
        out.append(_it("b64len", b, err(ERR_B64)))
    # "==" after whole quanta: the reference's decode_block takes it as a quantum of no characters and
    # steps its output pointer back by one (native/base64.c:643-655)
    out.append(_it("b64len", b"QUJD==", ok(b"AB")))
    out.append(_it("b64len", b"QUJDREVG==", ok(b"ABCDE")))
    return out


def _b64alpha():
    out = []
    for base, positions in ((b"QUJDREVG", range(8)), (b"QUJDREVGSElK", range(8, 12))):
        for p in positions:
            for c in range(256):
                if c == 0x22 or (c == 0x5C and p == len(base) - 1):
                    continue  # a raw quote ends the body; a last backslash opens it
                body = base[:p] + bytes([c]) + base[p + 1:]
                if c in B64 or (c == ord("=") and p == len(base) - 1):
                    imp = ok(base64.b64decode(body))
                else:
                    imp = err(ERR_B64)  # \r \n: skipped, and 7 (or 11) characters are left
                out.append(_it("b64alpha", body, imp))
    return out


def _b64ws():
    out = []
    base = b"QUJDREVGSElK"
    for ws in (b"\r", b"\n", b"\r\n", b"\n\n"):
        for p in range(13):
            body = base[:p] + ws + base[p:]
            # skipped inside; at the very end no character follows it and the last block is empty: an error
            out.append(_it("b64ws", body, ok(b"ABCDEFHIJ") if p < 12 else err(ERR_B64)))
    for e in (b"\\r", b"\\n"):  # a JSON escape is never unquoted before decoding: '\\' is no base64 character
        for p in range(13):
            out.append(_it("b64ws", base[:p] + e + base[p:], err(ERR_B64)))
    for n in (1, 2, 3, 4, 5, 6, 7, 8):
        c = enc(payload(n, 2))
        for k in range(1, 5):
            for p in range(len(c)):
                ws = (b"\n\r" * 2)[:k]
                # the two '=' are read one right after the other: nothing may stand between them
                between = c[p - 1:p + 1] == b"=="
                out.append(_it("b64ws", c[:p] + ws + c[p:], err(ERR_B64) if between else ok(payload(n, 2))))
            out.append(_it("b64ws", c + (b"\n\r" * 2)[:k], err(ERR_B64)))
        if c.endswith(b"="):
            out.append(_it("b64ws", c[:-1] + b"\n=", err(ERR_B64) if c.endswith(b"==") else ok(payload(n, 2))))
            out.append(_it("b64ws", c[:-1] + b"\n", err(ERR_B64)))  # the length says canonical, the characters do not
    for b in (b"QUJ\n", b"QU\n\n", b"QUJDQUJ\n", b"QUJDQ\n==", b"Q\n\n\n", b"\n\n\n\n", b"QUJDQQ=\n="):
        out.append(_it("b64ws", b, err(ERR_B64)))
    return out


def _b64bits():
    out = []
    for a in (0, 16, 37, 63):
        for b in range(64):
            out.append(_it("b64bits", bytes([B64[a], B64[b]]) + b"==", ok(bytes([(a << 2 | b >> 4) & 0xFF]))))
            out.append(_it("b64bits", b"QUJD" + bytes([B64[a], B64[a ^ 5], B64[b]]) + b"=",
                           ok(b"ABC" + bytes([(a << 2 | (a ^ 5) >> 4) & 0xFF, ((a ^ 5) << 4 | b >> 2) & 0xFF]))))
    return out


def _b64long():
    out = []
    lens = list(range(248, 273, 4)) + [508, 512, 516]
    for nb in lens:
        for pad in (0, 1, 2):
            p = payload(nb // 4 * 3 - pad, nb)
            c = enc(p)
            assert len(c) == nb
            out.append(_it("b64long", c, ok(p)))
            for at in (0, 15, 16, 127, 128, nb - 17, nb - 16, nb - 5, nb - 4, nb - 1):
                if c[at] != ord("="):  # the last character of the last chunk task where it is no padding
                    out.append(_it("b64long", c[:at] + b"*" + c[at + 1:], err(ERR_B64)))
            for at in (15, 128, nb - 17):
                out.append(_it("b64long", c[:at] + b"=" + c[at + 1:], err(ERR_B64)))
            out.append(_it("b64long", c[:131] + b"\n" + c[131:], ok(p)))
    for n in list(range(5, 11)) + list(range(29, 36)) + [47, 48, 49, 71, 72, 73]:
        p = payload(n, n)
        c = enc(p)
        out.append(_it("b64long", c, ok(p)))
        for at in (0, 7, 8, 31, 32, 33, len(c) - 5, len(c) - 4, len(c) - 3, len(c) - 1):
            if 0 <= at < len(c) and c[at] != ord("="):
                out.append(_it("b64long", c[:at] + b"_" + c[at + 1:], err(ERR_B64)))
        for at in (3, 8, 31, 32):
            if at < len(c) - 4:
                out.append(_it("b64long", c[:at] + b"=" + c[at + 1:], err(ERR_B64)))
    return out


_B64 = None


def j2t_b64():
    global _B64
    if _B64 is None:
        _B64 = _b64len() + _b64alpha() + _b64ws() + _b64bits() + _b64long()
    return list(_B64)


# -------------------------------------------------------------- t2j ----

ONE_EXTRA = {0x22: b'\\"', 0x5C: b"\\\\", 0x09: b"\\t", 0x0A: b"\\n", 0x0D: b"\\r"}


def qbyte(c):
    """What one byte becomes inside the quotes: two bytes for '"' '\\' \\t \\n
    \\r, \\u00XX for the other bytes under 0x20, itself otherwise."""
    if c in ONE_EXTRA:
        return ONE_EXTRA[c]
    if c < 0x20:
        return b"\\u00" + b"0123456789abcdef"[c >> 4:(c >> 4) + 1] + b"0123456789abcdef"[c & 15:(c & 15) + 1]
    return bytes([c])


def _q(fam, pieces):
    """pieces: bytes taken as plain (no byte of them escapes) or ints."""
    raw, text = bytearray(), bytearray()
    for p in pieces:
        if isinstance(p, int):
            raw.append(p)
            text += qbyte(p)
        else:
            assert not any(c < 0x20 or c in (0x22, 0x5C) for c in p)
            raw += p
            text += p
    return _it(fam, raw, ("q", b'"' + bytes(text) + b'"'))


FIVE = (0x00, 0x01, 0x08, 0x0B, 0x0C, 0x1F, 0x10, 0x07)
ONE = (0x22, 0x5C, 0x09, 0x0A, 0x0D)


def _q1():
    out = []
    for c in range(256):
        out.append(_q("q1", [c]))
        for p in range(16):
            out.append(_q("q1", [PLAIN[:p], c, PLAIN[:15 - p].upper()]))
    return out


def _qrun():
    out = []
    esc = list(ONE) + list(FIVE)
    for n in range(25):
        out.append(_q("qrun", [esc[(k * 5 + n) % len(esc)] for k in range(n)]))
        out.append(_q("qrun", [ONE[(k + n) % 5] for k in range(n)]))
        out.append(_q("qrun", [FIVE[(k + n) % 8] for k in range(n)]))
    for kind in (ONE, FIVE):
        for k in range(9):
            for rot in range(8):  # the k escaping bytes at rotating places of the word
                w = [kind[(j + rot) % len(kind)] if (j * 3 + rot) % 8 < k else b"w" for j in range(8)]
                out.append(_q("qrun", w))
                out.append(_q("qrun", [b"pq"] + w + [b"rst"]))
    return out


QTAIL_NEXT = (0x22, 0x5C, 0x0A, 0x01)  # the length of the string field that follows in the message


def _qtail():
    return [_q("qtail", [PLAIN[:n] if k % 2 else PLAIN[:n].upper()]) for n in range(1, 16) for k in range(2)]


def _qutf():
    out = []
    for b in (b"\x7f", b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"<>&", b"</script>", b"\x80", b"\xff", b"\xc0\x80", b"\xed\xa0\x80",
              b"\xf4\x90\x80\x80", b"\xe2\x80", b"\xc3", "é€😀".encode(), b"\xfe\xff", b"\xf8\x88\x80\x80\x80"):
        for pre in (0, 3, 7, 8):
            out.append(_it("qutf", PLAIN[:pre] + b + b"z", ("q", b'"' + PLAIN[:pre] + b + b'z"')))
    return out


_T2J = None


def t2j_strings():
    global _T2J
    if _T2J is None:
        _T2J = _q1() + _qrun() + _qtail() + _qutf()
    return list(_T2J)


def _enc_written_out(b):
    out = bytearray()
    for k in range(0, len(b), 3):
        q = b[k:k + 3]
        v = int.from_bytes(q + bytes(3 - len(q)), "big")
        s = bytes([B64[v >> 18], B64[(v >> 12) & 63], B64[(v >> 6) & 63], B64[v & 63]])
        out += s[:len(q) + 1] + b"=" * (3 - len(q))
    return bytes(out)


def t2j_binaries():
    out = []
    for n in range(41):
        out.append(payload(n, 3))
    allb = bytes(range(256))
    for n in (11, 12, 13, 23, 24, 25, 35, 36, 37):
        for a in range(0, 256, n):
            out.append((allb + allb)[a:a + n])
    for pos in range(4):  # every sextet value in each character position
        for s in range(64):
            sh = 18 - 6 * pos
            v3 = (s << sh | (0x2A5A5A & ~(63 << sh))).to_bytes(3, "big")
            out += [b"xyz" + v3, v3[:1], v3[:2]]  # in a whole quantum and in the two padded ones
    return [_it("b64e", b, ("b64", b'"' + _enc_written_out(b) + b'"')) for b in out]


def thin(items, keep, every):
    """items with the families of `every` ({family: step}) cut to one in step; `keep` families untouched."""
    seen, out = {}, []
    for it in items:
        k = seen.get(it.fam, 0)
        seen[it.fam] = k + 1
        if it.fam in keep or k % every.get(it.fam, 1) == 0:
            out.append(it)
    return out
