"""CPU: the string corpora of strgen.py against the compiled reference
(oracle/_ref), its C restatement (PortOracle) and a plain byte-at-a-time
Python model of the reference's unquote / quote / b64decode / b64encode
(written from native/parsing.c and native/base64.c, not from the kernels).
The corpus is only useful on the GPU if its expected values are beyond doubt,
so here every item's stated implication must hold in the model, the model
must give the reference's bytes and status words through the j2t / t2j entry
points (a STRING or binary field of a small struct, a map, a list, a STRING
root), the restatement must equal the reference, and well-formed canonical
items must mean what json and base64 say they mean."""
import base64
import json
import struct
from collections import Counter

import pytest

import oracle
import strgen
from strgen import ERR_B64, ERR_EOF, ERR_ESCAPE, ERR_INVAL, ERR_UNICODE
from dynamicgo_amd import thrift as T

F_STR, F_NOB64, F_UTF8 = 0x1, 0x41, 0x1 | 1 << 16
NOB64_T2J = 1 << 3
IDS = {"b": 1, "str": 2, "bin": 3, "s2": 4, "req": 5, "pad": 6}


def str_desc():
    """A flat struct (the flat kernel takes it) with two strings, a binary and a pad."""
    return T.struct_type("S", [
        T.FieldDescriptor(1, "b", T.builtin("bool"), T.OPTIONAL),
        T.FieldDescriptor(2, "str", T.builtin("string"), T.OPTIONAL),
        T.FieldDescriptor(3, "bin", T.builtin("binary"), T.OPTIONAL),
        T.FieldDescriptor(4, "s2", T.builtin("string"), T.OPTIONAL),
        T.FieldDescriptor(5, "req", T.builtin("i32"), T.REQUIRED),
        T.FieldDescriptor(6, "pad", T.builtin("string"), T.OPTIONAL),
    ])


def cont_desc():
    return T.struct_type("C", [
        T.FieldDescriptor(1, "ms", T.map_of(T.builtin("string"), T.builtin("string")), T.OPTIONAL),
        T.FieldDescriptor(2, "ls", T.list_of(T.builtin("string")), T.OPTIONAL),
        T.FieldDescriptor(3, "lb", T.list_of(T.builtin("binary")), T.OPTIONAL),
        T.FieldDescriptor(4, "str", T.builtin("string"), T.OPTIONAL),
    ])


# ---------------------------------------------------------------- model ----

UNQ = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13,
       ord("t"): 9}  # _UnquoteTab, 'u' apart
HEXD = b"0123456789abcdefABCDEF"


def m_scan(m, s):
    """advance_string: the offset just past the closing quote of the string
    whose body starts at m[s], or None (the input ends first). A backslash
    takes the next byte with it, whatever it is."""
    i = s
    while i < len(m):
        if m[i] == 0x22:
            return i + 1
        i += 2 if m[i] == 0x5C else 1
    return None


def _hex4(b):
    return int(b, 16) if len(b) == 4 and all(c in HEXD for c in b) else None


def m_unquote(b):
    """unquote (native/parsing.c:702-945, flags 0): ("ok", bytes) or ("err", code)."""
    out = bytearray()
    i, n = 0, len(b)
    while i < n:
        if b[i] != 0x5C:
            out.append(b[i])
            i += 1
            continue
        i += 2
        if i > n:
            return ("err", ERR_EOF)
        c = b[i - 1]
        if c in UNQ:
            out.append(UNQ[c])
            continue
        if c != ord("u"):
            return ("err", ERR_ESCAPE)
        if n - i < 4:
            return ("err", ERR_EOF)
        r0 = _hex4(b[i:i + 4])
        if r0 is None:
            return ("err", ERR_INVAL)
        i += 4
        if r0 < 0xD800 or r0 > 0xDFFF:
            out += strgen.utf8(r0)
            continue
        if n - i < 6 or r0 > 0xDBFF or b[i:i + 2] != b"\\u":
            return ("err", ERR_UNICODE)
        r1 = _hex4(b[i + 2:i + 6])
        if r1 is None:
            return ("err", ERR_INVAL)
        i += 6
        if r1 < 0xDC00 or r1 > 0xDFFF:
            return ("err", ERR_UNICODE)
        out += strgen.utf8(((r0 - 0xD800) << 10) + (r1 - 0xDC00) + 0x10000)
    return ("ok", bytes(out))


def _block(b, ip, out):
    """decode_block (native/base64.c:539-657) at b[ip]: (0, new ip) or (the
    error position + 1 relative to ip, ip reached)."""
    ie, p, nb, v = len(b), ip, 0, 0
    while nb < 4 and p < ie:
        ch = b[p]
        if ch in (13, 10):
            p += 1
            continue
        if ch not in strgen.B64:
            break
        v = v << 6 | strgen.B64.index(ch)
        p += 1
        nb += 1
    if nb == 1:
        return p - ip + 1, p
    if nb < 4:
        if p == ie:
            return p - ip + 1, p
        if nb == 3:
            p += 1
            if b[p - 1] != 0x3D:
                return p - ip, p
        else:
            if p >= ie - 1:
                return p - ip + 1, p
            for _ in range(2):
                p += 1
                if b[p - 1] != 0x3D:
                    return p - ip, p
        if p < ie:
            return p - ip + 1, p
        v <<= 6 * (4 - nb)
    if nb >= 2:
        out += bytes([v >> 16 & 0xFF, v >> 8 & 0xFF, v & 0xFF])[:nb - 1]
    elif out:
        del out[-1:]  # no character before "==": the output pointer steps back by one
    else:
        out.append(-1)  # marker: length -1 (nothing to step back over)
    return 0, p


def m_b64decode(b):
    """b64decode, mode 0 (native/base64.c:659-817): ("ok", bytes) or ("err",
    ERR_B64, the value the status word carries: -l - 1)."""
    if not b:
        return ("ok", b"")
    out, ip = [], 0
    while ip < len(b):
        q = b[ip:ip + 4]
        if len(q) == 4 and all(c in strgen.B64 for c in q):
            v = 0
            for c in q:
                v = v << 6 | strgen.B64.index(c)
            out += [v >> 16, v >> 8 & 0xFF, v & 0xFF]
            ip += 4
            continue
        dv, p = _block(b, ip, out)
        if dv:
            l = 0 - ip - dv  # ib - ip - dv with ip as decode_block found it (it advances only on success)
            return ("err", ERR_B64, -l - 1)
        ip = p
    if out == [-1]:
        return ("err", ERR_B64, 0)
    return ("ok", bytes(out))


def m_quote(b):
    """quote (native/parsing.c:487, _SingleQuoteTab) with the quotes round it."""
    out = bytearray(b'"')
    for c in b:
        if c == 0x22 or c == 0x5C:
            out += bytes([0x5C, c])
        elif c == 9:
            out += b"\\t"
        elif c == 10:
            out += b"\\n"
        elif c == 13:
            out += b"\\r"
        elif c < 0x20:
            out += b"\\u%04x" % c
        else:
            out.append(c)
    return bytes(out + b'"')


def m_b64encode(b):
    out = bytearray(b'"')
    for k in range(0, len(b), 3):
        q = b[k:k + 3]
        v = int.from_bytes(q.ljust(3, b"\0"), "big")
        four = [strgen.B64[v >> 18], strgen.B64[v >> 12 & 63], strgen.B64[v >> 6 & 63], strgen.B64[v & 63]]
        out += bytes(four[:len(q) + 1]) + b"=" * (3 - len(q))
    return bytes(out + b'"')


def first_bad_utf8(b):
    try:
        b.decode("utf-8")
        return -1
    except UnicodeDecodeError as e:
        return e.start


# ------------------------------------------------------- the messages ----

PAD = b'"pad":"' + b"p" * 600 + b'",'


def wrap(it, field, last, pad=False):
    """(message, offset of the body): the item as `field` of str_desc(), as
    the last value (before '}') or the first (before ',')."""
    head = b" " * it.lead + b"{" + (PAD if pad else b"")
    if last:
        head += b'"req":1,"' + field.encode() + b'":"'
        return head + it.body + b'"}', len(head)
    head += b'"' + field.encode() + b'":"'
    return head + it.body + b'","req":2}', len(head)


def tfield(name, data):
    if name == "req":
        return b"\x08" + struct.pack(">hi", IDS[name], data)
    return b"\x0b" + struct.pack(">hi", IDS[name], len(data)) + data


def model_message(it, field, last, flags, pad=False):
    """(status, thrift) the model says the reference gives, or None where the
    body closes its string elsewhere than at its end and goes on to succeed
    (what follows is then no longer the item)."""
    m, s = wrap(it, field, last, pad)
    e = m_scan(m, s)
    if e is None:
        return ERR_EOF | s << 8 | s << 40, b""
    seen = m[s:e - 1]
    binary = field == "bin" and not flags & 0x40
    if flags & (1 << 16) and not binary:
        bad = first_bad_utf8(seen)
        if bad >= 0:
            return ERR_INVAL | (s + bad) << 8 | seen[bad] << 40, b""
    r = m_b64decode(seen) if binary else m_unquote(seen)
    if r[0] == "err":
        return r[1] | e << 8 | (r[2] if binary else s) << 40, b""
    if e - 1 != s + len(it.body):
        return None
    padf = tfield("pad", b"p" * 600) if pad else b""
    if last:
        return 0, padf + tfield("req", 1) + tfield(field, r[1]) + b"\x00"
    return 0, padf + tfield(field, r[1]) + tfield("req", 2) + b"\x00"


def implied(it, binary):
    """The model on the body as a string sees it, in the terms of strgen's implications."""
    m = it.body + b'"'
    e = m_scan(m, 0)
    if e is None:
        return ("open", ERR_EOF)
    r = m_b64decode(m[:e - 1]) if binary else m_unquote(m[:e - 1])
    return r[:2]


# ---------------------------------------------------------------- tests ----

J2T_FAMILIES = {"esc", "uni", "sur", "phase", "count", "raw"}
B64_FAMILIES = {"b64len", "b64alpha", "b64ws", "b64bits", "b64long"}
T2J_FAMILIES = {"q1", "qrun", "qtail", "qutf"}


def test_corpus_families_are_populated():
    n = Counter(it.fam for it in strgen.j2t_strings())
    assert set(n) == J2T_FAMILIES and all(k >= 32 for k in n.values()), n
    b = Counter(it.fam for it in strgen.j2t_b64())
    assert set(b) == B64_FAMILIES and all(k >= 32 for k in b.values()), b
    q = Counter(it.fam for it in strgen.t2j_strings())
    assert set(q) == T2J_FAMILIES and all(k >= 30 for k in q.values()), q
    assert len(strgen.t2j_binaries()) >= 256 and len(strgen.long_strings()) >= 32
    assert len(strgen.key_bodies()) >= 1000 and len(strgen.long_keys()) == 36
    assert max(len(it.body) for it in strgen.long_strings()) <= 33100
    # the escape letters: 8 simple ones, 'u', and 247 that are none
    esc = [it for it in strgen.j2t_strings() if it.fam == "esc"]
    assert sum(it.imp == ("err", ERR_ESCAPE) for it in esc) == 247 * 4
    # deterministic: a second build gives the same corpus
    first = strgen.j2t_strings(), strgen.j2t_b64(), strgen.t2j_strings()
    strgen._J2T = strgen._B64 = strgen._T2J = None
    assert (strgen.j2t_strings(), strgen.j2t_b64(), strgen.t2j_strings()) == first
    thin = strgen.thin(first[0], ("uni",), {"phase": 7, "esc": 4})
    tn = Counter(it.fam for it in thin)
    assert tn["uni"] == n["uni"] and tn["phase"] == -(-n["phase"] // 7) and tn["esc"] == -(-n["esc"] // 4)


def test_implications_hold_in_the_model():
    bad = []
    for it in strgen.j2t_strings() + strgen.long_strings() + strgen.key_bodies() + strgen.long_keys():
        got = implied(it, False)
        if it.imp is None:
            if got != ("ok", it.body):  # the raw family: the model passes every such byte through
                bad.append((it, got))
        elif got != it.imp:
            bad.append((it.fam, it.body[:40], it.imp[:1] + (it.imp[1][:40] if it.imp[0] == "ok" else it.imp[1],), got))
    for it in strgen.j2t_b64():
        got = implied(it, True)
        if got != it.imp:
            bad.append((it.fam, it.body[:40], it.imp, got))
    for it in strgen.t2j_strings():
        if m_quote(it.body) != it.imp[1]:
            bad.append((it.fam, it.body, it.imp, m_quote(it.body)))
    for it in strgen.t2j_binaries():
        if m_b64encode(it.body) != it.imp[1]:
            bad.append((it.fam, it.body, it.imp, m_b64encode(it.body)))
    assert not bad, (len(bad), bad[:6])


def test_wellformed_items_mean_what_json_and_base64_say():
    n = 0
    for it in strgen.j2t_strings() + strgen.long_strings():
        if it.imp and it.imp[0] == "ok" and it.fam != "raw":
            try:
                want = json.loads(b'"' + it.body + b'"')
            except ValueError:
                continue  # escapes of control bytes and the like: not JSON, the reference still takes them
            assert it.imp[1] == want.encode("utf-8", "surrogatepass"), it
            n += 1
    assert n > 6000
    n = 0
    for it in strgen.j2t_b64():
        if it.imp[0] == "ok" and len(it.body) % 4 == 0 and not set(it.body) - set(strgen.B64 + b"="):
            assert base64.b64decode(it.body, validate=True) == it.imp[1], it
            n += 1
        if it.imp[0] == "ok" and it.fam == "b64ws":
            assert base64.b64decode(it.body) == it.imp[1], it  # the lenient decoder skips \r \n too
    assert n > 500
    for it in strgen.t2j_strings():
        if first_bad_utf8(it.body) < 0:
            assert json.loads(it.imp[1]).encode() == it.body, it
            if not any(c in (8, 12, 0x7F) for c in it.body):  # json.dumps writes \b \f, the reference \u0008 \u000c
                assert json.dumps(it.body.decode(), ensure_ascii=False).encode() == it.imp[1], it
    for it in strgen.t2j_binaries():
        assert b'"' + base64.b64encode(it.body) + b'"' == it.imp[1], it


def all_j2t_items():
    return strgen.j2t_strings() + strgen.j2t_b64() + strgen.long_strings()


def check_messages(chk, flags, model_flags=None):
    """Every item as str and as bin, first and last: the checker against the model."""
    fl = T.flatten(str_desc())
    items = all_j2t_items()
    bad, modelled = [], 0
    for field in ("str", "bin"):
        for last in (True, False):
            msgs = [wrap(it, field, last)[0] for it in items]
            rets, outs = chk.j2t_batch(fl, msgs, flags, nthreads=8)
            for k, it in enumerate(items):
                want = model_message(it, field, last, flags if model_flags is None else model_flags)
                if want is None:
                    continue
                modelled += 1
                if (int(rets[k]), outs[k]) != want:
                    bad.append((it.fam, field, last, msgs[k][:70], hex(int(rets[k])), hex(want[0]), outs[k][:30],
                                want[1][:30]))
                elif last and it.imp and it.imp[0] in ("err", "open") and not flags >> 16:
                    binary = field == "bin" and not flags & 0x40
                    if (it.fam in B64_FAMILIES) == binary:  # the implication's own reading of the body
                        assert int(rets[k]) & 0xFF == it.imp[1], (it, hex(int(rets[k])))
    assert not bad, (len(bad), bad[:6])
    assert modelled * 100 >= len(items) * 4 * 99, (modelled, len(items))


@pytest.mark.parametrize("flags", [F_STR, F_NOB64])
def test_port_equals_model(flags):
    check_messages(oracle.PortOracle(), flags)


def test_port_utf8_extension_equals_model():
    """DG_F_VALIDATE_UTF8 is the restatement's alone (the reference has no
    such flag): ERR_INVAL at the first invalid sequence of the raw body,
    before anything is unquoted."""
    check_messages(oracle.PortOracle(), F_UTF8)


@pytest.mark.parametrize("flags", [F_STR, F_NOB64])
def test_reference_equals_model(flags):
    ref = oracle.RefOracle()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    check_messages(ref, flags)


def container_messages(items):
    """Each item as a map key, a map value and a list element of cont_desc()."""
    msgs = []
    for it in items:
        b = it.body
        msgs.append(b'{"ms":{"' + b + b'":"v","k2":"w"},"str":"x"}')
        msgs.append(b'{"ms":{"k":"' + b + b'","k2":"' + b + b'"},"ls":["a","' + b + b'"]}')
        msgs.append(b'{"ls":["' + b + b'","' + b + b'"],"lb":["QUJD"]}')
    return msgs


def key_messages(items):
    """Each body as a struct-field key of str_desc(): one that names "str"
    once unquoted (the body spliced into the name) and one that names nothing."""
    msgs = []
    for it in items:
        msgs.append(b'{"' + it.body + b'":"v","req":1}')
        if it.imp[0] == "ok":
            msgs.append(b'{"req":1,"' + it.body + b'":[1,{"a":"\\""}],"str":"s"}')
    # keys that hit a field only after unquoting
    for e in (b"\\u0073tr", b"s\\u0074r", b"st\\u0072", b"\\u0073\\u0074\\u0072", b"s\\tr", b"\\/str", b"st\\u0052",
              b"\\u0053tr"):
        msgs.append(b'{"' + e + b'":"hit","req":1}')
        msgs.append(b'{"req":1,"' + e + b'":"hit"}')
    return msgs


def root_messages(items):
    return [b'"' + it.body + b'"' for it in items] + [it.body for it in items if it.imp and it.imp[0] == "ok"][:400]


def test_port_equals_reference_everywhere():
    """The restatement against the reference on every message shape the GPU
    tests use: fields, pads, containers, keys, long keys, roots, counts."""
    ref = oracle.RefOracle()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    port = oracle.PortOracle()
    fs, fc, fr = T.flatten(str_desc()), T.flatten(cont_desc()), T.flatten(T.builtin("string"))
    small = strgen.thin(all_j2t_items(), ("long",), {"phase": 7, "esc": 3, "b64alpha": 5, "raw": 3})
    keys = strgen.key_bodies()
    sets = [(fs, [wrap(it, f, last, pad)[0] for it in small for f in ("str", "bin") for last in (True, False)
                  for pad in (False, True) if pad or f == "str"]),
            (fs, [m for m, _, _ in strgen.count_messages()]),
            (fs, key_messages(keys + strgen.long_keys())),
            (fc, container_messages(keys[::3] + strgen.long_keys() + small[::5])),
            (fr, root_messages(small[::2]))]
    for fl, msgs in sets:
        for flags in (F_STR, F_NOB64):
            r1, o1 = ref.j2t_batch(fl, msgs, flags, nthreads=8)
            r2, o2 = port.j2t_batch(fl, msgs, flags, nthreads=8)
            bad = [(msgs[i][:70], hex(int(r1[i])), hex(int(r2[i]))) for i in range(len(msgs))
                   if int(r1[i]) != int(r2[i]) or o1[i] != o2[i]]
            assert not bad, (hex(flags), len(bad), bad[:5])


ROUTE_THIN = {"phase": 3, "esc": 6, "uni": 2, "sur": 3, "raw": 4, "b64alpha": 9, "b64ws": 2, "b64long": 3}


def route_items():
    """The items of one GPU route's batch: the error-heavy and the large
    families thinned, none under 24 items, the long family whole."""
    out = strgen.thin(all_j2t_items(), ("long",), ROUTE_THIN)
    n = Counter(it.fam for it in out)
    assert set(n) == J2T_FAMILIES | B64_FAMILIES | {"long"} and min(n.values()) >= 24, n
    return out


def route_messages(items, pad=False):
    """[(item, field, message)]: each item first (before ',') and last (before
    '}'), strings in "str", base64 bodies in "bin", count and long in both."""
    out = []
    for it in items:
        for field in ("str", "bin"):
            if (it.fam in B64_FAMILIES) == (field == "bin") or it.fam in ("count", "long"):
                for last in (False, True):
                    out.append((it, field, wrap(it, field, last, pad)[0]))
    return out


def test_route_batches_keep_the_error_share_under_half():
    """What test_gpu_strings.py's bail conditions rest on: in the batch of
    every route and flag word fewer than half the messages end in an error, so
    "fewer than half the batch bailed" can fail."""
    chk = oracle.RefOracle() or oracle.PortOracle()
    fl = T.flatten(str_desc())
    items = route_items()
    for pad in (False, True):
        msgs = [m for _, _, m in route_messages(items if not pad else items[::3], pad)]
        assert 1000 < len(msgs) < 16000, len(msgs)
        for flags in (F_STR, F_NOB64, F_UTF8):
            rets, _ = (oracle.PortOracle() if flags >> 16 else chk).j2t_batch(fl, msgs, flags, nthreads=8)
            errors = sum(int(r) != 0 for r in rets)
            # a third: the fast kernels also decline some well-formed messages (surrogate pairs, \\" and
            # \\\\ on the flat kernel, more than FL_NESC escapes, the long family)
            assert errors * 3 < len(msgs), (pad, hex(flags), errors, len(msgs))


def test_count_messages_mean_what_they_say():
    fl = T.flatten(str_desc())
    chk = oracle.RefOracle() or oracle.PortOracle()
    cm = strgen.count_messages()
    for flags in (F_STR, F_NOB64):
        rets, outs = chk.j2t_batch(fl, [m for m, _, _ in cm], flags, nthreads=4)
        for (m, fields, kept), r, o in zip(cm, rets, outs):
            assert int(r) == 0 and o == b"".join(tfield(k, v) for k, v in fields) + b"\x00", m
    # the seam: FL_NESC - 1, FL_NESC and FL_NESC + 1 backslashes of the kept kinds, in every split over
    # the two values; what is kept has no escaped key, no \\" or \\\\, no surrogate
    for n in (7, 8, 9, 10):
        hit = [(m, kept) for m, _, kept in cm if m.count(b"\\") == n and b'\\"' not in m and b"\\ud" not in m
               and b'{"str"' in m]
        assert len(hit) == 3 and all(kept == (n <= 8) for _, kept in hit), (n, hit)
    for m, _, kept in cm:
        if kept:
            assert m.count(b"\\") <= 8 and b'\\"' not in m and b"\\\\" not in m and b"\\ud" not in m and b'{"str"' in m
    assert sum(kept for _, _, kept in cm) >= 24 and sum(not kept for _, _, kept in cm) >= 24


# ------------------------------------------------------------------ t2j ----

def t2j_desc():
    return T.struct_type("Q", [
        T.FieldDescriptor(1, "str", T.builtin("string"), T.OPTIONAL),
        T.FieldDescriptor(2, "bin", T.builtin("binary"), T.OPTIONAL),
        T.FieldDescriptor(3, "ms", T.map_of(T.builtin("string"), T.builtin("string")), T.OPTIONAL),
        T.FieldDescriptor(4, "ls", T.list_of(T.builtin("string")), T.OPTIONAL),
        T.FieldDescriptor(5, "nx", T.builtin("string"), T.OPTIONAL),
        T.FieldDescriptor(6, "lb", T.list_of(T.builtin("binary")), T.OPTIONAL),
    ])


def _s(b):
    return struct.pack(">i", len(b)) + b


def t2j_messages(it):
    """[(thrift, JSON under options 0, JSON under NO_BASE64)] for one t2j item:
    alone, in a list, as a map key and value, as a binary; a qtail item also
    with the next field's header and length byte right behind it."""
    b = it.body
    if it.fam == "b64e":
        q, e = m_quote(b), it.imp[1]
        return [(b"\x0b\x00\x02" + _s(b) + b"\x00", b'{"bin":' + e + b"}", b'{"bin":' + q + b"}"),
                (b"\x0f\x00\x06\x0b" + struct.pack(">i", 2) + _s(b) + _s(b) + b"\x00", b'{"lb":[' + e + b"," + e + b"]}",
                 b'{"lb":[' + q + b"," + q + b"]}")]
    q = it.imp[1]
    out = [(b"\x0b\x00\x01" + _s(b) + b"\x00", b'{"str":' + q + b"}"),
           (b"\x0f\x00\x04\x0b" + struct.pack(">i", 3) + _s(b) + _s(b"") + _s(b) + b"\x00", b'{"ls":[' + q + b',"",' + q + b"]}"),
           (b"\x0d\x00\x03\x0b\x0b" + struct.pack(">i", 1) + _s(b) + _s(b) + b"\x00", b'{"ms":{' + q + b":" + q + b"}}"),
           (b"\x0b\x00\x02" + _s(b) + b"\x00", b'{"bin":' + m_b64encode(b) + b"}", b'{"bin":' + q + b"}")]
    if it.fam == "qtail":
        for n in strgen.QTAIL_NEXT:
            out.append((b"\x0b\x00\x01" + _s(b) + b"\x0b\x00\x05" + _s(b"n" * n) + b"\x00",
                        b'{"str":' + q + b',"nx":"' + b"n" * n + b'"}'))
    return [(m,) + ((j[0], j[0]) if len(j) == 1 else tuple(j)) for m, *j in out]


def test_reference_t2j_equals_model():
    chk = oracle.RefT2JOracle()
    if chk is None:
        pytest.skip("oracle/_ref not built")
    fl = T.flatten(t2j_desc())
    side = T.flatten_t2j(fl)
    bad = []
    for it in strgen.t2j_strings() + strgen.t2j_binaries():
        for m, j0, j1 in t2j_messages(it):
            for opts, want in ((0, j0), (NOB64_T2J, j1)):
                got = chk.t2j(fl, side, m, opts)
                if got != (0, want):
                    bad.append((it.fam, it.body[:24], opts, got, want))
    assert not bad, (len(bad), bad[:5])
