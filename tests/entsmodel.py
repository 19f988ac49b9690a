"""The entry columns restated ON THE DOCUMENT, beside modelgen.py (which is
imported, not changed): what Node.List of strings, Node.StrMap and Node.IntMap
give on the node a path leads to, from the typed document alone. Nothing here
reads Thrift bytes or imports a kernel or a *ref.py restatement."""
import base64
import struct

import modelgen as M

BOOL, INT, F64, STR = 1, 3, 4, 5  # DG_ENT_*
LISTSTR, STRMAP, INTMAP = 0x15, 0x20, 0x40
_VALUE_TYPES = {BOOL: (M.BOOL,), INT: tuple(M.INT_BITS), F64: (M.DOUBLE,), STR: (M.STRING,)}

# the columns of the "all" descriptor: 19 list<string>, 20 map<string, i64>, 13 map<byte, bool>, 14 map<i16, binary>,
# 16 map<i64, map<string, double>> under one of its keys; 12 (list values) and 15 (struct values) are what no kind takes
F, N = M.FIELD, M.INTKEY
POSITIVE = [([(F, 19)], LISTSTR), ([(F, 20)], STRMAP | INT), ([(F, 13)], INTMAP | BOOL), ([(F, 14)], INTMAP | STR),
            ([(F, 16), (N, 4)], STRMAP | F64)]
NEGATIVE = [([(F, 12)], STRMAP | INT), ([(F, 15)], INTMAP | INT), ([(F, 12)], STRMAP | STR)]
COLUMNS = POSITIVE + NEGATIVE


def _value(v, d, kind):
    if kind == BOOL:
        return int(v)
    if kind == INT:
        return v & 0xFF if d.type == M.BYTE else v & M.U64  # Node.int: a byte is unsigned
    if kind == F64:
        return struct.unpack(">Q", struct.pack(">d", v))[0]
    return base64.b64decode(v) if d.is_binary() else v.encode()


def entries(doc, td, path, kind):
    """One cell of an entry column: ("notfound", step), ("unsupported",) or ("ok", [(key, value), ...]) in
    document order: list(doc.items()) with an I08 key masked with 0xFF, a string key as its UTF-8 bytes, an integer
    value as the 64 bits Node.int gives, a double as its bits, a string as its bytes (a binary: decoded); a list of
    strings has None for every key. An empty container is OK whatever it holds."""
    r = M.sub(doc, td, path)
    if isinstance(r, int):
        return "notfound", r
    v, d = r
    if kind == LISTSTR:
        if d.type not in (M.LIST, M.SET):
            return ("unsupported",)
        if v and d.elem.type != M.STRING:
            return ("unsupported",)
        return "ok", [(None, _value(x, d.elem, STR)) for x in v]
    if d.type != M.MAP or (d.key.type != M.STRING if kind & STRMAP else d.key.type not in M.INT_BITS):
        return ("unsupported",)
    if v and d.elem.type not in _VALUE_TYPES[kind & 15]:
        return ("unsupported",)
    return "ok", [(k.encode() if kind & STRMAP else M.lookup_key(d.key.type, k) & M.U64, _value(x, d.elem, kind & 15))
                  for k, x in v.items()]
