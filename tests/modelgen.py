"""The document model of the thrift/generic parity tests (test_generic_codec.py,
test_gpu_generic_codec.py): typed Python documents, their JSON, and every
generic operation restated ON THE DOCUMENT. For a JSON document whose keys are
in document order the reference's j2t writes the canonical Thrift encoding of
it (fields in key order, elements and entries in order, STOP; under flag word
0x1 nothing is added), so an operation on T = j2t(doc, D) has a counterpart on
doc that the reference's compiled C can evaluate: edit the document, encode it
again. Nothing here reads Thrift bytes, imports a kernel or imports one of the
*ref.py restatements; the oracle is only ever asked for j2t.

A document: a struct is a dict alias -> value in document order, a map a dict
whose keys are str (string keys) or int (integer keys; dump() writes them as
JSON strings), a list or a set a list, a binary its base64 text, a double a
float. A path is a sequence of (kind, value) steps as the path tests write
them: FIELD id, INDEX i, STRKEY bytes, INTKEY int, BINKEY the key's wire bytes.

The reference's key rules: a string key compares its bytes; an integer key is
read at the map's own width, I16 / I32 / I64 signed and I08 UNSIGNED
(searchIntKey over ReadInt, thrift/generic/node.go:400-429, thrift/binary.go:
737-754), so a byte-keyed map is looked up with `key & 0xFF` and a negative
INTKEY step never finds anything in it."""
import base64
import copy
import json
import struct

import t2jgen
from dynamicgo_amd import thrift as T
from dynamicgo_amd import workloads as W

FIELD, INDEX, STRKEY, INTKEY, BINKEY = 1, 2, 3, 4, 5
BOOL, BYTE, DOUBLE, I16, I32, I64, STRING, STRUCT, MAP, SET, LIST = 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15
INT_BITS = {BYTE: 8, I16: 16, I32: 32, I64: 64}
COL_BOOL, COL_BYTE, COL_INT, COL_F64, COL_STR, COL_LEN, COL_LIST_INT, COL_LIST_F64 = 1, 2, 3, 4, 5, 6, 19, 20
COL_KINDS = (COL_BOOL, COL_BYTE, COL_INT, COL_F64, COL_STR, COL_LEN, COL_LIST_INT, COL_LIST_F64)
PRESENT_P = 0.65  # an optional / default field is in a struct
MAX_DEPTH = 4     # structs below it keep their REQUIRED fields only, containers below it are empty
U64 = (1 << 64) - 1

# about 4 keys per key type, so that a fixed key step hits often; byte and i16 keys include negative ones
KEY_VOCAB = {STRING: ["a", "k1", 'é"q', "key three"], BYTE: [1, -1, 100, -128], I16: [2, -2, 300, -32768],
             I32: [3, -3, 70000, 2 ** 31 - 1], I64: [4, -4, 2 ** 40, -2 ** 63]}
_PIECES = ["a", "xyz", "\n", "é", '"', "中", " ", "\\", "😀", "\t", "/", "Z9"]
_DOUBLES = [0.0, 5e-324, 1e300, -1.5, 0.1, 123456789.0]


def descriptors():
    """{name: descriptor}: the two the parity tests run on"""
    return {"nesting": W.nesting_desc(), "all": t2jgen.all_types_desc(alias_quirks=False)}


# ------------------------------------------------------------------ documents
def gen_doc(rng, td, depth=0, long_p=0.0):
    """A typed value for descriptor td. long_p: the share of strings that are 1.5 to 4 KB long."""
    t = td.type
    if t == BOOL:
        return rng.random() < 0.5
    if t in INT_BITS:
        b = INT_BITS[t]
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        return rng.choice([0, -1, 1, lo, hi, rng.randint(lo, hi), rng.randint(lo, hi), rng.randint(max(lo, -99), 99)])
    if t == DOUBLE:
        return rng.choice(_DOUBLES + [rng.uniform(-1e6, 1e6), round(rng.uniform(-100, 100), 2)])
    if t == STRING:
        if td.is_binary():
            return base64.b64encode(bytes(rng.randrange(256) for _ in range(rng.randint(0, 9)))).decode()
        if rng.random() < long_p:
            return "".join(rng.choice(_PIECES[:2] + _PIECES[3:6]) for _ in range(rng.randint(1000, 2000)))
        return "".join(rng.choice(_PIECES) for _ in range(rng.randint(0, 6)))
    if t in (LIST, SET):
        n = 0 if depth >= MAX_DEPTH else rng.randint(0, 4 if td.elem.type != STRUCT else 3)
        out = []
        for _ in range(n):
            v = gen_doc(rng, td.elem, depth + 1, long_p)
            if t == LIST or v not in out:  # a set: a duplicate-free array
                out.append(v)
        return out
    if t == MAP:
        n = 0 if depth >= MAX_DEPTH else rng.choice([0, 1, 2, 2, 3, 3, 4])
        return {k: gen_doc(rng, td.elem, depth + 1, long_p) for k in rng.sample(KEY_VOCAB[td.key.type], n)}
    if t == STRUCT:
        fields = [f for f in td.struct.fields if not f.vm]  # fields with a value mapping are left out
        rng.shuffle(fields)
        return {f.alias: gen_doc(rng, f.type, depth + 1, long_p) for f in fields
                if f.required == T.REQUIRED or (depth < MAX_DEPTH and rng.random() < PRESENT_P)}
    raise ValueError(t)


def dump(doc) -> bytes:
    return json.dumps(doc, separators=(",", ":"), ensure_ascii=False).encode()


_flat = {}


def flat(td):
    """T.flatten(td), once per descriptor object"""
    f = _flat.get(id(td))
    if f is None:
        f = _flat[id(td)] = (td, T.flatten(td))
    return f[1]


def encode(chk, td, doc) -> bytes:
    """The Thrift bytes of doc under td: the oracle's j2t under flag word 0x1 (allow unknown, nothing else)"""
    ret, out = chk.j2t(flat(td), dump(doc), 0x1)
    assert ret == 0, (hex(ret), dump(doc)[:80])
    return out


class Corpus:
    """n seeded documents of one descriptor and their messages; enc() is encode() with a memo, so that a value
    many operations ask for costs one oracle call"""
    SEEDS = {"nesting": 1101, "all": 2202}

    def __init__(self, chk, name, n=300, seed=0, long_p=(0.0,)):
        """long_p: document i is generated with long_p[i % len(long_p)]"""
        import random
        self.chk, self.name, self.td = chk, name, descriptors()[name]
        rng = random.Random(self.SEEDS[name] + seed)
        self.docs = [gen_doc(rng, self.td, long_p=long_p[i % len(long_p)]) for i in range(n)]
        self._memo = {}
        self.msgs = [self.enc(self.td, d) for d in self.docs]

    def enc(self, td, doc) -> bytes:
        key = (id(td), dump(doc))
        out = self._memo.get(key)
        if out is None:
            out = self._memo[key] = encode(self.chk, td, doc)
        return out

    def values(self, form, vtd):
        """the per-message values of one set form, seeded by the form's name"""
        import random
        rng = random.Random("%s/%s" % (self.name, form))
        return [gen_doc(rng, vtd, depth=2) for _ in self.docs]


# ---------------------------------------------------------------------- steps
def signed(v: int, bits: int) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def lookup_key(kt: int, k: int) -> int:
    """a document's integer key as the reference reads it back: I08 unsigned"""
    return k & 0xFF if kt == BYTE else k


def wire_key(ktd, k) -> bytes:
    """a document's key as it stands in the message"""
    if ktd.type == STRING:
        b = k.encode()
        return struct.pack(">i", len(b)) + b
    return (k & ((1 << INT_BITS[ktd.type]) - 1)).to_bytes(INT_BITS[ktd.type] // 8, "big")


_MISS = object()


def _step(doc, td, kind, val):
    """(the Python key of the child or _MISS, the child's descriptor or None, the key a new child would take)"""
    t = td.type
    if kind == FIELD and t == STRUCT:
        f = td.struct.field_by_id(val)
        if f is None:
            return _MISS, None, None
        return (f.alias if f.alias in doc else _MISS), f.type, f.alias
    if kind == INDEX and t in (LIST, SET):
        return (val if val < len(doc) else _MISS), td.elem, None
    if t == MAP and kind == STRKEY and td.key.type == STRING:
        k = val.decode()
        return (k if k in doc else _MISS), td.elem, k
    if t == MAP and kind == INTKEY and td.key.type in INT_BITS:
        for k in doc:
            if lookup_key(td.key.type, k) == val:
                return k, td.elem, k
        return _MISS, td.elem, signed(val, INT_BITS[td.key.type])
    if t == MAP and kind == BINKEY:
        for k in doc:
            if wire_key(td.key, k) == val:
                return k, td.elem, k
        new = val[4:].decode() if td.key.type == STRING else signed(int.from_bytes(val, "big"), 8 * len(val))
        return _MISS, td.elem, new
    raise ValueError("step %r on a value of type %d: not a path the model takes" % ((kind, val), t))


def _resolve(doc, td, path):
    """(missing step or None, the Python keys down to it, the value there, its descriptor)"""
    keys = []
    for s, (kind, val) in enumerate(path):
        k, nd, _ = _step(doc, td, kind, val)
        if k is _MISS:
            return s, keys, doc, td
        keys.append(k)
        doc, td = doc[k], nd
    return None, keys, doc, td


def _at(root, keys):
    for k in keys:
        root = root[k]
    return root


def _put(root, keys, value):
    """root with the value at keys exchanged for `value`"""
    if not keys:
        return value
    _at(root, keys[:-1])[keys[-1]] = value
    return root


def desc_at(td, path):
    """the descriptor a path leads to, or None where the descriptor has nothing"""
    for kind, val in path:
        if kind == FIELD:
            f = td.struct.field_by_id(val) if td.struct is not None else None
            if f is None:
                return None
            td = f.type
        else:
            td = td.elem
    return td


# ----------------------------------------------------------------- operations
def sub(doc, td, path):
    """GetByPath: (value, descriptor), or the index of the step where the document has nothing"""
    miss, _, v, d = _resolve(doc, td, path)
    return (v, d) if miss is None else miss


def replaced(doc, td, path, value):
    miss, keys, _, _ = _resolve(doc, td, path)
    assert miss is None and keys
    return _put(copy.deepcopy(doc), keys, value)


def _front(container, td, step, value):
    """container with the new key / element put first"""
    if td.type in (LIST, SET):
        return [value] + container
    k = _step(container, td, *step)[2]
    assert k is not None and k not in container, step
    out = {k: value}
    out.update(container)
    return out


def inserted_first(doc, td, path, value):
    miss, keys, v, d = _resolve(doc, td, path)
    assert miss == len(path) - 1
    new = copy.deepcopy(doc)
    return _put(new, keys, _front(_at(new, keys), d, path[-1], value))


def removed(doc, td, path):
    miss, keys, _, _ = _resolve(doc, td, path)
    assert miss is None and keys
    new = copy.deepcopy(doc)
    del _at(new, keys[:-1])[keys[-1]]
    return new


SET_OP, UNSET_OP = 1, 2


def edit(doc, td, op, path, value=None):
    """SetByPath / UnsetByPath: (class, document after it or None). Classes: replaced, inserted (only the last
    step missed: the new child goes first), deleted, untouched (an unset whose parent is missing), notfound (a
    set that misses before the last step; an unset whose parent is there and whose child is not)."""
    miss = _resolve(doc, td, path)[0]
    last = len(path) - 1
    if op == SET_OP:
        if miss is None:
            return "replaced", replaced(doc, td, path, value)
        return ("inserted", inserted_first(doc, td, path, value)) if miss == last else ("notfound", None)
    if miss is None:
        return "deleted", removed(doc, td, path)
    return ("notfound", None) if miss == last else ("untouched", doc)


def many(doc, td, op, parent, items):
    """SetMany / UnsetMany below `parent`; items: [(step, value)]. (class, existed mask, failing item, document):
    found items in place, missing ones first in item order, unsets on the original; the first item that fails
    gives the message its class."""
    miss, keys, v, d = _resolve(doc, td, parent)
    if miss is not None:
        return ("notfound", 0, 0, None) if op == SET_OP else ("untouched", 0, 0, doc)
    new = copy.deepcopy(doc)
    c = _at(new, keys)
    found = [_step(v, d, *st)[0] for st, _ in items]
    if op == UNSET_OP:
        for j, k in enumerate(found):
            if k is _MISS:
                return "notfound", 0, j, None
        for k in sorted(found, key=lambda k: -k if d.type in (LIST, SET) else 0):  # indexes address the original
            del c[k]
        return "dropped", (1 << len(items)) - 1, 0, new
    mask = 0
    for j, (k, (_, val)) in enumerate(zip(found, items)):
        if k is not _MISS:
            c[k] = val
            mask |= 1 << j
    for (st, val), k in reversed(list(zip(items, found))):
        if k is _MISS:
            c = _front(c, d, st, val)
    return "set", mask, 0, _put(new, keys, c)


class Kid:
    __slots__ = ("kind", "key", "key_bytes", "type", "depth", "parent", "n_desc", "value", "td")

    def __init__(self, *a):
        self.kind, self.key, self.key_bytes, self.type, self.depth, self.parent, self.n_desc, self.value, self.td = a


NO_PARENT = 0xFFFFFFFF
COMPLEX = (STRUCT, MAP, SET, LIST)


def _scan(v, d, recurse, out, parent, depth):
    if d.type == STRUCT:
        kids = [(FIELD, d.struct.names[a].id, b"", x, d.struct.names[a].type) for a, x in v.items()]
    elif d.type in (LIST, SET):
        kids = [(INDEX, i, b"", x, d.elem) for i, x in enumerate(v)]
    elif d.key.type == STRING:
        kids = [(STRKEY, len(k.encode()), k.encode(), x, d.elem) for k, x in v.items()]
    else:
        kids = [(INTKEY, lookup_key(d.key.type, k), b"", x, d.elem) for k, x in v.items()]
    for kind, key, kb, x, xd in kids:
        at = len(out)
        out.append(Kid(kind, key, kb, xd.type, depth, parent, 0, x, xd))
        if recurse and xd.type in COMPLEX:
            _scan(x, xd, recurse, out, at, depth + 1)
            out[at].n_desc = len(out) - at - 1


def children(doc, td, path=(), recurse=False):
    """Children of the node at path: ((type, key type, element type, direct), [Kid] in document order, preorder
    when recursive), or the index of the missing step. The node must be a container."""
    miss, _, v, d = _resolve(doc, td, path)
    if miss is not None:
        return miss
    assert d.type in COMPLEX
    out = []
    _scan(v, d, recurse, out, NO_PARENT, 1)
    kt = d.key.type if d.type == MAP else 0
    et = d.elem.type if d.type != STRUCT else 0
    return (d.type, kt, et, len(v)), out


def _int_cell(t, v):
    return v & 0xFF if t == BYTE else v & U64


def _bits(x: float) -> int:
    return struct.unpack(">Q", struct.pack(">d", x))[0]


def column(doc, td, path, kind):
    """One cell of a typed column: ("ok", value, length, elements, bytes) or ("notfound", step). The casts'
    rules: a byte read as INT is value & 0xFF, wider ints are sign-extended to 64 bits, doubles are their bit
    pattern, STR is the UTF-8 bytes (the decoded bytes of a binary), LEN a container's length. The kind must
    suit the descriptor's type at the path."""
    r = sub(doc, td, path)
    if isinstance(r, int):
        return "notfound", r
    v, d = r
    t = d.type
    if kind == COL_BOOL and t == BOOL:
        return "ok", int(v), 0, None, None
    if kind == COL_BYTE and t == BYTE:
        return "ok", v & 0xFF, 0, None, None
    if kind == COL_INT and t in INT_BITS:
        return "ok", _int_cell(t, v), 0, None, None
    if kind == COL_F64 and t == DOUBLE:
        return "ok", _bits(v), 0, None, None
    if kind == COL_STR and t == STRING:
        b = base64.b64decode(v) if d.is_binary() else v.encode()
        return "ok", None, len(b), None, b
    if kind == COL_LEN and t in (LIST, SET, MAP):
        return "ok", len(v), 0, None, None
    if kind == COL_LIST_INT and t in (LIST, SET) and d.elem.type in INT_BITS:
        return "ok", None, len(v), [_int_cell(d.elem.type, x) for x in v], None
    if kind == COL_LIST_F64 and t in (LIST, SET) and d.elem.type == DOUBLE:
        return "ok", None, len(v), [_bits(x) for x in v], None
    raise ValueError("column kind %d on type %d" % (kind, t))


# -------------------------------------------------------------- descriptors
def _has_struct(td):
    return td.type == STRUCT or any(x is not None and _has_struct(x) for x in (td.key, td.elem))


def narrow(rng, td, keep=0.6, require=0.0, depth=0):
    """A narrower descriptor for MarshalTo, of fresh struct objects throughout (the same struct on both sides
    is a compile-time ValueError by design). Each field is kept with probability `keep`; no field whose type
    holds a struct is kept below depth 3, so the recursive Node terminates. require: the share of kept fields
    that are not REQUIRED in td and become REQUIRED here."""
    t = td.type
    if t == STRUCT:
        sd = T.StructDescriptor(td.name)
        for f in td.struct.fields:
            if rng.random() >= keep or (depth >= 3 and _has_struct(f.type)):
                continue
            req = T.REQUIRED if f.required != T.REQUIRED and rng.random() < require else f.required
            sd.add_field(T.FieldDescriptor(f.id, f.name, narrow(rng, f.type, keep, require, depth + 1), req, f.alias, f.vm))
        return T.TypeDescriptor(STRUCT, td.name, struct=sd)
    if t in (LIST, SET):
        return T.TypeDescriptor(t, td.name, elem=narrow(rng, td.elem, keep, require, depth))
    if t == MAP:
        return T.TypeDescriptor(t, td.name, key=narrow(rng, td.key, keep, require, depth),
                                elem=narrow(rng, td.elem, keep, require, depth))
    return T.TypeDescriptor(t, td.name)


def first_missing_required(doc, td):
    """The field id j2t and the cut both stop at when td marks REQUIRED what doc lacks: structs end in document
    order (a nested one before the one that holds it), and a struct's missing fields are reported lowest id
    first. None when nothing is missing. Keys td does not know are skipped whole."""
    t = td.type
    if t == STRUCT:
        for a, v in doc.items():
            f = td.struct.names.get(a)
            if f is not None:
                r = first_missing_required(v, f.type)
                if r is not None:
                    return r
        lack = [f.id for f in td.struct.fields if f.required == T.REQUIRED and f.alias not in doc]
        return min(lack) if lack else None
    if t in (LIST, SET, MAP) and _has_struct(td.elem):
        for v in (doc.values() if t == MAP else doc):
            r = first_missing_required(v, td.elem)
            if r is not None:
                return r
    return None


def first_unknown(doc, td, wide):
    """(key, field id under `wide`) of the first key in document order that td does not know, or None"""
    t = td.type
    if t == STRUCT:
        for a, v in doc.items():
            f = td.struct.names.get(a)
            if f is None:
                return a, wide.struct.names[a].id
            r = first_unknown(v, f.type, wide.struct.names[a].type)
            if r is not None:
                return r
    elif t in (LIST, SET, MAP) and _has_struct(td.elem):
        for v in (doc.values() if t == MAP else doc):
            r = first_unknown(v, td.elem, wide.elem)
            if r is not None:
                return r
    return None


CUT_E_UNKNOWN, CUT_E_REQUIRED, CUT_DISALLOW_UNKNOWN = 3, 4, 2  # DG_CUT_* (include/dgj2t_defs.h)


def cut_want(chk, doc, to):
    """(ret, bytes) of MarshalTo(j2t(doc, D) -> to) under option word 0: j2t(doc, to) under flag word 0x1. Where
    `to` marks REQUIRED a field doc lacks, j2t's code 10 with the id in its value, which must be the model's
    id, becomes the cut's E_REQUIRED with the id in aux."""
    jr, out = chk.j2t(flat(to), dump(doc), 0x1)
    fid = first_missing_required(doc, to)
    if fid is None:
        assert jr == 0, hex(jr)
        return 0, out
    assert (jr & 0xFF, jr >> 40) == (10, fid), (hex(jr), fid)
    return CUT_E_REQUIRED | fid << 32, b""


def cut_unknown_want(chk, doc, frm, wide):
    """(ret, bytes) of MarshalTo(j2t(doc, wide): frm -> a field-for-field copy of frm) under DISALLOW_UNKNOWN: j2t(doc,
    frm) WITHOUT flag 0x1. Its code 12 carries the length of the unknown key, which must be the model's first
    unknown key; the cut's E_UNKNOWN carries that key's field id under `wide`."""
    jr, out = chk.j2t(flat(frm), dump(doc), 0)
    unk = first_unknown(doc, frm, wide)
    if unk is None:
        assert jr == 0, hex(jr)
        return 0, out
    assert (jr & 0xFF, jr >> 40) == (12, len(unk[0].encode())), (hex(jr), unk)
    return CUT_E_UNKNOWN | unk[1] << 32, b""


# ---------------------------------------------------------------- schema paths
F, I, S, N, B = FIELD, INDEX, STRKEY, INTKEY, BINKEY
# 1 to 4 steps across every container kind; EXIST can be found in a document, NEVER cannot
PATHS = {
    "nesting": {
        "exist": [[(F, 4)], [(F, 11)], [(F, 8), (F, 5)], [(F, 2), (I, 1), (F, 3)], [(F, 7), (S, b"a")],
                  [(F, 9), (N, 3)], [(F, 12), (N, -4)], [(F, 15), (S, b"k1"), (F, 1)], [(F, 5), (I, 2)],
                  [(F, 10), (I, 0)], [(F, 13), (I, 1)], [(F, 7), (B, b"\0\0\0\x02k1")],
                  [(F, 9), (B, b"\xff\xff\xff\xfd")], [(F, 2), (I, 0), (F, 6)]],
        "never": [[(F, 99)], [(F, 2), (I, 99), (F, 1)], [(F, 7), (S, b"nokey")], [(F, 9), (N, 12345)],
                  [(F, 8), (F, 2)], [(F, 12), (B, b"\0\0\0\0\0\0\0\x09")], [(F, 15), (S, b"k1"), (F, 77)],
                  [(F, 8), (F, 9), (F, 1), (F, 1)]],
    },
    "all": {
        "exist": [[(F, 4)], [(F, 9), (F, 2)], [(F, 10), (I, 1), (F, 2)], [(F, 12), (S, b"a")],
                  [(F, 12), (S, 'é"q'.encode()), (I, 0)], [(F, 13), (N, 255)], [(F, 13), (N, 1)], [(F, 14), (N, -2)],
                  [(F, 15), (N, 3), (F, 2)], [(F, 16), (N, 4), (S, b"k1")], [(F, 17), (F, 2), (F, 2), (F, 1)],
                  [(F, 17), (F, 3), (I, 0), (F, 1)], [(F, 11), (I, 1)], [(F, 20), (S, b"key three")],
                  [(F, 21), (F, 3), (I, 0)], [(F, 14), (B, b"\x80\x00")], [(F, 13), (B, b"\x80")],
                  [(F, 16), (N, -2 ** 63)]],
        "never": [[(F, 1000)], [(F, 13), (N, -1)], [(F, 10), (I, 99)], [(F, 12), (S, b"nokey")], [(F, 9), (F, 7)],
                  [(F, 15), (N, 12345), (F, 1)]],
    },
}
# the container paths of the Children tests, the root first
KID_PATHS = {"nesting": [[], [(F, 2)], [(F, 15)], [(F, 8)]], "all": [[], [(F, 13)], [(F, 17)], [(F, 16), (N, 4)]]}
# (path, kind): every kind in one plan of eight for "all"; "nesting" has no bool and no list<double>
COLUMNS = {
    "nesting": [([(F, 14)], COL_BYTE), ([(F, 6)], COL_INT), ([(F, 8), (F, 1)], COL_INT), ([(F, 3)], COL_F64),
                ([(F, 1)], COL_STR), ([(F, 11)], COL_STR), ([(F, 15)], COL_LEN), ([(F, 13)], COL_LIST_INT)],
    "all": [([(F, 1)], COL_BOOL), ([(F, 2)], COL_BYTE), ([(F, 3)], COL_INT), ([(F, 6)], COL_F64), ([(F, 8)], COL_STR),
            ([(F, 12)], COL_LEN), ([(F, 12), (S, b"a")], COL_LIST_INT), ([(F, 9), (F, 3)], COL_LIST_F64)],
}
COLUMNS_2 = {  # a second plan: the kinds over other widths and containers
    "nesting": [([(F, 4)], COL_INT), ([(F, 2), (I, 0), (F, 5)], COL_STR), ([(F, 5)], COL_LIST_INT), ([(F, 7)], COL_LEN),
                ([(F, 10)], COL_LEN), ([(F, 8), (F, 3)], COL_F64), ([(F, 8), (F, 6)], COL_STR), ([(F, 99)], COL_INT)],
    "all": [([(F, 2)], COL_INT), ([(F, 5)], COL_INT), ([(F, 7)], COL_STR), ([(F, 11)], COL_LIST_INT), ([(F, 11)], COL_LEN),
            ([(F, 22)], COL_F64), ([(F, 23)], COL_BOOL), ([(F, 24)], COL_BYTE)],
}
# the edit forms: (name, op, path); a set's value is generated under desc_at(path)
EDITS = {
    "nesting": [("replace i32", SET_OP, [(F, 4)]), ("unset field", UNSET_OP, [(F, 9)]),
                ("set field", SET_OP, [(F, 14)]), ("set nested string", SET_OP, [(F, 8), (F, 5)]),
                ("insert at a list's front", SET_OP, [(F, 5), (I, 1000)]), ("set list element", SET_OP, [(F, 10), (I, 1)]),
                ("set string key", SET_OP, [(F, 7), (S, b"k1")]), ("insert a new string key", SET_OP, [(F, 7), (S, b"new key")]),
                ("set i32 key", SET_OP, [(F, 9), (N, -3)]), ("set i64 key to a string", SET_OP, [(F, 12), (N, 2 ** 40)]),
                ("set struct in a map", SET_OP, [(F, 15), (S, b"a")]), ("set field of a list's struct", SET_OP, [(F, 2), (I, 0), (F, 1)]),
                ("unset list element 0", UNSET_OP, [(F, 13), (I, 0)]), ("unset string key", UNSET_OP, [(F, 7), (S, b"a")]),
                ("unset int key", UNSET_OP, [(F, 9), (N, 70000)]), ("unset nested field", UNSET_OP, [(F, 8), (F, 3)]),
                ("unset field of a map's struct", UNSET_OP, [(F, 15), (S, b"k1"), (F, 5)])],
    "all": [("replace i32", SET_OP, [(F, 4)]), ("unset field", UNSET_OP, [(F, 12)]), ("set double", SET_OP, [(F, 6)]),
            ("set nested string", SET_OP, [(F, 9), (F, 2)]), ("insert at a list's front", SET_OP, [(F, 19), (I, 1000)]),
            ("set set element", SET_OP, [(F, 11), (I, 1)]), ("set byte key", SET_OP, [(F, 13), (N, 255)]),
            ("insert a new byte key", SET_OP, [(F, 13), (N, 200)]), ("set i16 key to a binary", SET_OP, [(F, 14), (N, 300)]),
            ("set struct under an i32 key", SET_OP, [(F, 15), (N, 3)]), ("set a map under an i64 key", SET_OP, [(F, 16), (N, 4)]),
            ("set three steps down", SET_OP, [(F, 16), (N, -4), (S, b"a")]), ("set in the recursion", SET_OP, [(F, 17), (F, 2), (F, 1)]),
            ("set a list in a struct in a list", SET_OP, [(F, 10), (I, 0), (F, 3)]), ("set required field", SET_OP, [(F, 18)]),
            ("unset list element 0", UNSET_OP, [(F, 19), (I, 0)]), ("unset byte key", UNSET_OP, [(F, 13), (N, 128)]),
            ("unset nested struct", UNSET_OP, [(F, 17), (F, 2)]), ("unset i32 key's field", UNSET_OP, [(F, 15), (N, -3), (F, 3)])],
}
# the many-edits: (name, op, parent, steps); K = 2, 3 and 7, replaces and inserts mixed
MANY = {
    "nesting": [("2 fields", SET_OP, [], [(F, 4), (F, 14)]), ("3 fields below", SET_OP, [(F, 8)], [(F, 1), (F, 5), (F, 3)]),
                ("7 fields", SET_OP, [], [(F, 1), (F, 3), (F, 4), (F, 6), (F, 11), (F, 14), (F, 10)]),
                ("3 indexes", SET_OP, [(F, 5)], [(I, 0), (I, 500), (I, 2)]),
                ("7 string keys", SET_OP, [(F, 7)], [(S, k) for k in (b"a", b"n1", b"k1", b"n2", "é\"q".encode(), b"n3", b"key three")]),
                ("2 int keys", SET_OP, [(F, 9)], [(N, 3), (N, 99)]),
                ("unset 2 fields", UNSET_OP, [], [(F, 4), (F, 14)]), ("unset 3 indexes", UNSET_OP, [(F, 13)], [(I, 2), (I, 0), (I, 1)]),
                ("unset 2 keys below", UNSET_OP, [(F, 12)], [(N, 4), (N, -4)])],
    "all": [("2 fields", SET_OP, [], [(F, 4), (F, 6)]), ("3 fields below", SET_OP, [(F, 9)], [(F, 3), (F, 1), (F, 2)]),
            ("7 fields", SET_OP, [], [(F, 1), (F, 2), (F, 3), (F, 5), (F, 7), (F, 8), (F, 22)]),
            ("3 indexes", SET_OP, [(F, 19)], [(I, 700), (I, 0), (I, 600)]),
            ("7 byte keys", SET_OP, [(F, 13)], [(N, k) for k in (1, 2, 255, 3, 100, 128, 7)]),
            ("2 keys two steps down", SET_OP, [(F, 16), (N, 4)], [(S, b"a"), (S, b"zz")]),
            ("unset 2 fields", UNSET_OP, [], [(F, 3), (F, 22)]), ("unset 2 indexes", UNSET_OP, [(F, 19)], [(I, 0), (I, 1)]),
            ("unset 3 fields in the recursion", UNSET_OP, [(F, 17)], [(F, 1), (F, 2), (F, 3)])],
}
