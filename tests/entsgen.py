"""Built inputs of the entry-column tests, shared by the CPU build of the decode
(test_ents_host.py) and the GPU tests (test_gpu_ents.py): the kind x container
x key-type x value-type matrix with every type byte at size 0 and 1, keys and
values at the width edges, counts around the wave, the block, the emit chunk
and the staged emit's R, string lengths around the 4-byte prefix, maps cut
short, targets at every residue mod 16 and at the arena's end, nests around the
8 LDS frames, and the fuzz column sets."""
import random
import struct

import entsref as ER
import tgetref as R
from colsgen import DOUBLES, fld, lst, wstr

F, I = R.FIELD, R.INDEX
ONE = [(F, 1)]
ALL_KINDS = [(ONE, k) for k in ER.KINDS]
_FMT = {R.BOOL: ">B", R.BYTE: ">B", R.I16: ">H", R.I32: ">I", R.I64: ">Q", R.DOUBLE: ">Q"}


def mp(kt, vt, count, body=b""):
    return struct.pack(">BBi", kt, vt, count) + body


def one(t, j=0):
    """value j of wire type t: fixed widths with an alternating top bit, strings of 0..6 bytes"""
    if t == R.STRING:
        return wstr(bytes((j * 37 + q) & 0xFF for q in range(j % 7)))
    w = R._TYPE_SIZE[t]
    if t == R.BOOL:
        return bytes([j & 1])
    return struct.pack(_FMT[t], ((j + 1) * 0x9E3779B97F4A7C15 >> 7 ^ (j & 1) << (8 * w - 1)) & ((1 << 8 * w) - 1))


def entries(kt, vt, count):
    return b"".join(one(kt, j) + one(vt, j + 3) for j in range(count))


def msg(t, body, fid=1):
    return fld(t, fid, body) + b"\x00"


# ---------------------------------------------------------------- the matrix
STR_LENS = (0, 1, 3, 4, 5, 255)
EDGES = {R.BYTE: (0x00, 0x7F, 0x80, 0xFF), R.I16: (0x8000, 0xFFFF, 0x7FFF, 0), R.I32: (0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 1),
         R.I64: (1 << 63, (1 << 64) - 1, (1 << 63) - 1, 2)}
MATRIX_SETS = (ALL_KINDS[:8], ALL_KINDS[8:] + ALL_KINDS[:3])


def _body(t):
    """one value of type byte t if it can be written, else 8 bytes nothing can skip"""
    return one(t) if t in R._TYPE_SIZE or t == R.STRING else b"\0" * 8


def matrix_messages():
    """struct{1: X}. X: a map with every byte 0..255 as its key type (values
    i32) and as its value type (keys i32, keys string), a list with every byte
    as its element type, each at size 0 and at size 1 (the two map casts test
    the key byte at different moments: only size 0 reaches them when the byte
    cannot be skipped); every key type x value type the casts take, with
    the widths' edges as keys and as values; strings of every length of
    STR_LENS as elements, keys and values; a duplicate key; maps cut short
    inside the last key, the last value and a length prefix; nodes of the wrong
    class."""
    out = []
    for b in range(256):
        for size in (0, 1):
            out.append(msg(R.MAP, mp(b, R.I32, size, (_body(b) + one(R.I32)) * size)))
            out.append(msg(R.MAP, mp(R.I32, b, size, (one(R.I32) + _body(b)) * size)))
            out.append(msg(R.MAP, mp(R.STRING, b, size, (wstr(b"k") + _body(b)) * size)))
            out.append(msg(R.LIST if b & 1 else R.SET, lst(b, size, _body(b) * size)))
    for kt, ks in EDGES.items():
        keys = b"".join(struct.pack(_FMT[kt], k) for k in ks)
        w = R._TYPE_SIZE[kt]
        for vt, vs in list(EDGES.items()) + [(R.DOUBLE, DOUBLES[:4]), (R.BOOL, (0, 1, 2, 0xFF))]:
            out.append(msg(R.MAP, mp(kt, vt, 4, b"".join(keys[q * w:q * w + w] + struct.pack(_FMT[vt], v)
                                                         for q, v in enumerate(vs)))))
        out.append(msg(R.MAP, mp(kt, R.STRING, 4, b"".join(keys[q * w:q * w + w] + wstr(b"v" * q) for q in range(4)))))
        out.append(msg(R.MAP, mp(R.STRING, kt, 4, b"".join(wstr(b"k%d" % q) + keys[q * w:q * w + w] for q in range(4)))))
    out.append(msg(R.MAP, mp(R.STRING, R.DOUBLE, len(DOUBLES), b"".join(wstr(b"d") + struct.pack(">Q", d) for d in DOUBLES))))
    out.append(msg(R.MAP, mp(R.STRING, R.BOOL, 4, b"".join(wstr(b"") + bytes([b]) for b in (0, 1, 2, 0xFF)))))
    strs = [bytes((q * 7 + n) & 0xFF for q in range(n)) for n in STR_LENS]
    out.append(msg(R.LIST, lst(R.STRING, len(strs), b"".join(map(wstr, strs)))))
    out.append(msg(R.SET, lst(R.STRING, len(strs), b"".join(map(wstr, reversed(strs))))))
    out.append(msg(R.MAP, mp(R.STRING, R.STRING, len(strs), b"".join(wstr(a) + wstr(b) for a, b in zip(strs, reversed(strs))))))
    out.append(msg(R.MAP, mp(R.I16, R.STRING, len(strs), b"".join(struct.pack(">h", -q) + wstr(s) for q, s in enumerate(strs)))))
    out.append(msg(R.MAP, mp(R.STRING, R.I64, 3, wstr(b"a") + one(R.I64, 1) + wstr(b"b") + one(R.I64, 2) + wstr(b"a") + one(R.I64, 3))))
    out.append(msg(R.MAP, mp(R.I32, R.I32, 3, struct.pack(">6i", 7, 1, 8, 2, 7, 3))))
    whole = fld(R.MAP, 1, mp(R.STRING, R.STRING, 2, wstr(b"key") + wstr(b"value") + wstr(b"last key") + wstr(b"last value")))
    for cut in (1, 4, 11, 12, 14, 15, 20):  # in the last value, at its start, in its prefix, in the last key, in its prefix
        out.append(whole[:-cut])
    whole = fld(R.MAP, 1, mp(R.I32, R.STRING, 2, one(R.I32) + wstr(b"v") + one(R.I32, 1) + wstr(b"vv")))
    out += [whole[:-1], whole[:-3], whole[:-8]]
    whole = fld(R.LIST, 1, lst(R.STRING, 2, wstr(b"first") + wstr(b"second")))
    out += [whole[:-1], whole[:-7], whole[:-10]]
    out += [msg(R.MAP, mp(R.STRING, R.I64, 2 ** 31 - 1, wstr(b"a") + one(R.I64))), msg(R.MAP, mp(R.I32, R.I32, -1)),
            msg(R.LIST, lst(R.STRING, -1)), msg(R.LIST, lst(R.STRING, 2 ** 31 - 1, wstr(b"a")))]
    out += [b"\x00", msg(R.I32, b"\0\0\0\5"), msg(R.STRING, wstr(b"text")), msg(R.STRUCT, b"\x00"), msg(R.BOOL, b"\1"),
            msg(R.DOUBLE, b"\0" * 8), msg(R.MAP, mp(R.STRING, R.STRUCT, 1, wstr(b"s") + b"\x00")),
            msg(R.MAP, mp(R.STRING, R.LIST, 1, wstr(b"l") + lst(R.STRING, 1, wstr(b"x")))),
            msg(R.LIST, lst(R.LIST, 1, lst(R.STRING, 1, wstr(b"x")))), msg(R.MAP, mp(R.DOUBLE, R.I32, 1, b"\0" * 12)),
            msg(R.MAP, mp(R.BOOL, R.BOOL, 1, b"\1\1"))]
    return out


# ----------------------------------------------------------------- the counts
VAR_COUNTS = (0, 1, 2, 63, 64, 65, 257)
FIXED_COUNTS = VAR_COUNTS + (2049, 4097)  # one past an emit chunk, and two chunks and one
COUNT_COLUMNS = [(ONE, ER.LISTSTR), (ONE, ER.STRMAP | ER.INT), (ONE, ER.STRMAP | ER.STR), (ONE, ER.INTMAP | ER.STR),
                 (ONE, ER.INTMAP | ER.F64), (ONE, ER.INTMAP | ER.BOOL), (ONE, ER.INTMAP | ER.INT), (ONE, ER.STRMAP | ER.F64)]
VAR_SHAPES = ((None, R.STRING), (R.STRING, R.I64), (R.STRING, R.STRING), (R.I32, R.STRING), (R.BYTE, R.STRING),
              (R.STRING, R.DOUBLE), (R.STRING, R.BYTE))
FIXED_SHAPES = ((R.I32, R.DOUBLE), (R.BYTE, R.BOOL), (R.I64, R.I16), (R.I16, R.I64), (R.BYTE, R.BYTE), (R.I64, R.DOUBLE))


def shape_message(kt, vt, count):
    if kt is None:
        return msg(R.SET if count % 3 == 0 else R.LIST, lst(vt, count, b"".join(one(vt, j) for j in range(count))))
    return msg(R.MAP, mp(kt, vt, count, entries(kt, vt, count)))


def count_messages(seed=41):
    """every count of VAR_COUNTS under every variable-stride shape and of
    FIXED_COUNTS under every fixed-stride one, shuffled, between them empty
    structs and an i32 field"""
    rng = random.Random(seed)
    msgs = [shape_message(kt, vt, c) for kt, vt in VAR_SHAPES for c in VAR_COUNTS]
    msgs += [shape_message(kt, vt, c) for kt, vt in FIXED_SHAPES for c in FIXED_COUNTS]
    msgs += [b"\x00"] * 5 + [msg(R.I32, b"\0\0\0\5")] * 2
    rng.shuffle(msgs)
    return msgs


# ------------------------------------------------------- the staged emit's R
STAGE_RS = (4, 8, 16)
STAGE_COLUMNS = [([(F, 1)], ER.LISTSTR), ([(F, 2)], ER.STRMAP | ER.STR), ([(F, 3)], ER.INTMAP | ER.STR)]


def stage_messages(n=150, seed=43):
    """struct{1: list<string>, 2: map<string, string>, 3: map<i16, string>} with
    counts drawn from R - 1, R, R + 1 and 2 R + 1 of every R, 0 and 1:
    neighbours in a wave have unequal counts, and the last wave is not full"""
    rng = random.Random(seed)
    counts = sorted({c for r in STAGE_RS for c in (r - 1, r, r + 1, 2 * r + 1)} | {0, 1})
    out = []
    for _ in range(n):
        a, b, c = (rng.choice(counts) for _ in range(3))
        out.append(fld(R.LIST, 1, lst(R.STRING, a, b"".join(one(R.STRING, j) for j in range(a)))) +
                   fld(R.MAP, 2, mp(R.STRING, R.STRING, b, entries(R.STRING, R.STRING, b))) +
                   fld(R.MAP, 3, mp(R.I16, R.STRING, c, entries(R.I16, R.STRING, c))) + b"\x00")
    return out, counts


# ------------------------------------------ alignment and the end of the arena
TARGETS = {
    "list<string>": (R.LIST, lst(R.STRING, 2, wstr(b"ab") + wstr(b"tail"))),
    "set<string> ending in an empty one": (R.SET, lst(R.STRING, 2, wstr(b"x") + wstr(b""))),
    "map<string,i64>": (R.MAP, mp(R.STRING, R.I64, 2, entries(R.STRING, R.I64, 2))),
    "map<string,bool>": (R.MAP, mp(R.STRING, R.BOOL, 1, wstr(b"k") + b"\x01")),
    "map<string,string>": (R.MAP, mp(R.STRING, R.STRING, 2, entries(R.STRING, R.STRING, 2))),
    "map<i32,double>": (R.MAP, mp(R.I32, R.DOUBLE, 3, entries(R.I32, R.DOUBLE, 3))),
    "map<i8,i8>": (R.MAP, mp(R.BYTE, R.BYTE, 1, b"\xff\x80")),
    "map<i8,bool>": (R.MAP, mp(R.BYTE, R.BOOL, 2, b"\x80\x01\x01\x02")),
    "map<i64,string>": (R.MAP, mp(R.I64, R.STRING, 1, one(R.I64, 1) + wstr(b""))),
    "empty map": (R.MAP, mp(R.STRING, R.I32, 0)),
    "empty list": (R.LIST, lst(R.STRING, 0)),
}
ALIGN_COLUMNS = [([(F, 2)], k) for k in ER.KINDS[:8]]
ALIGN_COLUMNS_B = [([(F, 2)], ER.KINDS[8])]


def align_batch(target: str):
    """16 messages struct{1: string of 0..15 bytes, 2: the target} WITHOUT the
    STOP byte: the target starts at every residue mod 16 and is the last bytes
    of its message, the last message's the last of the arena."""
    t, body = TARGETS[target]
    return [fld(R.STRING, 1, wstr(b"x" * n)) + fld(t, 2, body) for n in range(16)]


# ------------------------------------------------------------ launch geometry
GEOMETRY_COLUMNS = [([(F, 1)], ER.LISTSTR), ([(F, 2)], ER.STRMAP | ER.INT), ([(F, 3)], ER.INTMAP | ER.F64),
                    ([(F, 4)], ER.INTMAP | ER.STR), ([(F, 5)], ER.STRMAP | ER.STR), ([(F, 6)], ER.INTMAP | ER.BOOL),
                    ([(F, 7)], ER.STRMAP | ER.F64), ([(F, 3)], ER.INTMAP | ER.INT)]
_GEO = ((R.LIST, None, R.STRING), (R.MAP, R.STRING, R.I32), (R.MAP, R.I16, R.DOUBLE), (R.MAP, R.I64, R.STRING),
        (R.MAP, R.STRING, R.STRING), (R.MAP, R.BYTE, R.BOOL), (R.MAP, R.STRING, R.DOUBLE))


def geometry_message(rng):
    """struct{1: list<string>, 2: map<string, i32>, 3: map<i16, double>, 4:
    map<i64, string>, 5: map<string, string>, 6: map<i8, bool>, 7: map<string,
    double>} of 0..4 entries, each field kept with p = 0.8"""
    out = bytearray()
    for fid, (t, kt, vt) in enumerate(_GEO, 1):
        if rng.random() >= 0.8:
            continue
        c, salt = rng.randrange(5), rng.randrange(100)
        body = b"".join((one(kt, j + salt) if kt else b"") + one(vt, j + salt + 1) for j in range(c))
        out += fld(t, fid, lst(vt, c, body) if kt is None else mp(kt, vt, c, body))
    return bytes(out) + b"\x00"


def geometry_messages(n, seed=5):
    rng = random.Random(seed)
    return [geometry_message(rng) for _ in range(n)]


# ------------------------------------------------------------ the deep pass
DEEP_DEPTHS = (6, 7, 8, 9, 10, 11, 12)
LDS_FRAMES = 8
DEEP_COLUMNS = [([(F, 2)], ER.STRMAP | ER.INT)] + [([(F, 1)] + [(I, 0)] * d, ER.LISTSTR) for d in DEEP_DEPTHS]
DEEP_LEAF = [b"ab", b"", b"leaf"]


def deep_message(d):
    """struct{1: d lists of one element around a list<string> of DEEP_LEAF, 2: map<string, i64> of 2}: skipping
    field 1 opens d + 1 frames; d index steps reach the leaf"""
    v = lst(R.STRING, len(DEEP_LEAF), b"".join(map(wstr, DEEP_LEAF)))
    for _ in range(d):
        v = lst(R.LIST, 1, v)
    return fld(R.LIST, 1, v) + fld(R.MAP, 2, mp(R.STRING, R.I64, 2, entries(R.STRING, R.I64, 2))) + b"\x00"


def deep_messages(per_depth=3):
    return [deep_message(d) for d in DEEP_DEPTHS for _ in range(per_depth)]


# ----------------------------------------------------------------- fuzz sets
# t2jgen.all_types_desc: 19 list<string>, 20 map<string, i64>, 13 map<i32, bool>, 14 map<i64, binary>, 12 and 15 maps
# with other values, 11 list<i32>, 3 an i32
FUZZ_A = [([(F, 19)], ER.LISTSTR), ([(F, 20)], ER.STRMAP | ER.INT), ([(F, 13)], ER.INTMAP | ER.BOOL),
          ([(F, 14)], ER.INTMAP | ER.STR), ([(F, 12)], ER.STRMAP | ER.STR), ([(F, 15)], ER.INTMAP | ER.INT),
          ([(F, 11)], ER.LISTSTR), ([(F, 3)], ER.STRMAP | ER.INT)]
FUZZ_B = [([(F, 20)], ER.STRMAP | ER.STR), ([(F, 20)], ER.INTMAP | ER.INT), ([(F, 13)], ER.INTMAP | ER.INT),
          ([(F, 14)], ER.STRMAP | ER.STR), ([(F, 1000)], ER.LISTSTR), ([(F, 19)], ER.STRMAP | ER.BOOL),
          ([(F, 19), (I, 0)], ER.LISTSTR), ([(F, 16)], ER.STRMAP | ER.F64)]
FUZZ_SEEDS = (1234, 4321)  # the messages' and the mutations': chosen so that the checker alone finds every status


def fuzz_corpus(n=1024):
    import t2jgen
    rng, mrng = random.Random(FUZZ_SEEDS[0]), random.Random(FUZZ_SEEDS[1])
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(n)]
    return [m if j % 2 else t2jgen.mutate(mrng, m) for j, m in enumerate(msgs)]


# ------------------------------------------------------------------- helpers
def expect(msgs, columns, root_type=R.STRUCT, first=0):
    """[the checker's cells of column k over msgs, for every column]"""
    return [ER.column(msgs, p, k, root_type, first) for p, k in columns]


def by_status(cells):
    """[count of OK, NOT_FOUND, E_READ, E_TYPE, E_UNSUPPORTED] over a column or a list of columns"""
    flat = [c for col in cells for c in col] if cells and isinstance(cells[0], list) else cells
    return [sum(c.status == st for c in flat) for st in range(5)]


CELL_FIELDS = ("status", "type", "step", "aux", "val", "len", "span")
ENTRY_FIELDS = ("keys", "klens", "vals", "vlens")


def arrays(col):
    """One column of checker cells as numpy arrays: the cell fields, the
    entries of its OK cells back to back and their offsets."""
    import numpy as np
    out = {f: np.array([getattr(c, f) for c in col], dtype=np.uint64) for f in CELL_FIELDS}
    out["off"] = np.concatenate([[0], np.cumsum([c.len for c in col])]).astype(np.uint64)
    for f in ENTRY_FIELDS:
        out[f] = np.array([e for c in col if c.vals for e in getattr(c, f)], dtype=np.uint64)
    return out


def same(got, want, what):
    """got / want: dicts as arrays() gives them (got may lack fields)"""
    import numpy as np
    for f in want:
        if f not in got or got[f] is None:
            continue
        g, w = np.asarray(got[f]).astype(np.uint64), want[f]
        assert g.shape == w.shape, "%s: %s has shape %s, checker %s" % (what, f, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s: %s differs at %s: got %#x, checker %#x" % (
            what, f, bad[:5].tolist(), int(g[bad[0]]), int(w[bad[0]]))


def written(kind):
    """the entry arrays a column of `kind` writes"""
    fs = ["vals"]
    if kind != ER.LISTSTR:
        fs.append("keys")
    if kind & ER.STRMAP:
        fs.append("klens")
    if kind == ER.LISTSTR or kind & 15 == ER.STR:
        fs.append("vlens")
    return fs


def write_corpus(path, msgs, columns, blob: bytes, root_type: int = R.STRUCT):
    """The file ents_host.cpp's stand-alone program (-DENTS_MAIN) reads: u32
    n_msgs, n_cols, root_type, off_steps, off_pool, blob length; the kinds (8
    bytes); the path-set blob; per message a u32 length and the bytes."""
    n_paths, _, off_steps, off_pool = struct.unpack_from("<4I", blob, 12)
    assert n_paths == len(columns)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<6I", len(msgs), n_paths, root_type, off_steps, off_pool, len(blob)))
        fh.write(bytes([k for _, k in columns]).ljust(8, b"\0") + blob)
        for m in msgs:
            fh.write(struct.pack("<I", len(m)) + m)
