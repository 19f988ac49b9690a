"""Built inputs of the map-row tests, shared by the CPU build of the map head and
index (test_mrows_host.py) and the GPU tests (test_gpu_mrows.py). Each set is a
(messages, parent path, row columns, root type, key kind) tuple; the pieces are
colsgen's, kidsgen's, rowsgen's and tgetgen's, put below a map: every key type
over every value type under both key kinds, all 256 key and value type bytes,
parents that are no map, headers ReadMapBegin refuses, keys at the width edges,
entries that end where their message or the arena ends, maps around the block
sizes between empty and failed messages, fixed-size maps (the arithmetic route)
beside the same data under string keys (the walk), and chains around the 8 LDS
frames inside the values."""
import random
import struct
from collections import namedtuple

import numpy as np

import colsgen as CG
import colsref as CR
import kidsgen as KG
import mrowsref as MR
import rowsgen as RG
import tgetgen as TG
import tgetref as R

F, I = R.FIELD, R.INDEX
ONE = [(F, 1)]
fld, wstr, lst = CG.fld, CG.wstr, CG.lst
STR, INT = MR.KEY_STR, MR.KEY_INT
Set = namedtuple("Set", "msgs parent columns root_type keys")
_KFMT = {R.BYTE: ">B", R.I16: ">H", R.I32: ">I", R.I64: ">Q"}


def ikey(kt, v):
    """an integer key of wire type kt, two's complement"""
    return struct.pack(_KFMT[kt], v % (1 << 8 * R._TYPE_SIZE[kt]))


def mmap(kt, vt, ents, size=None):
    """a map's bytes: ents = [(key bytes, value bytes)]"""
    return struct.pack(">BBi", kt, vt, len(ents) if size is None else size) + b"".join(k + v for k, v in ents)


def map_field(kt, vt, ents, fid=1, size=None):
    return fld(R.MAP, fid, mmap(kt, vt, ents, size))


# ---------------------------------------------------- key type x value type
_INNER = fld(R.I32, 1, struct.pack(">i", -7)) + fld(R.STRING, 2, wstr(b"in")) + b"\x00"
VALUES = {
    R.BOOL: [b"\x00", b"\x01", b"\x02"],
    R.I64: [struct.pack(">q", v) for v in (-2 ** 63, -1, 2 ** 63 - 1)],
    R.DOUBLE: [struct.pack(">Q", v) for v in CG.DOUBLES[:3]],
    R.STRING: [wstr(b""), wstr(b"abc"), wstr(bytes(range(40)))],
    R.STRUCT: [_INNER, b"\x00", fld(R.I64, 1, struct.pack(">q", 2 ** 40)) + b"\x00"],
    R.LIST: [lst(R.I32, 0), lst(R.I32, 2, b"\xff\xff\xff\xfe\0\0\0\1"), lst(R.STRING, 1, wstr(b"a"))],
    R.MAP: [mmap(R.I32, R.I32, []), mmap(R.I32, R.I64, [(b"\0\0\0\1", b"\0" * 8)]),
            mmap(R.STRING, R.STRING, [(wstr(b"k"), wstr(b"v"))])],
}
KEYS = {
    R.BYTE: [ikey(R.BYTE, v) for v in (0x00, 0x7F, 0x80)], R.I16: [ikey(R.I16, v) for v in (-1, 2 ** 15 - 1, -2 ** 15)],
    R.I32: [ikey(R.I32, v) for v in (-1, 2 ** 31 - 1, -2 ** 31)], R.I64: [ikey(R.I64, v) for v in (-2 ** 63, 2 ** 63 - 1, -1)],
    R.STRING: [wstr(b""), wstr(b"k"), wstr(b"a longer key of 27 bytes..")],
}
MATRIX_COLUMNS = [([], CR.LEN), ([(F, 1)], CR.INT), ([], CR.INT), ([], CR.STR), ([], CR.LIST_INT), ([], CR.F64),
                  ([], CR.BOOL), ([(I, 1)], CR.INT)]


def matrix_sets():
    msgs = [map_field(kt, vt, list(zip(ks, vs))) + b"\x00" for kt, ks in KEYS.items() for vt, vs in VALUES.items()]
    return {"matrix, str keys": Set(msgs, ONE, MATRIX_COLUMNS, R.STRUCT, STR),
            "matrix, int keys": Set(msgs, ONE, MATRIX_COLUMNS, R.STRUCT, INT)}


# --------------------------------------------------------------- the heads
HEAD_COLUMNS = [([(F, 1)], CR.INT), ([], CR.LEN)]


def head_sets():
    """what only the head sees: all 256 key type bytes and all 256 value type bytes at size 0 and 1, negative
    counts, a parent of every wire type, maps and others as the root, one message cut at every prefix"""
    out = {}
    msgs = [fld(R.MAP, 1, struct.pack(">BBi", kt, R.I32, size) + b"\0" * 16) + b"\x00" for kt in range(256) for size in (0, 1)]
    for kt in (R.I32, R.STRING):
        msgs += [fld(R.MAP, 1, struct.pack(">BBi", kt, vt, size) + b"\0" * 16) + b"\x00" for vt in range(256) for size in (0, 1)]
        msgs += [fld(R.MAP, 1, struct.pack(">BBi", kt, R.I32, c)) + b"\x00" for c in (-1, -2 ** 31)]
    for kind, name in ((STR, "str"), (INT, "int")):
        out["type bytes, %s keys" % name] = Set(msgs, ONE, HEAD_COLUMNS, R.STRUCT, kind)
        out["parents of every type, %s keys" % name] = Set(CG.matrix_messages() + list(KG.hand_messages().values()), ONE,
                                                           HEAD_COLUMNS, R.STRUCT, kind)
    ents = [(wstr(b"first"), _INNER), (wstr(b""), b"\x00"), (wstr(b"x"), fld(R.LIST, 3, lst(R.STRING, 1, wstr(b"x"))) + b"\x00")]
    whole = fld(R.I32, 7, b"\0\0\0\1") + map_field(R.STRING, R.STRUCT, ents) + fld(R.I32, 2, b"\0\0\0\2") + b"\x00"
    out["prefixes"] = Set(KG.prefixes(whole), ONE, HEAD_COLUMNS, R.STRUCT, STR)
    body = mmap(R.STRING, R.STRUCT, ents)
    ibody = mmap(R.I16, R.I64, [(b"\xff\xff", b"\0" * 8), (b"\0\1", b"\xff" * 8)])
    roots = [body, ibody, b"", body[:6], body[:5], ibody[:-1], mmap(R.DOUBLE, R.I32, []), whole]
    for rt in (R.MAP, R.STRUCT, R.LIST, R.I32, 0x1F):
        for kind, name in ((STR, "str"), (INT, "int")):
            out["root type %d, %s keys" % (rt, name)] = Set(roots, [], HEAD_COLUMNS, rt, kind)
    return out


# ------------------------------------------------------------------- keys
def key_sets():
    """keys at the width edges, string keys of length 0 and 1, duplicate keys, first entries at every residue mod 16
    with the last value the arena's last bytes, and a string key whose payload ends where the message and the arena
    end (the value is missing: E_READ, and the key's last byte is the last the walk may touch)"""
    v = struct.pack(">i", 5)
    out = {}
    edge = {R.BYTE: (0x00, 0x7F, 0x80, 0xFF), R.I16: (-1, 0, 2 ** 15 - 1, -2 ** 15), R.I32: (-1, 2 ** 31 - 1, -2 ** 31),
            R.I64: (-2 ** 63, 2 ** 63 - 1, -1, 0)}
    msgs = [map_field(kt, R.I32, [(ikey(kt, k), v) for k in ks]) + b"\x00" for kt, ks in edge.items()]
    msgs += [map_field(kt, R.STRING, [(ikey(kt, k), wstr(b"s%d" % j)) for j, k in enumerate(ks)]) + b"\x00"
             for kt, ks in edge.items()]  # the same keys on the walk
    msgs.append(map_field(R.I32, R.I32, [(ikey(R.I32, 3), v)] * 3 + [(ikey(R.I32, 4), v), (ikey(R.I32, 3), b"\0\0\0\6")]) + b"\x00")
    out["int key edges"] = Set(msgs, ONE, [([], CR.INT), ([], CR.STR)], R.STRUCT, INT)
    smsgs = [map_field(R.STRING, R.I32, [(wstr(b""), v), (wstr(b"k"), v), (wstr(b"k"), b"\0\0\0\6"), (wstr(b""), v)]) + b"\x00",
             map_field(R.STRING, R.STRING, [(wstr(b"dup"), wstr(b"a")), (wstr(b"dup"), wstr(b"b"))]) + b"\x00"]
    out["string keys"] = Set(smsgs, ONE, [([], CR.INT), ([], CR.STR)], R.STRUCT, STR)
    two = [(F, 2)]
    for name, (kt, vt, ents, cols, kind) in {
        "map<i32,i64>": (R.I32, R.I64, [(ikey(R.I32, -1), struct.pack(">q", -2)), (ikey(R.I32, 7), struct.pack(">q", 2 ** 62))],
                         [([], CR.INT)], INT),
        "map<byte,bool>": (R.BYTE, R.BOOL, [(b"\x80", b"\x01"), (b"\xff", b"\x00")], [([], CR.BOOL)], INT),
        "map<string,string>": (R.STRING, R.STRING, [(wstr(b"ab"), wstr(b"xyz")), (wstr(b""), wstr(b""))], [([], CR.STR)], STR),
        "map<i64,string>": (R.I64, R.STRING, [(ikey(R.I64, -2 ** 63), wstr(b"t"))], [([], CR.STR)], INT),
        "map<string,struct>": (R.STRING, R.STRUCT, [(wstr(b"k"), _INNER), (wstr(b"kk"), b"\x00")], RG.BOUND_COLUMNS, STR),
    }.items():
        msgs, base = [], 0
        for r in range(16):  # entry 0's key lies 16 + pad bytes into its message: at arena offset r mod 16
            msgs.append(fld(R.STRING, 1, wstr(b"x" * ((r - base - 16) % 16))) + map_field(kt, vt, ents, fid=2))
            base += len(msgs[-1])
        out["arena's end, " + name] = Set(msgs, two, cols, R.STRUCT, kind)
    good = map_field(R.STRING, R.I32, [(wstr(b"key"), v)]) + b"\x00"
    cut = map_field(R.STRING, R.I32, [(wstr(b"a"), v), (wstr(b"the last key"), b"")])
    out["a key ends the arena"] = Set([good, cut[:-3], good, cut], ONE, [([], CR.INT)], R.STRUCT, STR)
    return out


# ------------------------------------------------------------- geometry
MAP_SIZES = (0, 1, 2, 63, 64, 65, 257, 2049)


def geometry_batch(sizes, pool, kt, fails=True):
    """struct{1: map<kt, struct> of sizes[i] entries, the values taken from pool in turn, key j of a message the
    integer 7 * j - 100 or its decimal digits}; with fails, after every second one an empty struct (not found), a map
    cut short (E_READ) and an i32 (unsupported) in turn"""
    def key(j):
        return wstr(b"%d" % (7 * j - 100)) if kt == R.STRING else ikey(kt, 7 * j - 100)

    msgs, at = [], 0
    extra = [b"\x00", map_field(kt, R.STRUCT, [(key(0), pool[0]), (key(1), pool[1])])[:-2], fld(R.I32, 1, b"\0\0\0\1") + b"\x00"]
    for j, c in enumerate(sizes):
        msgs.append(map_field(kt, R.STRUCT, [(key(q), pool[(at + q) % len(pool)]) for q in range(c)]) + b"\x00")
        at += c
        if fails and j % 2:
            msgs.append(extra[(j // 2) % 3])
    return msgs


def fixed_batch(sizes, string_keys):
    """struct{1: map<i32, i64>}: the arithmetic route; with string_keys the same data as map<string, i64> with the key's
    four bytes as the payload: the walk. Between them an empty struct and a map one byte short."""
    msgs = []
    for j, c in enumerate(sizes):
        ents = [(ikey(R.I32, (q * 0x9E3779B1) % 2 ** 32), struct.pack(">q", q * 0x0123456789ABCDF - 2 ** 62)) for q in range(c)]
        if string_keys:
            ents = [(wstr(k), v) for k, v in ents]
        msgs.append(map_field(R.STRING if string_keys else R.I32, R.I64, ents) + b"\x00")
        if j % 3 == 1:
            msgs += [b"\x00", msgs[-1][:-2]]
    return msgs


# ------------------------------------------------------------- deep passes
def deep_sets():
    """the values are tgetgen's chain messages (structs that nest 6 to 12 levels): the head's and the index's skip of a
    value, and a row's lookup of field 2 behind the chain, open up to 12 frames"""
    chains = CG.deep_chains(per_depth=3)
    vals = [TG.chain_message(k, lf) for k, lf in chains]
    out = {}
    for kt, kind, name in ((R.STRING, STR, "str"), (R.I64, INT, "int")):
        key = (lambda j: wstr(b"key %d" % j)) if kt == R.STRING else (lambda j: ikey(R.I64, -j))
        msgs = [map_field(kt, R.STRUCT, [(key(q), v) for q, v in enumerate(vals[j:j + 4])]) + b"\x00"
                for j in range(0, len(vals), 3)]
        out["deep values, %s keys" % name] = Set(msgs, ONE, CG.DEEP_COLUMNS, R.STRUCT, kind)
    return out, chains


# -------------------------------------------------------------------- fuzz
# t2jgen.all_types_desc(): 12 map<string, list<i32>>, 13 map<byte, bool>, 14 map<i16, binary>, 15 map<i32, Inner{1: i64,
# 2: string, 3: list<double>}>, 16 map<i64, map<string, double>>, 20 map<string, i64>; field 1000 is the generator's
# unknown field, of a random type (maps of random key and value types among them)
FUZZ_PLANS = {
    "str f12": ([(F, 12)], [([], CR.LIST_INT), ([], CR.LEN), ([(I, 0)], CR.INT), ([(F, 1)], CR.INT)], STR),
    "int f15": ([(F, 15)], [([(F, 1)], CR.INT), ([(F, 2)], CR.STR), ([(F, 3)], CR.LIST_F64), ([(F, 3), (I, 0)], CR.F64),
                            ([], CR.LEN), ([(F, 4)], CR.INT)], INT),
    "str f1000": ([(F, 1000)], [([], CR.INT), ([], CR.STR), ([], CR.LEN)], STR),
    "int f1000": ([(F, 1000)], [([], CR.INT), ([], CR.STR), ([], CR.LEN)], INT),
}
# what the checker alone gives over the 2 048 messages and their mutated form, counted on the CPU:
# {(corpus, plan): (heads by status, cells by status, rows)}
FUZZ_WANT = {
    ("fuzz", "str f12"): ([(0, 1245), (1, 803)], [(0, 5148), (1, 633), (2, 1543)], 1831),
    ("fuzz", "int f15"): ([(0, 1212), (1, 836)], [(0, 4835), (1, 4240), (4, 1815)], 1815),
    ("fuzz", "str f1000"): ([(0, 22), (1, 1386), (4, 640)], [(0, 12), (4, 84)], 32),
    ("fuzz", "int f1000"): ([(0, 31), (1, 1386), (4, 631)], [(0, 30), (4, 105)], 45),
    ("mutated", "str f12"): ([(0, 791), (1, 333), (2, 923), (4, 1)], [(0, 3225), (1, 404), (2, 963)], 1148),
    ("mutated", "int f15"): ([(0, 796), (1, 293), (2, 958), (4, 1)], [(0, 3104), (1, 2765), (4, 1175)], 1174),
    ("mutated", "str f1000"): ([(0, 16), (1, 509), (2, 1056), (4, 467)], [(0, 7), (4, 59)], 22),
    ("mutated", "int f1000"): ([(0, 20), (1, 509), (2, 1056), (4, 463)], [(0, 17), (4, 70)], 29),
}


# ----------------------------------------------------------------- helpers
def arrays(want, P):
    """a checker batch ([mrowsref.Msg]) as the arrays the device returns: rowsgen.arrays' four and the keys (a dict of
    key and key_len over all rows)"""
    head, row_off, index, cols = RG.arrays(want, P)
    keys = [k for m in want for k in m.keys]
    return head, row_off, index, cols, {"key": np.array([k.val for k in keys], dtype=np.uint64),
                                        "key_len": np.array([k.len for k in keys], dtype=np.uint64)}


def same(got, want, what):
    """got / want: (head, row_off, index, cols, keys) as arrays() gives them; got's index, cols and keys may be None"""
    CG.same(got[0], want[0], what + ", head")
    CG.same({"row_off": got[1]}, {"row_off": want[1]}, what)
    if got[2] is not None:
        CG.same(got[2], want[2], what + ", index")
    if got[3] is not None:
        for k, w in enumerate(want[3]):
            CG.same(got[3][k], w, "%s, column %d" % (what, k))
    if got[4] is not None:
        CG.same(got[4], want[4], what + ", keys")


def expect(s: Set, first=0):
    return MR.batch(s.msgs, s.parent, s.columns, s.keys, s.root_type, first)


statuses = RG.statuses


def all_sets():
    """every set but the fuzz corpus, the long maps and the depth-limit chains, by name"""
    out = {}
    for group in (matrix_sets(), head_sets(), key_sets(), deep_sets()[0]):
        out.update(group)
    pool = RG.geometry_elements(64)
    out["geometry, str keys"] = Set(geometry_batch(MAP_SIZES[:7], pool, R.STRING), ONE, CG.GEOMETRY_COLUMNS, R.STRUCT, STR)
    out["geometry, i32 keys"] = Set(geometry_batch(MAP_SIZES[:7], pool, R.I32), ONE, CG.GEOMETRY_COLUMNS, R.STRUCT, INT)
    out["fixed maps"] = Set(fixed_batch(MAP_SIZES[:7], False), ONE, [([], CR.INT)], R.STRUCT, INT)
    out["fixed maps' data, string keys"] = Set(fixed_batch(MAP_SIZES[:7], True), ONE, [([], CR.INT)], R.STRUCT, STR)
    return out


def write_corpus(path, s: Set, parent_blob: bytes):
    """The file mrows_host.cpp's stand-alone program (-DMROWS_MAIN) reads: u32 n_msgs, root_type, key kind, the parent
    blob's length; the parent's path-set blob (generic.compile_paths); per message a u32 length and the bytes."""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4I", len(s.msgs), s.root_type, s.keys, len(parent_blob)) + parent_blob)
        for m in s.msgs:
            fh.write(struct.pack("<I", len(m)) + m)
