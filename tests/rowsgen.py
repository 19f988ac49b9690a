"""Built inputs of the row-column tests, shared by the CPU build of the walk
(test_rows_host.py) and the GPU tests (test_gpu_rows.py). Each set is a
(messages, parent path, row columns, root type) tuple; the pieces are colsgen's,
kidsgen's and tgetgen's, put below a list or set: every kind over every element
wire type, parents that are no list, headers ReadListBegin refuses, lists cut
short, elements that end where their field, their message or the arena ends,
lists around the block sizes between empty and failed messages, and chains
around the 8 LDS frames above the parent and inside the elements."""
import random
import struct
from collections import namedtuple

import numpy as np

import colsgen as CG
import colsref as CR
import kidsgen as KG
import rowsref as RR
import tgetgen as TG
import tgetref as R

F, I = R.FIELD, R.INDEX
ONE = [(F, 1)]
fld, wstr, lst = CG.fld, CG.wstr, CG.lst
Set = namedtuple("Set", "msgs parent columns root_type")


def rows_field(elems, et=R.STRUCT, t=R.LIST, fid=1, size=None):
    """field fid: a list or set of the given elements' bytes"""
    return fld(t, fid, lst(et, len(elems) if size is None else size, b"".join(elems)))


# ------------------------------------------------- kind x element-type matrix
def _well_formed(m):
    return R.get_by_path(m, []).status == R.OK


def matrix_sets():
    """colsgen's matrix one level down: its struct{1: <a value of wire type t>} messages are the elements of a
    list<struct> and of a set<struct> (the ones a skip refuses make a message of their own: its head is E_READ),
    and for every element type the values themselves are the elements, read through the empty sub-path"""
    structs = CG.matrix_messages()
    good = [m for m in structs if _well_formed(m)]
    bad = [m for m in structs if not _well_formed(m)]
    msgs = [rows_field(good, t=t) + b"\x00" for t in (R.LIST, R.SET)]
    msgs += [rows_field(good[:3] + [b] + good[3:5]) + b"\x00" for b in bad]
    msgs += [rows_field([]) + b"\x00", b"\x00"]
    out = {"struct elements": Set(msgs, ONE, CG.MATRIX_COLUMNS, R.STRUCT)}
    vals = {
        R.BOOL: [bytes([b]) for b in (0, 1, 2, 0xFF)], R.BYTE: [bytes([b]) for b in (0x00, 0x7F, 0x80, 0xFF)],
        R.I16: [struct.pack(">h", v) for v in (-2 ** 15, -1, 2 ** 15 - 1)],
        R.I32: [struct.pack(">i", v) for v in (-2 ** 31, -1, 2 ** 31 - 1)],
        R.I64: [struct.pack(">q", v) for v in (-2 ** 63, -1, 2 ** 63 - 1)],
        R.DOUBLE: [struct.pack(">Q", v) for v in CG.DOUBLES],
        R.STRING: [wstr(b""), wstr(b"abc"), wstr(bytes(range(40)))],
        R.LIST: [lst(R.I32, 0), lst(R.I32, 1, b"\xff\xff\xff\xfe"), lst(R.DOUBLE, 2, struct.pack(">QQ", *CG.DOUBLES[4:6])),
                 lst(R.BYTE, 3, b"\x7f\x80\xff"), lst(R.STRING, 2, wstr(b"a") + wstr(b"")), lst(5, 0)],
        R.SET: [lst(R.I16, 2, b"\x80\x00\x7f\xff"), lst(R.I64, 1, b"\x80" + b"\0" * 7)],
        R.MAP: [struct.pack(">BBi", R.I32, R.I32, 0), struct.pack(">BBi", R.I32, R.I64, 1) + b"\0" * 12],
    }
    msgs = []
    for et, vs in vals.items():
        for t in (R.LIST, R.SET):
            msgs.append(rows_field(vs, et, t) + b"\x00")
    out["scalar elements"] = Set(msgs, ONE, [([], k) for k in CR.KINDS], R.STRUCT)
    # the lists themselves as roots: the empty parent path
    out["as root"] = Set([m[3:-1] for m in msgs if m[0] == R.LIST], [], [([], k) for k in CR.KINDS], R.LIST)
    return out


# --------------------------------------------------------------- the heads
def head_sets():
    """what only the head sees: a parent of every wire type (colsgen's matrix under field 1; a STRUCT or MAP parent
    is unsupported after its skip), all 256 element type bytes at size 0 and 1, a negative count, kidsgen's
    hand-built headers, and one message cut at every prefix"""
    cols = [([(F, 1)], CR.INT), ([], CR.LEN)]
    out = {"parents of every type": Set(CG.matrix_messages() + list(KG.hand_messages().values()), ONE, cols, R.STRUCT)}
    msgs = [fld(R.LIST, 1, lst(et, size, b"\0" * 8)) + b"\x00" for et in range(256) for size in (0, 1)]
    msgs += [fld(t, 1, struct.pack(">Bi", R.I32, c)) + b"\x00" for t in (R.LIST, R.SET) for c in (-1, -2 ** 31)]
    out["element types"] = Set(msgs, ONE, cols, R.STRUCT)
    elems = [fld(R.I32, 1, struct.pack(">i", 5)) + fld(R.STRING, 2, wstr(b"ab")) + b"\x00", b"\x00",
             fld(R.LIST, 3, lst(R.STRING, 1, wstr(b"x"))) + fld(R.I32, 1, b"\0\0\0\7") + b"\x00"]
    whole = fld(R.I32, 7, b"\0\0\0\1") + rows_field(elems) + fld(R.I32, 2, b"\0\0\0\2") + b"\x00"
    out["prefixes"] = Set(KG.prefixes(whole), ONE, cols, R.STRUCT)
    # roots that are no list or set: unsupported with the root type, nothing skipped
    for rt in (R.STRUCT, R.MAP, R.I32, 0x1F):
        out["root type %d" % rt] = Set([whole, b"", b"\x00"], [], cols, rt)
    return out


# --------------------------------------------------------- element bounds
BOUND_COLUMNS = [([(F, 1)], CR.INT), ([(F, 2)], CR.INT), ([(F, 2)], CR.STR), ([(F, 3)], CR.F64), ([], CR.LEN)]


def bounds_sets():
    a = fld(R.I32, 1, struct.pack(">i", -5)) + b"\x00"                                          # lacks field 2
    b = fld(R.I32, 1, struct.pack(">i", 6)) + fld(R.I64, 2, struct.pack(">q", -2 ** 63)) + b"\x00"  # has it
    c = fld(R.I32, 1, struct.pack(">i", 7)) + fld(R.STRING, 2, wstr(b"tail")) + b"\x00"         # field 2 ends the element
    d = fld(R.DOUBLE, 3, struct.pack(">Q", CG.DOUBLES[5])) + b"\x00"
    out = {"lacks the next one's field": Set([rows_field([a, b, a, c, d, a]) + b"\x00"] * 3, ONE, BOUND_COLUMNS, R.STRUCT)}
    # 16 messages struct{1: a padding string, 2: the list} WITHOUT the STOP byte: the first elements start at every
    # residue mod 16 of the arena and the last element is the last bytes of its message, the last message's of the arena
    two = [(F, 2)]
    for name, (et, elems, cols) in {
        "list<i64>": (R.I64, [struct.pack(">q", v) for v in (1, -1, 2 ** 63 - 1)], [([], CR.INT), ([], CR.F64)]),
        "list<byte>": (R.BYTE, [b"\x80", b"\xff"], [([], CR.INT), ([], CR.BYTE), ([], CR.BOOL)]),
        "list<string>": (R.STRING, [wstr(b"ab"), wstr(b""), wstr(b"xyz")], [([], CR.STR), ([], CR.INT)]),
        "list<empty string>": (R.STRING, [wstr(b"")], [([], CR.STR)]),
        "list<struct>": (R.STRUCT, [a, c, d], BOUND_COLUMNS),
        "list<list<i16>>": (R.LIST, [lst(R.I16, 2, b"\x80\x00\x00\x01"), lst(R.I16, 0)], [([], CR.LIST_INT), ([], CR.LEN),
                                                                                           ([(I, 1)], CR.INT)]),
    }.items():
        msgs, base = [], 0
        for r in range(16):  # element 0 lies 15 + pad bytes into its message: at arena offset r mod 16
            msgs.append(fld(R.STRING, 1, wstr(b"x" * ((r - base - 15) % 16))) + rows_field(elems, et, fid=2))
            base += len(msgs[-1])
        out["arena's end, " + name] = Set(msgs, two, cols, R.STRUCT)
    return out


# ------------------------------------------------------------- geometry
LIST_SIZES = (0, 1, 2, 63, 64, 65, 257, 2049)


def geometry_elements(count, seed=7):
    """colsgen's geometry messages as the elements: struct{1: i32, 2: string, 3: list<i16>, 4: double, 5: bool,
    6: byte, 7: set<double>}, each field kept with p = 0.8"""
    rng = random.Random(seed)
    return [CG.geometry_message(rng) for _ in range(count)]


def geometry_batch(sizes, pool, fails=True):
    """struct{1: list<struct> of sizes[i] elements taken from pool in turn}; with fails, after every second one an
    empty struct (not found), a list cut short (E_READ) and an i32 (unsupported) in turn"""
    msgs, at = [], 0
    extra = [b"\x00", rows_field(pool[:2])[:-2], fld(R.I32, 1, b"\0\0\0\1") + b"\x00"]
    for j, c in enumerate(sizes):
        msgs.append(rows_field([pool[(at + q) % len(pool)] for q in range(c)]) + b"\x00")
        at += c
        if fails and j % 2:
            msgs.append(extra[(j // 2) % 3])
    return msgs


def sizes_for(total, seed=3):
    """list sizes 0..5 that sum to `total` exactly"""
    rng, out = random.Random(seed + total), []
    while sum(out) < total:
        out.append(min(rng.randrange(6), total - sum(out)))
    return out


# ------------------------------------------------------------- deep passes
def deep_sets():
    """both deep passes across the 8 LDS frames. above: the parent (field 2) lies behind a chain of 6-12 levels
    (field 1) that the lookup skips. inside: the elements are tgetgen's chain messages, so the head's and the index's
    skip of an element, and a row's lookup of field 2 behind the chain, open up to 12 frames."""
    chains = CG.deep_chains(per_depth=3)
    elems = geometry_elements(5)
    above = [TG.chain_message(k, lf)[:-8] + rows_field(elems[:1 + j % 5], fid=2) + b"\x00" for j, (k, lf) in enumerate(chains)]
    inside_elems = [TG.chain_message(k, lf) for k, lf in chains]
    inside = [rows_field(inside_elems[j:j + 4]) + b"\x00" for j in range(0, len(inside_elems), 3)]
    return {"above": Set(above, [(F, 2)], CG.GEOMETRY_COLUMNS[:4], R.STRUCT),
            "inside": Set(inside, ONE, CG.DEEP_COLUMNS, R.STRUCT)}, chains


# -------------------------------------------------------------------- fuzz
# t2jgen.all_types_desc(): field 10 is a list of Inner{1: i64, 2: string, 3: list<double>}; field 1000 is the
# generator's unknown field, of a random type (lists, sets and maps of random element types among them). The key step
# on Inner's list is the lookup's E_TYPE; the int-key step on field 1000's elements is, where they are maps of strings.
FUZZ_PLANS = {
    "f10": ([(F, 10)], [([(F, 1)], CR.INT), ([(F, 2)], CR.STR), ([(F, 3)], CR.LIST_F64), ([(F, 3)], CR.LEN),
                        ([(F, 3), (I, 0)], CR.F64), ([], CR.LEN), ([(F, 3), (R.STRKEY, b"k")], CR.INT), ([(F, 4)], CR.INT)]),
    "f1000": ([(F, 1000)], [([], CR.INT), ([], CR.STR), ([(F, 1)], CR.INT), ([(R.INTKEY, 1)], CR.INT), ([], CR.LEN)]),
}
# what the checker alone gives over the 2 048 messages and their mutated form, counted on the CPU:
# {(corpus, plan): (heads by status, cells by status, rows)}
FUZZ_WANT = {
    ("fuzz", "f10"): ([(0, 1249), (1, 799)], [(0, 8059), (1, 8056), (3, 1455), (4, 2510)], 2510),
    ("fuzz", "f1000"): ([(0, 120), (1, 1386), (4, 542)], [(0, 106), (1, 79), (2, 236), (3, 43), (4, 431)], 179),
    ("mutated", "f10"): ([(0, 800), (1, 299), (2, 949)], [(0, 5032), (1, 5158), (2, 3), (3, 902), (4, 1585)], 1585),
    ("mutated", "f1000"): ([(0, 88), (1, 509), (2, 1056), (4, 395)], [(0, 81), (1, 54), (2, 185), (3, 25), (4, 315)], 132),
}


# ----------------------------------------------------------------- helpers
HEAD_FIELDS = ("first", "count", "status", "type", "elem_type", "step")
ROW_FIELDS = ("off", "len", "msg")


def arrays(want, P):
    """a checker batch ([rowsref.Msg]) as the arrays the device returns: head (a dict of arrays), row_off, index
    (a dict), and per column the six cell fields over all rows, as colsgen.arrays gives them"""
    head = {f: np.array([getattr(m.head, f) for m in want], dtype=np.uint64) for f in HEAD_FIELDS}
    row_off = np.concatenate([[0], np.cumsum([len(m.rows) for m in want])]).astype(np.uint64)
    rows = [r for m in want for r in m.rows]
    index = {f: np.array([getattr(r, f) for r in rows], dtype=np.uint64) for f in ROW_FIELDS}
    cols = [CG.arrays([c[k] for m in want for c in m.cells]) for k in range(P)]
    return head, row_off, index, cols


def same(got, want, what):
    """got / want: (head, row_off, index, cols) as arrays() gives them; got's index may be None"""
    CG.same(got[0], want[0], what + ", head")
    CG.same({"row_off": got[1]}, {"row_off": want[1]}, what)
    if got[2] is not None:
        CG.same(got[2], want[2], what + ", index")
    for k, w in enumerate(want[3]):
        CG.same(got[3][k], w, "%s, column %d" % (what, k))


def expect(s: Set, first=0):
    return RR.batch(s.msgs, s.parent, s.columns, s.root_type, first)


def statuses(want):
    """(the heads' statuses, the cells' statuses) as sorted lists of (status, count)"""
    h, c = {}, {}
    for m in want:
        h[m.head.status] = h.get(m.head.status, 0) + 1
        for row in m.cells:
            for x in row:
                c[x.status] = c.get(x.status, 0) + 1
    return sorted(h.items()), sorted(c.items())


def all_sets():
    """every set but the fuzz corpus and the depth-limit chains, by name"""
    out = {}
    for group in (matrix_sets(), head_sets(), bounds_sets(), deep_sets()[0]):
        out.update(group)
    pool = geometry_elements(64)
    out["geometry"] = Set(geometry_batch(LIST_SIZES[:7], pool), ONE, CG.GEOMETRY_COLUMNS, R.STRUCT)
    return out


def write_corpus(path, s: Set, parent_blob: bytes, sub_blob: bytes):
    """The file rows_host.cpp's stand-alone program (-DROWS_MAIN) reads: u32 n_msgs, n_cols, root_type, the parent
    blob's length, the sub blob's length; the kinds (8 bytes); the two path-set blobs (generic.compile_paths); per
    message a u32 length and the bytes."""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5I", len(s.msgs), len(s.columns), s.root_type, len(parent_blob), len(sub_blob)))
        fh.write(bytes([k for _, k in s.columns]).ljust(8, b"\0") + parent_blob + sub_blob)
        for m in s.msgs:
            fh.write(struct.pack("<I", len(m)) + m)
