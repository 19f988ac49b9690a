"""Built inputs of the typed-column tests, shared by the CPU build of the decode
(test_cols_host.py) and the GPU tests (test_gpu_cols.py): every wire type under
every kind with values at the width edges, targets at every residue mod 16 and
at the arena's end, chains around the 8 LDS frames, lists of every element
width around the block sizes, and the fuzz column sets."""
import random
import struct

import colsref as CR
import tgetgen as TG
import tgetref as R

F, I = R.FIELD, R.INDEX
ONE = [(F, 1)]


def fld(t, fid, body=b""):
    return struct.pack(">bh", t, fid) + body


def wstr(s: bytes) -> bytes:
    return struct.pack(">i", len(s)) + s


def lst(et, count, body=b""):
    return struct.pack(">Bi", et, count) + body


# ------------------------------------------------------ kind x wire-type matrix
DOUBLES = (0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
           0x7FF8000000C0FFEE,  # a quiet NaN with a payload
           0x7FF4000000BADBAD,  # a signalling NaN with a payload
           0xFFF0000000000001,  # a signalling NaN, sign set, the smallest payload
           0x0000000000000001,  # the smallest denormal
           0x3FF8000000000000)  # 1.5


def matrix_messages():
    """struct{1: <a value of wire type t>} for t = 0..17 (0 ends the struct:
    the field is not found; 5, 7, 9 are no types; 1, 16, 17 are types nothing
    can skip), values at the width edges, containers with counts 0, 1 and
    2^31 - 1 over a short body."""
    vals = {
        0: [b""], 1: [b"\x01\x02"], 5: [b"\x00" * 8], 7: [b"\x00" * 8], 9: [b"\x00" * 8], 16: [b"\0\0\0\0"],
        17: [b"\0\0\0\0"],
        R.BOOL: [bytes([b]) for b in (0, 1, 2, 0xFF)],
        R.BYTE: [bytes([b]) for b in (0x00, 0x7F, 0x80, 0xFF)],
        R.I16: [struct.pack(">h", v) for v in (-2 ** 15, -1, 2 ** 15 - 1)],
        R.I32: [struct.pack(">i", v) for v in (-2 ** 31, -1, 2 ** 31 - 1)],
        R.I64: [struct.pack(">q", v) for v in (-2 ** 63, -1, 2 ** 63 - 1)],
        R.DOUBLE: [struct.pack(">Q", v) for v in DOUBLES],
        R.STRING: [wstr(b""), wstr(b"abc"), wstr(bytes(range(40)))],
        R.STRUCT: [b"\x00", fld(R.I32, 1, b"\0\0\0\x07") + b"\x00"],
        R.MAP: [struct.pack(">BBi", R.I32, R.I32, 0), struct.pack(">BBi", R.I32, R.I64, 1) + b"\0" * 12,
                struct.pack(">BBi", R.I32, R.I32, 2 ** 31 - 1) + b"\0" * 16,
                struct.pack(">BBi", R.STRING, R.I32, 2) + wstr(b"k") + b"\0\0\0\1" + wstr(b"kk") + b"\0\0\0\2"],
    }
    for t in (R.LIST, R.SET):
        vals[t] = [lst(R.I32, 0), lst(R.I32, 1, b"\xff\xff\xff\xfe"), lst(R.I32, 2 ** 31 - 1, b"\0" * 16),
                   lst(R.DOUBLE, 2, struct.pack(">QQ", DOUBLES[4], DOUBLES[1])), lst(R.I64, 1, b"\x80" + b"\0" * 7),
                   lst(R.BYTE, 3, b"\x7f\x80\xff"), lst(R.I16, 2, b"\x80\x00\x7f\xff"),
                   lst(R.STRING, 0), lst(R.STRING, 2, wstr(b"a") + wstr(b"")), lst(R.BOOL, 2, b"\x01\x00"),
                   lst(R.BOOL, 0), lst(5, 0), lst(5, 1, b"\0" * 8), lst(R.STRUCT, 1, b"\x00"),
                   lst(R.LIST, 1, lst(R.I32, 1, b"\0\0\0\1"))]
    out = []
    for t in range(18):
        for v in vals[t]:
            out.append(b"\x00" if t == 0 else fld(t, 1, v) + b"\x00")
    return out


MATRIX_COLUMNS = [(ONE, k) for k in CR.KINDS]

# ------------------------------------------ alignment and the end of the arena
TARGETS = {
    "bool": (R.BOOL, b"\x01"), "byte": (R.BYTE, b"\x80"), "i16": (R.I16, b"\x80\x01"), "i32": (R.I32, b"\x80\0\0\x01"),
    "i64": (R.I64, b"\x80\0\0\0\0\0\0\x01"), "double": (R.DOUBLE, struct.pack(">Q", DOUBLES[5])),
    "string": (R.STRING, wstr(b"tail")), "empty string": (R.STRING, wstr(b"")),
    "list<byte>": (R.LIST, lst(R.BYTE, 3, b"\x01\x80\xff")), "list<i32>": (R.LIST, lst(R.I32, 2, b"\x80\0\0\0\0\0\0\x02")),
    "set<double>": (R.SET, lst(R.DOUBLE, 1, struct.pack(">Q", DOUBLES[6]))), "empty list": (R.LIST, lst(R.I64, 0)),
    "map": (R.MAP, struct.pack(">BBi", R.BYTE, R.BYTE, 1) + b"\x01\x02"),
}
ALIGN_COLUMNS = [([(F, 2)], k) for k in CR.KINDS]


def align_batch(target: str):
    """16 messages struct{1: string of 0..15 bytes, 2: the target} WITHOUT the
    STOP byte: the target's value starts at every residue mod 16 and is the
    last bytes of its message, the last message's the last of the arena."""
    t, body = TARGETS[target]
    return [fld(R.STRING, 1, wstr(b"x" * n)) + fld(t, 2, body) for n in range(16)]


# ------------------------------------------------------------ launch geometry
GEOMETRY_COLUMNS = [([(F, 1)], CR.INT), ([(F, 2)], CR.STR), ([(F, 3)], CR.LIST_INT), ([(F, 4)], CR.F64),
                    ([(F, 3)], CR.LEN), ([(F, 5)], CR.BOOL), ([(F, 6)], CR.BYTE), ([(F, 7)], CR.LIST_F64)]


def geometry_message(rng):
    """struct{1: i32, 2: string, 3: list<i16>, 4: double, 5: bool, 6: byte, 7: set<double>}, each kept with p = 0.8"""
    out = bytearray()
    parts = [fld(R.I32, 1, struct.pack(">i", rng.randrange(-2 ** 31, 2 ** 31))),
             fld(R.STRING, 2, wstr(bytes(rng.randrange(256) for _ in range(rng.randrange(12))))),
             fld(R.LIST, 3, lst(R.I16, 3, struct.pack(">hhh", *(rng.randrange(-2 ** 15, 2 ** 15) for _ in range(3))))),
             fld(R.DOUBLE, 4, struct.pack(">d", rng.random() - 0.5)), fld(R.BOOL, 5, bytes([rng.randrange(3)])),
             fld(R.BYTE, 6, bytes([rng.randrange(256)])),
             fld(R.SET, 7, lst(R.DOUBLE, 2, struct.pack(">dd", rng.random(), -rng.random())))]
    for p in parts:
        if rng.random() < 0.8:
            out += p
    return bytes(out) + b"\x00"


def geometry_messages(n, seed=5):
    rng = random.Random(seed)
    return [geometry_message(rng) for _ in range(n)]


# ----------------------------------------------------------------- fuzz sets
FUZZ_A = [([(F, 1)], CR.BOOL), ([(F, 2)], CR.BYTE), ([(F, 3)], CR.INT), ([(F, 4)], CR.INT), ([(F, 5)], CR.INT),
          ([(F, 6)], CR.F64), ([(F, 7)], CR.STR), ([(F, 11)], CR.LIST_INT)]
FUZZ_B = [([(F, 1000)], CR.INT), ([(F, 1000)], CR.F64), ([(F, 1000)], CR.STR), ([(F, 1000)], CR.BOOL),
          ([(F, 1000)], CR.LEN), ([(F, 9), (F, 1)], CR.INT), ([(F, 11), (I, 2)], CR.INT), ([(F, 19)], CR.LIST_INT)]

# ---------------------------------------------------------- deep pass (chains)
DEEP_LIST_DEPTHS = (6, 7, 8, 9, 10, 11)
DEEP_COLUMNS = [([(F, 2)], CR.INT), ([(F, 1)], CR.LEN)] + \
    [([(F, 1)] + [(I, 0)] * d, CR.LIST_INT) for d in DEEP_LIST_DEPTHS]


def deep_chains(seed=21, per_depth=6):
    """(kinds, leaf) of chains of 6..12 levels: the all-L chains over leaf l
    (a list<i64> of 1, -1 that the list columns reach by index steps) and
    random ones."""
    rng = random.Random(seed)
    chains = [("L" * d, "l") for d in range(6, 13)]
    chains += [TG.random_chain(rng, d) for d in range(6, 13) for _ in range(per_depth)]
    rng.shuffle(chains)
    return chains


# --------------------------------------------------------------------- lists
LIST_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
LIST_COLUMNS = [(ONE, CR.LIST_INT), (ONE, CR.LIST_F64), (ONE, CR.LEN)]
_EL = {R.BYTE: ">B", R.I16: ">H", R.I32: ">I", R.I64: ">Q", R.DOUBLE: ">Q"}


def list_body(et, count, salt=0):
    """count elements of type et whose top bit alternates, so a missed sign or zero extension shows"""
    w = R._TYPE_SIZE[et]
    mask = (1 << (8 * w)) - 1
    return b"".join(struct.pack(_EL[et], ((j + salt) * 0x9E3779B97F4A7C15 >> 7 ^ (j & 1) << (8 * w - 1)) & mask)
                    for j in range(count))


def list_messages(seed=31):
    """struct{1: list or set<T> of c}: every count of LIST_COUNTS at every
    element width and double, as LIST and as SET, in shuffled order, between
    them empty structs (not found), empty lists, lists of strings and bools
    (unsupported when not empty), an i32 field (unsupported) and lists cut
    short in their last element (E_READ: the message ends early)."""
    rng = random.Random(seed)
    msgs = []
    for k, et in enumerate((R.BYTE, R.I16, R.I32, R.I64, R.DOUBLE)):
        for c in LIST_COUNTS:
            t = R.SET if (c + k) % 3 == 0 else R.LIST
            msgs.append(fld(t, 1, lst(et, c, list_body(et, c, salt=c))) + b"\x00")
        cut = fld(R.LIST, 1, lst(et, 65, list_body(et, 65)))
        msgs.append(cut[:-1])                       # the last element one byte short
        msgs.append(fld(R.LIST, 1, lst(et, 2 ** 31 - 1, list_body(et, 3))))
    msgs += [b"\x00"] * 6 + [fld(R.LIST, 1, lst(R.STRING, 0)) + b"\x00"] * 3
    msgs += [fld(R.LIST, 1, lst(R.STRING, 2, wstr(b"a") + wstr(b"bc"))) + b"\x00", fld(R.SET, 1, lst(R.BOOL, 2, b"\1\0")) + b"\x00",
             fld(R.I32, 1, b"\0\0\0\5") + b"\x00", fld(R.LIST, 1, lst(7, 0)) + b"\x00",
             fld(R.MAP, 1, struct.pack(">BBi", R.I32, R.I32, 1) + b"\0" * 8) + b"\x00"]
    rng.shuffle(msgs)
    return msgs


# ------------------------------------------------------------------- helpers
def expect(msgs, columns, root_type=R.STRUCT, first=0):
    """[the checker's cells of column k over msgs, for every column]"""
    return [CR.column(msgs, p, k, root_type, first) for p, k in columns]


def share(cells, status):
    flat = [c for col in cells for c in col] if cells and isinstance(cells[0], list) else cells
    return sum(c.status == status for c in flat) / max(len(flat), 1)


def write_corpus(path, msgs, columns, blob: bytes, root_type: int = R.STRUCT):
    """The file cols_host.cpp's stand-alone program (-DCOLS_MAIN) reads: u32
    n_msgs, n_cols, root_type, off_steps, off_pool, blob length; the kinds (8
    bytes); the path-set blob; per message a u32 length and the bytes."""
    n_paths, _, off_steps, off_pool = struct.unpack_from("<4I", blob, 12)
    assert n_paths == len(columns)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<6I", len(msgs), n_paths, root_type, off_steps, off_pool, len(blob)))
        fh.write(bytes([k for _, k in columns]).ljust(8, b"\0") + blob)
        for m in msgs:
            fh.write(struct.pack("<I", len(m)) + m)


CELL_FIELDS = ("status", "type", "step", "aux", "val", "len")


def arrays(col):
    """One column of checker cells as numpy arrays: the six cell fields, the
    elements of its OK list cells back to back (u64) and their offsets."""
    import numpy as np
    out = {f: np.array([getattr(c, f) for c in col], dtype=np.uint64) for f in CELL_FIELDS}
    counts = [len(c.elems) if c.elems else 0 for c in col]
    out["off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    out["elems"] = np.array([e for c in col if c.elems for e in c.elems], dtype=np.uint64)
    return out


def same(got, want, what):
    """got / want: dicts as arrays() gives them (got may lack elems / off)"""
    import numpy as np
    for f in want:
        if f not in got:
            continue
        g, w = np.asarray(got[f]).astype(np.uint64), want[f]
        assert g.shape == w.shape, "%s: %s has shape %s, checker %s" % (what, f, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s: %s differs at %s: got %#x, checker %#x" % (
            what, f, bad[:5].tolist(), int(g[bad[0]]), int(w[bad[0]]))
