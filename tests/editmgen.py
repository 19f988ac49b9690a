"""Inputs of the many-edit tests that the CPU build (test_editm_host.py) and the
GPU tests (test_gpu_editm.py) share. A case is one many-edit applied to a batch:
ManyCase(op, parent, items, msgs, root_type), parent as (kind, value) steps like
tgetref's, items a list of (step, values, val_type), values one `bytes` for all
messages or a list with one entry per message. The expected results come from
editmref alone."""
import random
import struct

import editgen as G
import editmref as M
import t2jgen
import tgetref as R
from editgen import field, wstr

F, I, S, N, B = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
SET, UNSET = M.SET_OP, M.UNSET_OP


class ManyCase:
    def __init__(self, op, parent, items, msgs, root_type=R.STRUCT, what=""):
        self.op, self.parent, self.msgs, self.root_type = op, list(parent), list(msgs), root_type
        self.items = [(it[0], it[1] if len(it) > 1 else b"", it[2] if len(it) > 2 else 0) for it in items]
        self.k = len(self.items)
        self.what = what or "%s %r + %r" % ("set" if op == SET else "unset", parent, [it[0] for it in self.items])
        self._want = None

    @property
    def steps(self):
        return [it[0] for it in self.items]

    @property
    def val_types(self):
        return [it[2] for it in self.items]

    @property
    def shared(self):
        """every message gets the same values"""
        return all(isinstance(it[1], bytes) for it in self.items)

    def value(self, i, j):
        v = self.items[j][1]
        return v if isinstance(v, bytes) else v[i]

    def items_for(self, i):
        return [(st, self.value(i, j), t) for j, (st, _, t) in enumerate(self.items)]

    def want(self, caps=None):
        """[(ret, out)] from the checker; caps: the slot sizes (None: large enough)"""
        if caps is None:
            if self._want is None:
                self._want = [M.edit_many(self.op, m, self.parent, self.items_for(i), self.root_type)
                              for i, m in enumerate(self.msgs)]
            return self._want
        return [M.edit_many(self.op, m, self.parent, self.items_for(i), self.root_type, c)
                for i, (m, c) in enumerate(zip(self.msgs, caps))]

    def bound(self, i):
        return M.slot_bound(self.op, self.items_for(i), len(self.msgs[i]))

    def sub(self, idx):
        idx = list(idx)
        items = [(st, v if isinstance(v, bytes) else [v[i] for i in idx], t) for st, v, t in self.items]
        c = ManyCase(self.op, self.parent, items, [self.msgs[i] for i in idx], self.root_type, self.what)
        if self._want is not None:
            c._want = [self._want[i] for i in idx]
        return c

    def per_message(self):
        """the same case with every value given per message"""
        n = len(self.msgs)
        items = [(st, [v] * n if isinstance(v, bytes) else v, t) for st, v, t in self.items]
        c = ManyCase(self.op, self.parent, items, self.msgs, self.root_type, self.what + ", per-message values")
        c._want = self._want
        return c


def items_blob(parent, steps) -> bytes:
    """the K full paths dg_editm_create takes"""
    from dynamicgo_amd import generic as X
    return X.compile_paths([G.paths_of(list(parent) + [st]) for st in steps])


def set_blob(parent, steps) -> bytes:
    """the {parent, full_1 .. full_K} path set the lookup runs on, as the host build takes it"""
    from dynamicgo_amd import generic as X
    return X.compile_paths([G.paths_of(parent)] + [G.paths_of(list(parent) + [st]) for st in steps])


# --------------------------------------------------------------------- fuzz
FUZZ_N = 100
_INNER = field(R.I64, 1, struct.pack(">q", 77)) + field(R.STRING, 2, wstr(b"in")) + b"\x00"
_I32 = struct.pack(">i", -1024)
_I64 = struct.pack(">q", 1 << 40)
_DBL = struct.pack(">d", 0.5)


def fuzz_cases(seed=78):
    """t2jgen.all_types_desc() messages and their mutated copies under item sets of K = 1, 2, 3, 5 and 7: every
    step class, parents 0 to 2 steps deep, values of the right and of the wrong type, shared and per message"""
    rng = random.Random(seed)
    td = t2jgen.all_types_desc()
    good = [t2jgen.gen_thrift(rng, td, keep_p=0.8) for _ in range(FUZZ_N)]
    msgs = good + [t2jgen.mutate(rng, m) for m in good]
    n = len(msgs)

    def per_msg(lo, hi):
        return [wstr(bytes(rng.randrange(256) for _ in range(rng.randrange(lo, hi)))) for _ in range(n)]

    def C(op, parent, items, what=""):
        return ManyCase(op, parent, items, msgs, what=what)

    return [
        C(SET, [], [((F, 18), wstr(b"x" * 33), R.STRING), ((F, 19), struct.pack(">bi", R.STRING, 0), R.LIST)]),
        C(SET, [], [((F, 18), per_msg(0, 40), R.STRING), ((F, 22), _DBL, R.DOUBLE), ((F, 21), _INNER, R.STRUCT)]),
        C(SET, [], [((F, 900 + k), v, t) for k, (v, t) in enumerate(((_I32, R.I32), (per_msg(0, 300), R.STRING), (_I64, R.I64),
                                                                     (b"\x01", R.BOOL), (_INNER, R.STRUCT)))],
          what="five inserts at the root"),
        C(SET, [], [((F, 999), _I32, R.I32)], what="one insert"),
        C(SET, [], [((F, 22), _DBL, R.DOUBLE), ((F, 18), wstr(b""), R.STRING)], what="two that are always there"),
        C(SET, [(F, 21)], [((F, 1), _I64, R.I64)], what="one nested replace"),
        C(SET, [], [((F, 1), b"\x01", R.BOOL), ((F, 2), b"\x7f", R.BYTE), ((F, 3), b"\x01\x02", R.I16), ((F, 4), _I32, R.I32),
                    ((F, 5), _I64, R.I64), ((F, 6), _DBL, R.DOUBLE), ((F, 22), _DBL, R.DOUBLE)], what="seven scalars"),
        C(SET, [], [((F, 3), b"\x01\x02", R.I16), ((F, 950), _I32, R.I32), ((F, 18), per_msg(0, 20), R.STRING)],
          what="replace, insert, replace"),
        C(SET, [(F, 21)], [((F, 1), _I64, R.I64), ((F, 2), per_msg(0, 20), R.STRING)]),
        C(SET, [(F, 21)], [((F, 77), _I64, R.I64), ((F, 78), wstr(b"seventy-eight"), R.STRING), ((F, 1), _I64, R.I64)],
          what="insert, insert, replace in a nested struct"),
        C(SET, [(F, 10)], [((I, 0), _INNER, R.STRUCT), ((I, 1000), _INNER, R.STRUCT)]),
        C(SET, [(F, 11)], [((I, 1000), _I64, R.I64), ((I, 1001), _I64[::-1], R.I64), ((I, 1000), _I64, R.I64)],
          what="three inserts into a set, one index twice"),
        C(SET, [(F, 20)], [((S, b"a"), _I64, R.I64), ((S, b"key-of-17-bytes.."), _I64, R.I64), ((B, wstr(b"zz")), _I64, R.I64)]),
        C(SET, [(F, 13)], [((N, 5), b"\x01", R.BOOL), ((N, 1), b"\x00", R.BOOL)]),
        C(SET, [(F, 14)], [((N, -2), per_msg(0, 9), R.STRING), ((N, 3), wstr(b""), R.STRING)]),
        C(SET, [(F, 15)], [((B, struct.pack(">i", 3)), _INNER, R.STRUCT)]),
        C(SET, [(F, 19)], [((I, k), wstr(b"e%d" % k * k), R.STRING) for k in range(4)] + [((I, 1000), per_msg(0, 30), R.STRING)],
          what="five elements of a list"),
        C(SET, [(F, 19)], [((I, k), wstr(b"E" * (3 * k)), R.STRING) for k in range(6)] + [((I, 1000), wstr(b"last"), R.STRING)],
          what="seven elements of a list"),
        C(SET, [], [((F, 18), _I32, R.I32), ((F, 7), wstr(b"ok"), R.STRING)], what="the first item of the wrong type"),
        C(SET, [], [((F, 22), _DBL, R.DOUBLE), ((F, 18), _I32, R.I32)], what="the second item of the wrong type"),
        C(SET, [(F, 19)], [((I, 1000), _I32, R.I32), ((I, 1001), _I32, R.I32)], what="i32 inserts into a list<string>"),
        C(SET, [(F, 99)], [((F, 1), _I32, R.I32), ((F, 2), _I32, R.I32)], what="below a field that is not there"),
        C(SET, [(F, 17), (F, 2)], [((F, 1), _I32, R.I32), ((F, 9), _I32, R.I32), ((F, 3), struct.pack(">bi", R.STRUCT, 0), R.LIST)]),
        C(UNSET, [], [((F, 18),), ((F, 19),)]),
        C(UNSET, [], [((F, 18),), ((F, 20),), ((F, 21),)]),
        C(UNSET, [], [((F, 32767),)]),
        C(UNSET, [], [((F, 22),), ((F, 23),), ((F, 24),), ((F, 21),), ((F, 18),)], what="unset five fields"),
        C(UNSET, [], [((F, k),) for k in (18, 19, 20, 21, 22, 23, 24)], what="unset seven fields"),
        C(UNSET, [(F, 21)], [((F, 1),), ((F, 2),)]),
        C(UNSET, [(F, 10)], [((I, 1),), ((I, 0),)]),
        C(UNSET, [(F, 19)], [((I, 0),), ((I, 1),), ((I, 2),)]),
        C(UNSET, [(F, 20)], [((S, b"k"),), ((N, 1),)]),
        C(UNSET, [(F, 18)], [((F, 1),), ((F, 2),)], what="unset below a string"),
        C(UNSET, [(F, 99)], [((F, 1),), ((F, 2),)], what="unset below a field that is not there"),
        C(UNSET, [(F, 17), (F, 2)], [((F, 1),), ((F, 3),)]),
    ]


def shares(cases):
    """the share of each outcome class over all (message, item set) cases, from the checker alone"""
    count, total = {}, 0
    for c in cases:
        for ret, _ in c.want():
            k = M.outcome(c.op, ret, c.k)
            count[k] = count.get(k, 0) + 1
            total += 1
    return {k: v / total for k, v in count.items()}


# ---------------------------------------------------------------- adjacency
VAL_LENS = (0, 1, 15, 16, 17, 33)


def adjacency_cases():
    """a struct of seven consecutive one-byte fields, all replaced (3 bytes between the cuts: the next field's
    header), and a list<byte> whose neighbouring elements are replaced or dropped (0 bytes between the cuts);
    the values, taken as given, 0 to 33 bytes long"""
    seven = b"".join(field(R.BYTE, k, bytes([0x40 + k])) for k in range(1, 8)) + b"\x00"
    lst = struct.pack(">bi", R.BYTE, 12) + bytes(range(0x61, 0x6D))
    out = []
    for r in range(len(VAL_LENS)):
        vals = [bytes(0x30 + (j + k) % 10 for k in range(VAL_LENS[(r + j) % len(VAL_LENS)])) for j in range(7)]
        out.append(ManyCase(SET, [], [((F, 7 - j), vals[j], R.BYTE) for j in range(7)], [seven, field(R.I32, 9, b"abcd") + seven],
                            what="seven one-byte fields, value lengths rotated by %d" % r))
        out.append(ManyCase(SET, [], [((I, 3 + j), vals[j], R.BYTE) for j in (2, 0, 1)], [lst], R.LIST,
                            what="three neighbours of a list<byte>, rotation %d" % r))
        out.append(ManyCase(SET, [], [((I, j), vals[j], R.BYTE) for j in range(7)], [lst], R.LIST,
                            what="the first seven of a list<byte>, rotation %d" % r))
    out.append(ManyCase(UNSET, [], [((I, 3),), ((I, 5),), ((I, 4),)], [lst], R.LIST, what="drop three neighbours"))
    out.append(ManyCase(UNSET, [], [((I, j),) for j in range(7)], [lst], R.LIST, what="drop the first seven"))
    out.append(ManyCase(UNSET, [], [((I, 11 - j),) for j in range(7)], [lst], R.LIST, what="drop the last seven"))
    out.append(ManyCase(UNSET, [], [((F, k),) for k in (2, 3, 4)], [seven], what="drop three neighbouring fields"))
    out.append(ManyCase(UNSET, [], [((F, k),) for k in range(1, 8)], [seven], what="drop all seven fields"))
    return out


# -------------------------------------------------------------------- phase
def phase_case():
    """struct{1: string[p], 2, 3, 4: string, 5: string[t]}: the first cut (the value of field 2) at every offset
    mod 16, three replaced values of 0 to 17 bytes, and tails that bring the output across a 16-byte and a
    1 KB boundary"""
    msgs, v2, v3, v4 = [], [], [], []
    k = 0
    for p in range(16):
        for t in (0, 5, 960, 975):
            for r in range(3):
                msgs.append(field(R.STRING, 1, wstr(b"p" * p)) + field(R.STRING, 2, wstr(b"old-2")) +
                            field(R.STRING, 3, wstr(b"")) + field(R.STRING, 4, wstr(b"old-four-is-longer")) +
                            field(R.STRING, 5, wstr(bytes(65 + q % 26 for q in range(t)))) + b"\x00")
                k += 1
                v2.append(wstr(b"2" * ((k * 7) % 18)))
                v3.append(wstr(b"3" * ((k * 5 + r) % 18)))
                v4.append(wstr(b"4" * ((k * 11 + 2 * r) % 18)))
    return ManyCase(SET, [], [((F, 4), v4, R.STRING), ((F, 2), v2, R.STRING), ((F, 3), v3, R.STRING)], msgs,
                    what="three cuts at every phase")


# ------------------------------------------------------ many items in a unit
def unit_cases():
    """outputs in which one 16-byte unit covers several whole items"""
    one = [bytes([0x51 + j]) for j in range(7)]
    lst = struct.pack(">bi", R.BYTE, 3) + b"abc"
    out = [
        ManyCase(SET, [], [((I, 100 + j), one[j], R.BYTE) for j in range(7)], [lst, struct.pack(">bi", R.BYTE, 0)], R.LIST,
                 what="seven one-byte inserts into a list"),
        ManyCase(SET, [], [((F, 10 + j), bytes([j & 1]), R.BOOL) for j in range(7)], [b"\x00", b""],
                 what="seven bool fields into a lone STOP"),
        ManyCase(SET, [], [((N, 10 + j), bytes([j & 1]), R.BOOL) for j in range(7)],
                 [struct.pack(">bbi", R.BYTE, R.BOOL, 0), struct.pack(">bbi", R.I64, R.BOOL, 0), b""], R.MAP,
                 what="seven entries into an empty map"),
        ManyCase(SET, [], [((I, j), bytes([j & 1]), R.BOOL) for j in range(7)], [struct.pack(">bi", R.BOOL, 0), b""], R.LIST,
                 what="seven bools into an empty list"),
    ]
    for c in G.smallest_cases():  # the single edit's smallest messages, alone and with a second item of the same kind
        st = c.path[-1]
        out.append(ManyCase(c.op, c.path[:-1], [(st, c.values, c.val_type)], c.msgs, c.root_type, what="smallest: " + c.what))
        other = (st[0], st[1] + 1)
        out.append(ManyCase(c.op, c.path[:-1], [(st, c.values, c.val_type), (other, c.values, c.val_type)], c.msgs, c.root_type,
                            what="smallest, two items: " + c.what))
    return out


# -------------------------------------------------------------------- count
def count_cases():
    """a list whose count starts at every offset 0-15 mod 16 of the output: count + k with carries (255, 65535),
    the 0x7FFFFFFF wrap (a list whose header says so: the index is past it before an element is read), and
    count - k across 256; a map the same way"""
    v = struct.pack(">i", 0x01020304)
    fs = range(16)
    out = []
    for k in (2, 7):
        ins = [((I, 0x7FFFFFFF), v, R.I32)] * k
        out.append(ManyCase(SET, [(F, 2)], ins, [G.count_list(f, c) for f in fs for c in (0, 255, 256 - k)] +
                            [G.count_list(f, c, 0) for f in fs for c in (65535, 0x7FFFFFFF, 0x7FFFFFFF - k + 1)],
                            what="%d list inserts" % k))
        out.append(ManyCase(SET, [(F, 2)], [((N, 100000 + j), v, R.I32) for j in range(k)],
                            [G.count_map(f, c) for f in fs for c in (0, 255)], what="%d map inserts" % k))
        out.append(ManyCase(UNSET, [(F, 2)], [((I, 3 * j),) for j in range(k)], [G.count_list(f, c) for f in fs for c in (256, 257, 22)],
                            what="%d list drops" % k))
        out.append(ManyCase(UNSET, [(F, 2)], [((N, 2 * j + 1),) for j in range(k)], [G.count_map(f, 256 + k // 3) for f in fs],
                            what="%d map drops" % k))
    return out


# ------------------------------------------------------------------ failures
def failure_cases():
    """one failing item at each of the 7 positions (a string where the field is an i32), overlapping items, a
    missed parent under UNSET"""
    m = b"".join(field(R.I32, k, struct.pack(">i", k)) for k in range(1, 8)) + b"\x00"
    i32 = struct.pack(">i", -5)
    out = []
    for bad in range(7):
        items = [((F, 1 + j), wstr(b"bad") if j == bad else i32, R.STRING if j == bad else R.I32) for j in range(7)]
        out.append(ManyCase(SET, [], items, [m, m], what="item %d fails" % bad))
    mp = struct.pack(">bbi", R.STRING, R.I32, 2) + wstr(b"a") + i32 + wstr(b"b") + i32
    out.append(ManyCase(SET, [], [((S, b"b"), i32, R.I32), ((S, b"a"), i32, R.I32), ((B, wstr(b"a")), i32, R.I32)], [mp], R.MAP,
                        what="STRKEY and BINKEY on one entry"))
    out.append(ManyCase(UNSET, [], [((S, b"a"),), ((B, wstr(b"a")),)], [mp], R.MAP, what="drop one entry twice"))
    lst = struct.pack(">bi", R.I32, 3) + i32 * 3
    out.append(ManyCase(SET, [], [((I, 1), i32, R.I32), ((I, 2), i32, R.I32), ((I, 1), i32, R.I32)], [lst], R.LIST,
                        what="an existing index twice"))
    out.append(ManyCase(SET, [], [((I, 9), i32, R.I32), ((I, 9), i32[::-1], R.I32)], [lst], R.LIST, what="a missing index twice"))
    out.append(ManyCase(UNSET, [(F, 9)], [((F, 1),), ((F, 2),)], [m], what="unset below a missed parent"))
    out.append(ManyCase(UNSET, [], [((F, 1),), ((F, 9),)], [m], what="the second item is not there"))
    return out


# ------------------------------------------------------------------ corpus
def write_corpus(path, case, caps):
    """editm_host.cpp's corpus file: u32 n_msgs, op, root_type, K, blob_len; u32 val_types[K]; the {parent,
    full_1..full_K} blob; per message u32 len, cap, vlen[K], the message, the K values"""
    blob = set_blob(case.parent, case.steps)
    k = case.k
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5I", len(case.msgs), case.op, case.root_type, k, len(blob)))
        fh.write(struct.pack("<%dI" % k, *case.val_types) + blob)
        for i, (m, c) in enumerate(zip(case.msgs, caps)):
            vs = [case.value(i, j) if case.op == SET else b"" for j in range(k)]
            fh.write(struct.pack("<%dI" % (2 + k), len(m), c, *map(len, vs)) + m + b"".join(vs))
