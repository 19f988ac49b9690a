"""Inputs of the edit tests that the CPU build (test_edit_host.py) and the GPU
tests (test_gpu_edit.py) share. A case is one edit applied to a batch:
Case(op, path, val_type, values, msgs, root_type), path as (kind, value) steps
like tgetref's, values one `bytes` for all messages or a list with one entry per
message. The expected results come from editref alone."""
import random
import struct

import editref as E
import t2jgen
import tgetgen
import tgetref as R

F, I, S, N, B = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
SET, UNSET = E.SET_OP, E.UNSET_OP


class Case:
    def __init__(self, op, path, msgs, val_type=0, values=b"", root_type=R.STRUCT, what=""):
        self.op, self.path, self.msgs, self.val_type, self.values, self.root_type = op, list(path), list(msgs), val_type, \
            values, root_type
        self.what = what or "%s %r" % ("set" if op == SET else "unset", path)
        self._want = None

    def value(self, i):
        return self.values if isinstance(self.values, bytes) else self.values[i]

    def want(self, caps=None):
        """[(ret, out)] from the checker; caps: the slot sizes (None: large enough)"""
        if caps is None:
            if self._want is None:
                self._want = [E.edit(self.op, m, self.path, self.value(i), self.val_type, self.root_type)
                              for i, m in enumerate(self.msgs)]
            return self._want
        return [E.edit(self.op, m, self.path, self.value(i), self.val_type, self.root_type, c)
                for i, (m, c) in enumerate(zip(self.msgs, caps))]

    def sub(self, idx):
        vals = self.values if isinstance(self.values, bytes) else [self.values[i] for i in idx]
        c = Case(self.op, self.path, [self.msgs[i] for i in idx], self.val_type, vals, self.root_type, self.what)
        if self._want is not None:
            c._want = [self._want[i] for i in idx]
        return c


def paths_of(steps):
    """(kind, value) steps as dynamicgo_amd.generic Path objects"""
    from dynamicgo_amd import generic as G
    return [G.Path(k, v) for k, v in steps]


def pair_blob(steps) -> bytes:
    """the (parent, full) path set of an edit, as the host build takes it"""
    from dynamicgo_amd import generic as G
    return G.compile_paths([paths_of(steps[:-1]), paths_of(steps)])


def wstr(s: bytes) -> bytes:
    return struct.pack(">i", len(s)) + s


def field(t, fid, v: bytes) -> bytes:
    return struct.pack(">bh", t, fid) + v


# --------------------------------------------------------------------- fuzz
FUZZ_N = 160
_INNER = field(R.I64, 1, struct.pack(">q", 77)) + field(R.STRING, 2, wstr(b"in")) + b"\x00"


def fuzz_cases(seed=77):
    """t2jgen.all_types_desc() messages and their mutated copies under about a
    dozen edits per op: every step kind last, depth 1 to 3, values of the right
    and of the wrong type, broadcast and per message."""
    rng = random.Random(seed)
    td = t2jgen.all_types_desc()
    good = [t2jgen.gen_thrift(rng, td, keep_p=0.8) for _ in range(FUZZ_N)]
    msgs = good + [t2jgen.mutate(rng, m) for m in good]
    n = len(msgs)

    def per_msg(lo, hi):
        return [wstr(bytes(rng.randrange(256) for _ in range(rng.randrange(lo, hi)))) for _ in range(n)]

    i32 = struct.pack(">i", -1024)
    cases = [
        Case(SET, [(F, 7)], msgs, R.STRING, per_msg(0, 40)),
        Case(SET, [(F, 18)], msgs, R.STRING, wstr(b"x" * 33)),
        Case(SET, [(F, 18)], msgs, R.I32, i32, what="set a string field to an i32"),
        Case(SET, [(F, 4)], msgs, R.I32, i32),
        Case(SET, [(F, 999)], msgs, R.STRING, per_msg(0, 300), what="insert field 999"),
        Case(SET, [(F, 9), (F, 2)], msgs, R.STRING, per_msg(0, 20)),
        Case(SET, [(F, 9), (F, 77)], msgs, R.I64, struct.pack(">q", -2), what="insert into a nested struct"),
        Case(SET, [(F, 10), (I, 0)], msgs, R.STRUCT, _INNER),
        Case(SET, [(F, 10), (I, 1000)], msgs, R.STRUCT, _INNER, what="insert into a list"),
        Case(SET, [(F, 11), (I, 1000)], msgs, R.I32, i32, what="insert an i32 into a set<i64>"),
        Case(SET, [(F, 12), (S, b"key-of-17-bytes..")], msgs, R.LIST, struct.pack(">bi", R.I32, 1) + i32),
        Case(SET, [(F, 13), (N, 5)], msgs, R.BOOL, b"\x01"),
        Case(SET, [(F, 14), (N, -2)], msgs, R.STRING, per_msg(0, 9)),
        Case(SET, [(F, 15), (B, struct.pack(">i", 3))], msgs, R.STRUCT, _INNER),
        Case(SET, [(F, 16), (N, 1), (S, b"x")], msgs, R.DOUBLE, struct.pack(">d", 0.5)),
        Case(SET, [(F, 17), (F, 2), (F, 1)], msgs, R.I32, i32),
        Case(UNSET, [(F, 7)], msgs),
        Case(UNSET, [(F, 18)], msgs),
        Case(UNSET, [(F, 19)], msgs),
        Case(UNSET, [(F, 32767)], msgs),
        Case(UNSET, [(F, 9), (F, 1)], msgs),
        Case(UNSET, [(F, 10), (I, 0)], msgs),
        Case(UNSET, [(F, 11), (I, 1)], msgs),
        Case(UNSET, [(F, 19), (I, 0)], msgs),
        Case(UNSET, [(F, 20), (S, b"k")], msgs),
        Case(UNSET, [(F, 13), (N, 1)], msgs),
        Case(UNSET, [(F, 18), (F, 1)], msgs, what="unset below a string"),
        Case(UNSET, [(F, 10), (F, 1)], msgs, what="unset a field of a list"),
        Case(UNSET, [(F, 17), (F, 2), (F, 1)], msgs),
        Case(UNSET, [(F, 21), (F, 1)], msgs),
    ]
    return cases


def shares(cases):
    """the share of each outcome class over all (message, edit) cases, from the checker alone"""
    count, total = {}, 0
    for c in cases:
        for ret, _ in c.want():
            k = E.outcome(c.op, ret)
            count[k] = count.get(k, 0) + 1
            total += 1
    return {k: v / total for k, v in count.items()}


# --------------------------------------------------------- alignment sweep
LENGTHS = tuple(range(0, 18)) + (31, 32, 33, 1023, 1024, 1025)


def sweep_message(p, old, s=3):
    """struct{1: string[p], 2: string[old], 3: string[s]}: the value of field 2
    starts 10 + p bytes into the message; None for p: no field 1 (3 bytes), None
    for s: nothing but the STOP behind it"""
    m = b"" if p is None else field(R.STRING, 1, wstr(bytes(65 + k % 26 for k in range(p))))
    m += field(R.STRING, 2, wstr(bytes(97 + k % 26 for k in range(old))))
    if s is not None:
        m += field(R.STRING, 3, wstr(b"Z" * s))
    return m + b"\x00"


def sweep_case():
    """a replace of field 2: every filler length against every new length and
    every old length against every new length (the third one rotating through
    the lengths), the three kinds of ends"""
    L = LENGTHS
    msgs, vals = [], []
    for a, p in enumerate(L):
        for b, new in enumerate(L):
            msgs.append(sweep_message(p, L[(a + b) % len(L)]))
            vals.append(wstr(bytes(48 + k % 10 for k in range(new))))
    for a, old in enumerate(L):
        for b, new in enumerate(L):
            msgs.append(sweep_message(L[(a + 2 * b + 1) % len(L)], old, s=None if (a + b) % 3 == 0 else b % 19))
            vals.append(wstr(bytes(48 + k % 10 for k in range(new))))
    for new in L:  # the shortest prefix a struct allows
        msgs.append(sweep_message(None, 5))
        vals.append(wstr(b"n" * new))
    return Case(SET, [(F, 2)], msgs, R.STRING, vals, what="alignment sweep")


def spacer(n):
    """a struct of exactly n >= 8 bytes (one string field 9)"""
    return field(R.STRING, 9, wstr(b"." * (n - 8))) + b"\x00"


def phase_layout(case_of, tested, bound):
    """Every source phase against every destination phase mod 16: `tested`
    (one message) 256 times, a spacer message in front of each that brings the
    tested message to source phase s in the arena and, through its slot's size,
    the tested slot to destination phase d (the arena and the first slot start
    at a multiple of 16). case_of(msgs) -> Case; bound(msg) -> the slot a
    message needs. Returns (case, caps)."""
    msgs, caps = [], []
    src = dst = 0
    for s in range(16):
        for d in range(16):
            fl = 8 + (s - src - 8) % 16
            sp = spacer(fl)
            msgs.append(sp)
            src += fl
            cap = bound(sp)
            cap += (d - dst - cap) % 16
            caps.append(cap)
            dst += cap
            assert src % 16 == s and dst % 16 == d
            msgs.append(tested)
            caps.append(bound(tested))
            src += len(tested)
            dst += caps[-1]
    return case_of(msgs), caps


# -------------------------------------------------------------- count patch
def count_list(f, count, real=None):
    """struct{1: string[f], 2: list<i32>}: the count's first byte is 11 + f into the message"""
    real = count if real is None else real
    return field(R.STRING, 1, wstr(b"f" * f)) + field(R.LIST, 2, struct.pack(">bi", R.I32, count) +
                                                       struct.pack(">%di" % real, *range(real))) + b"\x00"


def count_map(f, count, kt=R.I32, keys=None):
    """struct{1: string[f], 2: map<kt, i32>}: the count's first byte is 12 + f into the message"""
    fmt = {R.BYTE: ">b", R.I16: ">h", R.I32: ">i", R.I64: ">q"}
    body = b""
    for k in range(count):
        body += (wstr(keys[k]) if kt == R.STRING else struct.pack(fmt[kt], k + 1)) + struct.pack(">i", k)
    return field(R.STRING, 1, wstr(b"f" * f)) + field(R.MAP, 2, struct.pack(">bbi", kt, R.I32, count) + body) + b"\x00"


STR_KEYS = [bytes(75 + (3 * i + j) % 20 for j in range(n)) for i, n in enumerate((0, 1, 15, 16, 17, 100))]


def count_cases():
    """a list and a map whose count starts at every offset 0-15 mod 16 of the
    output (the slots are 16-aligned), inserts at counts 0, 1, 255, 256 and
    0x7FFFFFFF (a list whose header says so: the index is past it before an
    element is read), unsets at count 1; int-key inserts at every key width and
    string keys of 0 to 100 bytes"""
    v = struct.pack(">i", 0x01020304)
    fs = range(16)
    out = [
        Case(SET, [(F, 2), (I, 0x7FFFFFFF)], [count_list(f, c) for f in fs for c in (0, 1, 255, 256)] +
             [count_list(f, 0x7FFFFFFF, 0) for f in fs], R.I32, v, what="list insert"),
        Case(SET, [(F, 2), (N, 100000)], [count_map(f, c) for f in fs for c in (0, 1, 255, 256)], R.I32, v,
             what="map insert"),
        Case(UNSET, [(F, 2), (I, 0)], [count_list(f, 1) for f in fs], what="list unset"),
        Case(UNSET, [(F, 2), (N, 1)], [count_map(f, 1) for f in fs], what="map unset"),
        Case(UNSET, [(F, 2), (I, 200)], [count_list(f, c) for f in fs for c in (255, 256)], what="list unset, carry"),
    ]
    for kt in (R.BYTE, R.I16, R.I32, R.I64):
        for key in (-2, 0x7F, 200, 0x1234, -0x12345678, 0x0123456789ABCDEF):
            out.append(Case(SET, [(F, 2), (N, key)], [count_map(f, c, kt) for f in (0, 7) for c in (0, 3)], R.I32, v,
                            what="int key %d into a map keyed %d" % (key, kt)))
    for key in STR_KEYS:
        msgs = [count_map(f, c, R.STRING, STR_KEYS) for f in (0, 5, 11) for c in (0, 2, 6)]
        out.append(Case(SET, [(F, 2), (S, key)], msgs, R.I32, v, what="string key of %d bytes" % len(key)))
        out.append(Case(UNSET, [(F, 2), (S, key)], msgs, what="unset string key of %d bytes" % len(key)))
        out.append(Case(SET, [(F, 2), (B, wstr(key))], msgs, R.I32, v, what="binary key of %d bytes" % (4 + len(key))))
    return out


def smallest_cases():
    v = struct.pack(">i", 5)
    return [
        Case(SET, [(F, 1)], [b"\x00", b""], R.I32, v, what="a lone STOP, an empty message"),
        Case(UNSET, [(F, 1)], [b"\x00", b""]),
        Case(SET, [(I, 0)], [struct.pack(">bi", R.I32, 0), b""], R.I32, v, R.LIST, what="an empty list"),
        Case(UNSET, [(I, 0)], [struct.pack(">bi", R.I32, 0), b""], root_type=R.LIST),
        Case(SET, [(I, 0x7FFFFFFF)], [struct.pack(">bi", R.BYTE, 0x7FFFFFFF) + b"\x09"], R.BYTE, b"\x07", R.LIST,
             what="count 0x7FFFFFFF wraps"),
        Case(SET, [(N, 7)], [struct.pack(">bbi", R.I16, R.I32, 0), b""], R.I32, v, R.MAP, what="an empty map"),
        Case(UNSET, [(N, 7)], [struct.pack(">bbi", R.I16, R.I32, 0), b""], root_type=R.MAP),
        Case(SET, [(I, 0)], [struct.pack(">bi", R.STRING, 2) + wstr(b"ab") + wstr(b"cdef")], R.STRING, wstr(b"Q" * 40),
             R.LIST, what="no prefix but the header"),
        Case(SET, [(I, 1)], [struct.pack(">bi", R.STRING, 2) + wstr(b"ab") + wstr(b"cdef")], R.STRING, wstr(b"Q" * 40),
             R.LIST, what="a suffix of 0 bytes"),
        Case(UNSET, [(I, 1)], [struct.pack(">bi", R.STRING, 2) + wstr(b"ab") + wstr(b"cdef")], root_type=R.LIST,
             what="a suffix of 0 bytes"),
    ]


# -------------------------------------------------------------- deep values
def deep_cases():
    """a replaced and a dropped value nested 9 and 1023 deep (the lookup's deep
    pass feeds the splice); field 2 behind it, so the skip runs in both"""
    out = []
    for depth in (9, 1023):
        m = tgetgen.chain_message("S" * (depth - 1), "i")  # field 1 = a struct chain: depth - 1 structs below the top
        t = m[0]
        out.append(Case(SET, [(F, 1)], [m, m], t, field(R.I32, 1, struct.pack(">i", 1)) + b"\x00", what="replace %d deep" % depth))
        out.append(Case(UNSET, [(F, 1)], [m, m], what="drop %d deep" % depth))
        out.append(Case(SET, [(F, 2)], [m, m], R.I32, struct.pack(">i", -9), what="replace behind %d deep" % depth))
    return out


def with_big_stack(fn):
    """the recursive checker on inputs nested to MaxSkipDepth"""
    return tgetgen.deep_checker(fn)


# ------------------------------------------------------------------ corpus
def write_corpus(path, case, caps):
    """edit_host.cpp's corpus file: u32 n_msgs, op, root_type, val_type, blob_len; the (parent, full) blob;
    per message u32 len, cap, vlen, the message, the value"""
    blob = pair_blob(case.path)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5I", len(case.msgs), case.op, case.root_type, case.val_type, len(blob)) + blob)
        for i, (m, c) in enumerate(zip(case.msgs, caps)):
            v = case.value(i) if case.op == SET else b""
            fh.write(struct.pack("<3I", len(m), c, len(v)) + m + v)
