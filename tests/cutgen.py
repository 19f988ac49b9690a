"""Inputs of the cut tests (test_cut_host.py on the CPU, test_gpu_cut.py on the
GPU): a wide / narrow descriptor pair written for these tests, the fuzz corpus
over it, container chains around the frame limits, kept runs of chosen length
and alignment, plan shapes (wide flat structs, plans at the edge of the lane
route's LDS copy and far past it: test_gpu_cut_shapes.py), and the expectations
from the checker (cutref.py). Seeded; pure Python."""
import random
import struct

import cutref as R
import t2jgen
from dynamicgo_amd import thrift as T

OPT, DEF, REQ = T.OPTIONAL, T.DEFAULT, T.REQUIRED
ALL_OPTS = tuple(range(8))  # every word of WRITE_DEFAULT | DISALLOW_UNKNOWN | NOT_CHECK_REQ
FUZZ_SEED, FUZZ_N = 5, 257
LDS_FRAMES = 8  # CUT_LDS_DEPTH (dynamicgo_amd/csrc/cut_device.h)


def F(fid, name, td, req=OPT):
    return T.FieldDescriptor(fid, name, td, req)


def b(name):
    return T.builtin(name)


_PAIR = None


def pair():
    """(wide, narrow). Dropped: a scalar (1), a string (2), a struct (3), a
    list (4), a map (5). Kept and narrowed inside: a struct whose inner struct
    is narrowed (6), a list (7) and a map (8) of narrowed structs, a map with a
    narrowed struct key (9), a self-recursive struct (15). Copied whole: a list
    whose element descriptor is the same object on both sides (10), scalars,
    a set of i64. Required (11), default (12, 16, 17, 20, and 21 which only the
    narrow side has) and optional fields in `to`. Mid.differ (Mid field 4) is
    an i32 in `from` and a string in `to`."""
    global _PAIR
    if _PAIR:
        return _PAIR
    leaf = T.struct_type("Leaf", [F(1, "a", b("i64"), REQ), F(2, "b", b("string"), DEF),
                                  F(3, "c", T.list_of(b("double"))), F(4, "d", b("i32"))])
    leaf_n = T.struct_type("LeafN", [F(1, "a", b("i64"), REQ), F(2, "b", b("string"), DEF), F(5, "e", b("i16"), DEF)])
    key = T.struct_type("Key", [F(1, "k", b("string")), F(2, "x", b("i32"))])
    key_n = T.struct_type("KeyN", [F(1, "k", b("string"))])
    shared = T.struct_type("Shared", [F(1, "p", b("i32")), F(2, "q", b("string"))])
    node_sd, node_nsd = T.StructDescriptor("Node"), T.StructDescriptor("NodeN")
    node, node_n = T.TypeDescriptor(T.STRUCT, "Node", struct=node_sd), T.TypeDescriptor(T.STRUCT, "NodeN", struct=node_nsd)
    for f in (F(1, "val", b("i32")), F(2, "next", node), F(3, "kids", T.list_of(node)), F(4, "tag", b("string"))):
        node_sd.add_field(f)
    for f in (F(1, "val", b("i32"), DEF), F(2, "next", node_n), F(3, "kids", T.list_of(node_n))):
        node_nsd.add_field(f)
    mid = T.struct_type("Mid", [F(1, "leaf", leaf), F(2, "name", b("string")), F(3, "n", b("i32")),
                                F(4, "differ", b("i32"))])
    mid_n = T.struct_type("MidN", [F(1, "leaf", leaf_n, DEF), F(3, "n", b("i32")), F(4, "differ", b("string"))])
    wide = T.struct_type("Wide", [
        F(1, "s_drop", b("i32")), F(2, "str_drop", b("string")), F(3, "st_drop", leaf), F(4, "l_drop", T.list_of(b("string"))),
        F(5, "m_drop", T.map_of(b("string"), b("i64"))), F(6, "mid", mid), F(7, "leaves", T.list_of(leaf)),
        F(8, "by_name", T.map_of(b("string"), leaf)), F(9, "by_key", T.map_of(key, b("i32"))),
        F(10, "same_l", T.list_of(shared)), F(11, "req_s", b("string"), REQ), F(12, "def_l", T.list_of(b("string")), DEF),
        F(13, "opt_i", b("i64")), F(15, "node", node), F(16, "def_m", T.map_of(b("string"), b("i32")), DEF),
        F(17, "def_st", leaf, DEF), F(18, "kept_str", b("string")), F(19, "set_f", T.set_of(b("i64"))),
        F(20, "dbl", b("double"), DEF)])
    narrow = T.struct_type("Narrow", [
        F(6, "mid", mid_n), F(7, "leaves", T.list_of(leaf_n)), F(8, "by_name", T.map_of(b("string"), leaf_n)),
        F(9, "by_key", T.map_of(key_n, b("i32"))), F(10, "same_l", T.list_of(shared)), F(11, "req_s", b("string"), REQ),
        F(12, "def_l", T.list_of(b("string")), DEF), F(13, "opt_i", b("i64")), F(15, "node", node_n),
        F(16, "def_m", T.map_of(b("string"), b("i32")), DEF), F(17, "def_st", leaf_n, DEF), F(18, "kept_str", b("string")),
        F(19, "set_f", T.set_of(b("i64"))), F(20, "dbl", b("double"), DEF), F(21, "only_to", b("bool"), DEF)])
    _PAIR = (wide, narrow)
    return _PAIR


def expect(msgs, frm, to, opts=0):
    """[(ret, out)] from the checker"""
    return [R.marshal_to(m, frm, to, opts) for m in msgs]


_FUZZ = None


def fuzz():
    """(messages, mutated copies): FUZZ_N of each over the wide descriptor, with unknown fields"""
    global _FUZZ
    if _FUZZ is None:
        rng, mrng = random.Random(FUZZ_SEED), random.Random(FUZZ_SEED + 1000)
        msgs = [t2jgen.gen_thrift(rng, pair()[0], keep_p=0.5) for _ in range(FUZZ_N)]
        _FUZZ = (msgs, [t2jgen.mutate(mrng, m) for m in msgs])
    return _FUZZ


# ---- chains of cut containers over the recursive Node pair: S = the `next`
# struct (one container), L = one element of `kids` (a list and a struct) ----
def node_pair():
    w, n = pair()
    return w.struct.field_by_id(15).type, n.struct.field_by_id(15).type


def chain_message(kinds):
    """A Node message: the root struct, then one nested level per letter; the
    innermost Node holds val = 7 and a tag (dropped)"""
    head = b"".join(b"\x0c\x00\x02" if k == "S" else b"\x0f\x00\x03\x0c\x00\x00\x00\x01" for k in kinds)
    return head + b"\x08\x00\x01\x00\x00\x00\x07" + b"\x0b\x00\x04\x00\x00\x00\x02hi" + b"\x00" * (len(kinds) + 1)


def chain_containers(kinds):
    return 1 + sum(1 if k == "S" else 2 for k in kinds)


def chains_of(containers, rng, count=4):
    """`count` chains that open exactly `containers` cut containers: all structs first, then random mixes"""
    out = ["S" * (containers - 1)]
    while len(out) < count:
        kinds, left = "", containers - 1
        while left:
            k = rng.choice("SL") if left >= 2 else "S"
            kinds += k
            left -= 1 if k == "S" else 2
        out.append(kinds)
    return out


def deep_drop_message(depth):
    """Wide: st_drop (dropped) holding `depth` structs nested through field 1, then req_s"""
    return b"\x0c\x00\x03" + b"\x0c\x00\x01" * (depth - 1) + b"\x00" * depth + b"\x0b\x00\x0b\x00\x00\x00\x01r" + b"\x00"


# ---- kept runs of chosen length and alignment ----
_RUN = None


def run_pair():
    """pre (kept) | pad (dropped) | body (kept) | d2 (dropped) | STOP"""
    global _RUN
    if _RUN is None:
        w = T.struct_type("RunW", [F(1, "pre", b("string")), F(2, "pad", b("string")), F(3, "body", b("string")),
                                   F(4, "d2", b("i32"))])
        n = T.struct_type("RunN", [F(1, "pre", b("string")), F(3, "body", b("string"))])
        _RUN = (w, n)
    return _RUN


RUN_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)


def _str(fid, n, rng):
    return b"\x0b" + struct.pack(">hi", fid, n) + bytes(rng.randrange(1, 256) for _ in range(n))


def run_message(rng, run_len, dst_mis, src_mis, base):
    """A RunW message, placed at arena offset `base`, whose kept run between
    the two dropped fields is run_len bytes long (a string field of run_len - 7
    payload bytes; 0: no field at all; 1 has no such form and comes out as the
    lone STOP run every message ends with), starts at a source address that is
    src_mis modulo 16 and lands at output offset dst_mis modulo 16 (a kept
    prefix of dst_mis bytes, + 16 where a string field is longer than that)."""
    pre_len = dst_mis if dst_mis >= 7 else dst_mis + 16
    pre = _str(1, pre_len - 7, rng)
    pad_len = (src_mis - (base + len(pre) + 7)) % 16  # the dropped string: 7 bytes + its payload
    msg = pre + _str(2, pad_len, rng)
    if run_len >= 7:
        assert (base + len(msg)) % 16 == src_mis
        msg += _str(3, run_len - 7, rng)
    return msg + b"\x08\x00\x04\x00\x00\x00\x09" + b"\x00"


def run_messages(seed=3):
    """every run length x destination misalignment x source misalignment, back to back in one arena"""
    rng = random.Random(seed)
    msgs, base = [], 0
    for L in RUN_LENGTHS:
        if 1 < L < 7:
            continue
        for dm in range(16):
            for sm in range(16):
                msgs.append(run_message(rng, L, dm, sm, base))
                base += len(msgs[-1])
    return msgs


# ---- a message whose WriteDefault output outgrows its length by more than the
# host entry's first-pass slot (length + 256) ----
def grow_pair():
    inner = T.struct_type("GrowI", [F(1, "x", b("i32"))])
    inner_n = T.struct_type("GrowIN", [F(1, "x", b("i32")), F(2, "d1", b("i64"), DEF), F(3, "d2", b("i64"), DEF)])
    return (T.struct_type("GrowW", [F(1, "l", T.list_of(inner))]), T.struct_type("GrowN", [F(1, "l", T.list_of(inner_n))]))


def grow_message(n):
    return b"\x0f\x00\x01\x0c" + struct.pack(">i", n) + b"\x00" * n + b"\x00"


# ---- plan shapes: wide flat structs, plans at the edge of the lane route's LDS
# copy (CUT_LANE_PLAN, cut_kern.hip) and the fuzz pair with a plan far past it ----
def tab_len(blob):
    """the length of a plan's tables (its header's off_pool): what the lane route stages in LDS"""
    return struct.unpack_from("<I", blob, 40)[0]


def unset_bytes(blob):
    """the header's max_unset: the most literal bytes one STOP can write"""
    return struct.unpack_from("<I", blob, 48)[0]


def lane_plan_cap():
    import descgen
    return descgen.kernel_const("cut_kern.hip", "CUT_LANE_PLAN")


WIDE_TYPES = ("i32", "string", "i64", "double", "bool", "i16", "byte")
WIDE_NS = (1, 2, 63, 64, 65, 127, 128, 129, 300)
WIDE_MODES = ("dense", "neg", "sparse")
INT16_EDGES = (-32768, 32767, -1, 0)
_WIDE = {}


def wide_ids(n, mode, rng):
    if mode == "dense":
        return list(range(1, n + 1))
    if mode == "neg":  # the int16 extremes, -1 and 0, and a range around 0 with a fifth of it below
        ids = list(INT16_EDGES[:n])
        k = -(n // 5)
        while len(ids) < n:
            if k not in ids:
                ids.append(k)
            k += 1
        return sorted(ids)
    return sorted(rng.sample(range(-32768, 32768), n))


def flat_pair(name, ids, kept, req_of):
    """(from, to): flat structs over `ids`, the types cycling over WIDE_TYPES by
    position; `to` has the ids of `kept`; req_of[id] is a tracked field's
    requiredness in `to` (every other field is OPTIONAL, on both sides)"""
    ty = {fid: WIDE_TYPES[k % len(WIDE_TYPES)] for k, fid in enumerate(ids)}
    frm = T.struct_type(name + "W", [F(fid, "f%d" % k, b(ty[fid])) for k, fid in enumerate(ids)])
    to = T.struct_type(name + "N", [F(fid, "f%d" % k, b(ty[fid]), req_of.get(fid, OPT)) for k, fid in enumerate(ids)
                                    if fid in kept])
    return frm, to


def wide_pair(n, ids, seed=0, top="req"):
    """(wide, narrow): flat structs, n fields in `from` with ids by mode `ids`
    ("dense": 1..n; "neg": a range around 0 and -32768, -1, 0, 32767;
    "sparse": a sample of the whole int16 range). `to` keeps about 70 % of them
    (and at least 64 non-negative ids where `from` has that many); up to 64 of
    the kept non-negative ids are tracked: exactly 64 then. top = "req": about one
    tracked field in five is REQUIRED, the rest DEFAULT, and where 64 are
    tracked the highest one (bit 63 of the live mask) is REQUIRED. top = "def":
    every tracked field is DEFAULT, the highest included, so a message with none
    of them writes 64 literals at its STOP."""
    key = (n, ids, seed, top)
    if key not in _WIDE:
        rng = random.Random(1000 * seed + 7 * n + WIDE_MODES.index(ids))
        all_ids = wide_ids(n, ids, rng)
        kept = set(rng.sample(all_ids, max(1, round(0.7 * n))))
        spare = [i for i in all_ids if i >= 0 and i not in kept]
        if len(spare) + sum(i >= 0 for i in kept) >= 64:  # `from` has 64 non-negative ids: `to` keeps that many
            rng.shuffle(spare)
            while sum(i >= 0 for i in kept) < 64:
                kept.add(spare.pop())
        can = sorted(i for i in kept if i >= 0)
        tracked = sorted(rng.sample(can, 64)) if len(can) > 64 else can
        req_of = {i: REQ if top == "req" and rng.random() < 0.2 else DEF for i in tracked}
        if top == "req" and len(tracked) == 64:
            req_of[tracked[-1]] = REQ
        _WIDE[key] = flat_pair("Wide%d%s" % (n, ids), all_ids, kept, req_of)
    return _WIDE[key]


def tracked_ids(to):
    return sorted(fid for fid, on in to.struct.requires.items() if on)


def _scalar(rng, name):
    if name == "string":
        return _str(0, rng.randrange(13), rng)[3:]
    if name == "bool":
        return bytes([rng.randrange(2)])
    return bytes(rng.randrange(256) for _ in range({"i32": 4, "i64": 8, "double": 8, "i16": 2, "byte": 1}[name]))


FLAT_KINDS = ("all", "some", "bare", "some", "no_top", "unknown", "rand", "some", "type", "unknown")  # 6 in 10 can cut


def flat_message(rng, frm, to, kind):
    """A message over a flat pair, its fields in random order. all: every
    field; some: about half, every REQUIRED one among them; bare: no tracked
    field at all; no_top: as some, but without the highest tracked id; rand:
    about 60 % of the fields whatever they are; unknown: as some, and a field
    `from` does not have (with a negative id where one is free); type: as some,
    and one field under another wire type (a negative id where `from` has one)."""
    ids = sorted(frm.struct.ids)
    tr = tracked_ids(to)
    req = {i for i in tr if to.struct.field_by_id(i).required == REQ}
    if kind == "all":
        pick = list(ids)
    elif kind == "bare":
        pick = [i for i in ids if i not in tr and rng.random() < 0.5]
    elif kind == "rand":
        pick = [i for i in ids if rng.random() < 0.6]
    else:
        pick = [i for i in ids if i in req or rng.random() < 0.5]
        if kind == "no_top" and tr:
            pick = [i for i in pick if i != tr[-1]]
    rng.shuffle(pick)
    parts = [bytes([frm.struct.field_by_id(i).type.type]) + struct.pack(">h", i) + _scalar(rng, frm.struct.field_by_id(i).type.name)
             for i in pick]
    if kind == "unknown":
        fid = next(i for i in (-2, -7, -300, -32767, 32766, 5000, 901, 77) if i not in frm.struct.ids)
        parts.insert(rng.randrange(len(parts) + 1), b"\x0a" + struct.pack(">h", fid) + _scalar(rng, "i64"))
    if kind == "type":
        fid = rng.choice([i for i in ids if i < 0] or ids)
        wrong = "i32" if frm.struct.field_by_id(fid).type.name == "string" else "string"
        parts = [p for p in parts if struct.unpack_from(">h", p, 1)[0] != fid]
        parts.insert(rng.randrange(len(parts) + 1), bytes([b(wrong).type]) + struct.pack(">h", fid) + _scalar(rng, wrong))
    return b"".join(parts) + b"\x00"


def flat_messages(frm, to, seed, count=48, bad=16):
    """(messages, mutated copies of the first `bad`): the kinds of flat_message in turn"""
    rng, mrng = random.Random(seed), random.Random(seed + 1000)
    msgs = [flat_message(rng, frm, to, FLAT_KINDS[k % len(FLAT_KINDS)]) for k in range(count)]
    return msgs, [t2jgen.mutate(mrng, m) for m in msgs[:bad]]


class Family:
    """A descriptor pair with its messages (unmutated first, then the mutated
    copies) and the checker's answers per option word, computed once."""

    def __init__(self, name, frm, to, msgs, bad):
        self.name, self.frm, self.to, self.msgs, self.n_good = name, frm, to, msgs + bad, len(msgs)
        self._want, self._blob = {}, None

    def want(self, opts=0):
        if opts not in self._want:
            self._want[opts] = expect(self.msgs, self.frm, self.to, opts)
        return self._want[opts]

    def blob(self):
        if self._blob is None:
            from dynamicgo_amd import generic as X
            self._blob = X.compile_cut(self.frm, self.to)
        return self._blob

    def assert_worth_running(self):
        """at least half of the unmutated messages cut under option word 0"""
        ok = sum(r == 0 for r, _ in self.want(0)[:self.n_good])
        assert ok * 2 >= self.n_good, (self.name, ok, self.n_good)


_FAMILY = {}


def wide_family(n, ids, top="req"):
    key = ("wide", n, ids, top)
    if key not in _FAMILY:
        frm, to = wide_pair(n, ids, top=top)
        _FAMILY[key] = Family("wide %d %s %s" % (n, ids, top), frm, to, *flat_messages(frm, to, 31 * n + len(ids)))
    return _FAMILY[key]


# the cases of the CPU walk; the GPU runs those of WIDE_GPU_NS. top = "def" where 64 fields are tracked.
WIDE_DEF = ((64, "dense"), (129, "neg"), (300, "sparse"))
WIDE_GPU_NS = (64, 65, 129, 300)


def wide_cases(ns=WIDE_NS):
    return [(n, m, "req") for n in ns for m in WIDE_MODES] + [(n, m, "def") for n, m in WIDE_DEF if n in ns]


def _empty(td):
    w = bytearray()
    R.write_empty(w, td)
    return bytes(w)


def check_wide_corpus(cases):
    """What the wide families have to hold, from the checker alone: every
    family is worth running; every status but OVERFLOW and DEPTH occurs; an
    E_REQUIRED names a bit-63 field; an E_UNKNOWN or E_TYPE carries a negative
    id, sign-extended in aux; under WRITE_DEFAULT a message writes all 64
    literals of a struct that requires none."""
    seen, top_required, negative, all_lits = set(), 0, 0, 0
    for n, mode, top in cases:
        fam = wide_family(n, mode, top)
        fam.assert_worth_running()
        tr = tracked_ids(fam.to)
        if sum(i >= 0 for i in fam.frm.struct.ids) >= 64:
            assert len(tr) == 64, (fam.name, len(tr))
        if top == "def":
            assert len(tr) == 64 and not any(fam.to.struct.field_by_id(i).required == REQ for i in tr)
        elif len(tr) == 64:
            assert fam.to.struct.field_by_id(tr[-1]).required == REQ
        lits = [struct.pack(">Bh", fam.to.struct.field_by_id(i).type.type, i) for i in tr]
        lit_bytes = sum(len(h) + len(_empty(fam.to.struct.field_by_id(i).type)) for h, i in zip(lits, tr))
        for o in ALL_OPTS:
            for k, (m, (r, out)) in enumerate(zip(fam.msgs, fam.want(o))):
                st, aux = r & 0xFF, r >> 32
                seen.add(st)
                if st == R.E_REQUIRED and len(tr) == 64 and aux == tr[-1]:
                    top_required += 1
                if st in (R.E_UNKNOWN, R.E_TYPE) and aux >= 1 << 31:
                    fid = aux - (1 << 32)
                    assert -32768 <= fid < 0 and aux == fid & 0xFFFFFFFF and struct.pack(">h", fid) in m
                    negative += 1
                # every literal of a struct that requires nothing: the output is longer by all of them
                if o == R.WRITE_DEFAULT and top == "def" and r == 0 and len(out) - len(fam.want(0)[k][1]) == lit_bytes:
                    assert all(h in out for h in lits)
                    all_lits += 1
    assert seen == {R.OK, R.E_READ, R.E_TYPE, R.E_UNKNOWN, R.E_REQUIRED}, seen
    assert top_required >= 1 and negative >= 1 and all_lits >= 1, (top_required, negative, all_lits)


STAGED_DELTAS = (-8, 0, 8)
_STAGED_DROPPED = {-8: 9, 0: 10, 8: 11}


def staged_pair(delta):
    """A flat pair whose plan tables are exactly CUT_LANE_PLAN + delta bytes
    long: 100 kept fields (a node, a field and a child node each: 48 bytes), 17
    of them tracked (DEFAULT; a literal entry each: 8 bytes) and 10, 9 or 11
    dropped fields (8 bytes each) behind the 64-byte header and the root node."""
    key = ("staged", delta)
    if key not in _WIDE:
        from dynamicgo_amd import generic as X
        n = 100 + _STAGED_DROPPED[delta]
        ids = list(range(1, n + 1))
        kept = set(ids[:50] + ids[-50:])  # the dropped ones in the middle of the binary search
        pair = flat_pair("Staged%d" % (delta + 8), ids, kept, {i: DEF for i in sorted(kept)[::6]})
        got = tab_len(X.compile_cut(*pair))
        assert got == lane_plan_cap() + delta, "the plan's tables are %d bytes, not CUT_LANE_PLAN %+d" % (got, delta)
        _WIDE[key] = pair
    return _WIDE[key]


def staged_family(delta):
    key = ("staged", delta)
    if key not in _FAMILY:
        frm, to = staged_pair(delta)
        _FAMILY[key] = Family("staged %+d" % delta, frm, to, *flat_messages(frm, to, 77 + delta, 64, 16))
    return _FAMILY[key]


PAD_ID, PAD_FIELDS, PAD_SEED, PAD_N = 100, 330, 9, 160


def padded_pair():
    """pair() with one more field (100) on both sides: a struct of 330 scalar
    fields, narrowed in `to` (every tenth dropped, a few DEFAULT), which takes
    the plan's tables past 3 x CUT_LANE_PLAN: the whole fuzz shape with the plan
    read from device memory on the lane route."""
    if "padded" not in _WIDE:
        from dynamicgo_amd import generic as X
        wide, narrow = pair()
        ids = list(range(1, PAD_FIELDS + 1))
        pad_w, pad_n = flat_pair("Pad", ids, {i for i in ids if i % 10}, {i: DEF for i in (3, 64, 65, 257)})
        p = (T.struct_type("WideP", list(wide.struct.fields) + [F(PAD_ID, "pad", pad_w)]),
             T.struct_type("NarrowP", list(narrow.struct.fields) + [F(PAD_ID, "pad", pad_n)]))
        assert tab_len(X.compile_cut(*p)) > 3 * lane_plan_cap()
        _WIDE["padded"] = p
    return _WIDE["padded"]


def padded_family():
    """PAD_N messages and as many mutated copies over padded_pair, drawn as fuzz() draws its own"""
    if "padded" not in _FAMILY:
        frm, to = padded_pair()
        rng, mrng = random.Random(PAD_SEED), random.Random(PAD_SEED + 1000)
        msgs = [t2jgen.gen_thrift(rng, frm, keep_p=0.5) for _ in range(PAD_N)]
        _FAMILY["padded"] = Family("padded", frm, to, msgs, [t2jgen.mutate(mrng, m) for m in msgs])
    return _FAMILY["padded"]


def write_corpus(path, msgs, caps, blob, opts):
    """the file cut_walk_host.cpp's stand-alone program reads"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<3I", len(msgs), opts, len(blob)) + blob)
        for m, c in zip(msgs, caps):
            fh.write(struct.pack("<2I", len(m), c) + m)
