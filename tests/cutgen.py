"""Inputs of the cut tests (test_cut_host.py on the CPU, test_gpu_cut.py on the
GPU): a wide / narrow descriptor pair written for these tests, the fuzz corpus
over it, container chains around the frame limits, kept runs of chosen length
and alignment, and the expectations from the checker (cutref.py). Seeded; pure
Python."""
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


def write_corpus(path, msgs, caps, blob, opts):
    """the file cut_walk_host.cpp's stand-alone program reads"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<3I", len(msgs), opts, len(blob)) + blob)
        for m, c in zip(msgs, caps):
            fh.write(struct.pack("<2I", len(m), c) + m)
