"""Inputs and comparisons that the CPU build of the Children walk
(test_kids_host.py) and the GPU tests (test_gpu_kids.py) share: the fuzz paths,
hand-built messages for what the corpus lacks (BINKEY maps, int keys at their
extremes, headers only ReadListBegin / ReadMapBegin refuse), one message with
every container kind for the prefix cut, chains around the frame and depth
limits, the wide-route nodes, and the checker's answer as the arrays the device
returns."""
import random
import struct

import numpy as np

import kidsref as K
import t2jgen
import tgetgen as TG
import tgetref as R

F, I = R.FIELD, R.INDEX
LDS_LEVELS = 8  # KD_LDS_DEPTH (dynamicgo_amd/csrc/kids_device.h)

# paths over t2jgen.all_types_desc(): the root, every container field, one element, one nested struct, a scalar
FUZZ_PATHS = {
    "": [], "f9": [(F, 9)], "f10": [(F, 10)], "f10[0]": [(F, 10), (I, 0)], "f11": [(F, 11)], "f12": [(F, 12)],
    "f13": [(F, 13)], "f15": [(F, 15)], "f16": [(F, 16)], "f17": [(F, 17)], "f17.f3": [(F, 17), (F, 3)],
    "f19": [(F, 19)], "f20": [(F, 20)], "f18": [(F, 18)],
}
CONTAINER_PATHS = [k for k in FUZZ_PATHS if k != "f18"]


def fuzz_messages(n=2048):
    rng, mrng = random.Random(1234), random.Random(4321)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(n)]
    return msgs, [t2jgen.mutate(mrng, m) for m in msgs]


def expect(msgs, path, recurse, root_type=R.STRUCT):
    """The checker's answer as (head, rec_off, recs) arrays of generic.KIDS_HEAD_DTYPE / uint64 / KIDS_REC_DTYPE."""
    from dynamicgo_amd.generic import KIDS_HEAD_DTYPE, KIDS_REC_DTYPE
    heads, kids = [], []
    for m in msgs:
        h, ks = K.children(m, path, recurse, root_type)
        heads.append(tuple(h))
        kids.append(ks)
    head = np.array(heads, dtype=KIDS_HEAD_DTYPE).reshape(len(msgs))
    rec_off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in kids], out=rec_off[1:])
    recs = np.array([tuple(k) for ks in kids for k in ks], dtype=KIDS_REC_DTYPE).reshape(int(rec_off[-1]))
    return head, rec_off, recs


def same(got, want, what):
    """(head, rec_off, recs) field by field"""
    for name, g, w in zip(("head", "rec_off", "recs"), got, want):
        assert g.shape == w.shape, "%s: %s has shape %s, checker %s" % (what, name, g.shape, w.shape)
        for f in (w.dtype.names or [None]):
            a, b = (g, w) if f is None else (g[f], w[f])
            bad = np.argwhere(a != b)
            assert bad.size == 0, "%s: %s.%s differs at %s: got %s, checker %s" % (
                what, name, f, bad[:5].ravel().tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def share(head, status):
    return float((head["status"] == status).mean())


# ---------------------------------------------------------------- hand-built
def _wstr(s: bytes) -> bytes:
    return struct.pack(">i", len(s)) + s


def _field(t, fid, v):
    return struct.pack(">bh", t, fid) + v


def _map(kt, vt, ents):
    return struct.pack(">bbi", kt, vt, len(ents)) + b"".join(k + v for k, v in ents)


def _list(et, vals, size=None):
    return struct.pack(">bi", et, len(vals) if size is None else size) + b"".join(vals)


_I32 = lambda v: struct.pack(">i", v)  # noqa: E731
_EMPTY_STRUCT = b"\x00"
_SMALL_STRUCT = _field(R.I32, 1, _I32(5)) + b"\x00"


def hand_messages():
    """{name: message}: struct{1: <the case>, 2: i32 9}; looked at under path f1 and, for the nesting, the empty path."""
    cases = {
        "map<bool,i32>": (R.MAP, _map(R.BOOL, R.I32, [(b"\x01", _I32(1)), (b"\x00", _I32(2))])),
        "map<double,string>": (R.MAP, _map(R.DOUBLE, R.STRING, [(struct.pack(">d", 0.5), _wstr(b"half")),
                                                                (struct.pack(">d", -2.0), _wstr(b""))])),
        "map<struct,struct>": (R.MAP, _map(R.STRUCT, R.STRUCT, [(_SMALL_STRUCT, _SMALL_STRUCT), (_EMPTY_STRUCT, _EMPTY_STRUCT)])),
        "map<list,list>": (R.MAP, _map(R.LIST, R.LIST, [(_list(R.I16, [b"\0\1", b"\0\2"]), _list(R.STRING, [_wstr(b"x")])),
                                                        (_list(R.STRUCT, [_SMALL_STRUCT]), _list(R.I64, []))])),
        "map<i08,i32>": (R.MAP, _map(R.BYTE, R.I32, [(b"\x80", _I32(1)), (b"\xff", _I32(2)), (b"\x7f", _I32(3))])),
        "map<i16,i32>": (R.MAP, _map(R.I16, R.I32, [(struct.pack(">h", k), _I32(k)) for k in (-32768, 32767, -1)])),
        "map<i32,struct>": (R.MAP, _map(R.I32, R.STRUCT, [(_I32(k), _SMALL_STRUCT) for k in (-2 ** 31, 2 ** 31 - 1, -1)])),
        "map<i64,string>": (R.MAP, _map(R.I64, R.STRING, [(struct.pack(">q", k), _wstr(b"v")) for k in
                                                          (-2 ** 63, 2 ** 63 - 1, -1, 2 ** 32)])),
        "map<string,i32>": (R.MAP, _map(R.STRING, R.I32, [(_wstr(b""), _I32(0)), (_wstr(b"k"), _I32(1)),
                                                          (_wstr(bytes(range(256)) + b"y" * 44), _I32(300))])),
        "empty struct": (R.STRUCT, _EMPTY_STRUCT),
        "empty list": (R.LIST, _list(R.I32, [])),
        "empty map": (R.MAP, _map(R.STRING, R.STRUCT, [])),
        "list<type 5> of 0": (R.LIST, _list(5, [])),
        "list<list<type 5> of 0>": (R.LIST, _list(R.LIST, [_list(5, [])])),
        "map<type 5, i32> of 0": (R.MAP, _map(5, R.I32, [])),
        "map<i32, type 9> of 0": (R.MAP, _map(R.I32, 9, [])),
        "struct{list<type 7> of 0}": (R.STRUCT, _field(R.LIST, 1, _list(7, [])) + b"\x00"),
        "list of -1": (R.LIST, _list(R.I32, [], size=-1)),
        "map of -1": (R.MAP, struct.pack(">bbi", R.I32, R.I32, -1)),
        "list<list of -1>": (R.LIST, _list(R.LIST, [_list(R.I32, [], size=-1)])),
        "field type 18": (R.STRUCT, _field(R.I32, 1, _I32(1)) + struct.pack(">bh", 18, 2) + _I32(2) + b"\x00"),
        "field type 1": (R.STRUCT, struct.pack(">bh", 1, 2) + b"\x00"),
        "list<string>": (R.LIST, _list(R.STRING, [_wstr(b"a"), _wstr(b""), _wstr(b"ccc")])),
        "set<struct>": (R.SET, _list(R.STRUCT, [_SMALL_STRUCT, _EMPTY_STRUCT])),
        "string key of -1": (R.MAP, struct.pack(">bbi", R.STRING, R.I32, 1) + _I32(-1) + _I32(0)),
        "i32": (R.I32, _I32(77)),
        "string": (R.STRING, _wstr(b"scalar")),
        "short string": (R.STRING, _I32(50) + b"x"),
    }
    return {k: _field(t, 1, v) + _field(R.I32, 2, _I32(9)) + b"\x00" for k, (t, v) in cases.items()}


def every_kind_message() -> bytes:
    """~80 bytes holding a struct, a list, a set and maps of each key kind, nested two deep somewhere"""
    inner = _field(R.LIST, 1, _list(R.I16, [b"\0\1", b"\0\2"])) + _field(R.STRING, 2, _wstr(b"s")) + b"\x00"
    m = (_field(R.STRUCT, 1, inner) + _field(R.SET, 2, _list(R.STRING, [_wstr(b"ab")])) +
         _field(R.MAP, 3, _map(R.STRING, R.LIST, [(_wstr(b"k"), _list(R.BOOL, [b"\1"]))])) +
         _field(R.MAP, 4, _map(R.BYTE, R.STRUCT, [(b"\xfe", _EMPTY_STRUCT)])) +
         _field(R.MAP, 5, _map(R.DOUBLE, R.I32, [(struct.pack(">d", 1.0), _I32(4))])) + b"\x00")
    return m


def prefixes(m: bytes):
    return [m[:k] for k in range(len(m) + 1)]


# -------------------------------------------------------------------- chains
CHAIN_PATHS = [[], [(F, 1)]]


def lds_chains():
    """chains of every kind at depths 6-10, around the 8 LDS levels"""
    return [(k * d, lf) for k in TG.KINDS for d in range(6, 11) for lf in "ie"]


def limit_chains():
    """... and around MaxSkipDepth. The checker's recursive mode is quadratic in depth (it is the Go's), so the
    recursive runs take the depths next to the limit only."""
    return [(k * d, "i") for k in TG.KINDS for d in range(1018, 1028)]


def limit_chains_recursive():
    return [(k * d, "i") for k in "SLK" for d in (1022, 1023, 1024)]


# ---------------------------------------------------------------------- wide
WIDE_SIZES = (0, 1, 63, 64, 65, 1000)


def wide_messages():
    """{name: message}: struct{1: node, 2: i32} with node a list<i64>, set<i16>, list<bool>, map<i32,i64> or
    map<byte,bool> of each of WIDE_SIZES, and each of 65 entries cut inside the last one"""
    out = {}
    for n in WIDE_SIZES:
        nodes = {
            "list<i64>": (R.LIST, _list(R.I64, [struct.pack(">q", i * 3 - 5) for i in range(n)])),
            "set<i16>": (R.SET, _list(R.I16, [struct.pack(">h", i - 7) for i in range(n)])),
            "list<bool>": (R.LIST, _list(R.BOOL, [bytes([i & 1]) for i in range(n)])),
            "map<i32,i64>": (R.MAP, _map(R.I32, R.I64, [(_I32(i * 1000003 - 2 ** 31), struct.pack(">q", i)) for i in range(n)])),
            "map<byte,bool>": (R.MAP, _map(R.BYTE, R.BOOL, [(bytes([(i * 7) & 255]), bytes([i & 1])) for i in range(n)])),
        }
        for name, (t, v) in nodes.items():
            out["%s x %d" % (name, n)] = _field(t, 1, v) + _field(R.I32, 2, _I32(9)) + b"\x00"
            if n == 65:
                out["%s x 65, cut" % name] = _field(t, 1, v)[:-1]
    return out
