"""The yardstick of the Children tests: a pure-Python restatement of the
reference's GetByPath + Node.Children (thrift/generic/node.go:1133-1154;
PathNode.scanChildren and handleChild, path.go:796-836, 1121-1248) on
tgetref.Proto, written as the Go reads: every child is skipped with SkipType
and, in recursive mode, a complex child's bytes are then scanned AGAIN by a
recursive call on `p.Buf[ss:]` (skip-then-scan, quadratic in depth). It
returns the head and the records the device returns (include/dgj2t_defs.h
dg_kids_head, dg_kid_rec); the device is never compared with itself."""
from collections import namedtuple

import tgetref as R

UNSUPPORTED = 4  # DG_KIDS_E_UNSUPPORTED: meta.ErrUnsupportedType
NO_PARENT = 0xFFFFFFFF
COMPLEX = (R.STRUCT, R.MAP, R.SET, R.LIST)
INTS = (R.BYTE, R.I16, R.I32, R.I64)

Head = namedtuple("Head", "count direct start type key_type elem_type status")
Kid = namedtuple("Kid", "start end key_start parent key type kind depth n_desc")


def _scan(p: R.Proto, origin: int, t: int, recurse: bool, out: list, parent: int, depth: int):
    """scanChildren of a node of type t whose bytes are p.buf (p.read = 0);
    origin = where p.buf starts in the message. Returns (key type, element type)."""

    def handle_child(kind, key, key_start, et):  # path.go:796-836, with v.Path set by the caller
        ss = p.read
        p.skip_type(et)
        idx = len(out)
        out.append([origin + ss, origin + p.read, origin + key_start, parent, key, et, kind, depth, 0])
        if recurse and et in COMPLEX:
            sub = R.Proto(p.buf[ss:])  # p.Buf = p.Buf[ss:]; p.Read = 0
            _scan(sub, origin + ss, et, recurse, out, idx, depth + 1)
            p.read = ss + sub.read
            out[idx][8] = len(out) - idx - 1

    if t == R.STRUCT:
        while True:
            at = p.read
            et, fid = p.read_field_begin()
            if et == R.STOP:
                return 0, 0
            handle_child(R.FIELD, fid, at, et)
    if t in (R.LIST, R.SET):
        et, size = p.read_list_begin()
        for i in range(size):
            handle_child(R.INDEX, i, p.read, et)
        return 0, et
    if t == R.MAP:
        kt, et, size = p.read_map_begin()
        for _ in range(size):
            ks = p.read
            if kt == R.STRING:
                handle_child(R.STRKEY, len(p.read_string()), ks, et)
            elif kt in INTS:
                handle_child(R.INTKEY, p.read_int(kt), ks, et)
            else:
                p.skip_type(kt)
                handle_child(R.BINKEY, p.read - ks, ks, et)
        return kt, et
    raise AssertionError(t)


def children(buf: bytes, path=(), recurse: bool = False, root_type: int = R.STRUCT):
    """(Head, [Kid]) of v.GetByPath(path...).Children(&out, recurse, &Options{});
    path as tgetref.get_by_path takes it."""
    n = len(path)
    if n:
        r = R.get_by_path(buf, path, root_type)  # ends with SkipType(node): node.go:480
        if r.status != R.OK:
            return Head(0, r.step, 0, 0, 0, 0, r.status), []
        node, origin, t = buf[r.start:r.end], r.start, r.type
    else:
        node, origin, t = buf, 0, root_type  # node.go:440: no skip, the buffer is the whole message
    if t not in COMPLEX:
        return Head(0, n, origin, t, 0, 0, UNSUPPORTED), []
    out = []
    try:
        kt, et = _scan(R.Proto(node), 0 + origin, t, recurse, out, NO_PARENT, 1)
    except R.ReadError:
        return Head(0, n, 0, 0, 0, 0, R.E_READ), []  # Children leaves `out` untouched on an error
    return Head(len(out), sum(1 for k in out if k[7] == 1), origin, t, kt, et, R.OK), [Kid(*k) for k in out]


def key_bytes(buf: bytes, k: Kid) -> bytes:
    """The bytes of a STRKEY / BINKEY child's key."""
    return buf[k.key_start + 4:k.key_start + 4 + k.key] if k.kind == R.STRKEY else buf[k.key_start:k.key_start + k.key]
