"""The yardstick of the entry-column tests: tgetref.get_by_path followed by the
reference's Node.List with String per element, Node.StrMap and Node.IntMap
(thrift/generic/cast.go:198-286) over its iterators (iter.go:41-68, 105-135,
137-240) and ReadMapBegin / ReadListBegin, each rule cited where it is
restated. It returns the cell and the entries the device returns
(include/dgj2t.h dg_ents_*); it imports no kernel and the device is never
compared with itself."""
import struct
from collections import namedtuple

import tgetref as R

BOOL, INT, F64, STR = 1, 3, 4, 5  # DG_ENT_*: the value kinds
LISTSTR, STRMAP, INTMAP = 0x15, 0x20, 0x40
E_UNSUPPORTED = 4  # DG_COL_E_UNSUPPORTED: meta.ErrUnsupportedType
VALUE_KINDS = (BOOL, INT, F64, STR)
KINDS = (LISTSTR,) + tuple(m | v for m in (STRMAP, INTMAP) for v in VALUE_KINDS)
_VALID = {0, 1, 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15, 16, 17}  # Type.Valid, thrift/descriptor.go:60-67
_INTS = (R.BYTE, R.I16, R.I32, R.I64)  # Type.IsInt
# what Node.Interface (cast.go:342-356) gives on a value's wire type, by the value kind that reads it
_TAKES = {BOOL: (R.BOOL,), INT: _INTS, F64: (R.DOUBLE,), STR: (R.STRING,)}

# val: the cell's 8 bytes; span: the bytes from val to the container's end (OK cells); keys / klens / vals / vlens:
# the entries of an OK cell as unsigned ints (a list cell has no keys: zeros), None elsewhere
Cell = namedtuple("Cell", "status type step aux val len span keys klens vals vlens")


def _u64(v: int) -> int:
    return v & 0xFFFFFFFFFFFFFFFF


def _scalar(v: int, vt: int, p: R.Proto) -> int:
    """One value of wire type vt through the arm of Node.Interface that value kind v names"""
    if v == BOOL:  # Node.bool -> DecodeBool, binary.go:2152: int8(b[0]) == 1
        return 1 if p.read_byte() == 1 else 0
    if v == F64:  # Node.float64 -> DecodeDouble: the bits
        return struct.unpack(">Q", p.next(8))[0]
    return _u64(p.read_int(vt))  # Node.int, cast.go:124-138: I08 through DecodeByte, unsigned


def cell(buf: bytes, path, kind: int, root_type: int = R.STRUCT, base: int = 0) -> Cell:
    """Cell of (message, column): v.GetByPath(path...) and the cast of `kind`.
    base: the message's offset in the arena."""
    r = R.get_by_path(buf, path, root_type)

    def fail(status, typ, aux=0):
        return Cell(status, typ, r.step, aux, 0, 0, 0, None, None, None, None)

    if r.status != R.OK:  # self.IsError(): the error node as it is (cast.go:199, 228, 259)
        return Cell(r.status, r.type, r.step, r.aux, 0, 0, 0, None, None, None, None)
    t = r.type
    p = R.Proto(buf[r.start:r.end])  # self.raw()
    keys, klens, vals, vlens = [], [], [], []
    if kind == LISTSTR:
        if t not in (R.LIST, R.SET):  # should2("List", LIST, SET), cast.go:202
            return fail(E_UNSUPPORTED, t)
        try:
            et, size = p.read_list_begin()  # iterElems, iter.go:56-68
        except R.ReadError:
            return fail(R.E_READ, 0)  # cast.go:207
        hdr, typ, aux = 5, et, 0
        for _ in range(size):  # it.HasNext(): the lookup's skip has seen size whole elements
            if et != R.STRING:  # v.Interface -> e.String(): cast.go:165-181 takes STRING alone
                return fail(E_UNSUPPORTED, t, et)
            s = p.read_string()
            keys.append(0), klens.append(0)
            vals.append(base + r.start + p.read - len(s)), vlens.append(len(s))
    else:
        if t != R.MAP:  # should("StrMap" / "IntMap", MAP), cast.go:231, 262
            return fail(E_UNSUPPORTED, t)
        v = kind & 15
        if kind & INTMAP and buf[r.start] not in _INTS:  # self.kt.IsInt(), cast.go:265: the raw byte of node.go:66-68
            return fail(E_UNSUPPORTED, t, buf[r.start])
        try:
            kt, vt, size = p.read_map_begin()  # iterPairs, iter.go:41-54
        except R.ReadError:
            return fail(R.E_READ, 0)  # cast.go:235, 269
        hdr, typ, aux = 6, t, kt | vt << 8
        if kind & STRMAP and kt != R.STRING:  # cast.go:238, whatever the size
            return fail(E_UNSUPPORTED, t, aux)
        for _ in range(size):
            if vt not in _TAKES[v]:  # the first value's Interface (checked once: DESIGN 3.13)
                return fail(E_UNSUPPORTED, t, aux)
            if kind & STRMAP:  # NextStr, iter.go:178-200
                s = p.read_string()
                keys.append(base + r.start + p.read - len(s)), klens.append(len(s))
            else:  # NextInt: ReadInt, a byte comes back unsigned
                keys.append(_u64(p.read_int(kt))), klens.append(0)
            if v == STR:
                s = p.read_string()
                vals.append(base + r.start + p.read - len(s)), vlens.append(len(s))
            else:
                vals.append(_scalar(v, vt, p)), vlens.append(0)
    assert p.read == len(p.buf), "the lookup's skip and the walk disagree"
    return Cell(R.OK, typ, r.step, aux, base + r.start + hdr, len(vals), r.end - r.start - hdr, keys, klens, vals, vlens)


def column(msgs, path, kind: int, root_type: int = R.STRUCT, first: int = 0):
    """The cells of one column over a batch laid out back to back from arena offset `first`."""
    out, base = [], first
    for m in msgs:
        out.append(cell(m, path, kind, root_type, base))
        base += len(m)
    return out
