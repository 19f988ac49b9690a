"""The yardstick of the typed-column tests: tgetref.get_by_path followed by the
reference's casts (thrift/generic/cast.go) over its decoders
(thrift/binary.go), each rule cited where it is restated. It returns the cell
the device returns (include/dgj2t.h dg_cols_*); the device is never compared
with itself."""
import struct
from collections import namedtuple

import tgetref as R

BOOL, BYTE, INT, F64, STR, LEN, LIST = 1, 2, 3, 4, 5, 6, 16  # DG_COL_*
LIST_INT, LIST_F64 = LIST | INT, LIST | F64
E_UNSUPPORTED = 4  # DG_COL_E_UNSUPPORTED: meta.ErrUnsupportedType
KINDS = (BOOL, BYTE, INT, F64, STR, LEN, LIST_INT, LIST_F64)
_VALID = {0, 1, 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15, 16, 17}  # Type.Valid, thrift/descriptor.go:60-67
_INT_FMT = {R.BYTE: ">B", R.I16: ">h", R.I32: ">i", R.I64: ">q"}

# val: the cell's 8 bytes as an unsigned int; elems: a list cell's elements as unsigned ints (None elsewhere)
Cell = namedtuple("Cell", "status type step aux val len elems")


def _u64(v: int) -> int:
    return v & 0xFFFFFFFFFFFFFFFF


def _int(t: int, b: bytes):
    """Node.int, cast.go:124-138: I08 through DecodeByte (unsigned, int(byte)),
    I16 / I32 / I64 through DecodeInt16/32/64 (signed); None = the default arm,
    ErrUnsupportedType (cast.go:136)."""
    fmt = _INT_FMT.get(t)
    if fmt is None:
        return None
    return _u64(struct.unpack_from(fmt, b)[0])


def cell(buf: bytes, path, kind: int, root_type: int = R.STRUCT, base: int = 0) -> Cell:
    """Cell of (message, column): v.GetByPath(path...) and the cast of `kind`.
    base: the message's offset in the arena (STR and list values are arena
    offsets)."""
    r = R.get_by_path(buf, path, root_type)
    if r.status != R.OK:  # the cast returns the error node as it is (cast.go:51, 84, 101, 118, 142, 159, 199)
        return Cell(r.status, r.type, r.step, r.aux, 0, 0, None)
    t, at = r.type, buf[r.start:]

    def unsupported(aux=0):
        return Cell(E_UNSUPPORTED, t, r.step, aux, 0, 0, None)

    def ok(val, ln=0, typ=t, elems=None):
        return Cell(R.OK, typ, r.step, 0, _u64(val), ln, elems)

    if kind & LIST:
        if t not in (R.LIST, R.SET):  # should2("List", LIST, SET), cast.go:202
            return unsupported()
        et, size = at[0], struct.unpack_from(">i", at, 1)[0]
        if et not in _VALID:  # iterElems -> ReadListBegin, binary.go:625-649
            return Cell(R.E_READ, 0, r.step, 0, 0, 0, None)
        if size == 0:  # the loop of cast.go:211 never runs
            return ok(base + r.start + 5, 0, et, [])
        width = R._TYPE_SIZE.get(et, 0)
        if kind == LIST_INT:
            if et not in _INT_FMT:  # e.Int() on the first element: cast.go:136
                return unsupported(et)
            elems = [_int(et, at[5 + j * width:]) for j in range(size)]
        else:
            if et != R.DOUBLE:  # e.Float64(): cast.go:153
                return unsupported(et)
            elems = [struct.unpack_from(">Q", at, 5 + j * 8)[0] for j in range(size)]  # DecodeDouble: the bits
        return ok(base + r.start + 5, size, et, elems)
    if kind == BOOL:  # cast.go:107-114; DecodeBool, binary.go:2152: int8(b[0]) == 1
        return ok(1 if at[0] == 1 else 0) if t == R.BOOL else unsupported()
    if kind == BYTE:  # cast.go:90-97
        return ok(at[0]) if t == R.BYTE else unsupported()
    if kind == INT:
        v = _int(t, at)
        return ok(v) if v is not None else unsupported()
    if kind == F64:  # cast.go:148-155; the bits of the big-endian double
        return ok(struct.unpack_from(">Q", at)[0]) if t == R.DOUBLE else unsupported()
    if kind == STR:  # cast.go:165-195: String and Binary take STRING alone
        return ok(base + r.start + 4, r.end - r.start - 4) if t == R.STRING else unsupported()
    if kind == LEN:  # cast.go:57-68: the i32 at +1 (LIST, SET) or +2 (MAP)
        if t in (R.LIST, R.SET):
            return ok(struct.unpack_from(">i", at, 1)[0])
        if t == R.MAP:
            return ok(struct.unpack_from(">i", at, 2)[0])
        return unsupported()
    raise ValueError(kind)


def column(msgs, path, kind: int, root_type: int = R.STRUCT, first: int = 0):
    """The cells of one column over a batch laid out back to back from arena offset `first`."""
    out, base = [], first
    for m in msgs:
        out.append(cell(m, path, kind, root_type, base))
        base += len(m)
    return out
