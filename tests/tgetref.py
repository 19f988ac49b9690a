"""The yardstick of the path-lookup tests: a pure-Python restatement of the
reference's GetByPath (thrift/generic/node.go:292-484 with value.go:70-161's
LIST/SET rule), the Read*Begin checks it goes through (thrift/binary.go:562-649,
737-791) and skipType (thrift/binary_skip.go:109-204), written as the Go reads:
a protocol object with a read position, recursion for nesting, errors as
exceptions. It returns the record the device returns (include/dgj2t.h
dg_tget_rec); the device is never compared with itself."""
import struct
from collections import namedtuple

STOP, VOID, BOOL, BYTE, DOUBLE, I16, I32, I64, STRING, STRUCT, MAP, SET, LIST, UTF8, UTF16 = \
    0, 1, 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15, 16, 17
OK, NOT_FOUND, E_READ, E_TYPE = 0, 1, 2, 3
FIELD, INDEX, STRKEY, INTKEY, BINKEY = 1, 2, 3, 4, 5
MAX_SKIP_DEPTH = 1023

_VALID = {STOP, VOID, BOOL, BYTE, DOUBLE, I16, I32, I64, STRING, STRUCT, MAP, SET, LIST, UTF8, UTF16}
_TYPE_SIZE = {BOOL: 1, BYTE: 1, I16: 2, I32: 4, I64: 8, DOUBLE: 8}  # typeSize > 0

Rec = namedtuple("Rec", "start end type status step aux")


class ReadError(Exception):
    """anything the reference wraps as meta.ErrRead"""


class TypeError_(Exception):
    """meta.ErrDismatchType; arg = the map's key type"""


class NotFound(Exception):
    """errNotFound with what the search returns: (type, start, read position)"""


class Proto:
    """thrift.BinaryProtocol over one buffer: Buf and Read."""

    def __init__(self, buf: bytes):
        self.buf = buf
        self.read = 0

    # binary.go:2033-2045 / binary_skip.go:59-77
    def next(self, n: int) -> bytes:
        d = self.read + n
        if d > len(self.buf):
            raise ReadError("EOF")
        r = self.buf[self.read:d]
        self.read = d
        return r

    skipn = next

    def read_byte(self) -> int:
        return self.next(1)[0]

    def read_i16(self) -> int:
        return struct.unpack(">h", self.next(2))[0]

    def read_i32(self) -> int:
        return struct.unpack(">i", self.next(4))[0]

    def read_i64(self) -> int:
        return struct.unpack(">q", self.next(8))[0]

    def read_field_begin(self):  # binary.go:562-577
        t = self.read_byte()
        if t not in _VALID:
            raise ReadError("invalid data type")
        i = 0
        if t != STOP:
            i = self.read_i16()
        return t, i

    def read_map_begin(self):  # binary.go:585-617
        k = self.read_byte()
        if k not in _VALID:
            raise ReadError("invalid data type")
        v = self.read_byte()
        if v not in _VALID:
            raise ReadError("invalid data type")
        size = self.read_i32()
        if size < 0:
            raise ReadError("invalid data size")
        return k, v, size

    def read_list_begin(self):  # binary.go:625-649
        e = self.read_byte()
        if e not in _VALID:
            raise ReadError("invalid data type")
        size = self.read_i32()
        if size < 0:
            raise ReadError("invalid data size")
        return e, size

    def read_string(self) -> bytes:  # binary.go:767-791
        size = self.read_i32()
        if size < 0 or size > len(self.buf) - self.read:
            raise ReadError("invalid data size")
        r = self.buf[self.read:self.read + size]
        self.read += size
        return r

    def read_int(self, t: int) -> int:  # binary.go:737-754: a byte comes back unsigned
        if t == BYTE:
            return self.read_byte()
        if t == I16:
            return self.read_i16()
        if t == I32:
            return self.read_i32()
        if t == I64:
            return self.read_i64()
        raise ReadError("invalid data type")

    def skipstr(self):  # binary_skip.go:80-95: the size as uint32 in a 64-bit int
        readn = self.read + 4
        if readn > len(self.buf):
            raise ReadError("EOF")
        readn += struct.unpack(">I", self.buf[self.read:self.read + 4])[0]
        if readn > len(self.buf):
            raise ReadError("EOF")
        self.read = readn

    def skip_type(self, t: int):
        self._skip(t, MAX_SKIP_DEPTH)

    def _skip(self, t: int, depth: int):  # binary_skip.go:109-204
        """The struct case loops instead of recursing per nested struct field
        (same reads, same depth arithmetic), so 1023 levels fit Python's stack."""
        if depth <= 0:
            raise ReadError("exceed depth limit")
        n = _TYPE_SIZE.get(t, 0)
        if n > 0:
            return self.skipn(n)
        if t == STRING:
            return self.skipstr()
        if t == STRUCT:
            open_ = 1  # structs open on this chain, each one level deeper
            while open_:
                tp = self.next(1)[0]
                if tp == STOP:
                    open_ -= 1
                    continue
                self.skipn(2)
                n = _TYPE_SIZE.get(tp, 0)
                if n > 0:
                    self.skipn(n)
                elif tp == STRUCT:  # skipType(STRUCT, depth - open_)
                    if depth - open_ <= 0:
                        raise ReadError("exceed depth limit")
                    open_ += 1
                else:
                    self._skip(tp, depth - open_)
            return
        if t == MAP:
            b = self.next(6)
            kt, vt, sz = b[0], b[1], struct.unpack(">i", b[2:])[0]
            if sz < 0:
                raise ReadError("invalid data size")
            ksz, vsz = _TYPE_SIZE.get(kt, 0), _TYPE_SIZE.get(vt, 0)
            if ksz > 0 and vsz > 0:
                return self.skipn(sz * (ksz + vsz))
            for _ in range(sz):
                for et, esz in ((kt, ksz), (vt, vsz)):
                    if esz > 0:
                        self.skipn(esz)
                    elif et == STRING:
                        self.skipstr()
                    else:
                        self._skip(et, depth - 1)
            return
        if t in (SET, LIST):
            b = self.next(5)
            vt, sz = b[0], struct.unpack(">i", b[1:])[0]
            if sz < 0:
                raise ReadError("invalid data size")
            vsz = _TYPE_SIZE.get(vt, 0)
            if vsz > 0:
                return self.skipn(sz * vsz)
            for _ in range(sz):
                if vt == STRING:
                    self.skipstr()
                else:
                    self._skip(vt, depth - 1)
            return
        raise ReadError("invalid data size")


def search_field_id(p: Proto, fid: int):  # node.go:292-314
    while True:
        t, i = p.read_field_begin()
        if t == STOP:
            raise NotFound(STRUCT, 0, p.read)
        if fid == i:
            return t, p.read
        p.skip_type(t)


def search_index(p: Proto, idx: int, is_list: bool):  # node.go:316-338
    et, size = p.read_list_begin()
    if idx >= size:
        raise NotFound(LIST if is_list else SET, p.read, p.read)
    for _ in range(idx):
        p.skip_type(et)
    return et, p.read


def search_str_key(p: Proto, key: bytes):  # node.go:340-369
    kt, et, size = p.read_map_begin()
    if kt != STRING:
        raise TypeError_(kt)
    start = p.read
    for _ in range(size):
        if p.read_string() == key:
            return et, p.read
        p.skip_type(et)
    raise NotFound(MAP, start, p.read)


def search_bin_key(p: Proto, key: bytes):  # node.go:371-398
    kt, et, size = p.read_map_begin()
    start = p.read
    for _ in range(size):
        ks = p.read
        p.skip_type(kt)
        if p.buf[ks:p.read] == key:
            return et, p.read
        p.skip_type(et)
    raise NotFound(MAP, start, p.read)


def search_int_key(p: Proto, key: int):  # node.go:400-429
    kt, et, size = p.read_map_begin()
    start = p.read
    if kt not in (BYTE, I16, I32, I64):
        raise TypeError_(kt)
    for _ in range(size):
        if p.read_int(kt) == key:
            return et, p.read
        p.skip_type(et)
    raise NotFound(MAP, start, p.read)


def get_by_path(buf: bytes, path, root_type: int = STRUCT) -> Rec:
    """path: a sequence of (kind, value) steps, value an int (FIELD, INDEX,
    INTKEY) or bytes (STRKEY, BINKEY). Value.GetByPath, value.go:102-161, with
    the wire type standing in for the descriptor's."""
    p = Proto(buf)
    start, tt = 0, root_type
    is_list = tt == LIST
    for s, (kind, val) in enumerate(path):
        try:
            if kind == FIELD:
                tt, start = search_field_id(p, val)
                is_list = tt == LIST
            elif kind == INDEX:
                tt, start = search_index(p, val, is_list)
            elif kind == STRKEY:
                tt, start = search_str_key(p, val)
            elif kind == INTKEY:
                tt, start = search_int_key(p, val)
            elif kind == BINKEY:
                tt, start = search_bin_key(p, val)
            else:
                raise ValueError(kind)
        except ReadError:
            return Rec(0, 0, 0, E_READ, s, 0)
        except TypeError_ as e:
            return Rec(0, 0, 0, E_TYPE, s, e.args[0])
        except NotFound as e:
            t, st, rd = e.args
            return Rec(st, st, t, NOT_FOUND, s, rd)
    try:
        p.skip_type(tt)
    except ReadError:
        return Rec(0, 0, 0, E_READ, len(path), 0)
    return Rec(start, p.read, tt, OK, len(path), 0)


def raw(buf: bytes, r: Rec) -> bytes:
    return buf[r.start:r.end] if r.status == OK else b""
