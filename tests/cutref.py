"""The yardstick of the cut tests: a pure-Python restatement of the reference's
Value.MarshalTo / marshalTo / handleUnsets (thrift/generic/value.go:375-552),
RequiresBitmap.CheckRequires (thrift/utils.go:110-141) and
BinaryProtocol.WriteEmpty (thrift/binary.go:483-515), written as the Go reads:
a read protocol with a position (tgetref.Proto: the Read*Begin checks and
skipType), a write buffer, recursion for nesting, errors as exceptions. It
works on the thrift.py descriptors, never on the plan blob, and returns what
the device returns per message: (ret, bytes) with ret = status | aux << 32
(include/dgj2t.h dg_cut_*). The device is never compared with itself.

What is not the reference's (the deviations dg_cut states): the same struct
object on both sides and a `to` struct against another `from` raise ValueError
here too; more than MAX_DEPTH cut containers open give E_DEPTH."""
import struct

from tgetref import LIST, MAP, SET, STOP, STRUCT, Proto, ReadError

OK, E_READ, E_TYPE, E_UNKNOWN, E_REQUIRED, E_DEPTH, E_OVERFLOW = 0, 1, 2, 3, 4, 5, 0xF0
WRITE_DEFAULT, DISALLOW_UNKNOWN, NOT_CHECK_REQ = 1, 2, 4
MAX_DEPTH = 64  # DG_CUT_MAX_DEPTH
REQUIRED = 2    # thrift.REQUIRED


class CutError(Exception):
    """(status, aux)"""


def same(a, b):
    """`to.Elem() == from.Elem()` with the reference's shared builtins: the same
    object, or two base types of equal type and name"""
    if a is b:
        return True
    base = lambda d: d.struct is None and d.key is None and d.elem is None
    return base(a) and base(b) and a.type == b.type and a.name == b.name


def write_empty(w: bytearray, d):  # binary.go:483-515
    t = d.type
    if t in (2, 3):
        w += b"\0"
    elif t == 6:
        w += b"\0\0"
    elif t == 8:
        w += b"\0\0\0\0"
    elif t in (10, 4):
        w += b"\0" * 8
    elif t == 11:
        w += struct.pack(">i", 0)
    elif t in (LIST, SET):
        w += bytes([d.elem.type]) + struct.pack(">i", 0)
    elif t == MAP:
        w += bytes([d.key.type, d.elem.type]) + struct.pack(">i", 0)
    elif t == STRUCT:
        w += b"\0"
    else:
        raise ValueError("invalid type")


def handle_unsets(req: dict, sd, w: bytearray, write_default: bool):  # value.go:545-552 over utils.go:110-141
    for fid in sorted(req):  # the bitmap's bits, ascending
        if not req[fid]:
            continue
        f = sd.field_by_id(fid)
        if f.required == REQUIRED:
            raise CutError(E_REQUIRED, fid)
        if not write_default:
            continue
        w += struct.pack(">Bh", f.type.type, fid)  # WriteFieldBegin
        write_empty(w, f.type)


def marshal_to_(r: Proto, w: bytearray, frm, to, opts: int, depth: int):  # value.go:392-543
    t = to.type
    if t == STRUCT:
        if frm is to or (frm.struct is not None and frm.struct is to.struct):
            raise ValueError("the same struct on both sides")
        if frm.struct is None:
            raise ValueError("to is a struct, from is none")
        if depth >= MAX_DEPTH:
            raise CutError(E_DEPTH, 0)
        req = None
        if not opts & NOT_CHECK_REQ:
            req = dict(to.struct.requires)  # CopyTo
        while True:
            try:
                tt, i = r.read_field_begin()
            except ReadError:
                raise CutError(E_READ, 0)
            if tt == STOP:
                if not opts & NOT_CHECK_REQ:
                    handle_unsets(req, to.struct, w, bool(opts & WRITE_DEFAULT))
                w.append(0)  # WriteStructEnd
                break
            ff = frm.struct.field_by_id(i)
            if ff is None:
                if opts & DISALLOW_UNKNOWN:
                    raise CutError(E_UNKNOWN, i)
                skip(r, tt)
                continue
            if tt != ff.type.type:
                raise CutError(E_TYPE, i)
            tf = to.struct.field_by_id(i)
            if tf is None:
                skip(r, tt)
                continue
            w += struct.pack(">Bh", tt, i)  # WriteFieldBegin
            if not opts & NOT_CHECK_REQ:
                req[tf.id] = False
            marshal_to_(r, w, ff.type, tf.type, opts, depth + 1)
        return
    if t in (LIST, SET):
        if frm.type not in (LIST, SET):
            raise CutError(E_TYPE, 0)
        if not same(to.elem, frm.elem):
            try:
                et, size = r.read_list_begin()
            except ReadError:
                raise CutError(E_READ, 0)
            w += bytes([et]) + struct.pack(">i", size)
            if size == 0:
                return
            if depth >= MAX_DEPTH:
                raise CutError(E_DEPTH, 0)
            for _ in range(size):
                marshal_to_(r, w, frm.elem, to.elem, opts, depth + 1)
            return
    elif t == MAP:
        if frm.type != MAP:
            raise CutError(E_TYPE, 0)
        if not (same(to.elem, frm.elem) and same(to.key, frm.key)):
            try:
                kt, et, size = r.read_map_begin()
            except ReadError:
                raise CutError(E_READ, 0)
            w += bytes([kt, et]) + struct.pack(">i", size)
            if size == 0:
                return
            if depth >= MAX_DEPTH:
                raise CutError(E_DEPTH, 0)
            for _ in range(size):
                marshal_to_(r, w, frm.key, to.key, opts, depth + 1)
                marshal_to_(r, w, frm.elem, to.elem, opts, depth + 1)
            return
    # skip_val
    if to.type != frm.type:
        raise CutError(E_TYPE, 0)
    e = r.read
    skip(r, to.type)
    w += r.buf[e:r.read]


def skip(r: Proto, t: int):
    try:
        r.skip_type(t)
    except ReadError:
        raise CutError(E_READ, 0)


def marshal_to(buf: bytes, frm, to, opts: int = 0):
    """(ret, out): ret = status | (aux & 0xFFFFFFFF) << 32; out is empty unless ret is 0"""
    if frm.type != to.type:
        raise CutError(E_TYPE, 0)  # MarshalTo's own check: generic.compile_cut raises ConvError for it
    r, w = Proto(bytes(buf)), bytearray()
    try:
        marshal_to_(r, w, frm, to, opts, 0)
    except CutError as e:
        st, aux = e.args
        return st | (aux & 0xFFFFFFFF) << 32, b""
    return 0, bytes(w)


def overflow(need: int) -> int:
    """the ret of a message whose slot is too small for its `need` bytes"""
    return E_OVERFLOW | need << 32
