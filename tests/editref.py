"""The yardstick of the edit tests: a pure-Python restatement of the
reference's SetByPath + setNotFound + replace (thrift/generic/value.go:263-299,
node.go:825-920) and UnsetByPath + deleteChild (value.go:302-333,
node.go:1009-1127) on top of tgetref's Proto and GetByPath, written as the Go
reads: search, build the new node's bytes, cut the buffer in three. Where the
project deviates from the reference on purpose (include/dgj2t.h, "Deviations"),
the line is marked `# deviation N` and says what the Go does instead. It
returns what the device returns: (ret word, output bytes). The device is never
compared with itself."""
import struct

import tgetref as T
from tgetref import BYTE, I16, I32, I64, LIST, MAP, SET, STRING, STRUCT  # noqa: F401

SET_OP, UNSET_OP = 1, 2
OK, NOT_FOUND, E_READ, E_TYPE, E_OVERFLOW = 0, 1, 2, 3, 0xF0
EXISTED = 1 << 8
FIELD, INDEX, STRKEY, INTKEY, BINKEY = T.FIELD, T.INDEX, T.STRKEY, T.INTKEY, T.BINKEY
_INT_FMT = {BYTE: ">b", I16: ">h", I32: ">i", I64: ">q"}


def word(status, aux=0, existed=False):
    return status | (EXISTED if existed else 0) | (aux & 0xFFFFFFFF) << 32


def overflow(need):
    return word(E_OVERFLOW, min(need, 0xFFFFFFFF))


def _err(rec):
    """a lookup that failed, as the edit returns it (the Go returns the error node)"""
    return word(rec.status, 0 if rec.status == NOT_FOUND else rec.aux), b""


def _i32(x):
    """int32(x) as Go converts: wraps"""
    return struct.pack(">I", x & 0xFFFFFFFF)


def to_raw(kind, val, t):
    """Path.ToRaw(t) (path.go): the key as it stands in a message"""
    if kind == FIELD:
        return struct.pack(">Bh", t, val)
    if kind == STRKEY:
        return struct.pack(">i", len(val)) + val
    if kind == BINKEY:
        return val
    if kind == INTKEY:
        w = {BYTE: 1, I16: 2, I32: 4, I64: 8}[t]
        return (val & ((1 << (8 * w)) - 1)).to_bytes(w, "big")
    raise ValueError(kind)


def replace(buf, start, end, pat):  # node.go:825-855: three slices into a new buffer
    return buf[:start] + pat + buf[end:]


def set_by_path(buf, path, value, val_type, root_type=STRUCT):
    """SetByPath (node.go:895-920). path: (kind, value) steps, at least one."""
    assert len(path) >= 1  # deviation 7: the empty path is refused before any message is read
    v = T.get_by_path(buf, path, root_type)
    if v.status == OK:
        if v.type != val_type:  # replace: o.t != n.t
            return word(E_TYPE, v.type), b""
        return word(OK, existed=True), replace(buf, v.start, v.end, value)
    if not (v.status == NOT_FOUND and v.step == len(path) - 1):  # !isErrNotFoundLast
        return _err(v)
    kind, kval = path[-1]
    # setNotFound (node.go:857-892): by the container the search ended in
    if v.type == STRUCT:
        # deviation 1: the Go's errNotFoundLast node has start 0 (searchFieldId
        # returns 0 on a miss), so it inserts at byte 0 of the ROOT message;
        # here the front of the struct that was searched: the parent's start
        par = T.get_by_path(buf, path[:-1], root_type)
        if par.status != OK:
            return _err(par)
        return word(OK), replace(buf, par.start, par.start, to_raw(FIELD, kval, val_type) + value)
    if v.type in (LIST, SET):
        if buf[v.start - 5] != val_type:  # deviation 3: the Go does not look at the element type
            return word(E_TYPE, buf[v.start - 5]), b""
        size = struct.unpack(">i", buf[v.start - 4:v.start])[0]
        buf = buf[:v.start - 4] + _i32(size + 1) + buf[v.start:]
        return word(OK), replace(buf, v.start, v.start, value)
    if v.type == MAP:
        kt, vt = buf[v.start - 6], buf[v.start - 5]
        if vt != val_type:  # deviation 3
            return word(E_TYPE, vt), b""
        size = struct.unpack(">i", buf[v.start - 4:v.start])[0]
        buf = buf[:v.start - 4] + _i32(size + 1) + buf[v.start:]
        key = to_raw(kind, kval, kt)  # deviation 2: the Go encodes with ToRaw(n.t), the value's type
        return word(OK), replace(buf, v.start, v.start, key + value)
    raise AssertionError("errNotFound of type %d" % v.type)


def delete_child(buf, par, step, root_type, path):
    """deleteChild (node.go:1009-1103) on the parent's span: (ret, s, e, count patch or None)"""
    kind, kval = step
    if par.type == STRUCT:
        if kind != FIELD:
            return word(E_TYPE, par.type), None
    elif par.type in (LIST, SET):
        if kind != INDEX:
            return word(E_TYPE, par.type), None
    elif par.type == MAP:
        if kind not in (STRKEY, INTKEY, BINKEY):  # the Go: ToRaw gives nil, ErrInvalidParam
            return word(E_TYPE, par.type), None
    else:
        return word(E_TYPE, par.type), None  # deviation 6: the Go falls through its switch and replaces nothing
    # deviation 5: the child is found as the lookup finds it (its key compares), not by a raw compare
    v = T.get_by_path(buf, path, root_type)
    if v.status != OK:
        return _err(v)[0], None  # deviation 4: an absent map key deletes the LAST entry in the Go
    if par.type == STRUCT:
        return 0, (v.start - 3, v.end, None)
    if par.type in (LIST, SET):
        size = struct.unpack(">i", buf[par.start + 1:par.start + 5])[0]
        return 0, (v.start, v.end, (par.start + 1, _i32(size - 1)))  # ModifyI32(p.Read - 4, int32(size - 1))
    kt = buf[par.start]
    size = struct.unpack(">i", buf[par.start + 2:par.start + 6])[0]
    klen = len(to_raw(kind, kval, kt))
    return 0, (v.start - klen, v.end, (par.start + 2, _i32(size - 1)))


def unset_by_path(buf, path, root_type=STRUCT):
    """UnsetByPath (node.go:1105-1127)."""
    assert len(path) >= 1  # deviation 7
    par = T.get_by_path(buf, path[:-1], root_type)
    if par.status != OK:
        if par.status == NOT_FOUND:
            return word(OK), buf  # return nil: nothing to unset
        return _err(par)
    ret, cut = delete_child(buf, par, path[-1], root_type, path)
    if cut is None:
        return ret, b""
    s, e, patch = cut
    if patch is not None:
        buf = buf[:patch[0]] + patch[1] + buf[patch[0] + 4:]
    return word(OK, existed=True), replace(buf, s, e, b"")


def edit(op, buf, path, value=b"", val_type=0, root_type=STRUCT, cap=None):
    """(ret, out) as dg_edit_batch_device leaves them, for a slot of cap bytes (None: large enough)"""
    ret, out = set_by_path(buf, path, value, val_type, root_type) if op == SET_OP else unset_by_path(buf, path, root_type)
    if ret & 0xFF == OK and cap is not None and len(out) > cap:
        return overflow(len(out)), b""
    return ret, out


def out_len(ret, out):
    """d_out_len for a result of edit()"""
    return ret >> 32 if ret & 0xFF == E_OVERFLOW else len(out)


def slot_bound(op, path, length, val_len):
    """the longest output the edit can produce for a message of `length` bytes"""
    if op == UNSET_OP:
        return length
    kind, kval = path[-1]
    extra = {FIELD: 3, INDEX: 0, STRKEY: 4 + (len(kval) if kind == STRKEY else 0),
             BINKEY: len(kval) if kind == BINKEY else 0, INTKEY: 8}[kind]
    return length + val_len + extra


def outcome(op, ret):
    """replaced / inserted / deleted / untouched / an error name: the classes the tests count"""
    st = ret & 0xFF
    if st == OK:
        if op == SET_OP:
            return "replaced" if ret & EXISTED else "inserted"
        return "deleted" if ret & EXISTED else "untouched"
    return {NOT_FOUND: "ErrNotFound", E_READ: "ErrRead", E_TYPE: "ErrDismatchType", E_OVERFLOW: "ErrOverflow"}[st]
