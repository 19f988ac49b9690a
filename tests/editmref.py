"""The yardstick of the many-edit tests: a pure-Python restatement of the
reference's SetMany + setNotFound + replaceMany (thrift/generic/node.go:930-1007)
and of its UNSET counterpart, on tgetref's Proto and GetByPath, written as the Go
reads: look every item up below the parent, give each missing one a not-found
node at the front of the container, sort by where they stand, copy the buffer
once around them. Where the project deviates from the reference on purpose
(include/dgj2t.h, deviations 1-7 of dg_edit and 8-10 of dg_editm) the line is
marked `# deviation N`. It returns what the device returns: (ret word, output
bytes). The device is never compared with itself.

An item is (step, value, val_type), step a (kind, value) pair like tgetref's;
for UNSET value and val_type are ignored."""
import struct

import editref as E
import tgetref as T
from editref import (BINKEY, E_OVERFLOW, E_READ, E_TYPE, FIELD, INDEX, INTKEY, NOT_FOUND, OK, SET_OP,  # noqa: F401
                     STRKEY, UNSET_OP)
from tgetref import LIST, MAP, SET, STRUCT

E_SAME = 5
MAX_ITEMS = 7


def word(status, aux=0, mask=0, item=0):
    return status | mask << 8 | item << 16 | (aux & 0xFFFFFFFF) << 32


def overflow(need):
    return word(E_OVERFLOW, min(need, 0xFFFFFFFF))


def status_of(ret):
    return ret & 0xFF


def existed_of(ret, k):
    return tuple(bool(ret >> (8 + j) & 1) for j in range(k))


def item_of(ret):
    return ret >> 16 & 7


def step_class(kind):
    return 0 if kind == FIELD else 1 if kind == INDEX else 2


def check_items(items):
    """what dg_editm_create refuses"""
    if not 1 <= len(items) <= MAX_ITEMS:
        raise ValueError("%d items" % len(items))
    if len({step_class(it[0][0]) for it in items}) != 1:
        raise ValueError("mixed step classes")  # deviation 10: the Go takes them and fails per item, or not at all


class _Fail(Exception):
    def __init__(self, ret):
        self.ret = ret


def _fail(rec):
    """a lookup that failed, as the edit returns it: (status, aux)"""
    raise _Fail((rec.status, 0 if rec.status == NOT_FOUND else rec.aux))


def _set_item(buf, parent, step, value, t, root_type):
    """one item of SetMany: (start, end, new bytes, existed, count position or None). getMany finds it, or it
    gets errNotFoundLast at the container's front and setNotFound builds key + value"""
    path = list(parent) + [step]
    v = T.get_by_path(buf, path, root_type)
    if v.status == OK:
        if v.type != t:  # deviation 8: replaceMany copies the new bytes over whatever type stood there
            raise _Fail((E_TYPE, v.type))
        return v.start, v.end, value, True, None
    if not (v.status == NOT_FOUND and v.step == len(path) - 1):
        _fail(v)
    kind, kval = step
    if v.type == STRUCT:
        par = T.get_by_path(buf, parent, root_type)  # deviation 1 (SetMany itself: sp = self.v, the struct searched)
        if par.status != OK:
            _fail(par)
        return par.start, par.start, E.to_raw(FIELD, kval, t) + value, False, None
    if v.type in (LIST, SET):
        if buf[v.start - 5] != t:  # deviation 3
            raise _Fail((E_TYPE, buf[v.start - 5]))
        return v.start, v.start, value, False, v.start - 4
    if v.type == MAP:
        kt, vt = buf[v.start - 6], buf[v.start - 5]
        if vt != t:  # deviation 3
            raise _Fail((E_TYPE, vt))
        return v.start, v.start, E.to_raw(kind, kval, kt) + value, False, v.start - 4  # deviation 2
    raise AssertionError("errNotFound of type %d" % v.type)


def _unset_item(buf, parent, par, step, root_type):
    """one item of the UNSET counterpart: deleteChild on the ORIGINAL message"""
    ret, cut = E.delete_child(buf, par, step, root_type, list(parent) + [step])  # deviations 4, 5, 6
    if cut is None:
        raise _Fail((ret & 0xFF, ret >> 32))
    s, e, patch = cut
    return s, e, b"", True, None if patch is None else patch[0]


def edit_many(op, buf, parent, items, root_type=STRUCT, cap=None):
    """(ret, out) as dg_editm_batch_device leaves them, for a slot of cap bytes (None: large enough)"""
    check_items(items)
    par = None
    if op == UNSET_OP:
        par = T.get_by_path(buf, parent, root_type)
        if par.status == NOT_FOUND:  # UnsetByPath returns nil: nothing to unset
            return _fit(word(OK), buf, cap)
        if par.status != OK:
            return word(par.status, par.aux), b""
    cuts = []
    for j, (step, value, t) in enumerate(items):
        try:
            c = _set_item(buf, parent, step, value, t, root_type) if op == SET_OP else \
                _unset_item(buf, parent, par, step, root_type)
        except _Fail as f:  # the first failing item in item order; the message is edited as a whole or not at all
            return word(f.ret[0], f.ret[1], item=j), b""
        cuts.append(c + (j,))
    # ps.Sort(): by where the old value stands; the not-found nodes, which all stand at the container's
    # front and are empty, stay in the order the items were given, in front of a value that starts there
    cuts.sort(key=lambda c: (c[0], c[1] > c[0], c[5]))
    for a, b in zip(cuts, cuts[1:]):
        if a[1] > b[0]:  # deviation 9: the Go copies a negative-length or doubled slice
            return word(E_SAME, item=b[5]), b""
    mask = sum(1 << c[5] for c in cuts if c[3])
    patched = [c for c in cuts if c[4] is not None]
    if patched:  # setNotFound adds 1 per missing item to the same four bytes; deleteChild subtracts 1 per drop
        at = patched[0][4]
        assert all(c[4] == at for c in patched) and at + 4 <= cuts[0][0]
        size = struct.unpack(">i", buf[at:at + 4])[0]
        size += len(patched) if op == SET_OP else -len(patched)
        buf = buf[:at] + struct.pack(">I", size & 0xFFFFFFFF) + buf[at + 4:]
    out, offset = [], 0
    for s, e, pat, _, _, _ in cuts:  # replaceMany (node.go:930-958)
        out.append(buf[offset:s])
        out.append(pat)
        offset = e
    out.append(buf[offset:])
    return _fit(word(OK, mask=mask), b"".join(out), cap)


def _fit(ret, out, cap):
    if cap is not None and len(out) > cap:
        return overflow(len(out)), b""
    return ret, out


def out_len(ret, out):
    return ret >> 32 if status_of(ret) == E_OVERFLOW else len(out)


def slot_bound(op, items, length):
    """the longest output the many-edit can produce for a message of `length` bytes (items carry their values)"""
    if op == UNSET_OP:
        return length
    return length + sum(E.slot_bound(SET_OP, [it[0]], 0, len(it[1])) for it in items)


def chained(op, buf, parent, items, root_type=STRUCT):
    """the same edit as single edits of editref, in the order that gives SetMany's result when no item fails
    or overlaps another: SET the found items first, then the missing ones in reverse item order (each goes to
    the front); UNSET descending by where the item starts. Returns (ok, out): ok False when a step failed, None
    when the chain cannot say the same thing: a missing index that a previous insert of the chain brings into
    the list (the chain would then replace what it has just inserted, where SetMany inserts twice)."""
    path = lambda it: list(parent) + [it[0]]  # noqa: E731
    if op == SET_OP:
        # the found ones from the back of the message, so that a value of another length than the one it
        # replaces (values are taken as given) does not move an item the chain has yet to look up
        found = sorted((it for it in items if T.get_by_path(buf, path(it), root_type).status == OK),
                       key=lambda it: -T.get_by_path(buf, path(it), root_type).start)
        missing = [it for it in items if T.get_by_path(buf, path(it), root_type).status != OK]
        order = found + missing[::-1]
        v = T.get_by_path(buf, path(missing[0]), root_type) if missing else None
        if missing and v.status == NOT_FOUND and v.type in (LIST, SET):
            size = struct.unpack(">i", buf[v.start - 4:v.start])[0]
            # ... or a count that wraps below zero on the way, which the chain's next lookup refuses to read
            if any(it[0][1] < size + len(missing) for it in missing) or size + len(missing) > 0x7FFFFFFF:
                return None, b""
    else:
        order = sorted(items, key=lambda it: -T.get_by_path(buf, path(it), root_type).start)
    for it in order:
        ret, buf = E.edit(op, buf, path(it), it[1], it[2], root_type)
        if ret & 0xFF != OK:
            return False, b""
    return True, buf


def outcome(op, ret, k):
    """the classes the fuzz shares count"""
    st = status_of(ret)
    if st != OK:
        return {NOT_FOUND: "ErrNotFound", E_READ: "ErrRead", E_TYPE: "ErrDismatchType", E_SAME: "ErrSame",
                E_OVERFLOW: "ErrOverflow"}[st]
    n = sum(existed_of(ret, k))
    if op == UNSET_OP:
        return "dropped" if n else "untouched"
    return "all replaced" if n == k else "all inserted" if n == 0 else "mixed"
