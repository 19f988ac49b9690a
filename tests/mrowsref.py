"""The yardstick of the map-row tests. It restates nothing: the head and the
rows are kidsref.children (one level) on the MAP node behind
tgetref.get_by_path; a row's key comes from the kid's `key` / `key_start`, its
index entry is the kid's value span; a cell is colsref.cell (tgetref.get_by_path
and the cast) on the value's own bytes with the map's value type as the root
type. Its only own lines are the key-kind test and the order of the head's
steps (include/dgj2t.h, map plans). It returns what the device returns; the
device is never compared with itself."""
from collections import namedtuple

import colsref as CR
import kidsref as K
import tgetref as R
from rowsref import Head, Row

E_UNSUPPORTED = CR.E_UNSUPPORTED
KEY_STR, KEY_INT = 1, 2  # DG_ROWS_KEY_*
KEY_TYPES = {KEY_STR: (R.STRING,), KEY_INT: K.INTS}

Key = namedtuple("Key", "val len")  # d_key, d_key_len
Msg = namedtuple("Msg", "head rows keys cells")  # cells[j][k]: the checker's Cell of entry j under column k


def head_rows(buf: bytes, parent, key_kind: int, root_type: int = R.STRUCT, base: int = 0, msg: int = 0):
    """(Head, [Row], [Key], [the values' bytes]) of v.GetByPath(parent...) followed by Children(recurse = false) on a
    MAP node; base = the message's offset in the arena"""
    n = len(parent)
    t, start = root_type, 0
    if n:
        r = R.get_by_path(buf, parent, root_type)  # 1: the lookup with its final skip
        if r.status != R.OK:
            return Head(0, 0, r.status, 0, 0, r.step), [], [], []
        t, start = r.type, r.start
    if t != R.MAP:  # 2
        return Head(0, 0, E_UNSUPPORTED, t, 0, n), [], [], []
    try:  # 3: ReadMapBegin
        kt, _, _ = R.Proto(buf[start:]).read_map_begin()
    except R.ReadError:
        return Head(0, 0, R.E_READ, 0, 0, n), [], [], []
    if kt not in KEY_TYPES[key_kind]:  # 4: the key kind, at any size
        return Head(0, 0, E_UNSUPPORTED, R.MAP, kt, n), [], [], []
    h, kids = K.children(buf, parent, False, root_type)  # 5
    if h.status != R.OK:
        return Head(0, 0, h.status, 0, 0, n), [], [], []
    assert h.count == h.direct == len(kids) and h.start == start and h.key_type == kt
    keys = []
    for k in kids:
        if k.kind == R.STRKEY:
            keys.append(Key(base + k.key_start + 4, k.key))
        else:
            assert k.kind == R.INTKEY
            keys.append(Key(k.key % 2 ** 64, k.start - k.key_start))
    return (Head(base + h.start + 6, h.direct, R.OK, h.type, h.elem_type, n),
            [Row(base + k.start, k.end - k.start, msg) for k in kids], keys, [buf[k.start:k.end] for k in kids])


def message(buf: bytes, parent, columns, key_kind: int, root_type: int = R.STRUCT, base: int = 0, msg: int = 0) -> Msg:
    """columns: [(sub_path, kind)]"""
    h, rows, keys, vals = head_rows(buf, parent, key_kind, root_type, base, msg)
    cells = [[CR.cell(v, p, k, h.elem_type, r.off) for p, k in columns] for v, r in zip(vals, rows)]
    return Msg(h, rows, keys, cells)


def batch(msgs, parent, columns, key_kind: int, root_type: int = R.STRUCT, first: int = 0):
    """[Msg] over a batch laid out back to back from arena offset `first`"""
    out, base = [], first
    for i, m in enumerate(msgs):
        out.append(message(m, parent, columns, key_kind, root_type, base, i))
        base += len(m)
    return out
