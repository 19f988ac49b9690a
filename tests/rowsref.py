"""The yardstick of the row-column tests. It restates nothing: the head and the
rows are kidsref.children (one level) behind tgetref.get_by_path, a cell is
colsref.cell (tgetref.get_by_path and the cast) on the child's own bytes with
the list's element type as the root type. It returns what the device returns
(include/dgj2t.h dg_rows_*); the device is never compared with itself."""
from collections import namedtuple

import colsref as CR
import kidsref as K
import tgetref as R

E_UNSUPPORTED = CR.E_UNSUPPORTED

Head = namedtuple("Head", "first count status type elem_type step")  # dg_rows_head
Row = namedtuple("Row", "off len msg")  # dg_row_ent
Msg = namedtuple("Msg", "head rows cells")  # cells[j][k]: the checker's Cell of element j under column k


def head_rows(buf: bytes, parent, root_type: int = R.STRUCT, base: int = 0, msg: int = 0):
    """(Head, [Row], [the elements' bytes]) of v.GetByPath(parent...) followed by Children(recurse = false);
    base = the message's offset in the arena"""
    n = len(parent)
    t = root_type
    if n:
        r = R.get_by_path(buf, parent, root_type)  # the lookup with its final skip
        if r.status != R.OK:
            return Head(0, 0, r.status, 0, 0, r.step), [], []
        t = r.type
    if t not in (R.LIST, R.SET):  # STRUCT and MAP parents too: Children serves those
        return Head(0, 0, E_UNSUPPORTED, t, 0, n), [], []
    h, kids = K.children(buf, parent, False, root_type)
    if h.status != R.OK:
        return Head(0, 0, h.status, 0, 0, n), [], []
    assert h.count == h.direct == len(kids)
    return (Head(base + h.start + 5, h.direct, R.OK, h.type, h.elem_type, n),
            [Row(base + k.start, k.end - k.start, msg) for k in kids], [buf[k.start:k.end] for k in kids])


def message(buf: bytes, parent, columns, root_type: int = R.STRUCT, base: int = 0, msg: int = 0) -> Msg:
    """columns: [(sub_path, kind)]"""
    h, rows, elems = head_rows(buf, parent, root_type, base, msg)
    cells = [[CR.cell(e, p, k, h.elem_type, r.off) for p, k in columns] for e, r in zip(elems, rows)]
    return Msg(h, rows, cells)


def batch(msgs, parent, columns, root_type: int = R.STRUCT, first: int = 0):
    """[Msg] over a batch laid out back to back from arena offset `first`"""
    out, base = [], first
    for i, m in enumerate(msgs):
        out.append(message(m, parent, columns, root_type, base, i))
        base += len(m)
    return out
