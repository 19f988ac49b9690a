"""The checker of row column writes (include/dgj2t.h dg_rvals_*): a plain
restatement of the semantics, value by value with struct.pack, that shares no
code with the kernels; a cell's value alone is valsref's. encode_batch() is a
whole batch from inputs in the shapes the entries take (row_off and, per
column, numpy arrays indexed by row: val, len, src, elem_off, elems, present)
into the message-major arena of one item per message.

A message's item is 0C, the i32 big-endian count and its rows. A row is every
present column in column order, each as the 3-byte field header (wire type, id
big-endian) and the value, then 00. The message's status: RANGE (row_off[i] >
row_off[i + 1] or row_off[i + 1] > n_rows) is tested first, then SIZE (more than
2^31 - 1 rows, or an item of 2^32 bytes or more); either writes 0C 00 00 00 00.
A cell's status is vals' SIZE rule (item_size with the field header and the
STOP); the flagged cell is the empty value, its row and message stay OK. Row
ranges may overlap or leave gaps: every message writes its own range."""
import struct

import valsref as VR

T_STRUCT = 12
OK, E_SIZE, E_RANGE = 0, 1, 2
HDR = 5
ALL_KINDS = [k for k in range(0x100) if VR.kind_ok(k)]  # 19
assert len(ALL_KINDS) == 19


def plan_ok(kinds, field_ids, container) -> bool:
    return (container in (VR.T_LIST, VR.T_SET) and 1 <= len(kinds) <= VR.MAX_COLS and field_ids is not None
            and len(field_ids) == len(kinds) and all(VR.kind_ok(k) for k in kinds))


def list_header(count: int) -> bytes:
    return bytes([T_STRUCT]) + struct.pack(">i", count)


def cell_count(kind, col, g):
    """a present cell's string length or element count, as the inputs give it"""
    if kind == VR.STRING:
        return int(col["len"][g])
    if kind & (VR.LIST | VR.SET):
        return (int(col["elem_off"][g + 1]) - int(col["elem_off"][g])) & VR.M64
    return 0


def cell_size(kind, col, g, stop):
    """(bytes, status) of cell (g, this column) without touching a payload"""
    pres = col.get("present")
    if pres is not None and not pres[g]:
        return stop, OK
    size, st, _ = VR.item_size(kind, cell_count(kind, col, g), 3, stop)
    return size, st


def encode_cell(kind, fid, col, g, stop):
    """(item bytes, status) of cell (g, this column): field header, value, STOP behind a row's last column"""
    pres = col.get("present")
    item, st = b"", OK
    if pres is None or pres[g]:
        if kind & (VR.LIST | VR.SET):
            val, st = VR.encode_cell_list(kind, col, int(col["elem_off"][g]), cell_count(kind, col, g), 3, stop)
        elif kind == VR.STRING and VR.item_size(kind, int(col["len"][g]), 3, stop)[1] != OK:
            val, st = b"\0\0\0\0", E_SIZE
        else:
            val, st = VR.encode_cell(kind, col, g)
        item = VR.field_begin(kind, fid) + val
    return item + (b"\0" if stop else b""), st


def row_sizes(kinds, cols, n_rows):
    """the encoded bytes of every row, from the lengths alone"""
    K = len(kinds)
    return [sum(cell_size(kinds[j], cols[j], g, int(j == K - 1))[0] for j in range(K)) for g in range(n_rows)]


def message_status(a, b, n_rows, sizes=None, prefix=None):
    """RANGE first, then the count, then the item's bytes (prefix: the running sums of the rows' sizes)"""
    if a > b or b > n_rows:
        return E_RANGE
    if b - a > 2 ** 31 - 1:
        return E_SIZE
    if HDR + (prefix[b] - prefix[a]) >= 2 ** 32:
        return E_SIZE
    return OK


def statuses_only(kinds, row_off, n, n_rows, stride):
    """(off, status) of a batch whose rows all take `stride` bytes (a plan of scalars, every field present), from the
    offsets alone: what a sizing call answers without reading a per-row array"""
    off, status = [0], []
    for i in range(n):
        a, b = int(row_off[i]), int(row_off[i + 1])
        st = E_RANGE if a > b or b > n_rows else E_SIZE if b - a > 2 ** 31 - 1 or HDR + (b - a) * stride >= 2 ** 32 else OK
        status.append(st)
        off.append(off[-1] + HDR + ((b - a) * stride if st == OK else 0))
    return off, status


def encode_batch(kinds, field_ids, cols, row_off, n, n_rows, out_base=0):
    """(arena from out_base on, off[n + 1], status[n], cell_status[n_rows * K])"""
    K = len(kinds)
    assert plan_ok(kinds, field_ids, VR.T_LIST)
    cell_status = [cell_size(kinds[j], cols[j], g, int(j == K - 1))[1] for g in range(n_rows) for j in range(K)]
    prefix = [0]
    for size in row_sizes(kinds, cols, n_rows):
        prefix.append(prefix[-1] + size)
    rows = {}

    def row(g):
        """row g's bytes; only a row that an OK message owns is encoded, so only its payloads are looked at"""
        if g not in rows:
            items = [encode_cell(kinds[j], field_ids[j], cols[j], g, int(j == K - 1)) for j in range(K)]
            assert [st for _, st in items] == cell_status[g * K:(g + 1) * K]
            rows[g] = b"".join(item for item, _ in items)
            assert len(rows[g]) == prefix[g + 1] - prefix[g]
        return rows[g]

    out, off, status = [], [out_base], []
    for i in range(n):
        a, b = int(row_off[i]), int(row_off[i + 1])
        st = message_status(a, b, n_rows, prefix=prefix)
        item = list_header(b - a) + b"".join(row(g) for g in range(a, b)) if st == OK else list_header(0)
        out.append(item)
        status.append(st)
        off.append(off[-1] + len(item))
    return b"".join(out), off, status, cell_status
