"""The checker of typed column writes (include/dgj2t.h dg_vals_*): a plain
restatement of the semantics, value by value, that shares no code with the
kernels. encode() is one value as BinaryEncoding writes it; encode_batch() is a
whole batch from inputs in the shapes the entries take (numpy arrays: val, len,
src, elem_off, elems, present) into the message-major arena."""
import struct

BOOL, I08, DOUBLE, I16, I32, I64, STRING = 2, 3, 4, 6, 8, 10, 11
LIST, SET = 0x40, 0x80
T_SET, T_LIST = 14, 15
OK, E_SIZE = 0, 1
WIDTH = {BOOL: 1, I08: 1, DOUBLE: 8, I16: 2, I32: 4, I64: 8}
MAX_COLS = 16
M64 = (1 << 64) - 1


def kind_ok(kind: int) -> bool:
    if kind & (LIST | SET):
        return kind & (LIST | SET) != (LIST | SET) and (kind & 0x3F) in WIDTH
    return kind == STRING or kind in WIDTH


def wire_type(kind: int) -> int:
    return T_LIST if kind & LIST else T_SET if kind & SET else kind


def bits(v) -> int:
    """a cell's 64-bit input: an int taken mod 2^64, a float as its bits"""
    if isinstance(v, float):
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    return int(v) & M64


def scalar(t: int, v) -> bytes:
    """EncodeBool / EncodeByte / EncodeInt16 / 32 / 64 / EncodeDouble of the 64-bit input v"""
    v = bits(v)
    if t == BOOL:
        return b"\x01" if v else b"\x00"
    w = WIDTH[t]
    return (v & ((1 << 8 * w) - 1)).to_bytes(w, "big")


def item_size(kind: int, cnt: int, fh: int = 0, stop: int = 0):
    """(bytes of the item, status, cnt as written) of a present cell: cnt = a string's length or a container's count"""
    if kind in WIDTH:
        return fh + WIDTH[kind] + stop, OK, 0
    hdr, w = (fh + 4, 1) if kind == STRING else (fh + 5, WIDTH[kind & 0x3F])
    if cnt > 2 ** 31 - 1 or hdr + cnt * w + stop >= 2 ** 32:
        return hdr + stop, E_SIZE, 0
    return hdr + cnt * w + stop, OK, cnt


def encode(kind: int, v) -> bytes:
    """one value: a scalar's input, a string's bytes, a container's inputs"""
    if kind in WIDTH:
        return scalar(kind, v)
    if kind == STRING:
        v = bytes(v)
        return struct.pack(">i", len(v)) + v
    et = kind & 0x3F
    return bytes([et]) + struct.pack(">i", len(v)) + b"".join(scalar(et, e) for e in v)


def field_begin(kind: int, fid: int) -> bytes:
    return bytes([wire_type(kind)]) + struct.pack(">h", fid)


def encode_cell(kind: int, col, i: int):
    """(value bytes, status) of row i of a column given by its arrays"""
    if kind in WIDTH:
        return scalar(kind, int(col["val"][i])), OK
    if kind == STRING:
        ln = int(col["len"][i])
        if item_size(kind, ln)[1] != OK:
            return b"\0\0\0\0", E_SIZE
        at = int(col["val"][i])
        return struct.pack(">i", ln) + col["src"][at:at + ln].tobytes(), OK
    a, b = int(col["elem_off"][i]), int(col["elem_off"][i + 1])
    cnt = (b - a) & M64
    return encode_cell_list(kind, col, a, cnt)


def encode_cell_list(kind, col, a, cnt, fh=0, stop=0):
    et = kind & 0x3F
    if item_size(kind, cnt, fh, stop)[1] != OK:
        return bytes([et, 0, 0, 0, 0]), E_SIZE
    e = col["elems"][a:a + cnt]
    w = WIDTH[et]
    if et == BOOL:
        body = (e != 0).astype("u1").tobytes()
    else:
        body = e.astype(">u8").view("u1").reshape(-1, 8)[:, 8 - w:].tobytes()
    return bytes([et]) + struct.pack(">i", cnt) + body, OK


def encode_batch(kinds, cols, n: int, field_ids=None, out_base: int = 0):
    """(arena from out_base on, off[n * K + 1], status[n * K]): item j of message i at arena[off[i*K+j] - out_base ...]"""
    K = len(kinds)
    assert 1 <= K <= MAX_COLS and all(kind_ok(k) for k in kinds)
    fh = 3 if field_ids is not None else 0
    out, off, status = [], [out_base], []
    pos = out_base
    for i in range(n):
        for j, (kind, col) in enumerate(zip(kinds, cols)):
            stop = 1 if fh and j == K - 1 else 0
            pres = col.get("present")
            assert pres is None or fh
            item, st = b"", OK
            if pres is None or pres[i]:
                if kind & (LIST | SET):
                    a, b = int(col["elem_off"][i]), int(col["elem_off"][i + 1])
                    val, st = encode_cell_list(kind, col, a, (b - a) & M64, fh, stop)
                else:
                    val, st = encode_cell(kind, col, i)
                item = (field_begin(kind, field_ids[j]) if fh else b"") + val
            if stop:
                item += b"\0"
            out.append(item)
            status.append(st)
            pos += len(item)
            off.append(pos)
    return b"".join(out), off, status
