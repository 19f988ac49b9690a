"""The checker of entry column writes (include/dgj2t.h dg_evals_*): a plain
restatement of the semantics, value by value, that shares no code with the
kernels and imports no other checker. encode() is one container from Python
objects as BinaryEncoding writes it; encode_batch() is a whole batch from
inputs in the shapes the entries take (numpy arrays: ent_off, key, key_len,
val, val_len, key_src, val_src, present, and n_ent) into the message-major
arena."""
import struct

BOOL, I08, DOUBLE, I16, I32, I64, STRING = 2, 3, 4, 6, 8, 10, 11
LIST, SET, MAP = 0x40, 0x80, 0x100
T_MAP, T_SET, T_LIST = 13, 14, 15
OK, E_SIZE, E_RANGE = 0, 1, 2
WIDTH = {BOOL: 1, I08: 1, DOUBLE: 8, I16: 2, I32: 4, I64: 8}
KEY_TYPES = (I08, I16, I32, I64, STRING)
VAL_TYPES = (BOOL, I08, DOUBLE, I16, I32, I64, STRING)
MAX_COLS = 16
M64 = (1 << 64) - 1
LIST_STR, SET_STR = LIST | STRING, SET | STRING


def map_kind(kt: int, vt: int) -> int:
    return MAP | kt << 4 | vt


ALL_KINDS = [LIST_STR, SET_STR] + [map_kind(kt, vt) for kt in KEY_TYPES for vt in VAL_TYPES]


def kind_ok(kind: int) -> bool:
    return kind in ALL_KINDS


def is_map(kind: int) -> bool:
    return bool(kind & MAP)


def types(kind: int):
    """(key type or 0, value type)"""
    return ((kind >> 4) & 15, kind & 15) if is_map(kind) else (0, STRING)


def wire_type(kind: int) -> int:
    return T_MAP if is_map(kind) else T_LIST if kind & LIST else T_SET


def stride(kind: int) -> int:
    kt, vt = types(kind)
    return WIDTH[kt] + WIDTH[vt] if kt in WIDTH and vt in WIDTH else 0


def bits(v) -> int:
    """a 64-bit input: an int taken mod 2^64, a float as its bits"""
    if isinstance(v, float):
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    return int(v) & M64


def scalar(t: int, v) -> bytes:
    v = bits(v)
    if t == BOOL:
        return b"\x01" if v else b"\x00"
    w = WIDTH[t]
    return (v & ((1 << 8 * w) - 1)).to_bytes(w, "big")


def string(b) -> bytes:
    b = b.encode() if isinstance(b, str) else bytes(b)
    return struct.pack(">i", len(b)) + b


def one(t: int, v) -> bytes:
    return string(v) if t == STRING else scalar(t, v)


def header(kind: int, cnt: int) -> bytes:
    kt, vt = types(kind)
    return (bytes([kt, vt]) if is_map(kind) else bytes([STRING])) + struct.pack(">i", cnt)


def encode(kind: int, v) -> bytes:
    """one container: a list kind from a sequence of str / bytes, a map kind from a sequence of (key, value) pairs"""
    kt, vt = types(kind)
    v = list(v)
    if not is_map(kind):
        return header(kind, len(v)) + b"".join(string(e) for e in v)
    return header(kind, len(v)) + b"".join(one(kt, k) + one(vt, x) for k, x in v)


def field_begin(kind: int, fid: int) -> bytes:
    return bytes([wire_type(kind)]) + struct.pack(">h", fid)


def cell_status(kind: int, col, i: int, fh: int = 0, stop: int = 0):
    """(status, first entry, count as written) of row i of a present cell"""
    kt, vt = types(kind)
    a, b, n_ent = int(col["ent_off"][i]), int(col["ent_off"][i + 1]), int(col["n_ent"])
    if a > b or b > n_ent:
        return E_RANGE, 0, 0
    cnt = b - a
    if cnt > 2 ** 31 - 1:
        return E_SIZE, 0, 0
    total = fh + (6 if is_map(kind) else 5) + stop
    if stride(kind):
        total += cnt * stride(kind)
    else:
        for t, name in ((kt, "key_len"), (vt, "val_len")):
            if not cnt:  # an empty cell reads no array
                break
            if t == STRING:
                lens = col[name][a:b]
                if int(lens.max()) > 2 ** 31 - 1:
                    return E_SIZE, 0, 0
                total += 4 * cnt + int(lens.astype("u8").sum())
            elif t:
                total += cnt * WIDTH[t]
    if total >= 2 ** 32:
        return E_SIZE, 0, 0
    return OK, a, cnt


def encode_cell(kind: int, col, i: int, fh: int = 0, stop: int = 0):
    """(value bytes, status) of row i of a column given by its arrays"""
    kt, vt = types(kind)
    st, a, cnt = cell_status(kind, col, i, fh, stop)
    out = [header(kind, cnt)]
    for e in range(a, a + cnt):
        for t, v, ln, src in ((kt, "key", "key_len", "key_src"), (vt, "val", "val_len", "val_src")):
            if t == STRING:
                at, n = int(col[v][e]), int(col[ln][e])
                out.append(struct.pack(">i", n) + col[src][at:at + n].tobytes())
            elif t:
                out.append(scalar(t, int(col[v][e])))
    return b"".join(out), st


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
                val, st = encode_cell(kind, col, i, fh, stop)
                item = (field_begin(kind, field_ids[j]) if fh else b"") + val
            if stop:
                item += b"\0"
            out.append(item)
            status.append(st)
            pos += len(item)
            off.append(pos)
    return b"".join(out), off, status
