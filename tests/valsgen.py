"""Built inputs of typed column writes (dg_vals_*), shared by the host check
(test_vals_host.py) and the GPU tests (test_gpu_vals.py). A column is a dict of
numpy arrays in the shapes the entries take: val (u64), len (u32), src (u8),
elem_off (u64), elems (u64), present (u8, struct mode only). A case is (name,
kinds, field_ids or None, cols, n)."""
import random
import struct

import numpy as np

import valsref as VR

M64 = VR.M64
GUARD = 0xAA

# each integer width: 0, 1, -1, both edges, one past each edge
INTS = {VR.I08: [0, 1, -1, 127, -128, 128, -129, 255, 256],
        VR.I16: [0, 1, -1, 2 ** 15 - 1, -2 ** 15, 2 ** 15, -2 ** 15 - 1, 0xFFFF, 0x10000],
        VR.I32: [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 31, -2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32],
        VR.I64: [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 63, 2 ** 64 - 1, 0x0102030405060708, 0x8000000000000001]}
BOOLS = [0, 1, 2, 0xFF, -1, 2 ** 63]
# quiet and signalling NaNs with payloads, +-0.0, the smallest denormal, +-inf, as bits
DOUBLES = [0x7FF8000000000001, 0xFFF80000DEADBEEF, 0x7FF0000000000001, 0xFFF4000000000123, 0, 0x8000000000000000, 1,
           0x8000000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000, 0xC00921FB54442D18]
STRING_LENS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 16385]
LIST_COUNTS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
ELEM_TYPES = [VR.BOOL, VR.I08, VR.DOUBLE, VR.I16, VR.I32, VR.I64]
GEOMETRY_N = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
FIELD_IDS = [1, 255, 256, 32767, -1]


def scalar_col(values, n=None):
    n = n or len(values)
    return {"val": np.array([VR.bits(values[i % len(values)]) for i in range(n)], dtype=np.uint64)}


def string_col(payloads, phase=0):
    """The payloads in one arena, payload i at a residue (phase + 7 i) mod 16,
    filler between them, the LAST payload as the arena's last bytes, and then
    16 guard bytes that no output may show."""
    src, val = bytearray(), []
    for i, p in enumerate(payloads):
        while len(src) % 16 != (phase + 7 * i) % 16:
            src.append(0xEE)
        val.append(len(src))
        src += p
    src += bytes([GUARD]) * 16
    return {"val": np.array(val, dtype=np.uint64), "len": np.array([len(p) for p in payloads], dtype=np.uint32),
            "src": np.frombuffer(bytes(src), dtype=np.uint8)}


def list_col(lists, lead=0):
    """elem_off starts at `lead` (elements of some other column before it)"""
    off = np.concatenate([[lead], lead + np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = [VR.bits(e) for x in lists for e in x]
    return {"elem_off": off, "elems": np.array([0x5A5A5A5A5A5A5A5A] * lead + flat, dtype=np.uint64)}


def payload(rng, ln):
    return bytes(rng.randrange(1, 256) if (k & 7) else 0x80 | (k >> 3 & 0x7F) for k in range(ln)) if ln < 64 else \
        rng.randbytes(ln)


def elem_values(rng, et, cnt):
    pool = BOOLS if et == VR.BOOL else DOUBLES if et == VR.DOUBLE else INTS[et]
    return [pool[k % len(pool)] if k < 2 * len(pool) else rng.getrandbits(64) for k in range(cnt)]


def matrix_cases():
    kinds = [VR.BOOL, VR.I08, VR.I16, VR.I32, VR.I64, VR.DOUBLE]
    pools = [BOOLS, INTS[VR.I08], INTS[VR.I16], INTS[VR.I32], INTS[VR.I64], DOUBLES]
    n = max(len(p) for p in pools)
    yield "matrix", kinds, None, [scalar_col(p, n) for p in pools], n
    for kind, p in zip(kinds, pools):
        yield "matrix kind %d" % kind, [kind], None, [scalar_col(p)], len(p)


def string_cases():
    """every length, every source residue; `shift` 1-byte BOOL columns in front move the output's residues"""
    rng = random.Random(11)
    for shift in range(16):
        lens = STRING_LENS if shift in (0, 5) else STRING_LENS[:17]
        pay = [payload(rng, ln) for ln in lens]
        if shift % 2:
            pay.reverse()
        cols = [scalar_col([i & 1], len(pay)) for i in range(shift)] + [string_col(pay, phase=shift)]
        yield "strings shift %d" % shift, [VR.BOOL] * shift + [VR.STRING], None, cols, len(pay)


def list_cases():
    rng = random.Random(12)
    for et in ELEM_TYPES:
        a = [elem_values(rng, et, c) for c in LIST_COUNTS]
        b = [elem_values(rng, et, c) for c in reversed(LIST_COUNTS)]
        yield "lists of %d" % et, [VR.LIST | et, VR.SET | et], None, [list_col(a), list_col(b, lead=3)], len(a)
    for et in (VR.I08, VR.I32, VR.DOUBLE):
        yield "empty lists of %d" % et, [VR.LIST | et], None, [list_col([[]] * 70)], 70
        lone = [[]] * 256
        lone[101] = elem_values(rng, et, 4097)
        yield "one list of %d among empties" % et, [VR.SET | et], None, [list_col(lone)], 256


GEOMETRY_KINDS = [VR.I32, VR.STRING, VR.BOOL, VR.LIST | VR.I16, VR.DOUBLE, VR.STRING, VR.SET | VR.I64, VR.I08, VR.I64,
                  VR.LIST | VR.BOOL, VR.I16, VR.STRING, VR.LIST | VR.DOUBLE, VR.SET | VR.I32, VR.BOOL, VR.LIST | VR.I08]


def column_for(rng, kind, n, long_at=None):
    """a column of short values; row long_at gets one that spans several chunks of the body pass"""
    if kind == VR.STRING:
        pay = [payload(rng, rng.choice((0, 1, 5, 8, 13, 24, 40))) for _ in range(n)]
        if long_at is not None:
            pay[long_at] = payload(rng, 40000)
        return string_col(pay, phase=rng.randrange(16))
    if kind & (VR.LIST | VR.SET):
        ls = [elem_values(rng, kind & 0x3F, rng.choice((0, 0, 1, 2, 3, 9))) for _ in range(n)]
        if long_at is not None:
            ls[long_at] = elem_values(rng, kind & 0x3F, 5000)
        return list_col(ls)
    return scalar_col([rng.getrandbits(64) for _ in range(n)])


def geometry_case(K, n, seed=0, ids=False):
    rng = random.Random(1000 * K + n + seed)
    kinds = GEOMETRY_KINDS[:K]
    long_at = n // 2 if n in (65, 1025) else None
    cols = [column_for(rng, k, n, long_at if j == 1 else None) for j, k in enumerate(kinds)]
    fids = None
    if ids:
        fids = [FIELD_IDS[j % len(FIELD_IDS)] - (j // len(FIELD_IDS)) * 7 for j in range(K)]
        for j, c in enumerate(cols):
            if j % 3 != 2:
                c["present"] = np.array([rng.random() < 0.6 for _ in range(n)], dtype=np.uint8)
    return "geometry K=%d n=%d%s" % (K, n, " struct" if ids else ""), kinds, fids, cols, n


def struct_cases():
    """K = 3 with all 8 present combinations in one batch; the field ids' edges; absent columns around bodies"""
    rng = random.Random(13)
    n = 8
    kinds = [VR.I32, VR.STRING, VR.LIST | VR.DOUBLE]
    cols = [scalar_col([7, -7, 2 ** 31], n), string_col([payload(rng, ln) for ln in (0, 1, 9, 16, 17, 300, 4, 8)]),
            list_col([elem_values(rng, VR.DOUBLE, c) for c in (0, 1, 2, 3, 9, 64, 5, 8)])]
    for j, c in enumerate(cols):
        c["present"] = np.array([i >> j & 1 for i in range(n)], dtype=np.uint8)
    yield "struct presence", kinds, [1, 255, 256], cols, n
    kinds = [VR.BOOL, VR.I64, VR.STRING, VR.SET | VR.I16, VR.DOUBLE]
    cols = [column_for(rng, k, 67) for k in kinds]
    cols[1]["present"] = np.array([i % 3 != 0 for i in range(67)], dtype=np.uint8)
    cols[4]["present"] = np.array([i % 2 for i in range(67)], dtype=np.uint8)
    yield "struct field ids", kinds, FIELD_IDS, cols, 67
    yield "struct scalars", [VR.I16, VR.BOOL, VR.I64], [3, -32768, 9], [column_for(rng, k, 130) for k in
                                                                         (VR.I16, VR.BOOL, VR.I64)], 130
    for K in (1, 16):
        yield geometry_case(K, 257, ids=True)


def all_cases(geometry_k=(1, 2, 3, 7, 16), geometry_n=(1, 64, 65, 257)):
    yield from matrix_cases()
    yield from string_cases()
    yield from list_cases()
    yield from struct_cases()
    for K in geometry_k:
        for n in geometry_n:
            yield geometry_case(K, n)


def corpus_bytes(case) -> bytes:
    """a case as the stand-alone program of vals_host.cpp reads it: u32 K, n, has_ids; K kind bytes; K i16 ids; per
    column six u64 array lengths (in elements: val, len, src, elem_off, elems, present) and the arrays"""
    _, kinds, fids, cols, n = case
    K = len(kinds)
    out = [struct.pack("<3I", K, n, fids is not None), bytes(kinds), struct.pack("<%dh" % K, *(fids or [0] * K))]
    for c in cols:
        arrs = [c.get(f) for f in ("val", "len", "src", "elem_off", "elems", "present")]
        out.append(struct.pack("<6Q", *[0 if a is None else len(a) for a in arrs]))
        out += [a.tobytes() for a in arrs if a is not None]
    return b"".join(out)
