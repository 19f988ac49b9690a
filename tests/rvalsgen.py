"""Built inputs of row column writes (dg_rvals_*), shared by the host check
(test_rvals_host.py) and the GPU tests (test_gpu_rvals.py). A column is a dict
of numpy arrays indexed by row, in valsgen's shapes: val (u64), len (u32), src
(u8), elem_off (u64), elems (u64), present (u8). A case is (name, kinds,
field_ids, cols, row_off, n, n_rows): message i owns the rows [row_off[i],
row_off[i + 1])."""
import random
import struct

import numpy as np

import rvalsref as RR
import valsgen as VG
import valsref as VR

GUARD = VG.GUARD
CHUNK = 16384  # VL_CHUNK: the arena's bytes a block of the body pass takes a round
ROW_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2049]
SCALARS = [VR.BOOL, VR.I08, VR.I16, VR.I32, VR.I64, VR.DOUBLE]
POOLS = [VG.BOOLS, VG.INTS[VR.I08], VG.INTS[VR.I16], VG.INTS[VR.I32], VG.INTS[VR.I64], VG.DOUBLES]
assert {0, 1, 2, 2 ** 63} <= set(VG.BOOLS)


def offsets(counts, lead=0):
    return np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.uint64)


def field_ids(K):
    return [VG.FIELD_IDS[j % len(VG.FIELD_IDS)] - (j // len(VG.FIELD_IDS)) * 7 for j in range(K)]


def case(name, kinds, cols, row_off, n_rows, fids=None):
    row_off = np.asarray(row_off, dtype=np.uint64)
    return name, list(kinds), fids or field_ids(len(kinds)), cols, row_off, len(row_off) - 1, n_rows


def matrix_cases():
    """all 19 kinds: the width edges, NaN payloads, BOOL inputs 0 / 1 / 2 / 2^63, as scalars and as elements"""
    rng = random.Random(21)
    n_rows = max(len(p) for p in POOLS)
    cols = [VG.scalar_col(p, n_rows) for p in POOLS]
    cols.append(VG.string_col([VG.payload(rng, ln) for ln in range(n_rows)], phase=3))
    lists = [VG.list_col([VG.elem_values(rng, et, (g * 5) % 23) for g in range(n_rows)], lead=et) for et in SCALARS]
    yield case("matrix scalars, string, lists", SCALARS + [VR.STRING] + [VR.LIST | et for et in SCALARS], cols + lists,
               [0, 5, n_rows], n_rows)
    sets = [VG.list_col([VG.elem_values(rng, et, (g * 7) % 19) for g in range(n_rows)]) for et in SCALARS]
    yield case("matrix sets", [VR.SET | et for et in SCALARS], sets, [0, 1, 1, n_rows], n_rows)
    yield case("matrix scalars alone", SCALARS, [VG.scalar_col(p, n_rows) for p in POOLS], [0, 4, n_rows], n_rows)


def present_col(rng, n_rows, p=0.6):
    return np.array([rng.random() < p for _ in range(n_rows)], dtype=np.uint8)


def count_cases():
    """messages of every row count; one message of 4097 rows between messages of 0 and 1"""
    rng = random.Random(22)
    n_rows = sum(ROW_COUNTS)
    kinds = [VR.I32, VR.STRING]
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    yield case("row counts", kinds, cols, offsets(ROW_COUNTS), n_rows)
    yield case("row counts, scalars", [VR.I16, VR.DOUBLE, VR.BOOL], [VG.column_for(rng, k, n_rows) for k in (VR.I16, VR.DOUBLE, VR.BOOL)],
               offsets(list(reversed(ROW_COUNTS))), n_rows)
    kinds = VG.GEOMETRY_KINDS[:7]
    n_rows = 4098
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    for j in (0, 3, 6):
        cols[j]["present"] = present_col(rng, n_rows)
    yield case("one of 4097 rows between 0 and 1", kinds, cols, offsets([0, 4097, 1]), n_rows)


def partition(rng, n_rows, n):
    cuts = sorted(rng.randrange(n_rows + 1) for _ in range(n - 1))
    return np.array([0] + cuts + [n_rows], dtype=np.uint64)


def geometry_case(K, n_rows, n=None, seed=0, present=True):
    """K columns of mixed kinds over n_rows rows (valsgen's geometry columns, row n_rows // 2 with a string of
    several body chunks when n_rows is 65 or 1025), cut into n messages at random"""
    _, kinds, _, cols, _ = VG.geometry_case(K, n_rows, seed, ids=present)
    rng = random.Random(31 * K + n_rows + seed)
    n = n or max(1, n_rows // 3)
    return case("geometry K=%d rows=%d n=%d%s" % (K, n_rows, n, "" if present else " all present"), kinds, cols,
                partition(rng, n_rows, n), n_rows)


def present_cases():
    """K = 3 with all 8 present combinations: a row with nothing present, a last column absent behind a scalar and
    behind a body"""
    name, kinds, fids, cols, n_rows = next(iter(VG.struct_cases()))
    yield case("presence", kinds, cols, [0, 3, 3, 8], n_rows, fids)
    rng = random.Random(23)
    kinds = [VR.STRING, VR.I64, VR.LIST | VR.I16]
    n_rows = 40
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    cols[1]["present"] = np.array([g % 2 for g in range(n_rows)], dtype=np.uint8)
    cols[2]["present"] = np.array([g % 3 == 0 for g in range(n_rows)], dtype=np.uint8)  # STOP behind a string's body
    yield case("last column absent", kinds, cols, [0, 1, 2, 20, 40], n_rows)
    cols = [dict(c, present=np.zeros(n_rows, dtype=np.uint8)) for c in cols]
    yield case("nothing present", kinds, cols, [0, 7, 40], n_rows)


def string_cases():
    """K = 1, a STRING: row 0 is a message of its own whose string of `shift` bytes moves every later payload by one
    output residue; the other rows take every length at every source residue"""
    rng = random.Random(24)
    for shift in range(16):
        lens = VG.STRING_LENS if shift in (0, 5) else list(range(0, 256, 15)) + VG.STRING_LENS[:17]
        pay = [VG.payload(rng, shift)] + [VG.payload(rng, ln) for ln in lens]
        if shift % 2:
            pay[1:] = pay[:0:-1]
        yield case("strings shift %d" % shift, [VR.STRING], [VG.string_col(pay, phase=shift)], [0, 1, 1 + len(lens) // 2, len(pay)],
                   len(pay))
    pay = [VG.payload(rng, ln) for ln in range(256)]
    yield case("strings of 0 to 255 bytes", [VR.STRING, VR.BOOL], [VG.string_col(pay), VG.scalar_col([1, 0], 256)], [0, 100, 256], 256)


def list_cases():
    """inner lists of 0 to 4097 elements of every element type"""
    rng = random.Random(25)
    for et in VG.ELEM_TYPES:
        a = [VG.elem_values(rng, et, c) for c in VG.LIST_COUNTS]
        b = [VG.elem_values(rng, et, c) for c in reversed(VG.LIST_COUNTS)]
        yield case("lists of %d" % et, [VR.LIST | et, VR.SET | et], [VG.list_col(a), VG.list_col(b, lead=3)], [0, 7, 7, len(a)], len(a))


def chunk_cases():
    """arenas of 1, 2 and 3 chunks of the body pass"""
    rng = random.Random(26)
    for chunks in (1, 2, 3):
        total = chunks * CHUNK - 1000
        n_rows = 24
        pay = [VG.payload(rng, total // n_rows - 8) for _ in range(n_rows)]
        yield case("arena of %d chunks" % chunks, [VR.STRING], [VG.string_col(pay, phase=chunks)], [0, 9, 10, n_rows], n_rows)


def overlap_cases():
    """rows owned twice (across a RANGE message) and rows owned by nobody"""
    rng = random.Random(27)
    kinds = [VR.I32, VR.STRING, VR.LIST | VR.DOUBLE]
    n_rows = 30
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    cols[0]["present"] = present_col(rng, n_rows)
    yield case("overlap and gaps", kinds, cols, [2, 12, 5, 14, 14, 20, 0, 3, 25], n_rows)
    yield case("all of it twice", kinds, cols, [0, n_rows, 0, n_rows], n_rows)


def flag_cases():
    """RANGE: row_off[i] > row_off[i + 1], row_off[i + 1] > n_rows, both; SIZE: a message of three rows of 2^31 - 64
    bytes each (the lengths alone say so: no payload is read); string cells of 2^31 and 2^32 - 1 bytes and a list cell
    whose count wraps, flagged themselves, their rows OK"""
    rng = random.Random(28)
    kinds = [VR.I08, VR.STRING]
    n_rows = 12
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    yield case("range flags", kinds, cols, [0, 4, 2, 13, 12, 12, 2 ** 63, 5, 9], n_rows)
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    cols[1]["len"] = cols[1]["len"].copy()
    cols[1]["len"][3:6] = 2 ** 31 - 64
    cols[1]["len"][8] = 2 ** 31
    cols[1]["len"][10] = 2 ** 32 - 1
    yield case("size flags", kinds, cols, [0, 3, 6, 8, 9, 12], n_rows)
    lists = VG.list_col([[1, 2]] * n_rows)
    lists["elem_off"] = lists["elem_off"].copy()
    lists["elem_off"][5:] -= 8  # row 4 is [8, 2): its count wraps to 2^64 - 6
    yield case("a list cell of a wrapped count", [VR.LIST | VR.I08, VR.I16], [lists, VG.scalar_col([7], n_rows)], [0, 4, 5, 12], n_rows)


def count_flag_case():
    """K = 1, a scalar, every field present (the fixed-stride route), n_rows = 2^31 + 8: a count of 2^31 is E_SIZE,
    behind RANGE; 2^31 - 1 rows of 12 bytes are E_SIZE by their bytes. The one-row array is never read: a sizing call."""
    n_rows = 2 ** 31 + 8
    row_off = [0, 2 ** 31, 2 ** 31 + 1, n_rows + 1, 5, 6, 2 ** 31 + 5, 2 ** 31 + 8]
    name, kinds, fids, cols, row_off, n, _ = case("count of 2^31", [VR.I64], [VG.scalar_col([1])], row_off, n_rows)
    want = RR.statuses_only(kinds, row_off, n, n_rows, 12)
    assert want[1] == [RR.E_SIZE, RR.OK, RR.E_RANGE, RR.E_RANGE, RR.OK, RR.E_SIZE, RR.OK]
    return (name, kinds, fids, cols, row_off, n, n_rows), want


def all_cases(geometry_k=(1, 2, 7, 16), geometry_rows=(1, 64, 65, 257)):
    yield from matrix_cases()
    yield from count_cases()
    yield from present_cases()
    yield from string_cases()
    yield from list_cases()
    yield from chunk_cases()
    yield from overlap_cases()
    yield from flag_cases()
    for K in geometry_k:
        for rows in geometry_rows:
            yield geometry_case(K, rows)
    yield geometry_case(3, 130, present=False, seed=1)
    yield scalar_case()


def scalar_case(n_rows=257, n=40):
    """16 scalar columns, the widest first (the largest closed-form offsets), every field present: the fixed-stride route"""
    rng = random.Random(29)
    kinds = [VR.I64, VR.DOUBLE] * 5 + SCALARS
    cols = [VG.column_for(rng, k, n_rows) for k in kinds]
    return case("16 scalars rows=%d n=%d" % (n_rows, n), kinds, cols, partition(rng, n_rows, n), n_rows)


def corpus_bytes(c) -> bytes:
    """a case as the stand-alone program of rvals_host.cpp reads it: u32 K, n; u64 n_rows; K kind bytes; K i16 ids;
    n + 1 u64 row offsets; per column six u64 array lengths (in elements: val, len, src, elem_off, elems, present) and
    the arrays"""
    _, kinds, fids, cols, row_off, n, n_rows = c
    K = len(kinds)
    out = [struct.pack("<2IQ", K, n, n_rows), bytes(kinds), struct.pack("<%dh" % K, *fids), row_off.tobytes()]
    for col in cols:
        arrs = [col.get(f) for f in ("val", "len", "src", "elem_off", "elems", "present")]
        out.append(struct.pack("<6Q", *[0 if a is None else len(a) for a in arrs]))
        out += [a.tobytes() for a in arrs if a is not None]
    return b"".join(out)
