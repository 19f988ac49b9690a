"""Built inputs of entry column writes (dg_evals_*), shared by the host check
(test_evals_host.py) and the GPU tests (test_gpu_evals.py). A column is a dict
of numpy arrays in the shapes the entries take: ent_off (u64), key (u64),
key_len (u32), val (u64), val_len (u32), key_src and val_src (u8), present (u8,
struct mode only), and n_ent (an int). A case is (name, kinds, field_ids or
None, cols, n)."""
import random
import struct

import numpy as np

import evalsref as ER

GUARD = 0xAA
CANARY = 0x5A5A5A5A5A5A5A5A
# each integer width: 0, +-1, both edges, one past each edge; 0xFF under I08
INTS = {ER.I08: [0, 1, -1, 127, -128, 128, 255, 256, 2 ** 63],
        ER.I16: [0, 1, -1, 2 ** 15 - 1, -2 ** 15, 2 ** 15, 0xFFFF, 0x10000, 2 ** 63],
        ER.I32: [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 63],
        ER.I64: [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 63, 2 ** 64 - 1, 0x0102030405060708, 2 ** 7, 2 ** 15, 2 ** 31]}
BOOLS = [0, 1, 2, 2 ** 63, 0xFF, -1]
# NaNs with payloads (quiet and signalling), +-0.0, denormals, infinities, as bits
DOUBLES = [0x7FF8000000000001, 0xFFF80000DEADBEEF, 0x7FF0000000000001, 0, 0x8000000000000000, 1, 0x8000000000000001,
           0x7FF0000000000000, 0x3FF0000000000000, 0xC00921FB54442D18]
COUNTS = list(range(0, 258)) + [2049, 4097]
GEOMETRY_K = (1, 2, 7, 16)
GEOMETRY_N = (1, 63, 64, 65, 255, 256, 257)
FIELD_IDS = [1, 255, 256, 32767, -1]


def payload(rng, ln):
    return bytes(rng.randrange(1, 256) if (k & 7) else 0x80 | (k >> 3 & 0x7F) for k in range(ln)) if ln < 64 else \
        rng.randbytes(ln)


def pool(t):
    return BOOLS if t == ER.BOOL else DOUBLES if t == ER.DOUBLE else INTS[t]


def value(rng, t, k):
    """entry k's key or value of type t: the pool first (so keys repeat: duplicates), then random"""
    if t == ER.STRING:
        return payload(rng, (0, 1, 5, 8, 13, 3, 24)[k % 7])
    p = pool(t)
    return p[k % len(p)] if k < 2 * len(p) else rng.getrandbits(64)


def _arena(payloads, phase):
    """payload i at a residue (phase + 7 i) mod 16, filler between them, the
    LAST payload as the arena's last bytes, then 16 guard bytes"""
    src, at = bytearray(), []
    for i, p in enumerate(payloads):
        while len(src) % 16 != (phase + 7 * i) % 16:
            src.append(0xEE)
        at.append(len(src))
        src += p
    src += bytes([GUARD]) * 16
    return np.array(at, dtype=np.uint64), np.frombuffer(bytes(src), dtype=np.uint8)


def entry_col(kind, rows, phase=0, lead=0, tail=2):
    """rows[i] = message i's container: a list kind's elements (bytes), a map
    kind's (key, value) pairs. `lead` entries of some other owner lie before
    the first, `tail` canary entries behind n_ent."""
    kt, vt = ER.types(kind)
    flat = [e if ER.is_map(kind) else (None, e) for r in rows for e in r]
    filler = (b"" if kt == ER.STRING else 0, b"" if vt == ER.STRING else 0)
    flat = [filler] * lead + flat
    n_ent = len(flat)
    c = {"ent_off": np.concatenate([[lead], lead + np.cumsum([len(r) for r in rows])]).astype(np.uint64), "n_ent": n_ent}
    for t, side, x in ((kt, "key", 0), (vt, "val", 1)):
        if not t:
            continue
        if t == ER.STRING:
            at, c[side + "_src"] = _arena([bytes(e[x]) for e in flat], phase + 3 * x)
            c[side] = np.concatenate([at, [CANARY] * tail]).astype(np.uint64)
            c[side + "_len"] = np.array([len(e[x]) for e in flat] + [0x7FFFFFF0] * tail, dtype=np.uint32)
        else:
            c[side] = np.array([ER.bits(e[x]) for e in flat] + [CANARY] * tail, dtype=np.uint64)
    return c


def rows_for(rng, kind, counts):
    kt, vt = ER.types(kind)
    if not ER.is_map(kind):
        return [[value(rng, vt, k) for k in range(c)] for c in counts]
    return [[(value(rng, kt, k), value(rng, vt, k + i)) for k in range(c)] for i, c in enumerate(counts)]


def matrix_cases():
    """every legal kind: keys and values over their pools' edges, duplicate keys, empty strings"""
    rng = random.Random(21)
    for kind in ER.ALL_KINDS:
        counts = [0, 1, 2, 3, 12, 23, 9]
        yield "matrix kind %#x" % kind, [kind], None, [entry_col(kind, rows_for(rng, kind, counts), phase=kind)], len(counts)


def kind_messages():
    """struct{1: X} for every container of matrix_cases(), as evalsref writes it: what the round trip with the read
    side reads where entsgen's messages hold no container of a kind (their BOOL bytes are not all 0 or 1)"""
    msgs = []
    for _, kinds, _, cols, n in matrix_cases():
        arena, off, _ = ER.encode_batch(kinds, cols, n, [1])
        msgs += [arena[a:b] for a, b in zip(off, off[1:])]
    return msgs


COUNT_KINDS = [ER.LIST_STR, ER.map_kind(ER.STRING, ER.I64), ER.map_kind(ER.I32, ER.DOUBLE), ER.map_kind(ER.I64, ER.STRING)]


def count_cases():
    """0 to 257, 2 049 and 4 097 entries, unequal neighbours; one container of 4 097 between containers of 0 and 1"""
    rng = random.Random(22)
    for kind in COUNT_KINDS:
        counts = COUNTS if kind != ER.LIST_STR else COUNTS[::-1]
        yield "counts of %#x" % kind, [kind], None, [entry_col(kind, rows_for(rng, kind, counts), lead=3)], len(counts)
        lone = [0, 1] * 5 + [0, 4097, 1] + [1, 0] * 5
        yield "one of 4097 of %#x" % kind, [kind], None, [entry_col(kind, rows_for(rng, kind, lone))], len(lone)


def string_cases():
    """lengths 0 to 255 and 16 385 at every source residue; `shift` one-byte-stride columns of shift entries in front
    move the output's residues"""
    rng = random.Random(23)
    kss, kis = ER.map_kind(ER.STRING, ER.STRING), ER.map_kind(ER.I08, ER.BOOL)
    for shift in range(16):
        lens = list(range(256)) + [16385] if shift in (0, 5) else [(shift + 3 * k) % 41 for k in range(24)] + [255]
        if shift % 2:
            lens.reverse()
        rows = [[payload(rng, ln) for ln in lens[a:a + 9]] for a in range(0, len(lens), 9)]
        n = len(rows)
        pairs = [[(payload(rng, ln), payload(rng, (ln * 7 + shift) % 50)) for ln in lens[a:a + 9]] for a in range(0, len(lens), 9)]
        front = entry_col(kis, [[(k, k & 1)] * shift for k in range(n)])
        yield "strings shift %d" % shift, [kis, ER.LIST_STR, kss], None, \
            [front, entry_col(ER.LIST_STR, rows, phase=shift), entry_col(kss, pairs, phase=shift + 5)], n


GEOMETRY_KINDS = [ER.map_kind(ER.I32, ER.DOUBLE), ER.LIST_STR, ER.map_kind(ER.STRING, ER.I64), ER.map_kind(ER.I08, ER.BOOL),
                  ER.map_kind(ER.I64, ER.STRING), ER.SET_STR, ER.map_kind(ER.I16, ER.I16), ER.map_kind(ER.STRING, ER.STRING),
                  ER.map_kind(ER.I64, ER.I64), ER.map_kind(ER.STRING, ER.BOOL), ER.LIST_STR, ER.map_kind(ER.I32, ER.I08),
                  ER.map_kind(ER.I16, ER.STRING), ER.map_kind(ER.STRING, ER.DOUBLE), ER.map_kind(ER.I08, ER.I32), ER.SET_STR]


def geometry_case(K, n, seed=0, ids=False):
    """fixed-stride and variable kinds mixed in one plan; with ids, present masks on two columns of three"""
    rng = random.Random(1000 * K + n + seed)
    kinds = GEOMETRY_KINDS[:K]
    cols = [entry_col(k, rows_for(rng, k, [rng.choice((0, 0, 1, 2, 3, 9)) for _ in range(n)]), phase=j, lead=j % 3)
            for j, k in enumerate(kinds)]
    fids = None
    if ids:
        fids = [FIELD_IDS[j % len(FIELD_IDS)] - (j // len(FIELD_IDS)) * 7 for j in range(K)]
        for j, c in enumerate(cols):
            if j % 3 != 2:
                c["present"] = np.array([rng.random() < 0.6 for _ in range(n)], dtype=np.uint8)
    return "geometry K=%d n=%d%s" % (K, n, " struct" if ids else ""), kinds, fids, cols, n


def struct_cases():
    """K = 3 with all 8 present combinations (the all-absent message is STOP alone); the field ids' edges"""
    rng = random.Random(24)
    kinds = [ER.map_kind(ER.I32, ER.I64), ER.LIST_STR, ER.map_kind(ER.STRING, ER.STRING)]
    cols = [entry_col(k, rows_for(rng, k, [2, 0, 1, 3, 9, 64, 5, 8])) for k in kinds]
    for j, c in enumerate(cols):
        c["present"] = np.array([i >> j & 1 for i in range(8)], dtype=np.uint8)
    yield "struct presence", kinds, [1, 255, 256], cols, 8
    for K in (1, 5, 16):
        yield geometry_case(K, 67, ids=True)


def flag_cases():
    """Range flags: offsets that decrease, overlap, leave gaps and pass n_ent. Size flags: lengths of 2^31 and 2^32 - 1
    on entries whose payload offset 0 would run far past the arena if it were read."""
    rng = random.Random(25)
    off = np.array([0, 5, 3, 8, 12, 10, 10, 2, 7, 11, 10], dtype=np.uint64)
    for kind in (ER.LIST_STR, ER.map_kind(ER.STRING, ER.I64), ER.map_kind(ER.I16, ER.DOUBLE), ER.map_kind(ER.I32, ER.STRING)):
        c = entry_col(kind, rows_for(rng, kind, [10]), tail=4)
        c["ent_off"] = off
        yield "ranges of %#x" % kind, [kind], None, [c], len(off) - 1
        c = dict(entry_col(kind, rows_for(rng, kind, [10]), tail=4), ent_off=off,
                 present=np.array([1, 1, 1, 0, 0, 1, 1, 1, 1, 1], dtype=np.uint8))
        yield "ranges of %#x, struct" % kind, [kind], [7], [c], len(off) - 1
    for kind, side in ((ER.LIST_STR, "val"), (ER.map_kind(ER.STRING, ER.I64), "key"), (ER.map_kind(ER.I32, ER.STRING), "val"),
                       (ER.map_kind(ER.STRING, ER.STRING), "val")):
        c = entry_col(kind, rows_for(rng, kind, [3, 2, 0, 4, 1, 2]))
        for e, ln in ((1, 2 ** 31), (7, 2 ** 32 - 1), (10, 2 ** 31 - 1)):
            c[side + "_len"] = c[side + "_len"].copy()
            c[side + "_len"][e] = ln
            c[side] = c[side].copy()
            c[side][e] = 0
        # entries 1 and 7 flag their cells by a length, entry 10's 2^31 - 1 bytes make its cell's item 2^32 or more
        # only beside another such entry: cell 5 = entries 10, 11
        c[side + "_len"][11] = 2 ** 31 - 1
        c[side][11] = 0
        yield "sizes of %#x" % kind, [kind], None, [c], 6


def count_flag_case(ids=False):
    """A fixed-stride kind whose sizing call reads d_ent_off alone: n_ent = 2^32 - 1 over arrays of two entries. A
    count of 2^31 is E_SIZE; a count above 2^31 - 1 that also passes n_ent is E_RANGE (tested first), and so is what
    decreases; the cells between are empty. For sizing calls only."""
    kind = ER.map_kind(ER.I32, ER.DOUBLE)
    c = {"ent_off": np.array([0, 2 ** 31, 2 ** 31, 2 ** 32 + 5, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31 - 1], dtype=np.uint64),
         "n_ent": 2 ** 32 - 1, "key": np.zeros(2, dtype=np.uint64), "val": np.zeros(2, dtype=np.uint64)}
    return "counts beyond 2^31 - 1", [kind], [3] if ids else None, [c], 6


def all_cases(geometry_k=GEOMETRY_K, geometry_n=GEOMETRY_N, counts=True):
    yield from matrix_cases()
    if counts:
        yield from count_cases()
    yield from string_cases()
    yield from struct_cases()
    yield from flag_cases()
    for K in geometry_k:
        for n in geometry_n:
            yield geometry_case(K, n)


FIELDS = ("ent_off", "key", "key_len", "val", "val_len", "key_src", "val_src", "present")
WIDTHS = (8, 8, 4, 8, 4, 1, 1, 1)


def corpus_bytes(case) -> bytes:
    """a case as the stand-alone program of evals_host.cpp reads it: u32 K, n, has_ids; K u16 kinds; K i16 ids; per
    column n_ent and eight u64 array lengths (in elements, FIELDS' order) and the arrays"""
    _, kinds, fids, cols, n = case
    K = len(kinds)
    out = [struct.pack("<3I", K, n, fids is not None), struct.pack("<%dH" % K, *kinds), struct.pack("<%dh" % K, *(fids or [0] * K))]
    for c in cols:
        arrs = [c.get(f) for f in FIELDS]
        out.append(struct.pack("<9Q", c["n_ent"], *[0 if a is None else len(a) for a in arrs]))
        out += [a.tobytes() for a in arrs if a is not None]
    return b"".join(out)
