"""CPU: the entry-column decode itself (dynamicgo_amd/csrc/ents_device.h: en_cell
behind tg_walk, en_fixed, en_next: the code the kernels run) built for the host
by ents_host.cpp and compared, cell by cell and entry by entry, with the
checker (entsref.py) over all of entsgen's inputs, the ones the GPU tests of
test_gpu_ents.py use. Every message is followed by 16 bytes of 0xAA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import entsgen as EG
import entsref as ER
import tgetref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import to_paths

HERE = os.path.dirname(os.path.abspath(__file__))


def build_ents(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "ents_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host decode with" % B.HIPCC)


@pytest.fixture(scope="module")
def entslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_ents(str(tmp_path_factory.mktemp("ents") / "libentshost.so"), ("-shared",)))
    lib.cell.restype = C.c_int
    lib.cell.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                         C.c_uint64, C.POINTER(C.c_uint32)]
    lib.emit.restype = C.c_uint32
    lib.emit.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    return lib


@pytest.fixture(scope="module")
def decode(entslib):
    """decode(msgs, columns, root_type) -> ([arrays of column k as entsgen.arrays gives them], deep[n, P])"""
    lib = entslib

    def run(msgs, columns, root_type=R.STRUCT):
        blob = G.compile_paths(to_paths([p for p, _ in columns]))
        off_steps, off_pool = np.frombuffer(blob, dtype="<u4", count=8)[5:7].tolist()
        blob += b"\0" * 16
        n = len(msgs)
        cols = [{f: np.zeros(n, dtype=np.uint64) for f in EG.CELL_FIELDS} for _ in columns]
        ents = [{f: [] for f in EG.ENTRY_FIELDS} for _ in columns]
        deep = np.zeros((n, len(columns)), dtype=bool)
        out = (C.c_uint32 * 8)()
        base = 0
        for i, m in enumerate(msgs):
            buf = m + b"\xAA" * 16
            for k, (_, kind) in enumerate(columns):
                deep[i, k] = lib.cell(buf, len(m), blob, off_steps, off_pool, k, root_type, kind, base, out)
                st, ty, step, aux, ln, span, lo, hi = out
                val = lo | hi << 32
                for f, v in zip(EG.CELL_FIELDS, (st, ty, step, aux, val, ln, span)):
                    cols[k][f][i] = v
                if st != R.OK or not ln:
                    assert ln == 0 and (st == R.OK or (val == 0 and span == 0))
                    continue
                key, v = np.zeros(ln, dtype=np.uint64), np.zeros(ln, dtype=np.uint64)
                klen, vlen = np.zeros(ln, dtype=np.uint32), np.zeros(ln, dtype=np.uint32)
                got = lib.emit(buf, val - base, ln, span, aux, kind, key.ctypes.data, klen.ctypes.data, v.ctypes.data,
                               vlen.ctypes.data)
                assert got == ln, (i, k, got, ln)
                if kind & ER.STRMAP:
                    key += np.uint64(base)
                if kind == ER.LISTSTR or kind & 15 == ER.STR:
                    v += np.uint64(base)
                for f, a in zip(EG.ENTRY_FIELDS, (key, klen, v, vlen)):
                    ents[k][f].append(a.astype(np.uint64))
            base += len(m)
        for k in range(len(columns)):
            for f in EG.ENTRY_FIELDS:
                cols[k][f] = np.concatenate(ents[k][f]) if ents[k][f] else np.zeros(0, dtype=np.uint64)
        return cols, deep

    return run


def check(decode, msgs, columns, what, root_type=R.STRUCT):
    want = EG.expect(msgs, columns, root_type)
    got, deep = decode(msgs, columns, root_type)
    for k in range(len(columns)):
        EG.same(got[k], EG.arrays(want[k]), "%s, column %d" % (what, k))
    return want, deep


def matrix_properties(sets):
    """what the matrix must hold for the two map casts' check orders to be told apart, on the checker alone"""
    a, b = sets
    by = dict(zip(ER.KINDS, a + b[:1]))
    msgs = EG.matrix_messages()
    for kind, col in by.items():
        got = EG.by_status(col)
        assert got[R.OK] and got[R.NOT_FOUND] and got[R.E_READ] and got[ER.E_UNSUPPORTED], (kind, got)
    invalid = [t for t in range(256) if t not in ER._VALID]
    assert len(invalid) == 241
    sm, im = by[ER.STRMAP | ER.INT], by[ER.INTMAP | ER.INT]
    for j in range(256 * 8):
        t, size, shape = j // 8, j // 4 % 2, j % 4
        if t in ER._VALID or shape == 3:
            continue
        if size == 0 and shape == 0:  # an invalid key byte over an empty map: StrMap reads the header, IntMap tests first
            assert sm[j].status == R.E_READ and im[j].status == ER.E_UNSUPPORTED and im[j].aux == t, (t, sm[j], im[j])
        elif size == 0 and shape == 1:  # an int key and an invalid value byte: both read the header
            assert sm[j].status == R.E_READ and im[j].status == R.E_READ
        elif size == 0:  # a string key and an invalid value byte
            assert sm[j].status == R.E_READ and im[j].status == ER.E_UNSUPPORTED and im[j].aux == R.STRING
        else:  # size 1: the lookup's own skip fails first
            assert sm[j].status == R.E_READ and im[j].status == R.E_READ and sm[j].type == 0
    for t in (R.STOP, R.VOID, R.UTF8, R.UTF16):  # Valid(), though nothing can skip them
        j = t * 8
        assert sm[j].status == ER.E_UNSUPPORTED and sm[j].aux == t | R.I32 << 8 and im[j].status == ER.E_UNSUPPORTED
        assert sm[j + 2].status == R.OK and sm[j + 2].len == 0 and sm[j + 2].aux == R.STRING | t << 8
        assert im[j + 1].status == R.OK and im[j + 1].aux == R.I32 | t << 8
        assert by[ER.LISTSTR][j + 3].status == R.OK and by[ER.LISTSTR][j + 3].type == t
    keys = {k for c in im if c.status == R.OK for k in c.keys}
    assert {0x7F, 0x80, 0xFF, 2 ** 64 - 2 ** 15, 2 ** 64 - 2 ** 31, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1} <= keys
    assert {0x80, 0xFF, 2 ** 64 - 2 ** 15, 2 ** 63} <= {v for c in im + sm if c.status == R.OK for v in c.vals}
    assert any(c.status == R.OK and c.vals == [0, 1, 0, 0] for c in by[ER.INTMAP | ER.BOOL])
    assert any(c.status == R.OK and c.keys == [7, 8, 7] for c in im)  # duplicates kept, in wire order
    for kind in (ER.LISTSTR, ER.STRMAP | ER.STR, ER.INTMAP | ER.STR):
        assert any(c.status == R.OK and sorted(c.vlens) == sorted(EG.STR_LENS) for c in by[kind]), kind
    assert any(c.status == R.OK and c.klens == list(EG.STR_LENS) for c in by[ER.STRMAP | ER.STR])
    return msgs


def test_kind_by_type_matrix(decode):
    msgs = EG.matrix_messages()
    sets = [check(decode, msgs, cols, "matrix")[0] for cols in EG.MATRIX_SETS]
    matrix_properties(sets)


def test_counts(decode):
    msgs = EG.count_messages()
    want, _ = check(decode, msgs, EG.COUNT_COLUMNS, "counts")
    for col, (_, kind) in zip(want, EG.COUNT_COLUMNS):
        fixed = kind & ER.INTMAP and kind & 15 != ER.STR
        assert {c.len for c in col if c.status == R.OK} >= set(EG.FIXED_COUNTS if fixed else EG.VAR_COUNTS), kind


def test_counts_around_the_staged_emits_rows(decode):
    msgs, counts = EG.stage_messages()
    want, _ = check(decode, msgs, EG.STAGE_COLUMNS, "stage")
    for col in want:
        assert {c.len for c in col} == set(counts)
        assert sum(a.len != b.len for a, b in zip(col, col[1:])) > len(col) * 0.8


def test_alignment_and_the_arenas_end(decode):
    for name in EG.TARGETS:
        msgs = EG.align_batch(name)
        want, _ = check(decode, msgs, EG.ALIGN_COLUMNS, "target %s" % name)
        wb, _ = check(decode, msgs, EG.ALIGN_COLUMNS_B, "target %s" % name)
        assert sum(c.status == R.OK for col in want + wb for c in col) >= 16, name
        assert len({R.get_by_path(m, [(R.FIELD, 2)]).start % 16 for m in msgs}) == 16


def test_geometry_messages(decode):
    msgs = EG.geometry_messages(257)
    want, _ = check(decode, msgs, EG.GEOMETRY_COLUMNS, "geometry")
    got = EG.by_status(want)
    assert got[R.OK] > 0.6 * 257 * 8 and got[R.NOT_FOUND] > 0.1 * 257 * 8


def test_nests_around_the_lds_frames(decode):
    msgs = EG.deep_messages()
    want, deep = check(decode, msgs, EG.DEEP_COLUMNS, "nests")
    depth = [d for d in EG.DEEP_DEPTHS for _ in range(3)]
    assert (deep[:, 0] == (np.array(depth) + 1 > EG.LDS_FRAMES)).all() and deep[:, 0].any() and not deep[:, 0].all()
    assert all(c.status == R.OK and c.len == 2 for c in want[0])
    for col, d in zip(want[1:], EG.DEEP_DEPTHS):
        for c, md in zip(col, depth):
            assert (c.status == R.OK and c.vlens == [2, 0, 4]) if md == d else c.status != R.OK


def test_fuzz_inputs(decode):
    """the first 400 messages of the mutated fuzz corpus under both column sets"""
    msgs = EG.fuzz_corpus(400)
    for cols in (EG.FUZZ_A, EG.FUZZ_B):
        check(decode, msgs, cols, "fuzz")


def test_fuzz_corpus_holds_every_status():
    """the seeds of the corpus the GPU test runs, judged by the checker alone"""
    msgs = EG.fuzz_corpus()
    for cols in (EG.FUZZ_A, EG.FUZZ_B):
        got = EG.by_status(EG.expect(msgs, cols))
        assert got[R.OK] and got[R.NOT_FOUND] and got[R.E_READ] and got[ER.E_UNSUPPORTED], got


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """ents_host.cpp as a program (-DENTS_MAIN: every message, the blob and
    every cell's entries in a heap block of their own) over corpus files: the
    counts and the sum it prints are the checker's."""
    need_hipcc()
    sets = [(EG.matrix_messages(), EG.MATRIX_SETS[0]), (EG.matrix_messages(), EG.MATRIX_SETS[1]),
            (EG.count_messages(), EG.COUNT_COLUMNS), (EG.stage_messages()[0], EG.STAGE_COLUMNS),
            (EG.deep_messages(1), EG.DEEP_COLUMNS)] + [(EG.align_batch(t), EG.ALIGN_COLUMNS) for t in EG.TARGETS]
    files, by, ents, total, cells = [], [0] * 5, 0, 0, 0
    for j, (msgs, cols) in enumerate(sets):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        EG.write_corpus(files[-1], msgs, cols, G.compile_paths(to_paths([p for p, _ in cols])))
        for p, kind in cols:  # the program gives every message the arena offset 0
            for m in msgs:
                c = ER.cell(m, p, kind)
                cells += 1
                by[c.status] += 1
                if c.status == R.OK and c.len:
                    ents += c.len
                    sk, sv = bool(kind & ER.STRMAP), kind == ER.LISTSTR or kind & 15 == ER.STR
                    total += sum(c.keys) - (c.val * c.len if sk else 0) + sum(c.klens)
                    total += sum(c.vals) - (c.val * c.len if sv else 0) + sum(c.vlens)
    exe = build_ents(str(tmp_path / "entshost"), ("-DENTS_MAIN",))
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    assert out.startswith("%d cells, " % cells), out
    assert out.strip().endswith("OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d; %d entries, sum %d" % (
        *by, ents, total % 2 ** 64)), out
