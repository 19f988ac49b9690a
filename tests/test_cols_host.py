"""CPU: the typed-column decode itself (dynamicgo_amd/csrc/cols_device.h: cl_cell
behind tg_walk, cl_elem, cl_find: the code the kernels run) built for the host
by cols_host.cpp and compared, cell by cell and element by element, with the
checker (colsref.py) over all of colsgen's inputs, the ones the GPU tests of
test_gpu_cols.py use. Every message is followed by 16 bytes of 0xAA."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import colsgen as CG
import colsref as CR
import t2jgen
import tgetgen as TG
import tgetref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import to_paths

HERE = os.path.dirname(os.path.abspath(__file__))


def build_cols(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "cols_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host decode with" % B.HIPCC)


@pytest.fixture(scope="module")
def colslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_cols(str(tmp_path_factory.mktemp("cols") / "libcolshost.so"), ("-shared",)))
    lib.cell.restype = C.c_int
    lib.cell.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                         C.c_uint64, C.POINTER(C.c_uint32)]
    lib.elem.restype = C.c_uint64
    lib.elem.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64]
    lib.find.restype = C.c_uint64
    lib.find.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def decode(colslib):
    """decode(msgs, columns, root_type) -> ([arrays of column k as colsgen.arrays gives them], deep[n, P])"""
    lib = colslib

    def run(msgs, columns, root_type=R.STRUCT):
        blob = G.compile_paths(to_paths([p for p, _ in columns]))
        off_steps, off_pool = np.frombuffer(blob, dtype="<u4", count=8)[5:7].tolist()
        blob += b"\0" * 16
        n = len(msgs)
        cols = [{f: np.zeros(n, dtype=np.uint64) for f in CG.CELL_FIELDS} for _ in columns]
        elems = [[] for _ in columns]
        offs = [[0] for _ in columns]
        deep = np.zeros((n, len(columns)), dtype=bool)
        out = (C.c_uint32 * 7)()
        base = 0
        for i, m in enumerate(msgs):
            buf = m + b"\xAA" * 16
            for k, (_, kind) in enumerate(columns):
                deep[i, k] = lib.cell(buf, len(m), blob, off_steps, off_pool, k, root_type, kind, base, out)
                st, ty, step, aux, ln, lo, hi = out
                val = lo | hi << 32
                for f, v in zip(CG.CELL_FIELDS, (st, ty, step, aux, val, ln)):
                    cols[k][f][i] = v
                if kind & CR.LIST and st == R.OK:  # the element decode, from the message alone
                    elems[k] += [lib.elem(buf, val - base, ty, j) for j in range(ln)]
                offs[k].append(len(elems[k]))
            base += len(m)
        for k in range(len(columns)):
            cols[k]["elems"] = np.array(elems[k], dtype=np.uint64)
            cols[k]["off"] = np.array(offs[k], dtype=np.uint64)
        return cols, deep

    return run


def check(decode, msgs, columns, what, root_type=R.STRUCT):
    want = CG.expect(msgs, columns, root_type)
    got, deep = decode(msgs, columns, root_type)
    for k in range(len(columns)):
        CG.same(got[k], CG.arrays(want[k]), "%s, column %d" % (what, k))
    return want, deep


def test_kind_by_wire_type_matrix(decode):
    msgs = CG.matrix_messages()
    want, _ = check(decode, msgs, CG.MATRIX_COLUMNS, "matrix")
    for st in (R.OK, R.NOT_FOUND, R.E_READ, CR.E_UNSUPPORTED):
        assert CG.share(want, st) > 0.01, st
    for col, (_, kind) in zip(want, CG.MATRIX_COLUMNS):  # every kind has a cell it takes
        assert any(c.status == R.OK for c in col), kind
    ints = [c.val for c in want[2] if c.status == R.OK]  # Node.Int: the unsigned byte and the widths' edges
    assert {0x80, 0xFF, 2 ** 64 - 2 ** 15, 2 ** 64 - 2 ** 31, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1} <= set(ints)
    assert [c.val for c in want[0] if c.status == R.OK] == [0, 1, 0, 0]  # DecodeBool: 2 and 0xFF are false
    assert {c.val for c in want[3] if c.status == R.OK} == set(CG.DOUBLES)
    lens = [c.val for c in want[5] if c.status == R.OK]
    assert 0 in lens and 1 in lens and 2 ** 31 - 1 not in lens  # the count over a short body is the lookup's E_READ


def test_alignment_and_the_arenas_end(decode):
    for name in CG.TARGETS:
        msgs = CG.align_batch(name)
        want, _ = check(decode, msgs, CG.ALIGN_COLUMNS, "target %s" % name)
        assert sum(c.status == R.OK for col in want for c in col) >= 16, name


def test_geometry_messages(decode):
    msgs = CG.geometry_messages(257)
    want, _ = check(decode, msgs, CG.GEOMETRY_COLUMNS, "geometry")
    assert CG.share(want, R.OK) > 0.6 and CG.share(want, R.NOT_FOUND) > 0.1


def test_chains_around_the_lds_frames(decode):
    chains = CG.deep_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want, deep = check(decode, msgs, CG.DEEP_COLUMNS, "chains")
    for col, path in ((0, [(R.FIELD, 2)]), (1, [(R.FIELD, 1)])):
        frames = np.array([TG.chain_frames(k, lf, path) for k, lf in chains])
        assert (deep[:, col] == (frames > TG.LDS_FRAMES)).all()
        assert deep[:, col].any() and not deep[:, col].all()
    assert all(c.status == R.OK and c.val == 9 for c in want[0])
    hit = [(k, lf) == ("L" * d, "l") for d in CG.DEEP_LIST_DEPTHS for k, lf in chains]
    cells = [c for col in want[2:] for c in col]
    assert all(c.status == R.OK and c.elems == [1, 2 ** 64 - 1] for c, h in zip(cells, hit) if h) and sum(hit) == 6


def test_lists(decode):
    msgs = CG.list_messages()
    want, _ = check(decode, msgs, CG.LIST_COLUMNS, "lists")
    for col in want[:2]:
        assert sorted({c.len for c in col if c.status == R.OK}) == sorted(CG.LIST_COUNTS)
        for st in (R.NOT_FOUND, R.E_READ, CR.E_UNSUPPORTED):
            assert any(c.status == st for c in col), st
    assert {c.type for c in want[0] if c.status == R.OK and c.len} == {R.BYTE, R.I16, R.I32, R.I64}
    for et, w in ((R.BYTE, 1), (R.I16, 2), (R.I32, 4)):  # both extensions are on show at every narrow width
        es = [e for c in want[0] if c.status == R.OK and c.type == et for e in c.elems]
        assert any(e >> 63 for e in es) == (et != R.BYTE) and any(e >> (8 * w - 1) & 1 for e in es)


def test_fuzz_inputs(decode):
    """the first 400 messages of the fuzz corpus and of its mutated form, both column sets"""
    rng, mrng = random.Random(1234), random.Random(4321)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(400)]
    bad = [t2jgen.mutate(mrng, m) for m in msgs]
    for ms, what in ((msgs, "fuzz"), (bad, "mutated")):
        for cols in (CG.FUZZ_A, CG.FUZZ_B):
            check(decode, ms, cols, what)


def test_find_is_the_upper_bound(colslib):
    """cl_find, the emit's search: over offsets with runs of empty messages, every element finds the message that
    owns it, from the whole range and from every range narrowed to a chunk of 2048 elements"""
    rng = random.Random(3)
    counts = [rng.choice((0, 0, 1, 2, 63, 64, 257, 700)) for _ in range(300)] + [0, 0]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n, total = len(counts), int(off[-1])
    owner = np.repeat(np.arange(n), counts)
    p = off.ctypes.data
    for g in range(total):
        assert colslib.find(p, 0, n, g) == owner[g], g
    for base in range(0, total, 2048):  # CL_EMIT_CHUNK
        last = min(base + 2047, total - 1)
        lo, hi = colslib.find(p, 0, n, base), colslib.find(p, 0, n, last) + 1
        for g in (base, (base + last) // 2, last):
            assert colslib.find(p, lo, hi, g) == owner[g], (base, g)


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """cols_host.cpp as a program (-DCOLS_MAIN: every message and the blob in a
    heap block of their own, 16 spare bytes each) over a corpus file: the
    counts and the sum it prints are the checker's."""
    need_hipcc()
    chains = CG.deep_chains(per_depth=1)
    sets = [(CG.matrix_messages(), CG.MATRIX_COLUMNS), (CG.list_messages(), CG.LIST_COLUMNS),
            ([TG.chain_message(k, lf) for k, lf in chains], CG.DEEP_COLUMNS)] + \
        [(CG.align_batch(t), CG.ALIGN_COLUMNS) for t in CG.TARGETS]
    files, by, elems, total, cells = [], [0] * 5, 0, 0, 0
    for j, (msgs, cols) in enumerate(sets):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        CG.write_corpus(files[-1], msgs, cols, G.compile_paths(to_paths([p for p, _ in cols])))
        # the program gives every message the arena offset 0
        want = [[CR.cell(m, p, k) for m in msgs] for p, k in cols]
        for col, (_, kind) in zip(want, cols):
            for c in col:
                cells += 1
                by[c.status] += 1
                if c.elems is not None and c.status == R.OK:
                    elems += len(c.elems)
                    total += sum(c.elems)
                elif kind != CR.STR and not kind & CR.LIST:
                    total += c.val
    exe = build_cols(str(tmp_path / "colshost"), ("-DCOLS_MAIN",))
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    assert out.startswith("%d cells, " % cells), out
    assert out.strip().endswith("OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d; %d elements, sum %d" % (
        *by, elems, total % 2 ** 64)), out
